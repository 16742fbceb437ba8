/* avt_fitscore.h — C ABI of the fit score: how well a fitted avatar explains the depth image it was fitted to, in integers,
 * part of libavatar_hip.so.
 *
 * The reference's only judgement of a fit is visual: live-demo.cpp:428-445 renders the avatar over the camera image and a
 * person looks at it.  The trackers' own loss test counts labelled pixels (frameDecision, live-demo.cpp:335-383), and the
 * objective measures data point to nearest model point only: a limb stretched into free space costs nothing.  The score is the
 * overlay in numbers, both directions, per body part.
 *
 * THE RULE.
 *
 * Inputs and selection.  Per image: a model depth image R (float32, renderDepth: 0 = no model), a model part image M (uint8,
 * renderPartMask: 255 = none), an observed depth image D (float32) and a box tl.x tl.y br.x br.y, inclusive.  All images are
 * rows x cols.  P = num_parts, given at creation, 1 <= P <= 254.  tol is a float in metres, >= 0, +inf allowed; NaN or negative
 * is refused.  stride >= 1.  A pixel (r, c) is selected iff r % stride == 0 && c % stride == 0, counted from the image origin,
 * not from the box.
 *
 * Per selected pixel.
 *   m = R > 0.f                    the model covers the pixel (NaN is not > 0)
 *   d = inside box && D > 0.f      the camera saw foreground: zero, negative and NaN depths are not data, +inf is.  Outside the
 *                                  box nothing is data, whatever D holds (the masked depth of avt_bgsub keeps the raw scene
 *                                  there).  A box with br.x == -1 is the whole image, whatever its other three values.  An empty
 *                                  box (tl > br in either axis), or one that does not lie inside the image, selects no observed
 *                                  pixel; that is not an error.  Host boxes and boxes read from device memory obey the same rule.
 *   row p = M if m && M < P, else P: a model pixel whose mask byte is 255, and every pixel without model.  (The depth fill works
 *                                  by rows and the mask fill by columns, so the two coverages differ at edges; both cases count.)
 *   A selected pixel with P <= M < 255 fails the call, whatever R is; the message names num_parts; the handle then holds no result.
 *   delta = (double)R - (double)D, one IEEE subtraction.  With tol promoted to double, tested in this order:
 *       m && d, fabs(delta) <= tol   AGREE       model and data agree
 *       m && d, delta < -tol         IN_FRONT    the model is nearer than the surface the camera saw: free space violated
 *       m && d, otherwise            BEHIND      data in front of the model (delta > tol)
 *       m && !d                      MODEL_ONLY  model where the camera saw background
 *       !m && d                      DATA_ONLY   data the model does not cover; always row P
 *       !m && !d                     -           counts nothing
 *   (R and D both +inf give a NaN delta, which fails the first two tests: BEHIND.)
 *   For m && d pixels, um = rint(fmin(fabs(delta), 1000.0) * 1e6), rounded to nearest even, converted to a signed 64-bit integer
 *   (fmin drops a NaN: the clamp).  It is one multiplication and one rounding: nothing to contract.  um is added to ABS_UM, and to
 *   ABS_UM_AGREE when the class is AGREE.
 *
 * Result.  Per image a (P + 1) x 7 row-major table of signed 64-bit integers, columns AVT_FITSCORE_AGREE .. _ABS_UM_AGREE.
 * Every entry is an integer sum: it does not depend on the launch shape, on how images are split into calls, or on arrival
 * order.  The sums are 64-bit from the first place at which two pixels meet (five clamped pixels already pass 2^32).  Each call
 * replaces the previous result.
 *
 * Derived figures (ark/FitScore.h derive(), fitscore.metrics): host arithmetic on the integers, for each row and for the column
 * sums: integer sums first, each converted to double once, then the division (and for the errors one multiplication by 1e-6);
 * NaN on a zero denominator.  both = AGREE + IN_FRONT + BEHIND.
 *   iou                 both / (both + MODEL_ONLY + DATA_ONLY)             (total only: DATA_ONLY has no part)
 *   agree               AGREE / both
 *   violation           (IN_FRONT + MODEL_ONLY) / (both + MODEL_ONLY)      the share of model pixels the observation contradicts
 *   unexplained         (BEHIND + DATA_ONLY) / (both + DATA_ONLY)          (total only)
 *   mean_abs_err        ABS_UM / both * 1e-6                               metres
 *   mean_abs_err_agree  ABS_UM_AGREE / AGREE * 1e-6
 * No thresholds come with them: nobody has measured what a good or a bad fit scores on real data.
 *
 * Conventions: row-major images; a handle owns a non-blocking stream on its device.  Functions return 0 on success;
 * avt_last_error() (avt.h) describes a failure.
 */
#ifndef AVT_FITSCORE_H_
#define AVT_FITSCORE_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct avt_fitscore avt_fitscore;
struct avt_renderer;      /* avt_render.h */
struct avt_bgsub;         /* avt_bgsub.h */

/* the columns of a table row */
enum { AVT_FITSCORE_AGREE = 0, AVT_FITSCORE_IN_FRONT, AVT_FITSCORE_BEHIND, AVT_FITSCORE_MODEL_ONLY, AVT_FITSCORE_DATA_ONLY, AVT_FITSCORE_ABS_UM,
       AVT_FITSCORE_ABS_UM_AGREE, AVT_FITSCORE_COLS };

/* A scorer of up to max_images images per call with num_parts parts on `device` (the numbers behind the display of
 * live-demo.cpp:428-445).  The tables, the boxes and the image indices of a call live in device scratch sized here, so the two
 * calls that read their images on the device allocate nothing; avt_fitscore_images and avt_fitscore_rendered also stage host
 * images, in buffers that grow to the largest batch seen.  device < 0 makes a host-only handle that checks arguments and
 * refuses to score. */
int avt_fitscore_create(int device, int num_parts, int max_images, avt_fitscore** out);
void avt_fitscore_destroy(avt_fitscore* fs);

/* live-demo.cpp:428-445 in numbers, every image on the host: n_images x rows x cols model_depth (R), model_mask (M), observed
 * (D); boxes n_images x 4 ints, NULL: whole images.  Staged in bounded batches.  Returns with the result on the host. */
int avt_fitscore_images(avt_fitscore* fs, int n_images, int rows, int cols, const float* model_depth, const unsigned char* model_mask,
                        const float* observed, const int* boxes, float tol, int stride);

/* live-demo.cpp:428-445 in numbers, the model side read where r's last run left it (it must have rendered AVT_RENDER_DEPTH |
 * AVT_RENDER_PART_MASK): image i of that run against observed[i] (host, the run's image count x height x width) and boxes[i]
 * (NULL: whole images).  Returns after the scorer's stream has finished, so the renderer may run again at once.  Both handles
 * must be on one device. */
int avt_fitscore_rendered(avt_fitscore* fs, struct avt_renderer* r, const float* observed, const int* boxes, float tol, int stride);

/* live-demo.cpp:428-445 in numbers, both sides read where they lie: image i of r's last run against image obs_index[i] (host
 * ints, NULL: i) of bg's last avt_bgsub_run_resident, its masked depth inside the box that run left on the device.  No image is
 * copied and the host waits once, at the end, for a few hundred integers per image; bg's next upload, run and destroy wait for
 * the scoring.  All three handles must be on one device, the image sizes must match, and bg must have a run behind it. */
int avt_fitscore_rendered_from_bgsub(avt_fitscore* fs, struct avt_renderer* r, struct avt_bgsub* bg, const int* obs_index, float tol, int stride);

/* The result of the last call (the numbers of live-demo.cpp:428-445): table = n_images x (num_parts + 1) x AVT_FITSCORE_COLS,
 * either pointer may be NULL.  Fails with "no score" when no call succeeded since creation or the last one failed. */
int avt_fitscore_get(avt_fitscore* fs, long long* table, int* n_images);
/* waits for the handle's stream (every scoring call above already returns after it; live-demo.cpp:428-445 has no counterpart) */
int avt_fitscore_sync(avt_fitscore* fs);

#ifdef __cplusplus
}
#endif
#endif
