/* avt_subsample.h — C ABI of the device-side subsampling of label batches into a context's resident frames, part of
 * libavatar_hip.so.
 *
 * The reference's trackers walk the interval grid of the labelled depth image on the host (demo.cpp:216-250) and hand the kept
 * points to the optimiser.  Here the XYZ maps (avt_bgsub), the labels (avt_rtree / avt_rforest) and the frame slots (avt_ctx)
 * are all device memory, so the walk runs there and nothing but a table of counts comes back.
 *
 * THE RULE (demo.cpp:216-250, as tracker.subsample and ark::subsampleGrid state it).
 *
 * Inputs per image i: a rows x cols uint8 label image (255 = background), the rows x cols x 3 float32 XYZ map of the same image,
 * an inclusive box tl.x tl.y br.x br.y, interval[i] >= 1, and the context's num_parts.
 *
 * Grid.  The pixels (tl.y + a * interval, tl.x + b * interval) with row <= br.y and column <= br.x, in raster order (rows outer,
 * columns inner).  A box with tl.x > br.x or tl.y > br.y has no grid pixel: the frame has 0 points (what the background
 * subtractor leaves for an empty mask, e.g. (129,99),(0,0)).  Any other HOST box that does not lie inside the image is refused
 * before anything is queued (br.x == -1 stands for the whole image).  A box read from device memory (boxes == NULL) cannot be
 * refused in advance: one that does not lie inside the image has no grid pixel either, as the trackers treat it.
 *
 * Kept pixels.  A grid pixel is kept iff its label != 255.  The k-th kept pixel in raster order becomes point k of frame i:
 *   data[3k + 0] = (double)x, data[3k + 1] = -(double)y, data[3k + 2] = (double)z, labels[k] = (int)label
 * widened first, then negated (demo.cpp:245); bits are copied, nothing is clamped or filtered (NaN, inf, -0, denormals pass).
 *
 * Counts.  count[i][0] is the number of kept pixels, count[i][1 + q] the number with label q, q < num_parts.
 *
 * Bad label.  A kept label >= num_parts (demo.cpp:236-243 exits there) fails the call; the message names the first such image.
 * Overflow.  count[i][0] > max_points_per_frame fails the call the same way; no kernel writes past a frame slot.
 * After either failure no frame is resident or pending, and the handle stays usable.
 *
 * Centroid (demo.cpp:253).  Only for the images the caller asks for and only when count > 0.  Per coordinate c:
 * s = 0; for k in frame order: s += data[3k + c]; in double, then s / (double)count, one IEEE division: bit for bit what
 * ark::reinitState and tracker.reinit_state compute.  The sum is serial by definition: one lane per (image, coordinate).
 *
 * Commit.  A subsample call writes the points into slots 0 .. n - 1 of the context and leaves the frames PENDING: nothing is
 * resident, avt_optimize_resident* refuses.  avt_frames_subsample_commit makes them resident with N[i] = keep[i] ? count[i][0] : 0
 * by avt_frames_upload's bookkeeping: a changed number of frames invalidates the resident state, the same number keeps
 * it.  No data moves.  The host path hands a lost stream over as an empty frame; with keep = fitted both paths leave the context
 * with identical bytes, counts and launch shape.
 *
 * Conventions: functions return 0 on success; the last-error text of avt.h describes a failure.  Everything is queued on the
 * context's stream, which waits for the forest handle's and the background subtractor's streams by events; the host waits
 * once, at the end, for the table.  Scratch lives in the context and only grows.
 */
#ifndef AVT_SUBSAMPLE_H_
#define AVT_SUBSAMPLE_H_

#ifdef __cplusplus
extern "C" {
#endif

struct avt_ctx;           /* avt.h */
struct avt_rtree;         /* avt_rtree.h */
struct avt_rforest;       /* avt_rforest.h */
struct avt_bgsub;         /* avt_bgsub.h */

/* The sizes the kernels are built around, for tests that want to stand on their boundaries (no counterpart in demo.cpp:216-250):
 * grid pixels per workgroup of the counting and the writing kernel, and chunk counts one pass of the scan takes. */
#define AVT_SUBSAMPLE_CHUNK 256
#define AVT_SUBSAMPLE_SCAN_WIDTH 256
int avt_frames_subsample_constants(int* chunk, int* scan_width);

/* demo.cpp:216-250 (and :253 for the centroids) for the n = labelled images behind `rt`, image i into frame slot i of `ctx`.
 *   boxes == NULL: the boxes bg's last avt_bgsub_run_resident left on the device; refused unless the labels behind the handle
 *                  are those of that run (avt_rtree_predict_best_from_bgsub, then optionally the post-processing).
 *   boxes != NULL: n x 4 host ints; labels of any origin (avt_rtree_labels_upload); bg needs only resident XYZ maps (an
 *                  avt_bgsub_images_upload, or a depth upload).
 *   n must match bg's image count and size and be <= the context's max_frames; all three handles on one device.
 *   intervals: n ints >= 1.  want_centroid: n bytes or NULL (none).
 *   counts_out: n x (1 + num_parts) ints.  centroid_out: n x 3 doubles (may be NULL when nothing is asked for); rows that were
 *   not asked for, or whose count is 0, are not written.  boxes_out: NULL or n x 4 ints, the boxes used.
 * Everything is validated before anything is queued.  On success the frames are pending (avt_frames_subsample_commit). */
int avt_frames_subsample_rtree(struct avt_ctx* ctx, struct avt_rtree* rt, struct avt_bgsub* bg, const int* boxes, const int* intervals,
                               const unsigned char* want_centroid, int* counts_out, double* centroid_out, int* boxes_out);
/* demo.cpp:216-250 with the labels behind a forest */
int avt_frames_subsample_rforest(struct avt_ctx* ctx, struct avt_rforest* rf, struct avt_bgsub* bg, const int* boxes, const int* intervals,
                                 const unsigned char* want_centroid, int* counts_out, double* centroid_out, int* boxes_out);

/* The pending frames become resident (the hand-over of demo.cpp:216-250's cloud to the optimiser): keep n bytes, NULL = all;
 * frame i has count[i][0] points where keep[i], else 0.  Fails with "nothing pending" unless a subsample call succeeded since the
 * last install of frames. */
int avt_frames_subsample_commit(struct avt_ctx* ctx, const unsigned char* keep);

#ifdef __cplusplus
}
#endif
#endif
