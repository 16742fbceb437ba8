/* avt_bgsub.h — C ABI of the background subtraction on the GPU (the tracker's front end), part of
 * libavatar_hip.so.
 *
 * The first stage of every frame of the reference's trackers: `ark::BGSubtractor::run` (BGSubtractor.cpp:159-163)
 * turns an XYZ map into a per-pixel component mask and the foreground box, which the demos use to blank the depth
 * image before the forest (demo.cpp:179-192, live-demo.cpp:317-332).  The result is the reference's, bit for bit:
 *
 *   mask byte   255 invalid or background; 254 unvisited (only when the run is capped, below); 0..253 component ids
 *   thresholds  (float)(1200000.0 / (rows * cols) * rel), in double, rel promoted exactly  (BGSubtractor.cpp:160-161)
 *   near test   z == 0, or a 3x3 background neighbour (clipped) with z != 0 at squared distance < nn   (:30-76)
 *   components  candidates joined across 4-neighbour edges with !(squared distance > neighb), a component of fewer than
 *               max(rows * cols / 1000, 100) pixels is 255; kept components get ids in raster order of their first
 *               pixel                                                                                        (:80-123)
 *   cap         the 254th kept component (id 253) ends the run (:124): later pixels stay 254, the box keeps its
 *               previous value, comps stay in id order
 *   box         min / max column and first / last row of non-255 pixels; empty: (cols-1, rows-1), (0, 0)  (:128-151)
 *   comps       {size, id} of the kept components, sorted by size then id, both descending                   (:152-154)
 *
 * Besides the mask a run returns the demos' use of it: the masked depth (z, set to 0 inside the box where the mask is
 * >= 254) and fg_count, the pixels with mask < 254 inside the box (live-demo.cpp:318-332's subCnz).
 *
 * Conventions: images are row-major rows x cols x 3 float32 (cv::Vec3f layout), cols < 65536 (the reference packs
 * (r << 16) + c).  A handle owns a non-blocking stream on its device.  Functions return 0 on success;
 * avt_last_error() (avt.h) describes a failure.  AVT_STATUS_DEVICE_FAULT (3, avt.h) means a kernel ran out of a bounded
 * retry and could not vouch for its result.
 */
#ifndef AVT_BGSUB_H_
#define AVT_BGSUB_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct avt_bgsub avt_bgsub;

#define AVT_BGSUB_MAX_COMPS 254

/* Per-image result: top_left / bot_right are (x, y) and inclusive; on input they are the previous box (cv::Point()
 * = (0, 0) before the first run, BGSubtractor.h), kept as they are when the run is capped. */
typedef struct avt_bgsub_frame {
    int top_left[2];
    int bot_right[2];
    int capped;                              /* 1: the run ended at the 254th kept component (BGSubtractor.cpp:124) */
    int fg_count;                            /* pixels with mask < 254 inside the box                              */
    int n_comps;                             /* entries of comps                                                   */
    int comps[AVT_BGSUB_MAX_COMPS][2];       /* {size, id}: sorted as comps_by_size (:153), id order when capped    */
} avt_bgsub_frame;

/* BGSubtractor(cv::Mat background) (BGSubtractor.h): n_backgrounds images of rows x cols x 3 float32 are copied to
 * `device`.  backgrounds may be NULL (all zero until avt_bgsub_set_background). */
int avt_bgsub_create(int device, int n_backgrounds, int rows, int cols, const float* backgrounds, avt_bgsub** out);
void avt_bgsub_destroy(avt_bgsub* bg);
/* bgsub.background = ... (live-demo.cpp:207): replaces background `index`. */
int avt_bgsub_set_background(avt_bgsub* bg, int index, const float* xyz);

/* cv::Mat BGSubtractor::run(image, comps_by_size) (BGSubtractor.cpp:159-163) on one host image against background
 * `background_index`: mask_out rows x cols bytes, masked_depth_out rows x cols float32 (nullable), info in: previous
 * box, out: the result.  numThreads has no counterpart.  Uses the first resident slot. */
int avt_bgsub_run(avt_bgsub* bg, int background_index, const float* xyz, float nn_rel, float neighb_rel, unsigned char* mask_out,
                  float* masked_depth_out, avt_bgsub_frame* info);

/* Batch form for many streams or a recorded sequence: upload n images (n x rows x cols x 3), image i against
 * background bg_index[i] (NULL: background i); prev_boxes n x 4 (tl.x tl.y br.x br.y), NULL: every slot keeps the box
 * of its previous run ((0,0),(0,0) for a slot new to the handle).  avt_bgsub_run_resident queues one launch sequence
 * on the handle's stream; avt_bgsub_download waits for it and copies image `image` out (mask_out, masked_depth_out
 * nullable; comps sorted as in avt_bgsub_run); avt_bgsub_sync waits for the stream. */
int avt_bgsub_images_upload(avt_bgsub* bg, int n_images, const float* images, const int* bg_index, const int* prev_boxes);
int avt_bgsub_run_resident(avt_bgsub* bg, float nn_rel, float neighb_rel);
int avt_bgsub_download(avt_bgsub* bg, int image, unsigned char* mask_out, float* masked_depth_out, avt_bgsub_frame* info);
int avt_bgsub_sync(avt_bgsub* bg);

/* Depth images in: the recorded-data path of the reference never receives an XYZ map, it reads a one-channel depth image
 * (util::readDepth, Util.cpp:176-209; demo.cpp:126,166) and expands it with CameraIntrin::depthToXYZ
 * (Calibration.cpp:82-95).  These entries take the depth image (row-major rows x cols float32) and a camera
 * {fx, fy, cx, cy}, upload a third of the bytes and expand on the device, bit for bit depthToXYZ's float expression
 *   x = ((float)c - cx) * z / fx,  y = ((float)r - cy) * z / fy,  z = z
 * (IEEE division, nothing fused, denormals kept, nothing clamped or validated: a zero, negative, infinite or NaN depth
 * or fx == 0 gives what IEEE gives).  Everything after the expansion is the XYZ path's.
 *
 * avt_bgsub_depth_upload is avt_bgsub_images_upload with depth images (n x rows x cols) and one camera per image
 * (intrin n x 4): same argument checks, same bg_index / prev_boxes, same end state (avt_bgsub_run_resident next).  The
 * depth is staged in the buffer of the run's masked depth, which holds nothing anyone may read between an upload and the
 * next run (a reader on another stream is waited for first, as before any upload).
 * avt_bgsub_run_depth is avt_bgsub_run on one depth image (intrin 4 floats).
 * avt_bgsub_set_background_depth is avt_bgsub_set_background (live-demo.cpp:207) from a depth image; it is staged in the
 * run's label scratch (dead between runs), not in the masked depth: the last run's result stays downloadable across a
 * change of background, as it does for an XYZ one.  It also overwrites the first camera of the last depth upload, which
 * nothing reads any more: that upload's expansion was queued by the upload itself, in front of this call.
 * avt_bgsub_xyz_download copies the resident XYZ map of image `image` out (rows x cols x 3), after either kind of upload:
 * for a caller who wants the map itself (a display, readXYZ's result, Util.cpp:211-217). */
int avt_bgsub_depth_upload(avt_bgsub* bg, int n_images, const float* depth, const float* intrin, const int* bg_index, const int* prev_boxes);
int avt_bgsub_run_depth(avt_bgsub* bg, int background_index, const float* depth, const float* intrin, float nn_rel, float neighb_rel,
                        unsigned char* mask_out, float* masked_depth_out, avt_bgsub_frame* info);
int avt_bgsub_set_background_depth(avt_bgsub* bg, int index, const float* depth, const float* intrin);
int avt_bgsub_xyz_download(avt_bgsub* bg, int image, float* xyz_out);

#ifdef __cplusplus
}
#endif
#endif
