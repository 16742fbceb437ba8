/* avt_rforest.h — C ABI of a forest of several trained trees run as one (ark::RForest), part of libavatar_hip.so.
 *
 * The reference's tools load any number of models and classify each pixel from all of them (rtree-run.cpp:82-122,
 * rtree-run-dataset.cpp:98-159): RTree::predict(depth) per model, the per-part distributions added in model order, the
 * arg-max per pixel.  A forest here is T trees, 1 <= T <= AVT_RFOREST_MAX_TREES, that share num_parts, the part map and the
 * part-map type; anything else is refused at creation with a message.
 *
 * THE RULE.  For a pixel that is walked, let leaf_t be the leaf tree t reaches and d_t its distribution.  Then
 *     sum[p] = (((d_0[p] + d_1[p]) + d_2[p]) + ...)                               in float32, tree order, starting from tree
 * 0's value and not from 0, never contracted (result = model_results; result[i] += ..., rtree-run-dataset.cpp:128-138), and
 *     label  = the first p in ascending order with sum[p] > best, best starting at 0.f            (rtree-run-dataset.cpp:143-158):
 * ties go to the lowest index, a pixel whose sums are all <= 0 or NaN gets 255, and a NaN never wins (the test is `>`).
 * rtree-run.cpp:101-103 divides the sums by T before its arg-max; that is an OpenCV scalar division whose rounding cannot be
 * pinned without OpenCV, so the contract here is the UNDIVIDED sum of rtree-run-dataset.
 *
 * TWO WALKING RULES, each the reference call it extends:
 *   distribution form  RTree::predict(depth) (RTree.cpp:3156-3182): every pixel with depth > 0, probes bounded by the image;
 *                      out = num_parts planes of sums, 0 elsewhere.
 *   label form         RTree::predictBest(depth, ..., interval, top_left, bot_right, fill_in_gaps) (RTree.cpp:3184-3262), as
 *                      avt_rtree_predict_best walks: the interval grid inside the box with the first row skipped, pixels with
 *                      depth == 0 skipped, probes bounded by the region of interest, upscaleGrid's fill clamped to the row.
 *                      Only the last step differs from one tree: leafBestMatch is replaced by the sum and arg-max above, so
 *                      with T = 1 the labels are avt_rtree_predict_best's wherever the leaf has a positive entry.
 *
 * THE SCORE.  rtree-run-dataset calls itself an "empirical validation tool": it shows the arg-max image beside the dataset's
 * part mask.  The score is that comparison in numbers.  Let P = num_parts.  It is a (P + 1) x (P + 1) matrix of 64-bit counts,
 * row-major as conf[truth][predicted]; index P means "none" (255) on either axis.  Of every image, every pixel (r, c) with
 * r % stride == 0 and c % stride == 0 is scored (stride >= 1; 1 takes every pixel):
 *   prediction q  the distribution form's rule and nothing new: a pixel is walked iff depth > 0 (zero, negative and NaN depths
 *                 are not); probes are bounded by the whole image (stride selects which pixels are scored, never what a probe
 *                 reads); every tree is walked; sum and arg-max as in THE RULE; q = P when no sum exceeds 0 and for a pixel
 *                 that is not walked.
 *   truth t       the mask byte, 255 mapped to P.  A byte >= P that is not 255 is refused, as avt_rtree_transfer_* refuses it:
 *                 the call fails with a message that names num_parts and adds nothing to the totals, not even the counts of
 *                 the images before the bad one.
 *   counting      t == P and q == P counts nothing, so conf[P][P] is always 0; otherwise ++conf[t][q].  Row P holds pixels the
 *                 forest labels that the truth calls background; column P holds labelled pixels the forest leaves unlabelled
 *                 (no positive depth, or a leaf sum that is all <= 0 or NaN).
 * Depth values are taken as they come, as predict takes them.  Totals accumulate over calls until a reset and do not depend on
 * how the images are split into calls or batches; counts are 64-bit from the first flush out of a workgroup to the caller.
 *
 * Conventions are avt_rtree.h's: row-major images, float32 depth in metres with 0 = background, uint8 labels with 255 = none,
 * inclusive regions with bot_right.x == -1 for the whole image.  Functions return 0 on success; avt_last_error() (avt.h)
 * describes a failure.
 */
#ifndef AVT_RFOREST_H_
#define AVT_RFOREST_H_

#include "avt_rtree.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AVT_RFOREST_MAX_TREES 16

typedef struct avt_rforest avt_rforest;
struct avt_renderer;      /* avt_render.h */

/* The models of rtree-run-dataset.cpp:98-104, in this order.  Copies the trees (they may be destroyed afterwards) and uploads
 * the packed forest to `device`; device < 0 makes a host-only forest that validates and answers avt_rforest_info but whose
 * inference calls fail.  The trees themselves may be host-only or on any device. */
int avt_rforest_create(const avt_rtree* const* trees, int n_trees, int device, avt_rforest** out);
void avt_rforest_destroy(avt_rforest* rf);
/* models.size(), numParts, partMap.size() and its type (rtree-run-dataset.cpp:98-104), nodes and leaves over all trees; any
 * pointer may be NULL. */
int avt_rforest_info(const avt_rforest* rf, int* n_trees, int* num_parts, int* part_map_len, int* part_map_type, int* total_nodes, int* total_leafs);

/* Distribution form: the summed planes of rtree-run-dataset.cpp:124-138 (RTree::predict per model, RTree.cpp:3156-3182);
 * dist_out = num_parts planes of rows x cols float32. */
int avt_rforest_predict(avt_rforest* rf, const float* depth, int rows, int cols, float* dist_out);
/* Label form: RTree::predictBest's walk (RTree.cpp:3184-3262) with the arg-max of rtree-run-dataset.cpp:143-158; host image
 * in, host labels out (rows x cols bytes). */
int avt_rforest_predict_best(avt_rforest* rf, const float* depth, int rows, int cols, int interval, int tl_x, int tl_y, int br_x, int br_y,
                             int fill_in_gaps, unsigned char* labels_out);

/* Resident forms, as the tree's (avt_rtree.h): the labelling of demo.cpp:179-204 for a batch of streams. */
int avt_rforest_images_upload(avt_rforest* rf, int n_images, int rows, int cols, const float* depth);
/* boxes: n_images x 4 host ints tl.x tl.y br.x br.y, inclusive; br.x == -1 is the whole image; an empty box (tl > br in either
 * axis) leaves that image all 255 and is no error; a box shorter than `interval` rows labels nothing.  A box outside the image
 * or a bad interval fails before anything is queued (demo.cpp:179-204 per stream). */
int avt_rforest_predict_best_resident_boxes(avt_rforest* rf, int interval, const int* boxes, int fill_in_gaps);
/* demo.cpp:179-204 without the host in between: labels every image of `bg`'s last avt_bgsub_run_resident inside the box that
 * run left on the device, reading the masked depth where it lies.  No copy of the depth, no host synchronisation: the forest's
 * stream waits for the run, and bg's next images_upload, run_resident and destroy wait for the labelling.  A box on the device
 * that does not lie inside the image labels nothing.  Both handles must be on one device; `bg` must have a run behind it. */
int avt_rforest_predict_best_from_bgsub(avt_rforest* rf, struct avt_bgsub* bg, int interval, int fill_in_gaps);
/* One image's labels / every image's labels of the last labelling call (demo.cpp:179-204), and the wait for the stream. */
int avt_rforest_labels_download(avt_rforest* rf, int image, unsigned char* labels_out);
int avt_rforest_labels_download_all(avt_rforest* rf, unsigned char* labels_out);
int avt_rforest_sync(avt_rforest* rf);

/* RTree::postProcess for a batch on the device, as the tree's (avt_rtree.h, RTree.cpp:3422-3449, with the DELIBERATE DIFFERENCE
 * described there: connected components on the interval grid, the reference's rule bit for bit at interval 1 only), with the
 * first member's num_parts and part-map type, which is what postProcess depends on. */
int avt_rforest_labels_upload(avt_rforest* rf, int n_images, int rows, int cols, const unsigned char* labels);
/* RTree.cpp:3422-3449 in place on the images of the last labelling call; see avt_rtree_post_process_resident and its deliberate difference. */
int avt_rforest_post_process_resident(avt_rforest* rf, int interval, const int* boxes, double dist_to_pre_weight);
/* RTree.cpp:3422-3449 inside the device boxes of bg's last run; see avt_rtree_post_process_from_bgsub and its deliberate difference. */
int avt_rforest_post_process_from_bgsub(avt_rforest* rf, struct avt_bgsub* bg, int interval, double dist_to_pre_weight);
/* com_pre of RTree.cpp:3422-3449 per image slot; see avt_rtree_com_pre_set / _get and the deliberate difference of the stage they serve. */
int avt_rforest_com_pre_set(avt_rforest* rf, int first, int n, const double* com, const unsigned char* valid);
int avt_rforest_com_pre_get(avt_rforest* rf, int first, int n, double* com, unsigned char* valid);

/* THE SCORE above.  The totals start at zero, and score_reset puts them back there. */
int avt_rforest_score_reset(avt_rforest* rf);
/* n_images host images of rows x cols: float32 depth and uint8 part masks (255 = none).  They are staged in buffers of the call,
 * in bounded batches: the resident images and labels of images_upload and of the labelling calls stay as they were. */
int avt_rforest_score_images(avt_rforest* rf, int n_images, int rows, int cols, const float* depth, const unsigned char* part_mask, int stride);
/* The depth and part-mask images of r's last run (it must have rendered AVT_RENDER_DEPTH | AVT_RENDER_PART_MASK), read where
 * they lie: no copy, no image crosses to the host.  Returns after the forest's stream has finished, so the renderer may run
 * again at once.  Both handles must be on one device. */
int avt_rforest_score_rendered(avt_rforest* rf, struct avt_renderer* r, int stride);
/* The totals since the last reset: confusion = (num_parts + 1)^2 counts conf[truth][predicted], the number of images and the
 * number of pixels the stride selected; zeros on a forest that has scored nothing.  Any pointer may be NULL. */
int avt_rforest_score_get(avt_rforest* rf, long long* confusion, long long* n_images, long long* n_pixels);

#ifdef __cplusplus
}
#endif
#endif
