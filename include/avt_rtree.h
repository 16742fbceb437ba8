/* avt_rtree.h — C ABI of the body-part forest inference, part of libavatar_hip.so.
 *
 * The stage immediately before the fitting path: `ark::RTree` turns a foreground depth image into the per-pixel
 * body-part labels AvatarOptimizer::optimize() consumes (demo.cpp:196-268).  Each entry point names the reference
 * interface it replaces (file:line relative to the reference tree); include/ark/RTree.h re-creates the class on top.
 *
 * Conventions: images are row-major, depth is float32 metres with 0 = background (demo.cpp:185-191), labels are
 * uint8 with 255 = none; a region of interest is (top_left, bot_right) inclusive, bot_right.x == -1 means the whole
 * image (RTree.cpp:3190-3193).  A probe offset / depth that leaves int32 (a tiny, subnormal or infinite quotient) lands
 * outside the image and reads the background depth, as the reference's conversion does; a NaN depth is outside the
 * contract: the reference's conversion of a NaN quotient to int is undefined.  Functions return 0 on success;
 * avt_last_error() (avt.h) describes a failure.
 */
#ifndef AVT_RTREE_H_
#define AVT_RTREE_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct avt_rtree avt_rtree;
struct avt_bgsub;              /* include/avt_bgsub.h */

/* The members of `class RTree` (RTree.h:171-184): nodes, leafData, numParts, partMap (+ its type). */
typedef struct avt_rtree_desc {
    int n_nodes;               /* nodes.size(); node 0 is the root                           (RTree.h:171) */
    int n_leafs;               /* leafData.size()                                            (RTree.h:172) */
    int num_parts;             /* numParts, < 128 (post-processing marks visited labels +128) (RTree.h:175) */
    const float* feature;      /* n_nodes x 5: u.x u.y v.x v.y thresh                        (RTree.h:28-41) */
    const int* links;          /* n_nodes x 3: lnode rnode leafid (leafid == -1: internal)    (RTree.h:36-40) */
    const float* leaf_data;    /* n_leafs x num_parts row-major distributions                 (RTree.h:172) */
    int part_map_len;          /* 0: no part map                                              (RTree.h:177) */
    const int* part_map;       /* SMPL joint -> part                                          (RTree.cpp:3465-3509) */
    int part_map_type;         /* 0 contiguous, 1 disjoint                                    (RTree.cpp:3471-3476) */
} avt_rtree_desc;

/* RTree(int num_parts) + filled members.  Copies everything, uploads the packed tree to `device`; device < 0 makes a
 * host-only tree (file formats, members, post-processing) whose inference calls fail. */
int avt_rtree_create(const avt_rtree_desc* desc, int device, avt_rtree** out);
/* RTree::loadFile (RTree.cpp:2967-3064): binary 'R'..'T' or legacy text format, plus "<path>.partmap" if present. */
int avt_rtree_load(const char* path, int device, avt_rtree** out);
/* RTree::exportFile (RTree.cpp:3066-3120), binary format. */
int avt_rtree_export(const avt_rtree* rt, const char* path);
void avt_rtree_destroy(avt_rtree* rt);
int avt_rtree_info(const avt_rtree* rt, int* n_nodes, int* n_leafs, int* num_parts, int* part_map_len, int* part_map_type);
/* copies the members out; any pointer may be NULL.  leaf_best = leafBestMatch (RTree.cpp:3451-3463). */
int avt_rtree_get(const avt_rtree* rt, float* feature, int* links, float* leaf_data, unsigned char* leaf_best, int* part_map);

/* cv::Mat RTree::predictBest(depth, num_threads, interval, top_left, bot_right, fill_in_gaps) (RTree.cpp:3184-3262):
 * host image in, host labels out (rows x cols bytes).  Runs on the GPU; num_threads has no counterpart. */
int avt_rtree_predict_best(avt_rtree* rt, const float* depth, int rows, int cols, int interval, int tl_x, int tl_y, int br_x, int br_y,
                           int fill_in_gaps, unsigned char* labels_out);

/* std::vector<cv::Mat> RTree::predict(depth) (RTree.cpp:3156-3182): the leaf distribution of every pixel with depth > 0,
 * probes bounded by the image; out = num_parts planes of rows x cols float32 (0 where depth <= 0). */
int avt_rtree_predict(avt_rtree* rt, const float* depth, int rows, int cols, float* dist_out);

/* Batch form for resident images (throughput use, bench.py): upload n images once, label them all with one launch
 * sequence on the tree's stream, download what is needed.  avt_rtree_sync waits for the stream. */
int avt_rtree_images_upload(avt_rtree* rt, int n_images, int rows, int cols, const float* depth);
int avt_rtree_predict_best_resident(avt_rtree* rt, int interval, int tl_x, int tl_y, int br_x, int br_y, int fill_in_gaps);
int avt_rtree_labels_download(avt_rtree* rt, int image, unsigned char* labels_out);
int avt_rtree_sync(avt_rtree* rt);

/* The labelling of demo.cpp:179-204 for a batch of streams: every image inside its own box, as predictBest(depth, ..., interval,
 * bgsub.topLeft, bgsub.botRight) gives it per image.  boxes: n_images x 4 host ints tl.x tl.y br.x br.y, inclusive, copied on
 * the tree's stream; br.x == -1 is the whole image; an empty box (tl > br in either axis, background subtraction's "no
 * foreground") leaves that image all 255 and is no error; a box shorter than `interval` rows labels nothing (the first row
 * touched is tl.y + interval).  A box outside the image or a bad interval fails before anything is queued. */
int avt_rtree_predict_best_resident_boxes(avt_rtree* rt, int interval, const int* boxes, int fill_in_gaps);
/* demo.cpp:179-204 without the host in between: labels every image of `bg`'s last avt_bgsub_run_resident, each inside the box
 * that run left on the device, reading the masked depth where it lies.  No copy of the depth, no host synchronisation: the
 * tree's stream waits for the run, and bg's next images_upload, run_resident and destroy wait for the labelling.  A box on the
 * device that does not lie inside the image (an empty mask, a capped run's unusable previous box) labels nothing.  Both handles
 * must be on one device; `bg` must have a run behind it.  Afterwards avt_rtree_labels_download[_all] serve these images; the
 * tree has no resident depth of its own until the next avt_rtree_images_upload. */
int avt_rtree_predict_best_from_bgsub(avt_rtree* rt, struct avt_bgsub* bg, int interval, int fill_in_gaps);
/* The labels of every image of the last labelling call (demo.cpp:179-204 for all streams): n_images x rows x cols bytes, one
 * copy and one wait. */
int avt_rtree_labels_download_all(avt_rtree* rt, unsigned char* labels_out);

/* void RTree::postProcess(image, com_pre, interval, num_threads, top_left, bot_right, dist_to_pre_weight) const
 * (RTree.cpp:3422-3449): largest-component selection per part ('contiguous' part maps) or small-piece removal
 * ('disjoint'), then up-scaling of the interval grid.  Host code, as in the reference (a sequential flood fill whose
 * scan order defines the result).  com_pre: 2 x num_parts column-major; com_pre_valid == 0 means "not sized yet"
 * (the resize branch of :3431-3435). */
int avt_rtree_post_process(const avt_rtree* rt, unsigned char* image, int rows, int cols, double* com_pre, int com_pre_valid, int interval,
                           int tl_x, int tl_y, int br_x, int br_y, double dist_to_pre_weight);

/* ---- RTree::postProcess for a batch of label images on the device (DESIGN.md par. 8) -----------------------------------
 * The rule is connected components per part on the interval grid: the grid is the pixels (tl.y + a interval, tl.x + b interval)
 * inside the box, two grid pixels are neighbours when they are `interval` apart in one axis, a component is a maximal
 * 4-connected set of equal labels < num_parts.  'Contiguous' part maps keep, per part, the component with the largest score
 * (size - weight x squared distance of its centre of mass to the slot's previous one, in double, if that is > 0; equal scores:
 * the component whose first raster pixel comes first); 'disjoint' ones drop components smaller than 0.05 % of the grid.  Then
 * the grid is up-scaled as the host code does it.
 * DELIBERATE DIFFERENCE: at interval 1 this is RTree::postProcess (RTree.cpp:3422-3449) and avt_rtree_post_process bit for bit,
 * labels and com_pre.  Above it, the reference's downward probe reads row r + 1 but records row r + interval (RTree.cpp:176),
 * which makes its result depend on the scan order; the device stage is the reference with that probe reading row r + interval.
 * A label that is neither 255 nor < num_parts fails the call (non-zero, with a message); that image and its memory are left as
 * they were, the other images of the batch are processed.  The host version's silent -128 of values 128..254 is not reproduced.
 * A box that is empty or (from the device) does not lie inside the image leaves the labels alone and sets every com_pre.x of
 * its slot to -1 ('contiguous'), what the host code makes of an all-255 image.
 * Image i of a batch uses memory slot i.  All images run in one launch sequence on the handle's stream; the call then waits for
 * the stream once to read the images' status words. */

/* n_images x rows x cols label bytes from the host become the images of "the last labelling call" (labels that another
 * classifier made); the handle has no resident depth of its own afterwards. */
int avt_rtree_labels_upload(avt_rtree* rt, int n_images, int rows, int cols, const unsigned char* labels);
/* RTree::postProcess (RTree.cpp:3422-3449; see DELIBERATE DIFFERENCE above) in place on the images of the last labelling call.
 * boxes: n x 4 host ints tl.x tl.y br.x br.y, inclusive, NULL = whole images; br.x == -1 is the whole image, an empty box
 * (tl > br) is no error; a box outside the image or a bad interval fails before anything is queued. */
int avt_rtree_post_process_resident(avt_rtree* rt, int interval, const int* boxes, double dist_to_pre_weight);
/* RTree::postProcess (RTree.cpp:3422-3449; see DELIBERATE DIFFERENCE above) on the labels of avt_rtree_predict_best_from_bgsub,
 * every image inside the box that bg's last run left on the device.  Ordered with bg exactly as that labelling is: the tree's
 * stream waits for the run, bg's next images_upload, run_resident and destroy wait for this stage. */
int avt_rtree_post_process_from_bgsub(avt_rtree* rt, struct avt_bgsub* bg, int interval, double dist_to_pre_weight);
/* com_pre of RTree::postProcess (RTree.cpp:3422-3449; the device stage's memory across frames, see DELIBERATE DIFFERENCE above)
 * for the slots [first, first + n): com is n x num_parts x 2 doubles (x, y per part, the layout of avt_rtree_post_process),
 * valid n bytes (0 = not sized yet; NULL on set = all sized).  A slot that was never set is not sized and reads as x = -1,
 * y = 0.  The memory is resident on the device and survives labelling calls and images_upload. */
int avt_rtree_com_pre_set(avt_rtree* rt, int first, int n, const double* com, const unsigned char* valid);
int avt_rtree_com_pre_get(avt_rtree* rt, int first, int n, double* com, unsigned char* valid);

#ifdef __cplusplus
}
#endif
#endif
