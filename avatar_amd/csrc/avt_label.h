// avt_label.h (private) — the labelling handle: what a tree (avt_rtree) and a forest (avt_rforest) are behind their classifier.
// Resident depth images and label images on one stream, one box per image, the hand-over from the background subtractor, the
// device post-processing with its per-slot memory, the downloads.  Both handles derive from AvtLabelHandle; the image side is
// written once over it (avt_label.cpp).  What differs between the kinds is passed in: the words of the error texts, the kernel
// launch, and the few checks only one of them makes.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "avt_bgsub_internal.h"
#include "avt_host.h"
#include "avt_post.h"

struct AvtLabelHandle {
    int device = 0;
    int num_parts = 0;
    std::vector<int> part_map;
    int part_map_type = 0;
    hipStream_t stream = nullptr;
    DevBuf<float> d_depth;           // the resident images and their labels: one capacity, in pixels
    DevBuf<unsigned char> d_labels;
    int n_images = 0, rows = 0, cols = 0;     // n_images: resident depth images of the handle's own (0 after a hand-over from bgsub)
    int n_labels = 0;                         // images d_labels holds (rows x cols each): what labels_download serves
    DevBuf<int> d_boxes;                      // n x 4 regions of interest of predict_best_resident_boxes
    AvtPostState post;                        // post_process_resident / _from_bgsub: scratch and the per-slot com_pre memory
};

// the words of a kind's error texts: "<prefix>: ...", "<abi>_<function>: ...", "null <noun>"
struct AvtLabelNames { const char *prefix, *abi, *noun; };

// one box per image from device memory (stride in ints), depth from any device buffer, labels into h->d_labels, on h->stream
typedef int (*AvtLabelLaunchBoxes)(AvtLabelHandle* h, const float* d_depth, const int* d_boxes, int box_stride, int n_images, int rows, int cols,
                                   int interval, int fill);
// h's one resident image into num_parts planes at d_out
typedef int (*AvtLabelLaunchDist)(AvtLabelHandle* h, int rows, int cols, float* d_out);

int avt_label_roi_ok(const AvtLabelNames& k, int rows, int cols, int interval, int& tlx, int& tly, int& brx, int& bry);
// max_images: 0 = any number
int avt_label_images_upload(AvtLabelHandle* h, const AvtLabelNames& k, int max_images, int n_images, int rows, int cols, const float* depth);
int avt_label_labels_download(AvtLabelHandle* h, const AvtLabelNames& k, int image, unsigned char* out);
int avt_label_labels_download_all(AvtLabelHandle* h, const AvtLabelNames& k, unsigned char* out);
int avt_label_predict_resident_boxes(AvtLabelHandle* h, const AvtLabelNames& k, int interval, const int* boxes, int fill, AvtLabelLaunchBoxes launch);
int avt_label_predict_from_bgsub(AvtLabelHandle* h, const AvtLabelNames& k, int max_images, avt_bgsub* bg, int interval, int fill, AvtLabelLaunchBoxes launch);
// side_limit: refuse 32768 rows or columns and more before the upload
int avt_label_predict_dist(AvtLabelHandle* h, const AvtLabelNames& k, bool side_limit, const float* depth, int rows, int cols, float* dist_out,
                           AvtLabelLaunchDist launch);
int avt_label_sync(AvtLabelHandle* h, const AvtLabelNames& k, bool refuse_host_only);
void avt_label_teardown(AvtLabelHandle* h);      // drains and destroys the stream; the buffers go with the handle
int avt_label_com_pre_set(AvtLabelHandle* h, const AvtLabelNames& k, int first, int n, const double* com, const unsigned char* valid);
int avt_label_com_pre_get(AvtLabelHandle* h, const AvtLabelNames& k, int first, int n, double* com, unsigned char* valid);

// the device post-processing (avt_post.hip) behind a handle; `who` is the entry point's name
int avt_post_resident(AvtLabelHandle* h, const char* who, int interval, const int* boxes, double dist_to_pre_weight);
int avt_post_from_bgsub(AvtLabelHandle* h, avt_bgsub* bg, const char* who, int interval, double dist_to_pre_weight);
// label images that did not come from the handle's own labelling (another classifier, a file, a test): they become the images
// of "the last labelling call"; the handle has no resident depth of its own afterwards
int avt_post_labels_upload(AvtLabelHandle* h, const char* who, int n, int rows, int cols, const unsigned char* labels);
