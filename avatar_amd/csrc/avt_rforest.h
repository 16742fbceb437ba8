// avt_rforest.h (private) — host-side forest and the device image of it: every tree's nodes in one array (child links rebased,
// a leaf's rnode is its row in the one leaf table), per-tree root offsets, one table of distributions
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/avt_rforest.h"
#include "avt_host.h"
#include "avt_rtree.h"

struct avt_rforest {
    int device = 0;
    int n_trees = 0, num_parts = 0;
    std::vector<int> part_map;
    int part_map_type = 0;
    std::vector<RtNodeDev> nodes;    // all trees, tree t's node i at roots[t] + i
    std::vector<int> roots;          // n_trees offsets into `nodes`
    std::vector<float> leaf;         // total leaves x num_parts, tree order
    // device
    hipStream_t stream = nullptr;
    DevBuf<RtNodeDev> d_nodes;
    DevBuf<int> d_roots;
    DevBuf<float> d_leaf;
    DevBuf<float> d_depth;           // the resident images and their labels: one capacity, in pixels
    DevBuf<unsigned char> d_labels;
    int n_images = 0, rows = 0, cols = 0;     // n_images: resident depth images of the forest's own (0 after a hand-over from bgsub)
    int n_labels = 0;                         // images d_labels holds (rows x cols each)
    DevBuf<int> d_boxes;
    // the score (avt_rforest_score_*): the totals live on the host, a call counts into a scratch matrix on the device and is
    // added only when its bad-label flag is clear
    std::vector<long long> score_conf;        // (num_parts + 1)^2, empty until the first good call
    long long score_images = 0, score_pixels = 0;
    DevBuf<unsigned long long> d_score;
    DevBuf<int> d_score_bad;
    AvtPostState post;                        // avt_rforest_post_process_resident / _from_bgsub: scratch and the per-slot com_pre memory
};

// distribution form: d_depth is the forest's one resident image, d_out num_parts planes
int avt_rforest_launch_predict_dist(avt_rforest* rf, int rows, int cols, float* d_out);
// label form, one box for all images (d_boxes == nullptr) or one box per image from device memory (stride in ints); clears the
// labels to 255 first; grid sized as avt_rtree_launch_predict / avt_rtree_launch_predict_boxes size theirs
int avt_rforest_launch_predict(avt_rforest* rf, const float* d_depth, const int* d_boxes, int box_stride, int n_images, int rows, int cols, int interval,
                               int tlx, int tly, int brx, int bry, int fill);
// the score: (truth, predicted) counts of n_images depth / mask images on the device added to d_conf ((num_parts + 1)^2), d_bad
// set when a mask byte is >= num_parts and not 255; one lane per pixel of the stride grid
int avt_rforest_launch_score(avt_rforest* rf, const float* d_depth, const unsigned char* d_mask, int n_images, int rows, int cols, int stride,
                             unsigned long long* d_conf, int* d_bad);
