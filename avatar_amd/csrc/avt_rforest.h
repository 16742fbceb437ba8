// avt_rforest.h (private) — host-side forest and the device image of it: every tree's nodes in one array (child links rebased,
// a leaf's rnode is its row in the one leaf table), per-tree root offsets, one table of distributions
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/avt_rforest.h"
#include "avt_host.h"
#include "avt_rtree.h"

struct avt_rforest : AvtLabelHandle {
    int n_trees = 0;
    std::vector<RtNodeDev> nodes;    // all trees, tree t's node i at roots[t] + i
    std::vector<int> roots;          // n_trees offsets into `nodes`
    std::vector<float> leaf;         // total leaves x num_parts, tree order
    // device
    DevBuf<RtNodeDev> d_nodes;
    DevBuf<int> d_roots;
    DevBuf<float> d_leaf;
    // the score (avt_rforest_score_*): the totals live on the host, a call counts into a scratch matrix on the device and is
    // added only when its bad-label flag is clear
    std::vector<long long> score_conf;        // (num_parts + 1)^2, empty until the first good call
    long long score_images = 0, score_pixels = 0;
    DevBuf<unsigned long long> d_score;
    DevBuf<int> d_score_bad;
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
