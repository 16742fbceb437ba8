// avt_rtree.h (private) — host-side tree and the device image of it
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/avt_rtree.h"
#include "avt_host.h"
#include "avt_label.h"

// one tree node as the kernel reads it: two 16-byte loads
struct RtNodeDev {
    float ux, uy, vx, vy;
    float thresh;
    int lnode;      // internal: left child; leaf: best-match label
    int rnode;      // internal: right child; leaf: leaf id (row of the distribution table)
    int leaf;       // 1: leaf
};

struct avt_rtree : AvtLabelHandle {
    std::vector<float> feature;      // n x 5
    std::vector<int> links;          // n x 3
    std::vector<float> leaf_data;    // nl x num_parts
    std::vector<unsigned char> leaf_best;
    // device
    DevBuf<RtNodeDev> d_nodes;
    DevBuf<float> d_leaf;            // [n_leafs][num_parts] distributions
    DevBuf<unsigned long long> d_tcount;      // trainTransfer's (leaf, part) counts since the last avt_rtree_transfer_finish
};

int avt_rtree_launch_predict_dist(avt_rtree* rt, int rows, int cols, float* d_out);
int avt_rtree_launch_predict(avt_rtree* rt, int n_images, int rows, int cols, int interval, int tlx, int tly, int brx, int bry, int fill);
// one box per image from device memory (stride in ints), depth from any device buffer; sizes the grid from the image
int avt_rtree_launch_predict_boxes(avt_rtree* rt, const float* d_depth, const int* d_boxes, int box_stride, int n_images, int rows, int cols,
                                   int interval, int fill);
// after leaf_data changed (trainTransfer): re-derives leafBestMatch and uploads nodes and distributions again (avt_rtree.cpp)
int avt_rtree_refresh_leaves(avt_rtree* rt);
