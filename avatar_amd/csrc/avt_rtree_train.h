// avt_rtree_train.h (private) — the trainer's device records and kernel launches (include/avt_rtree_train.h is the ABI)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/avt_rtree_train.h"
#include "avt_rtree.h"

// one image in the trainer's pixel store: the crop [x0, x0 + w) x [y0, y0 + h) of its non-zero depth, row stride w
struct RtImg {
    long long off;
    int x0, y0, w, h;
    int pad[2];
};
// the samples, structure of arrays: image index, x | y << 16, the pixel's own depth, the label
struct RtSamples {
    int* img;
    int* xy;
    float* d;
    unsigned char* lab;
};
// one open node of a level: its samples [start, end) and its path key (root 1, children 2k, 2k + 1)
struct RtNode {
    int start, end;
    unsigned long long key;
};
// the best feature of one chunk of features of one node (f < 0: none has a valid threshold)
struct RtChunk {
    double gain;
    float thresh;
    int f;
};
// a searched node's choice: u.x u.y v.x v.y thresh, the feature index, its gain, and after the partition the left count
struct RtRes {
    float feat[5];
    int f;
    int nleft;
    int pad;
    double gain;
};
struct RtTrainArgs {
    uint64_t seed;
    int P, T, F;
    float maxp;
};

int rt_launch_img_scan(hipStream_t s, const float* depth, const unsigned char* mask, int n, int rows, int cols, int* out7);
int rt_launch_crop(hipStream_t s, const float* depth, int n, int rows, int cols, const RtImg* imgs, float* store);
int rt_launch_select(hipStream_t s, const float* depth, const unsigned char* mask, int n, int rows, int cols, int k, uint64_t seed, int img_base,
                     const long long* out_off, int* scratch, RtSamples out);
int rt_launch_count(hipStream_t s, const RtNode* nodes, int m, const unsigned char* lab, int P, int* counts);
int rt_launch_search(hipStream_t s, bool large, const int* list, int nlist, int nchunks, int fchunk, const RtNode* nodes, const int* counts, RtSamples in,
                     const RtImg* imgs, const float* store, RtTrainArgs a, RtChunk* out, int* tap_hist = nullptr, float* tap_minmax = nullptr);
int rt_launch_choose(hipStream_t s, const int* list, int nlist, int nchunks, const RtNode* nodes, const RtChunk* chunks, RtTrainArgs a, RtRes* res);
int rt_launch_partition(hipStream_t s, const int* list, int nlist, const RtNode* nodes, RtRes* res, RtSamples in, RtSamples out, const RtImg* imgs,
                        const float* store);
int rt_launch_transfer(hipStream_t s, const RtNodeDev* nodes, const float* depth, const unsigned char* mask, int n, int rows, int cols, int P,
                       unsigned long long* counts, int* bad);
size_t rt_search_lds_bytes(int P, int T, bool large);
int rt_search_set_attributes(size_t bytes);

// the last run's depth and part-mask images of a renderer, visible to `s` after the renderer's queued work (avt_render.hip)
int avt_renderer_images_for(avt_renderer* r, hipStream_t s, const float** depth, const unsigned char** mask, int* n, int* width, int* height);
