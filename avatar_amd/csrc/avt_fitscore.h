// avt_fitscore.h (private) — the handle of include/avt_fitscore.h and the launch of its one kernel
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/avt_fitscore.h"
#include "avt_host.h"

struct avt_fitscore {
    int device = 0, num_parts = 0, max_images = 0;
    hipStream_t stream = nullptr;
    // sized at creation: the call's tables, bad-label flag, boxes (4 ints per image) and image indices
    DevBuf<unsigned long long> d_table;       // max_images x (num_parts + 1) x AVT_FITSCORE_COLS
    DevBuf<int> d_bad, d_boxes, d_index;
    // staging of host images (avt_fitscore_images, the observed side of avt_fitscore_rendered): grown to the largest batch seen
    DevBuf<float> d_model, d_obs;
    DevBuf<unsigned char> d_mask;
    // the last call's result; n_result == 0: no score
    std::vector<long long> table;
    int n_result = 0;
};

// What one launch sequence scores: n_images images starting at the pointers given.  Image i's model side is model / mask + i *
// rows * cols and its table is table + i * cells; its observed side is image j of `obs` with the box at boxes + j * box_stride
// (boxes == nullptr: the whole image), j = obs_index ? obs_index[i] : i.  All pointers are device memory.
struct FitScoreJob {
    const float* model;
    const unsigned char* mask;
    const float* obs;
    const int* boxes;
    int box_stride;
    const int* obs_index;
    int n_images, rows, cols, stride;
    float tol;
};

// adds the job's counts to d_table and sets *d_bad when a selected mask byte is >= num_parts and not 255; one lane per pixel of the
// stride grid, blockIdx.z the image, in chunks of 65535 images
int avt_fitscore_launch(avt_fitscore* fs, const FitScoreJob& job, unsigned long long* d_table, int* d_bad);
