// avt_rforest.hip — a forest of T trees per pixel on gfx950: the per-model RTree::predict + sum + arg-max of
// rtree-run-dataset.cpp:98-159, in the two walking forms of include/avt_rforest.h (RTree::predict(depth), RTree.cpp:3156-3182;
// RTree::predictBest(depth, ...), :3184-3262, with upscaleGrid, :70-99, folded in as in avt_rtree.hip).
//
// One lane per pixel, as in k_rtree_predict.  A pixel's T walks are T independent chains of dependent loads (node -> two
// depth probes -> next node), so they are advanced in lock step: each trip of the walk moves every unfinished tree one level,
// four trees at a time with their node loads issued together.  The walk state of tree t (the current node, then ~leaf row
// once it arrived) lives in LDS as s_state[t][lane]: a lane touches its own column only, so no barrier is needed, and nothing
// is indexed at run time in private memory (the private segment is 0 bytes).  After the walk the parts are streamed: for
// each part the T table entries are added in tree order, starting from tree 0's value, and the running best is carried
// (first p with sum > best, best starting at 0.f): T x num_parts cached loads, no per-part accumulators, and for the label
// form no plane is ever written.  Built with -ffp-contract=off; the probe arithmetic is rt_score_by_feature, unchanged.
#include <algorithm>

#include "avt_rforest.h"
#include "avt_rtree_score.h"

#define RF_LANES 256
#define RF_GROUP 4      // trees whose node loads are issued together

// All T walks of the pixel (c, r) with depth `sample`, probes bounded by [lox, hix] x [loy, hiy].  On return col[t * RF_LANES]
// holds tree t's row of the leaf table, t < T.
__device__ __forceinline__ void rf_walk(const RtNodeDev* __restrict__ nodes, const int* __restrict__ roots, int T, int* col,
                                        const float* __restrict__ d, int cols, int lox, int loy, int hix, int hiy, int c, int r, float sample) {
    const int Tpad = (T + RF_GROUP - 1) / RF_GROUP * RF_GROUP;        // <= AVT_RFOREST_MAX_TREES, a multiple of RF_GROUP
    for (int t = 0; t < Tpad; ++t) col[t * RF_LANES] = t < T ? roots[t] : -1;      // a slot past T counts as arrived
    const float4* nv = (const float4*)nodes;
    bool walking = true;
    while (walking) {
        walking = false;
        for (int g = 0; g < Tpad; g += RF_GROUP) {
            int n[RF_GROUP];
            float4 a[RF_GROUP], b[RF_GROUP];
#pragma unroll
            for (int k = 0; k < RF_GROUP; ++k) n[k] = col[(g + k) * RF_LANES];
#pragma unroll
            for (int k = 0; k < RF_GROUP; ++k) {          // an arrived tree re-reads node 0: in bounds, and dropped below
                const int i = n[k] >= 0 ? n[k] : 0;
                a[k] = nv[2 * i];
                b[k] = nv[2 * i + 1];
            }
#pragma unroll
            for (int k = 0; k < RF_GROUP; ++k) {
                if (n[k] < 0) continue;
                if (__float_as_int(b[k].w)) {
                    n[k] = ~__float_as_int(b[k].z);
                } else {
                    n[k] = (rt_score_by_feature(d, cols, 0, 0, lox, loy, hix, hiy, c, r, sample, a[k]) < b[k].x) ? __float_as_int(b[k].y) : __float_as_int(b[k].z);
                    walking = true;
                }
                col[(g + k) * RF_LANES] = n[k];
            }
        }
    }
    for (int t = 0; t < T; ++t) col[t * RF_LANES] = ~col[t * RF_LANES];
}

// sum[p] = ((d_0[p] + d_1[p]) + d_2[p]) + ... in float32, tree order
__device__ __forceinline__ float rf_sum(const float* __restrict__ leaf, const int* col, int T, int num_parts, int p) {
    float s = leaf[(size_t)col[0] * num_parts + p];
#pragma unroll 4
    for (int t = 1; t < T; ++t) s = s + leaf[(size_t)col[t * RF_LANES] * num_parts + p];
    return s;
}

// Label form.  boxes == nullptr: the one region (tlx, tly)-(brx, bry) for every image, gcols x grows grid pixels.  Otherwise
// image blockIdx.z's region is boxes[img * box_stride + 0..3]; the launch covers the interval grid of the whole image, a lane
// outside its image's grid exits, and a box that does not lie inside the image labels nothing (as k_rtree_predict_boxes).
__global__ __launch_bounds__(RF_LANES) void k_rforest_label(const RtNodeDev* __restrict__ nodes, const int* __restrict__ roots,
                                                            const float* __restrict__ leaf, int T, int num_parts, const float* __restrict__ depth,
                                                            unsigned char* __restrict__ labels, const int* __restrict__ boxes, int box_stride, int rows,
                                                            int cols, int interval, int tlx, int tly, int brx, int bry, int gcols, int grows, int fill) {
    __shared__ int s_state[AVT_RFOREST_MAX_TREES * RF_LANES];
    const int img = blockIdx.z;
    if (boxes) {
        const int* box = boxes + (size_t)img * box_stride;
        tlx = box[0]; tly = box[1]; brx = box[2]; bry = box[3];
        if (!(0 <= tlx && tlx <= brx && brx < cols && 0 <= tly && tly <= bry && bry < rows)) return;
        grows = (bry - tly) / interval; gcols = (brx - tlx) / interval + 1;
    }
    const int gc = blockIdx.x * 16 + (threadIdx.x & 15), gr = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (gc >= gcols || gr >= grows) return;
    // r = (row += interval): the first row of the region is skipped; r <= bry < rows, c <= brx < cols
    const int r = tly + interval * (gr + 1), c = tlx + interval * gc;
    const float* d = depth + (size_t)img * rows * cols;
    unsigned char* out = labels + (size_t)img * rows * cols;
    const float sample = d[(size_t)r * cols + c];
    unsigned char lab = 255;
    if (sample != 0.f) {
        int* col = s_state + threadIdx.x;
        rf_walk(nodes, roots, T, col, d, cols, tlx, tly, brx, bry, c, r, sample);
        float best = 0.f;
        for (int p = 0; p < num_parts; ++p) {
            const float s = rf_sum(leaf, col, T, num_parts, p);
            if (s > best) { best = s; lab = (unsigned char)p; }      // a NaN never wins, a tie stays with the lower index
        }
    }
    if (fill && interval > 1) {       // upscaleGrid: the cell [r, r+interval) x [c, c+interval), rows <= bot_right.y, width clamped
        for (int rr = r; rr < r + interval && rr <= bry; ++rr)
            for (int cc = c; cc < c + interval && cc < cols; ++cc) out[(size_t)rr * cols + cc] = lab;
    } else if (lab != 255) {
        out[(size_t)r * cols + c] = lab;
    }
}

// Distribution form: every pixel with depth > 0, probes bounded by the image, num_parts planes of sums out (0 elsewhere)
__global__ __launch_bounds__(RF_LANES) void k_rforest_dist(const RtNodeDev* __restrict__ nodes, const int* __restrict__ roots,
                                                           const float* __restrict__ leaf, int T, int num_parts, const float* __restrict__ depth,
                                                           float* __restrict__ out, int rows, int cols) {
    __shared__ int s_state[AVT_RFOREST_MAX_TREES * RF_LANES];
    const int c = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (c >= cols || r >= rows) return;
    const float sample = depth[(size_t)r * cols + c];
    const size_t plane = (size_t)rows * cols, o = (size_t)r * cols + c;
    if (!(sample > 0.f)) {
        for (int p = 0; p < num_parts; ++p) out[(size_t)p * plane + o] = 0.f;
        return;
    }
    int* col = s_state + threadIdx.x;
    rf_walk(nodes, roots, T, col, depth, cols, 0, 0, cols - 1, rows - 1, c, r, sample);
    for (int p = 0; p < num_parts; ++p) out[(size_t)p * plane + o] = rf_sum(leaf, col, T, num_parts, p);
}

// Scoring (include/avt_rforest.h, "THE SCORE"): walk, sum, arg-max, compare with the part mask and count, fused.  One lane per
// pixel of the stride grid, 16 x 16 of them per workgroup, blockIdx.z the image; the walk is the distribution form's (depth >
// 0, probes bounded by this image: `d` is the image's own base, so a probe never reads a neighbour of the batch).  The (truth,
// predicted) pairs are counted in a workgroup histogram in LDS and its non-zero cells are flushed to the call's 64-bit matrix
// with integer atomics, so the result does not depend on any order.  A workgroup counts at most 256 pairs, so two 16-bit cells
// share a word (the add is 1 or 1 << 16 and never carries): (P + 1)^2 cells take 32 KiB at P = 127 next to s_state's 16 KiB,
// below the 64 KiB every launch is granted, and one path serves every P.  A tile with no walked and no labelled pixel leaves
// before it touches the histogram (an avatar render is mostly background).  No label image, no plane is written.
__global__ __launch_bounds__(RF_LANES) void k_rforest_score(const RtNodeDev* __restrict__ nodes, const int* __restrict__ roots,
                                                            const float* __restrict__ leaf, int T, int P, const float* __restrict__ depth,
                                                            const unsigned char* __restrict__ mask, int rows, int cols, int stride, int gcols,
                                                            int grows, unsigned long long* __restrict__ conf, int* __restrict__ bad) {
    __shared__ int s_state[AVT_RFOREST_MAX_TREES * RF_LANES];
    extern __shared__ unsigned int s_hist[];          // ((P + 1)^2 + 1) / 2 words
    const int gc = blockIdx.x * 16 + (threadIdx.x & 15), gr = blockIdx.y * 16 + (threadIdx.x >> 4);
    const size_t base = (size_t)blockIdx.z * rows * cols;
    const float* d = depth + base;
    int r = 0, c = 0, t = P;
    float sample = 0.f;
    if (gc < gcols && gr < grows) {                   // r <= rows - 1, c <= cols - 1
        r = gr * stride; c = gc * stride;
        sample = d[(size_t)r * cols + c];
        const int m = mask[base + (size_t)r * cols + c];
        if (m < P) t = m;
        else if (m != 255) atomicOr(bad, 1);          // refused by the host: the call's counts are dropped
    }
    const bool walked = sample > 0.f;                 // zero, negative and NaN depths are not walked
    if (!__syncthreads_or(walked || t != P)) return;
    const int words = ((P + 1) * (P + 1) + 1) / 2;
    for (int i = threadIdx.x; i < words; i += RF_LANES) s_hist[i] = 0u;
    __syncthreads();
    int q = P;
    if (walked) {
        int* col = s_state + threadIdx.x;
        rf_walk(nodes, roots, T, col, d, cols, 0, 0, cols - 1, rows - 1, c, r, sample);
        float best = 0.f;
        for (int p = 0; p < P; ++p) {
            const float s = rf_sum(leaf, col, T, P, p);
            if (s > best) { best = s; q = p; }        // a NaN never wins, a tie stays with the lower index
        }
    }
    const int cell = (t != P || q != P) ? t * (P + 1) + q : -1;
#ifdef AVT_RF_SCORE_MERGE
    // timing experiment (libavatar_hip_rf_score_merge.so, tools/rforest_score_measure.py): the lanes of a wave that share a cell
    // add once, through the lowest of them; same counts
    for (unsigned long long todo = __ballot(cell >= 0); todo;) {
        const int lead = __shfl(cell, __ffsll((long long)todo) - 1);
        const unsigned long long same = __ballot(cell == lead);
        if ((threadIdx.x & 63) == __ffsll((long long)todo) - 1) atomicAdd(&s_hist[lead >> 1], (unsigned int)__popcll(same) << (16 * (lead & 1)));
        todo &= ~same;
    }
#else
    if (cell >= 0) atomicAdd(&s_hist[cell >> 1], 1u << (16 * (cell & 1)));
#endif
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += RF_LANES) {
        const unsigned int w = s_hist[i];
        if (w & 0xffffu) atomicAdd(&conf[2 * i], (unsigned long long)(w & 0xffffu));
        if (w >> 16) atomicAdd(&conf[2 * i + 1], (unsigned long long)(w >> 16));       // the cell past an odd count stays 0
    }
}

int avt_rforest_launch_predict_dist(avt_rforest* rf, int rows, int cols, float* d_out) {
    dim3 grid((cols + 15) / 16, (rows + 15) / 16);
    hipLaunchKernelGGL(k_rforest_dist, grid, dim3(RF_LANES), 0, rf->stream, rf->d_nodes, rf->d_roots, rf->d_leaf, rf->n_trees, rf->num_parts, rf->d_depth,
                       d_out, rows, cols);
    return hipGetLastError() != hipSuccess;
}

int avt_rforest_launch_predict(avt_rforest* rf, const float* d_depth, const int* d_boxes, int box_stride, int n_images, int rows, int cols, int interval,
                               int tlx, int tly, int brx, int bry, int fill) {
    const size_t npix = (size_t)n_images * rows * cols;
    if (hipMemsetAsync(rf->d_labels, 255, npix, rf->stream) != hipSuccess) return 1;
    // one box: rows tly + interval, ... <= bry and cols tlx, tlx + interval, ... <= brx; boxes on the device: the whole image's grid
    const int grows = d_boxes ? (rows - 1) / interval : (bry - tly) / interval;
    const int gcols = d_boxes ? (cols - 1) / interval + 1 : (brx - tlx) / interval + 1;
    if (grows <= 0 || gcols <= 0) return 0;
    dim3 grid((gcols + 15) / 16, (grows + 15) / 16, n_images);
    hipLaunchKernelGGL(k_rforest_label, grid, dim3(RF_LANES), 0, rf->stream, rf->d_nodes, rf->d_roots, rf->d_leaf, rf->n_trees, rf->num_parts, d_depth,
                       rf->d_labels, d_boxes, box_stride, rows, cols, interval, tlx, tly, brx, bry, gcols, grows, fill);
    return hipGetLastError() != hipSuccess;
}

int avt_rforest_launch_score(avt_rforest* rf, const float* d_depth, const unsigned char* d_mask, int n_images, int rows, int cols, int stride,
                             unsigned long long* d_conf, int* d_bad) {
    const int P = rf->num_parts, grows = (rows - 1) / stride + 1, gcols = (cols - 1) / stride + 1;
    const size_t lds = 4 * (size_t)(((P + 1) * (P + 1) + 1) / 2), npix = (size_t)rows * cols;
    for (int i0 = 0; i0 < n_images; i0 += 65535) {    // blockIdx.z is the image
        dim3 grid((gcols + 15) / 16, (grows + 15) / 16, std::min(65535, n_images - i0));
        hipLaunchKernelGGL(k_rforest_score, grid, dim3(RF_LANES), lds, rf->stream, rf->d_nodes, rf->d_roots, rf->d_leaf, rf->n_trees, P,
                           d_depth + i0 * npix, d_mask + i0 * npix, rows, cols, stride, gcols, grows, d_conf, d_bad);
        if (hipGetLastError() != hipSuccess) return 1;
    }
    return 0;
}
