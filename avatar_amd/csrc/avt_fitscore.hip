// avt_fitscore.hip — the fit score on gfx950 (include/avt_fitscore.h, THE RULE): the overlay of live-demo.cpp:428-445 as a
// (P + 1) x 7 table of 64-bit integers per image, one kernel for every source of the images.
//
// blockIdx.z is the image.  A workgroup covers 64 x 16 pixels of the stride grid: a wave takes one grid row at a time, a lane
// FS_ROWS = 4 pixels of one grid column, four rows apart.  At stride 1 a wave reads 256 contiguous bytes of each depth image and 64
// of the mask per row, 9 bytes per selected pixel (the observed depth is not read outside the box).  The kernel is memory-bound,
// and with one pixel per lane it was bound by latency, not by bytes: a wave issued one round of loads and left.  So a lane issues
// the loads of its four pixels before it looks at any of them.  Most pixels of a real frame are in neither image: a workgroup with
// nothing to count leaves after one __syncthreads_or, before it touches LDS, and in one that stays a wave with nothing to count
// only keeps the barriers.  Counts meet in an LDS table of the workgroup: 32-bit cells for the five classes (a workgroup adds at
// most 1024 to one) and 64-bit cells for the two micrometre sums, which pass 2^32 with five clamped pixels.  At P = 254 that is
// 9180 bytes, so unlike k_rforest_score's (P + 1)^2 histogram it needs no packing.  Each workgroup flushes its
// non-zero cells once with 64-bit global atomics: integer adds, so the result does not depend on any order.  No float is
// accumulated anywhere.  Built with -ffp-contract=off (the rule has one subtraction, one multiplication and one rounding).
#include <algorithm>

#include "avt_fitscore.h"

#define FS_LANES 256
#define FS_TILE_W 64
#ifndef FS_ROWS
#define FS_ROWS 4         // grid rows per lane: their loads are issued together (1 and 8 were timed beside it)
#endif
#define FS_TILE_H (FS_LANES / FS_TILE_W * FS_ROWS)
#define FS_COUNTS 5       // AGREE .. DATA_ONLY; the two sums follow

__global__ __launch_bounds__(FS_LANES) void k_fit_score(FitScoreJob j, int img0, int gcols, int grows, int P, unsigned long long* __restrict__ table,
                                                        int* __restrict__ bad) {
    extern __shared__ unsigned long long s_um[];                  // (P + 1) x 2 sums, then (P + 1) x FS_COUNTS counts
    unsigned int* s_cnt = (unsigned int*)(s_um + 2 * (P + 1));
    const int img = img0 + blockIdx.z;
    const int gc = blockIdx.x * FS_TILE_W + (threadIdx.x & (FS_TILE_W - 1)), gr0 = blockIdx.y * FS_TILE_H + threadIdx.x / FS_TILE_W;
    const size_t npix = (size_t)j.rows * j.cols;
    const int oi = j.obs_index ? j.obs_index[img] : img;          // checked by the host
    int tlx = 0, tly = 0, brx = -1, bry = -1;
    if (j.boxes) {
        const int* box = j.boxes + (size_t)oi * j.box_stride;
        tlx = box[0]; tly = box[1]; brx = box[2]; bry = box[3];
    }
    if (brx == -1) { tlx = 0; tly = 0; brx = j.cols - 1; bry = j.rows - 1; }
    const bool box_ok = 0 <= tlx && tlx <= brx && brx < j.cols && 0 <= tly && tly <= bry && bry < j.rows;    // a box outside the image: no data
    const int c = gc * j.stride;
    const bool col_in = box_ok && tlx <= c && c <= brx;
    // the lane's FS_ROWS pixels: grid rows gr0, gr0 + 4, ...; all loads first, so that they are in flight together
    float R[FS_ROWS], D[FS_ROWS];
    int M[FS_ROWS];
#pragma unroll
    for (int k = 0; k < FS_ROWS; ++k) {
        const int gr = gr0 + k * (FS_LANES / FS_TILE_W);
        R[k] = 0.f; D[k] = 0.f; M[k] = 255;
        if (gc < gcols && gr < grows) {
            const int r = gr * j.stride;                          // r <= rows - 1, c <= cols - 1
            const size_t o = (size_t)r * j.cols + c;
            R[k] = j.model[img * npix + o];
            M[k] = j.mask[img * npix + o];
            if (col_in && tly <= r && r <= bry) D[k] = j.obs[oi * npix + o];
        }
    }
    int row[FS_ROWS], cls[FS_ROWS];
    long long um[FS_ROWS];
    bool any = false;
#pragma unroll
    for (int k = 0; k < FS_ROWS; ++k) {
        if (M[k] >= P && M[k] != 255) atomicOr(bad, 1);           // refused by the host: the call holds no result
        const bool m = R[k] > 0.f, d = D[k] > 0.f;                // NaN is neither
        row[k] = m && M[k] < P ? M[k] : P;
        cls[k] = -1;
        um[k] = 0;
        if (m && d) {
            const double tol = (double)j.tol, delta = (double)R[k] - (double)D[k], a = fabs(delta);
            cls[k] = a <= tol ? AVT_FITSCORE_AGREE : delta < -tol ? AVT_FITSCORE_IN_FRONT : AVT_FITSCORE_BEHIND;
            um[k] = (long long)rint(fmin(a, 1000.0) * 1e6);
        } else if (m) {
            cls[k] = AVT_FITSCORE_MODEL_ONLY;
        } else if (d) {
            cls[k] = AVT_FITSCORE_DATA_ONLY;
        }
        any |= cls[k] >= 0;
    }
    if (!__syncthreads_or(any)) return;
    for (int i = threadIdx.x; i < 2 * (P + 1); i += FS_LANES) s_um[i] = 0ull;
    for (int i = threadIdx.x; i < FS_COUNTS * (P + 1); i += FS_LANES) s_cnt[i] = 0u;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FS_ROWS; ++k) {
        if (cls[k] < 0) continue;
        atomicAdd(&s_cnt[row[k] * FS_COUNTS + cls[k]], 1u);
        if (um[k]) {
            atomicAdd(&s_um[2 * row[k]], (unsigned long long)um[k]);
            if (cls[k] == AVT_FITSCORE_AGREE) atomicAdd(&s_um[2 * row[k] + 1], (unsigned long long)um[k]);
        }
    }
    __syncthreads();
    unsigned long long* out = table + (size_t)img * (P + 1) * AVT_FITSCORE_COLS;
    for (int i = threadIdx.x; i < AVT_FITSCORE_COLS * (P + 1); i += FS_LANES) {
        const int p = i / AVT_FITSCORE_COLS, k = i % AVT_FITSCORE_COLS;
        const unsigned long long v = k < FS_COUNTS ? (unsigned long long)s_cnt[p * FS_COUNTS + k] : s_um[2 * p + k - FS_COUNTS];
        if (v) atomicAdd(&out[i], v);
    }
}

int avt_fitscore_launch(avt_fitscore* fs, const FitScoreJob& job, unsigned long long* d_table, int* d_bad) {
    const int P = fs->num_parts, grows = (job.rows - 1) / job.stride + 1, gcols = (job.cols - 1) / job.stride + 1;
    const size_t lds = (size_t)(P + 1) * (2 * sizeof(unsigned long long) + FS_COUNTS * sizeof(unsigned int));
    for (int i0 = 0; i0 < job.n_images; i0 += 65535) {            // blockIdx.z is the image
        dim3 grid((gcols + FS_TILE_W - 1) / FS_TILE_W, (grows + FS_TILE_H - 1) / FS_TILE_H, std::min(65535, job.n_images - i0));
        hipLaunchKernelGGL(k_fit_score, grid, dim3(FS_LANES), lds, fs->stream, job, i0, gcols, grows, P, d_table, d_bad);
        if (hipGetLastError() != hipSuccess) return 1;
    }
    return 0;
}
