// avt_bgsub.hip — background subtraction on gfx950 (include/avt_bgsub.h): BGSubtractor::run (BGSubtractor.cpp:10-163)
// as a near-background test plus a union-find connected-component labelling whose roots are the smallest raster index
// of every component, so the partition, the roots and hence the ids are the reference's whatever the scheduling.
//
// Depth images in (avt_bgsub_depth_upload and its kin): k_bgs_backproject expands n x N uploaded depth floats into the
// resident XYZ images with CameraIntrin::depthToXYZ's float expression (Calibration.cpp:82-95); the rest runs unchanged.
//
// Launch sequence per run (every kernel batched over the images on a grid dimension):
//   k_bgs_local    32x32 tile per 256-thread workgroup: the 3x3 near-background test against an LDS copy of the
//                  background tile and its one-pixel halo (:30-76), then union-find over the tile's 4-neighbour edges
//                  with LDS atomicMin (the tile's XYZ in LDS); writes the tile-local root (a global index) per pixel
//                  (-1: not a candidate) and zeroes the size counter of every local root
//   k_bgs_border   one lane per edge across a tile border: lock-free union in global memory, larger root under smaller
//   k_bgs_flatten  every pixel to its root; component sizes counted with one atomic per (wave, root), not per pixel
//   k_bgs_compact  kept roots (size >= min_pts, :114) into a per-image list
//   k_bgs_ids      one workgroup per image sorts the list by index: the rank is the id (:95-123), the 254th kept root
//                  caps the run (:124)
//   k_bgs_mask     the mask byte, the foreground box by per-wave min / max and integer atomics (:128-151)
//   k_bgs_depth    the demos' use of the mask (demo.cpp:183-192, live-demo.cpp:317-332): depth zeroed inside the box
//                  where the mask is >= 254, pixels < 254 inside the box counted
// Every retry loop is bounded; a bound that runs out sets the handle's sticky fault word (AVT_STATUS_DEVICE_FAULT).
// Float arithmetic is the reference's, operation by operation: this file is built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <string>
#include <vector>

#include "avt_internal.h"
#include "avt_bgsub_internal.h"

#define BGS_TILE 32
#define BGS_HALO (BGS_TILE + 2)
#define BGS_LIST_CAP 1024      // kept components per image: each has >= max(N/1000, 100) pixels, so at most 1009 of them
#define BGS_FAULT_LOCAL 1u     // LDS union ran out of its bound
#define BGS_FAULT_GLOBAL 2u    // global union / find ran out of its bound
#define BGS_FAULT_LIST 4u      // more kept roots than BGS_LIST_CAP (cannot happen with the bound above)

struct BgsInfo {               // per image, device resident
    int box[4];                // tl.x tl.y br.x br.y: in the previous box, out this run's (kept when capped)
    int acc[4];                // min col, min row, -max col, -max row of non-255 pixels (atomicMin)
    int n_kept, capped, cap_root, fg_count, n_comps, pad[3];
    int comps[AVT_BGSUB_MAX_COMPS][2];
    int list[BGS_LIST_CAP];
};

struct avt_bgsub {
    int device = 0, n_bg = 0, rows = 0, cols = 0;
    hipStream_t stream = nullptr;
    DevBuf<float> d_bg;                    // n_bg x N x 3
    DevBuf<float> d_img;                   // cap x N x 3, cap = d_info.cap images (reserve() grows d_info last)
    DevBuf<int> d_bgidx;                   // cap
    DevBuf<int> d_label;                   // cap x N: parent / root index, -1 not a candidate.  Dead once a run has ended (nothing reads it
                                           // after k_bgs_mask): avt_bgsub_set_background_depth stages its depth image in slot 0 of it
    DevBuf<int> d_count;                   // cap x N: size at a root; after k_bgs_ids -1 - code at a kept root
    DevBuf<unsigned char> d_mask;          // cap x N
    DevBuf<float> d_depth;                 // cap x N: a run's masked depth; between a depth upload and its k_bgs_backproject the staged depth
    DevBuf<float> d_intrin;                // cap x 4: fx fy cx cy of every image of a depth upload, read by the k_bgs_backproject that the
                                           // upload queues and by nothing later; avt_bgsub_set_background_depth overwrites entry 0
    DevBuf<BgsInfo> d_info;                // cap
    DevBuf<unsigned> d_fault;              // sticky fault word of the handle
    int n_images = 0;
    bool ran = false;                      // a run_resident followed the last upload: d_depth and the boxes are that run's
    // hand-over to a reader on another stream (avt_bgsub_internal.h): ev_ready is recorded on `stream` for the reader to wait
    // on, ev_reader on the reader's stream; while reader_pending, whatever overwrites or frees the result waits for ev_reader
    hipEvent_t ev_ready = nullptr, ev_reader = nullptr;
    bool reader_pending = false;
};

namespace {

__device__ __forceinline__ float sqdist(float a0, float a1, float a2, float b0, float b1, float b2) {
    const float d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2;
    return (d0 * d0 + d1 * d1) + d2 * d2;        // BGSubtractor.cpp:47 / :86, left to right, no contraction
}

__device__ __forceinline__ int ld_rel(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_wg(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// parents always point to a smaller index, so a chain is strictly decreasing; the bounds only guard against a broken invariant
__device__ int find_lds(const int* L, int x, bool& ok) {
    for (int i = 0; i < BGS_TILE * BGS_TILE; ++i) {
        const int y = ld_wg(&L[x]);
        if (y == x) return x;
        x = y;
    }
    ok = false;
    return x;
}

__device__ void union_lds(int* L, int a, int b, bool& ok) {
    for (int it = 0; it < 4 * BGS_TILE * BGS_TILE; ++it) {
        a = find_lds(L, a, ok); b = find_lds(L, b, ok);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);     // link the larger root under the smaller
        if (old == a) return;
        a = old;                                 // a was linked meanwhile: join its new parent with b
    }
    ok = false;
}

__device__ int find_g(const int* L, int x, int npix, bool& ok) {
    for (int i = 0; i < npix; ++i) {
        const int y = ld_rel(&L[x]);
        if (y == x) return x;
        x = y;
    }
    ok = false;
    return x;
}

__device__ void union_g(int* L, int a, int b, int npix, bool& ok) {
    for (int it = 0; it < (1 << 20); ++it) {
        a = find_g(L, a, npix, ok); b = find_g(L, b, npix, ok);
        if (!ok || a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
    ok = false;
}

__global__ __launch_bounds__(256) void k_bgs_local(const float* __restrict__ bgs, const int* __restrict__ bgidx, const float* __restrict__ imgs,
                                                   int* __restrict__ label, int* __restrict__ count, BgsInfo* __restrict__ info,
                                                   unsigned* __restrict__ fault, int rows, int cols, float nn_thresh, float neighb_thresh) {
    __shared__ float s_bg[BGS_HALO * BGS_HALO * 3];
    __shared__ float s_px[BGS_TILE * BGS_TILE * 3];
    __shared__ int s_L[BGS_TILE * BGS_TILE];
    const int img = blockIdx.z, t = threadIdx.x;
    const size_t npix = (size_t)rows * cols;
    const float* bg = bgs + (size_t)bgidx[img] * npix * 3;
    const float* px = imgs + (size_t)img * npix * 3;
    const int r0 = blockIdx.y * BGS_TILE, c0 = blockIdx.x * BGS_TILE;
    if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) {      // per-run state of the image (later kernels of this run use it)
        BgsInfo& in = info[img];
        in.acc[0] = INT_MAX; in.acc[1] = INT_MAX; in.acc[2] = INT_MAX; in.acc[3] = INT_MAX;
        in.n_kept = 0; in.capped = 0; in.cap_root = INT_MAX; in.fg_count = 0; in.n_comps = 0;
    }
    // background tile + halo; outside the image z = 0, which the test skips as it skips a zero-depth neighbour: the
    // window clipped at the border (:33-34)
    for (int i = t; i < BGS_HALO * BGS_HALO; i += 256) {
        const int r = r0 + i / BGS_HALO - 1, c = c0 + i % BGS_HALO - 1;
        float x = 0.f, y = 0.f, z = 0.f;
        if (r >= 0 && r < rows && c >= 0 && c < cols) {
            const float* p = bg + ((size_t)r * cols + c) * 3;
            x = p[0]; y = p[1]; z = p[2];
        }
        s_bg[3 * i] = x; s_bg[3 * i + 1] = y; s_bg[3 * i + 2] = z;
    }
    for (int i = t; i < BGS_TILE * BGS_TILE; i += 256) {
        const int r = r0 + (i >> 5), c = c0 + (i & 31);
        float x = 0.f, y = 0.f, z = 0.f;
        if (r < rows && c < cols) {
            const float* p = px + ((size_t)r * cols + c) * 3;
            x = p[0]; y = p[1]; z = p[2];
        }
        s_px[3 * i] = x; s_px[3 * i + 1] = y; s_px[3 * i + 2] = z;
    }
    __syncthreads();
    // near-background test (:56-71): -1 invalid (255), else the pixel's own index (a root of its own)
    for (int i = t; i < BGS_TILE * BGS_TILE; i += 256) {
        const int ly = i >> 5, lx = i & 31;
        int lab = -1;
        const float x = s_px[3 * i], y = s_px[3 * i + 1], z = s_px[3 * i + 2];
        if (r0 + ly < rows && c0 + lx < cols && z != 0.f) {
            lab = i;
            for (int dy = 0; dy < 3 && lab >= 0; ++dy)
                for (int dx = 0; dx < 3; ++dx) {
                    const float* b = &s_bg[3 * ((ly + dy) * BGS_HALO + lx + dx)];
                    if (b[2] == 0.f) continue;
                    if (sqdist(b[0], b[1], b[2], x, y, z) < nn_thresh) { lab = -1; break; }
                }
        }
        s_L[i] = lab;
    }
    __syncthreads();
    // edges to the left and upper neighbour inside the tile: joined unless the squared distance is > neighb (:86)
    bool ok = true;
    for (int i = t; i < BGS_TILE * BGS_TILE; i += 256) {
        if (s_L[i] < 0) continue;
        const int ly = i >> 5, lx = i & 31;
        const float x = s_px[3 * i], y = s_px[3 * i + 1], z = s_px[3 * i + 2];
        if (lx > 0 && s_L[i - 1] >= 0 && !(sqdist(x, y, z, s_px[3 * (i - 1)], s_px[3 * (i - 1) + 1], s_px[3 * (i - 1) + 2]) > neighb_thresh))
            union_lds(s_L, i, i - 1, ok);
        if (ly > 0 && s_L[i - 32] >= 0 && !(sqdist(x, y, z, s_px[3 * (i - 32)], s_px[3 * (i - 32) + 1], s_px[3 * (i - 32) + 2]) > neighb_thresh))
            union_lds(s_L, i, i - 32, ok);
    }
    __syncthreads();
    // the local root (smallest tile index = smallest raster index inside the tile) as a global index
    for (int i = t; i < BGS_TILE * BGS_TILE; i += 256) {
        const int r = r0 + (i >> 5), c = c0 + (i & 31);
        if (r >= rows || c >= cols) continue;
        int g = -1;
        if (s_L[i] >= 0) {
            const int root = find_lds(s_L, i, ok);
            g = (r0 + (root >> 5)) * cols + c0 + (root & 31);
            if (root == i) count[(size_t)img * npix + g] = 0;     // only local roots can be global roots
        }
        label[(size_t)img * npix + (size_t)r * cols + c] = g;
    }
    if (!ok) atomicOr(fault, BGS_FAULT_LOCAL);
}

__global__ __launch_bounds__(256) void k_bgs_border(const float* __restrict__ imgs, int* __restrict__ label, unsigned* __restrict__ fault, int rows,
                                                    int cols, float neighb_thresh, int nvb, int nhb) {
    const int img = blockIdx.y;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nv = (long long)nvb * rows;
    if (e >= nv + (long long)nhb * cols) return;
    int p, q;
    if (e < nv) {                                 // across the vertical border k: (r, 32(k+1) - 1) - (r, 32(k+1))
        const int k = (int)(e / rows), r = (int)(e % rows), c = BGS_TILE * (k + 1) - 1;
        p = r * cols + c; q = p + 1;
    } else {                                      // across the horizontal border k
        const long long e2 = e - nv;
        const int k = (int)(e2 / cols), c = (int)(e2 % cols), r = BGS_TILE * (k + 1) - 1;
        p = r * cols + c; q = p + cols;
    }
    const int npix = rows * cols;
    int* L = label + (size_t)img * npix;
    if (L[p] < 0 || L[q] < 0) return;
    const float* a = imgs + ((size_t)img * npix + p) * 3;
    const float* b = imgs + ((size_t)img * npix + q) * 3;
    if (sqdist(a[0], a[1], a[2], b[0], b[1], b[2]) > neighb_thresh) return;
    bool ok = true;
    union_g(L, p, q, npix, ok);
    if (!ok) atomicOr(fault, BGS_FAULT_GLOBAL);
}

__global__ __launch_bounds__(256) void k_bgs_flatten(int* __restrict__ label, int* __restrict__ count, unsigned* __restrict__ fault, int npix) {
    const int img = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    int* L = label + (size_t)img * npix;
    int* cnt = count + (size_t)img * npix;
    int root = -1;
    bool ok = true;
    if (p < npix && ld_rel(&L[p]) >= 0) {
        root = find_g(L, p, npix, ok);
        __hip_atomic_store(&L[p], root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!ok) atomicOr(fault, BGS_FAULT_GLOBAL);
    // one atomic per distinct root of the wave (a wave is 64 consecutive pixels: mostly one root or none)
    bool live = root >= 0;
    for (int it = 0; it < 64; ++it) {
        const unsigned long long m = __ballot(live);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const int lr = __shfl(root, leader, 64);
        const unsigned long long same = __ballot(live && root == lr);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&cnt[lr], __popcll(same));
        if (live && root == lr) live = false;
    }
}

__global__ __launch_bounds__(256) void k_bgs_compact(const int* __restrict__ label, const int* __restrict__ count, BgsInfo* __restrict__ info,
                                                     unsigned* __restrict__ fault, int npix, int min_pts) {
    const int img = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const size_t o = (size_t)img * npix + p;
    if (label[o] != p || count[o] < min_pts) return;
    const int slot = atomicAdd(&info[img].n_kept, 1);
    if (slot < BGS_LIST_CAP) info[img].list[slot] = p;
    else atomicOr(fault, BGS_FAULT_LIST);
}

__global__ __launch_bounds__(1024) void k_bgs_ids(int* __restrict__ count, BgsInfo* __restrict__ info, int npix) {
    __shared__ int s[BGS_LIST_CAP];
    const int img = blockIdx.x, t = threadIdx.x;
    BgsInfo& in = info[img];
    const int nk = min(in.n_kept, BGS_LIST_CAP);
    s[t] = t < nk ? in.list[t] : INT_MAX;
    __syncthreads();
    for (int k = 2; k <= BGS_LIST_CAP; k <<= 1)            // bitonic sort, ascending
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int o = t ^ j;
            if (o > t) {
                const int a = s[t], b = s[o];
                if (((t & k) == 0) == (a > b)) { s[t] = b; s[o] = a; }
            }
            __syncthreads();
        }
    int* cnt = count + (size_t)img * npix;
    if (t < nk) {
        const int r = s[t], code = min(t, AVT_BGSUB_MAX_COMPS);
        if (t < AVT_BGSUB_MAX_COMPS) { in.comps[t][0] = cnt[r]; in.comps[t][1] = t; }
        cnt[r] = -1 - code;
    }
    if (t == 0) {
        in.capped = nk >= AVT_BGSUB_MAX_COMPS;
        in.cap_root = nk >= AVT_BGSUB_MAX_COMPS ? s[AVT_BGSUB_MAX_COMPS - 1] : INT_MAX;
        in.n_comps = min(nk, AVT_BGSUB_MAX_COMPS);
    }
}

__device__ __forceinline__ int wave_min(int v) {
    for (int s = 32; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
    return v;
}

__global__ __launch_bounds__(256) void k_bgs_mask(const int* __restrict__ label, const int* __restrict__ count, BgsInfo* __restrict__ info,
                                                  unsigned char* __restrict__ mask, int npix, int cols) {
    const int img = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    BgsInfo& in = info[img];
    const int capped = in.capped, cap_root = in.cap_root;
    int code = 255;
    if (p < npix) {
        const size_t o = (size_t)img * npix + p;
        const int r = label[o];
        if (r >= 0) {
            const int v = count[(size_t)img * npix + r];
            // a kept root carries -1 - its code; a small component is 255, or 254 when the run stopped before reaching it
            code = v < 0 ? -1 - v : ((capped && r > cap_root) ? 254 : 255);
        }
        mask[o] = (unsigned char)code;
    }
    if (capped) return;                                     // the box keeps its previous value (:124)
    const bool fg = code != 255;
    if (!__ballot(fg)) return;
    const int r = p / cols, c = p - r * cols;
    const int a0 = wave_min(fg ? c : INT_MAX), a1 = wave_min(fg ? r : INT_MAX);
    const int a2 = wave_min(fg ? -c : INT_MAX), a3 = wave_min(fg ? -r : INT_MAX);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&in.acc[0], a0); atomicMin(&in.acc[1], a1); atomicMin(&in.acc[2], a2); atomicMin(&in.acc[3], a3);
    }
}

__global__ __launch_bounds__(256) void k_bgs_depth(const float* __restrict__ imgs, const unsigned char* __restrict__ mask, BgsInfo* __restrict__ info,
                                                   float* __restrict__ depth, int npix, int rows, int cols) {
    const int img = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    BgsInfo& in = info[img];
    int tlx, tly, brx, bry;
    if (in.capped) {
        tlx = in.box[0]; tly = in.box[1]; brx = in.box[2]; bry = in.box[3];
    } else if (in.acc[0] == INT_MAX) {                    // no foreground: the loop of :131-151 leaves the initial values
        tlx = cols - 1; tly = rows - 1; brx = 0; bry = 0;
    } else {
        tlx = in.acc[0]; tly = in.acc[1]; brx = -in.acc[2]; bry = -in.acc[3];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && !in.capped) { in.box[0] = tlx; in.box[1] = tly; in.box[2] = brx; in.box[3] = bry; }
    bool fg = false;
    if (p < npix) {
        const size_t o = (size_t)img * npix + p;
        const int r = p / cols, c = p - r * cols;
        const bool inside = r >= tly && r <= bry && c >= tlx && c <= brx;
        const unsigned char m = mask[o];
        float z = imgs[o * 3 + 2];
        if (inside && m >= 254) z = 0.f;
        fg = inside && m < 254;
        depth[o] = z;
    }
    const unsigned long long b = __ballot(fg);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(&in.fg_count, __popcll(b));
}

// CameraIntrin::depthToXYZ (Calibration.cpp:82-95) for one pixel: int to float, minus the centre, times z, over the focal
// length; a true IEEE division, nothing fused (this file is built with -ffp-contract=off)
__device__ __forceinline__ void backproject(float z, int r, int c, float fx, float fy, float cx, float cy, float& x, float& y) {
    x = ((float)c - cx) * z / fx;
    y = ((float)r - cy) * z / fy;
}

// A copy's shape: 4 B in, 12 B out per pixel.  A lane takes four consecutive pixels of image blockIdx.y, one 16-byte load
// and three 16-byte stores (48 contiguous bytes), where both addresses are 16-byte aligned (an image's base is when its
// offset in pixels is a multiple of 4: the first image of a buffer always, every image when npix % 4 == 0) and four pixels
// are left; the scalar form otherwise.  Row and column follow the pixel index: a group may cross row ends.
__global__ __launch_bounds__(256) void k_bgs_backproject(const float* __restrict__ depth, const float* __restrict__ intrin, float* __restrict__ xyz,
                                                         int npix, int cols) {
    const int img = blockIdx.y;
    const int p0 = (int)(blockIdx.x * 256 + threadIdx.x) * 4;        // < npix + 1024 <= 2^30 + 1023 (avt_bgsub_create)
    if (p0 >= npix) return;
    const size_t base = (size_t)img * npix;
    const float* d = depth + base + p0;
    float* o = xyz + (base + p0) * 3;
    const float fx = intrin[4 * img], fy = intrin[4 * img + 1], cx = intrin[4 * img + 2], cy = intrin[4 * img + 3];
    int r = p0 / cols, c = p0 - r * cols;
    if ((((size_t)d | (size_t)o) & 15) == 0 && p0 + 4 <= npix) {
        const float4 z4 = *reinterpret_cast<const float4*>(d);
        const float z[4] = {z4.x, z4.y, z4.z, z4.w};
        float v[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            backproject(z[k], r, c, fx, fy, cx, cy, v[3 * k], v[3 * k + 1]);
            v[3 * k + 2] = z[k];
            if (++c == cols) { c = 0; ++r; }
        }
        float4* o4 = reinterpret_cast<float4*>(o);
        o4[0] = make_float4(v[0], v[1], v[2], v[3]);
        o4[1] = make_float4(v[4], v[5], v[6], v[7]);
        o4[2] = make_float4(v[8], v[9], v[10], v[11]);
        return;
    }
    const int left = min(4, npix - p0);
    for (int k = 0; k < left; ++k) {
        const float z = d[k];
        float x, y;
        backproject(z, r, c, fx, fy, cx, cy, x, y);
        o[3 * k] = x; o[3 * k + 1] = y; o[3 * k + 2] = z;
        if (++c == cols) { c = 0; ++r; }
    }
}

// before the stream overwrites what a reader on another stream may still read
int wait_for_reader(avt_bgsub* bg) {
    if (!bg->reader_pending) return 0;
    AVT_HIP(hipStreamWaitEvent(bg->stream, bg->ev_reader, 0));
    bg->reader_pending = false;
    return 0;
}

int reserve(avt_bgsub* bg, int n) {
    // d_info stands for the whole group: it grows last, and it is released when anything below fails, so that a call after
    // a failure allocates again whatever is missing (and, as ever after a failure, every slot starts at cv::Point())
    const size_t old = bg->d_info.cap;             // slots whose boxes carry over
    if ((size_t)n <= old) return 0;
    AVT_HIP(hipStreamSynchronize(bg->stream));
    const size_t N = (size_t)bg->rows * bg->cols;
    bg->n_images = 0;
    const int rc = [&]() -> int {
        if (bg->d_img.reserve(n * N * 3)) return 1;
        if (bg->d_bgidx.reserve(n)) return 1;
        if (bg->d_label.reserve(n * N)) return 1;
        if (bg->d_count.reserve(n * N)) return 1;
        if (bg->d_mask.reserve(n * N)) return 1;
        if (bg->d_depth.reserve(n * N)) return 1;
        if (bg->d_intrin.reserve(n * 4)) return 1;
        // the slots the handle had keep their previous boxes (avt_bgsub.h: a batch without prev_boxes uses them); only the
        // new slots start at cv::Point()
        if (bg->d_info.grow(n, old, bg->stream, false)) return 1;
        AVT_HIP(hipMemsetAsync(bg->d_info + old, 0, (n - old) * sizeof(BgsInfo), bg->stream));
        AVT_HIP(hipStreamSynchronize(bg->stream));
        return 0;
    }();
    if (rc) bg->d_info.release();
    return rc;
}

// the reference's threshold (BGSubtractor.cpp:160-161): int pixel count, double arithmetic, rounded to float by ffill's parameter
float thresh(int rows, int cols, float rel) { return (float)(1200000.0 / (rows * cols) * (double)rel); }

int check_fault(avt_bgsub* bg) {
    unsigned f = 0;
    AVT_HIP(hipMemcpyAsync(&f, bg->d_fault, sizeof(unsigned), hipMemcpyDeviceToHost, bg->stream));
    AVT_HIP(hipStreamSynchronize(bg->stream));
    if (!f) return 0;
    AVT_HIP(hipMemsetAsync(bg->d_fault, 0, sizeof(unsigned), bg->stream));
    AVT_HIP(hipStreamSynchronize(bg->stream));
    avt_set_error("avt_bgsub: a kernel ran out of a bounded retry (fault word " + std::to_string(f) + "); the result is not valid");
    return AVT_STATUS_DEVICE_FAULT;
}

int create_impl(int device, int n_bg, int rows, int cols, const float* backgrounds, avt_bgsub** out) {
    if (!out || n_bg <= 0 || rows <= 0 || cols <= 0 || cols >= 65536 || (long long)rows * cols >= (1ll << 30)) {
        avt_set_error("avt_bgsub_create: bad arguments (rows, cols > 0, cols < 65536, n_backgrounds > 0)");
        return 1;
    }
    AVT_HIP(hipSetDevice(device));
    avt_bgsub* bg = new avt_bgsub();
    bg->device = device; bg->n_bg = n_bg; bg->rows = rows; bg->cols = cols;
    const size_t floats = (size_t)n_bg * rows * cols * 3, bytes = floats * sizeof(float);
    auto fail = [&]() { avt_bgsub_destroy(bg); return 1; };
    if (hipStreamCreateWithFlags(&bg->stream, hipStreamNonBlocking) != hipSuccess || bg->d_bg.reserve(floats) || bg->d_fault.reserve(1)) {
        avt_set_error("avt_bgsub_create: device allocation failed");
        return fail();
    }
    hipError_t e = backgrounds ? hipMemcpyAsync(bg->d_bg, backgrounds, bytes, hipMemcpyHostToDevice, bg->stream)
                               : hipMemsetAsync(bg->d_bg, 0, bytes, bg->stream);
    if (e == hipSuccess) e = hipMemsetAsync(bg->d_fault, 0, sizeof(unsigned), bg->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(bg->stream);
    if (e != hipSuccess) { avt_set_error(std::string("avt_bgsub_create: ") + hipGetErrorString(e)); return fail(); }
    *out = bg;
    return 0;
}

// n depth images at `staged` (device, n x N floats) with their cameras in d_intrin into n XYZ images at `xyz`
void launch_backproject(avt_bgsub* bg, int n, const float* staged, float* xyz) {
    const int npix = bg->rows * bg->cols;
    hipLaunchKernelGGL(k_bgs_backproject, dim3((npix + 1023) / 1024, n), dim3(256), 0, bg->stream, staged, bg->d_intrin, xyz, npix, bg->cols);
}

// `intrin` null: `src` is the XYZ map; else `src` is a depth image (rows x cols) and intrin its camera (fx fy cx cy)
int set_background_impl(avt_bgsub* bg, int index, const float* src, const float* intrin, bool from_depth) {
    if (!bg || !src || (from_depth && !intrin) || index < 0 || index >= bg->n_bg) {
        avt_set_error(from_depth ? "avt_bgsub_set_background_depth: bad arguments" : "avt_bgsub_set_background: bad arguments");
        return 1;
    }
    AVT_HIP(hipSetDevice(bg->device));
    const size_t N = (size_t)bg->rows * bg->cols;
    float* dst = bg->d_bg + (size_t)index * N * 3;
    if (!from_depth) {
        AVT_HIP(hipMemcpyAsync(dst, src, N * 3 * sizeof(float), hipMemcpyHostToDevice, bg->stream));
    } else {
        // staged in the first slot of d_label, a run's scratch that holds nothing once the run has ended (d_depth would do for
        // size, but the last run's masked depth stays downloadable across a change of background, as it does for an XYZ one)
        if (reserve(bg, 1)) return 1;
        float* staged = reinterpret_cast<float*>((int*)bg->d_label);
        AVT_HIP(hipMemcpyAsync(staged, src, N * sizeof(float), hipMemcpyHostToDevice, bg->stream));
        AVT_HIP(hipMemcpyAsync(bg->d_intrin, intrin, 4 * sizeof(float), hipMemcpyHostToDevice, bg->stream));
        launch_backproject(bg, 1, staged, dst);
        AVT_HIP(hipGetLastError());
    }
    AVT_HIP(hipStreamSynchronize(bg->stream));
    return 0;
}

// intrin null: `src` holds n XYZ maps; else n depth images and intrin n x 4 (fx fy cx cy per image)
int upload_impl(avt_bgsub* bg, int n, const float* src, const float* intrin, bool from_depth, const int* bg_index, const int* prev_boxes) {
    const char* name = from_depth ? "avt_bgsub_depth_upload" : "avt_bgsub_images_upload";
    if (!bg || !src || (from_depth && !intrin) || n <= 0) { avt_set_error(std::string(name) + ": bad arguments"); return 1; }
    std::vector<int> idx(n);
    for (int i = 0; i < n; ++i) {
        idx[i] = bg_index ? bg_index[i] : i;
        if (idx[i] < 0 || idx[i] >= bg->n_bg) { avt_set_error(std::string(name) + ": background index out of range"); return 1; }
    }
    AVT_HIP(hipSetDevice(bg->device));
    if (wait_for_reader(bg)) return 1;
    bg->ran = false;
    if (reserve(bg, n)) return 1;
    const size_t N = (size_t)bg->rows * bg->cols;
    if (!from_depth) {
        AVT_HIP(hipMemcpyAsync(bg->d_img, src, (size_t)n * N * 3 * sizeof(float), hipMemcpyHostToDevice, bg->stream));
    } else {
        // staged in d_depth: the reader of the last run's masked depth has been waited for above, and the next run rewrites it
        AVT_HIP(hipMemcpyAsync(bg->d_depth, src, (size_t)n * N * sizeof(float), hipMemcpyHostToDevice, bg->stream));
        AVT_HIP(hipMemcpyAsync(bg->d_intrin, intrin, (size_t)n * 4 * sizeof(float), hipMemcpyHostToDevice, bg->stream));
        launch_backproject(bg, n, bg->d_depth, bg->d_img);
        AVT_HIP(hipGetLastError());
    }
    AVT_HIP(hipMemcpyAsync(bg->d_bgidx, idx.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, bg->stream));
    if (prev_boxes)
        for (int i = 0; i < n; ++i) AVT_HIP(hipMemcpyAsync(bg->d_info[i].box, prev_boxes + 4 * (size_t)i, 4 * sizeof(int), hipMemcpyHostToDevice, bg->stream));
    AVT_HIP(hipStreamSynchronize(bg->stream));     // idx is on this stack frame
    bg->n_images = n;
    return 0;
}

int run_resident_impl(avt_bgsub* bg, float nn_rel, float neighb_rel) {
    if (!bg || bg->n_images <= 0) { avt_set_error("avt_bgsub_run_resident: no images resident"); return 1; }
    AVT_HIP(hipSetDevice(bg->device));
    if (wait_for_reader(bg)) return 1;
    const int rows = bg->rows, cols = bg->cols, n = bg->n_images, npix = rows * cols;
    const float nn = thresh(rows, cols, nn_rel), nb = thresh(rows, cols, neighb_rel);
    const int min_pts = std::max(npix / 1000, 100);                                   // BGSubtractor.cpp:19
    const int tx = (cols + BGS_TILE - 1) / BGS_TILE, ty = (rows + BGS_TILE - 1) / BGS_TILE;
    hipLaunchKernelGGL(k_bgs_local, dim3(tx, ty, n), dim3(256), 0, bg->stream, bg->d_bg, bg->d_bgidx, bg->d_img, bg->d_label, bg->d_count, bg->d_info,
                       bg->d_fault, rows, cols, nn, nb);
    const long long edges = (long long)(tx - 1) * rows + (long long)(ty - 1) * cols;
    if (edges > 0)
        hipLaunchKernelGGL(k_bgs_border, dim3((unsigned)((edges + 255) / 256), n), dim3(256), 0, bg->stream, bg->d_img, bg->d_label, bg->d_fault, rows,
                           cols, nb, tx - 1, ty - 1);
    const dim3 g1((npix + 255) / 256, n);
    hipLaunchKernelGGL(k_bgs_flatten, g1, dim3(256), 0, bg->stream, bg->d_label, bg->d_count, bg->d_fault, npix);
    hipLaunchKernelGGL(k_bgs_compact, g1, dim3(256), 0, bg->stream, bg->d_label, bg->d_count, bg->d_info, bg->d_fault, npix, min_pts);
    hipLaunchKernelGGL(k_bgs_ids, dim3(n), dim3(BGS_LIST_CAP), 0, bg->stream, bg->d_count, bg->d_info, npix);
    hipLaunchKernelGGL(k_bgs_mask, g1, dim3(256), 0, bg->stream, bg->d_label, bg->d_count, bg->d_info, bg->d_mask, npix, cols);
    hipLaunchKernelGGL(k_bgs_depth, g1, dim3(256), 0, bg->stream, bg->d_img, bg->d_mask, bg->d_info, bg->d_depth, npix, rows, cols);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { avt_set_error(std::string("avt_bgsub_run_resident: launch failed: ") + hipGetErrorString(e)); return 1; }
    bg->ran = true;
    return 0;
}

int download_impl(avt_bgsub* bg, int image, unsigned char* mask_out, float* depth_out, avt_bgsub_frame* info) {
    if (!bg || image < 0 || image >= bg->n_images) { avt_set_error("avt_bgsub_download: bad arguments"); return 1; }
    AVT_HIP(hipSetDevice(bg->device));
    const size_t N = (size_t)bg->rows * bg->cols;
    if (mask_out) AVT_HIP(hipMemcpyAsync(mask_out, bg->d_mask + image * N, N, hipMemcpyDeviceToHost, bg->stream));
    if (depth_out) AVT_HIP(hipMemcpyAsync(depth_out, bg->d_depth + image * N, N * sizeof(float), hipMemcpyDeviceToHost, bg->stream));
    BgsInfo h;
    AVT_HIP(hipMemcpyAsync(&h, bg->d_info + image, offsetof(BgsInfo, list), hipMemcpyDeviceToHost, bg->stream));
    if (int rc = check_fault(bg)) return rc;                                          // synchronises the stream
    if (info) {
        info->top_left[0] = h.box[0]; info->top_left[1] = h.box[1]; info->bot_right[0] = h.box[2]; info->bot_right[1] = h.box[3];
        info->capped = h.capped; info->fg_count = h.fg_count; info->n_comps = h.n_comps;
        std::vector<std::pair<int, int>> v(h.n_comps);
        for (int i = 0; i < h.n_comps; ++i) v[i] = {h.comps[i][0], h.comps[i][1]};
        if (!h.capped) std::sort(v.begin(), v.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a > b; });  // :153
        for (int i = 0; i < h.n_comps; ++i) { info->comps[i][0] = v[i].first; info->comps[i][1] = v[i].second; }
    }
    return 0;
}

int xyz_download_impl(avt_bgsub* bg, int image, float* xyz_out) {
    if (!bg || !xyz_out || image < 0 || image >= bg->n_images) { avt_set_error("avt_bgsub_xyz_download: bad arguments (no such resident image)"); return 1; }
    AVT_HIP(hipSetDevice(bg->device));
    const size_t n = (size_t)bg->rows * bg->cols * 3;
    AVT_HIP(hipMemcpyAsync(xyz_out, bg->d_img + image * n, n * sizeof(float), hipMemcpyDeviceToHost, bg->stream));
    AVT_HIP(hipStreamSynchronize(bg->stream));
    return 0;
}

int run_impl(avt_bgsub* bg, int background_index, const float* src, const float* intrin, bool from_depth, float nn_rel, float neighb_rel,
             unsigned char* mask_out, float* depth_out, avt_bgsub_frame* info) {
    if (!bg || !src || (from_depth && !intrin) || !mask_out) { avt_set_error(from_depth ? "avt_bgsub_run_depth: null argument" : "avt_bgsub_run: null argument"); return 1; }
    int box[4] = {0, 0, 0, 0};
    if (info) { box[0] = info->top_left[0]; box[1] = info->top_left[1]; box[2] = info->bot_right[0]; box[3] = info->bot_right[1]; }
    if (upload_impl(bg, 1, src, intrin, from_depth, &background_index, box)) return 1;
    if (run_resident_impl(bg, nn_rel, neighb_rel)) return 1;
    return download_impl(bg, 0, mask_out, depth_out, info);
}

}  // namespace

// ---- avt_bgsub_internal.h
int avt_bgsub_last_run(avt_bgsub* bg, avt_bgsub_view* out) {
    if (!bg || !out || bg->n_images <= 0 || !bg->ran) { avt_set_error("avt_bgsub: no run behind the handle (avt_bgsub_run_resident after the last upload)"); return 1; }
    static_assert(sizeof(BgsInfo) % sizeof(int) == 0 && offsetof(BgsInfo, box) == 0, "the boxes are read as ints at a stride of one BgsInfo");
    // d_img is read-only to every kernel of a run (k_bgs_local, k_bgs_border, k_bgs_depth take it const; the masked depth goes to
    // d_depth): the view's XYZ maps are the originals, which is what demo.cpp:245 reads
    *out = avt_bgsub_view{bg->device, bg->n_images, bg->rows, bg->cols, bg->d_depth, (const int*)(BgsInfo*)bg->d_info, (int)(sizeof(BgsInfo) / sizeof(int)),
                          bg->d_img};
    return 0;
}

int avt_bgsub_resident(avt_bgsub* bg, avt_bgsub_view* out, bool* ran) {
    if (!bg || !out || bg->n_images <= 0) { avt_set_error("avt_bgsub: no images resident behind the handle (an upload first)"); return 1; }
    *out = avt_bgsub_view{bg->device, bg->n_images, bg->rows, bg->cols, bg->d_depth, (const int*)(BgsInfo*)bg->d_info, (int)(sizeof(BgsInfo) / sizeof(int)),
                          bg->d_img};
    if (ran) *ran = bg->ran;
    return 0;
}

int avt_bgsub_reader_begin(avt_bgsub* bg, hipStream_t reader) {
    if (!bg->ev_ready) AVT_HIP(hipEventCreateWithFlags(&bg->ev_ready, hipEventDisableTiming));
    if (!bg->ev_reader) AVT_HIP(hipEventCreateWithFlags(&bg->ev_reader, hipEventDisableTiming));
    if (wait_for_reader(bg)) return 1;         // one reader event: an earlier reader is ordered in front of this one
    AVT_HIP(hipEventRecord(bg->ev_ready, bg->stream));
    AVT_HIP(hipStreamWaitEvent(reader, bg->ev_ready, 0));
    return 0;
}

int avt_bgsub_reader_end(avt_bgsub* bg, hipStream_t reader) {
    AVT_HIP(hipEventRecord(bg->ev_reader, reader));
    bg->reader_pending = true;
    return 0;
}

// ---- exported entry points: no C++ exception crosses the C ABI
extern "C" {
int avt_bgsub_create(int device, int n_backgrounds, int rows, int cols, const float* backgrounds, avt_bgsub** out) {
    return avt_guard("avt_bgsub_create", [&]() -> int { return create_impl(device, n_backgrounds, rows, cols, backgrounds, out); });
}

void avt_bgsub_destroy(avt_bgsub* bg) {
    if (!bg) return;
    if (bg->reader_pending) (void)hipEventSynchronize(bg->ev_reader);    // a reader on another stream is done with the buffers
    if (bg->stream) (void)hipStreamSynchronize(bg->stream);
    // the buffers go with `delete`, after the stream: it has just been drained, so nothing is queued on them either way
    if (bg->stream) (void)hipStreamDestroy(bg->stream);
    if (bg->ev_ready) (void)hipEventDestroy(bg->ev_ready);
    if (bg->ev_reader) (void)hipEventDestroy(bg->ev_reader);
    delete bg;
}

int avt_bgsub_set_background(avt_bgsub* bg, int index, const float* xyz) {
    return avt_guard("avt_bgsub_set_background", [&]() -> int { return set_background_impl(bg, index, xyz, nullptr, false); });
}

int avt_bgsub_run(avt_bgsub* bg, int background_index, const float* xyz, float nn_rel, float neighb_rel, unsigned char* mask_out,
                  float* masked_depth_out, avt_bgsub_frame* info) {
    return avt_guard("avt_bgsub_run", [&]() -> int { return run_impl(bg, background_index, xyz, nullptr, false, nn_rel, neighb_rel, mask_out, masked_depth_out, info); });
}

int avt_bgsub_images_upload(avt_bgsub* bg, int n_images, const float* images, const int* bg_index, const int* prev_boxes) {
    return avt_guard("avt_bgsub_images_upload", [&]() -> int { return upload_impl(bg, n_images, images, nullptr, false, bg_index, prev_boxes); });
}

int avt_bgsub_run_resident(avt_bgsub* bg, float nn_rel, float neighb_rel) {
    return avt_guard("avt_bgsub_run_resident", [&]() -> int { return run_resident_impl(bg, nn_rel, neighb_rel); });
}

int avt_bgsub_download(avt_bgsub* bg, int image, unsigned char* mask_out, float* masked_depth_out, avt_bgsub_frame* info) {
    return avt_guard("avt_bgsub_download", [&]() -> int { return download_impl(bg, image, mask_out, masked_depth_out, info); });
}

int avt_bgsub_depth_upload(avt_bgsub* bg, int n_images, const float* depth, const float* intrin, const int* bg_index, const int* prev_boxes) {
    return avt_guard("avt_bgsub_depth_upload", [&]() -> int { return upload_impl(bg, n_images, depth, intrin, true, bg_index, prev_boxes); });
}

int avt_bgsub_run_depth(avt_bgsub* bg, int background_index, const float* depth, const float* intrin, float nn_rel, float neighb_rel,
                        unsigned char* mask_out, float* masked_depth_out, avt_bgsub_frame* info) {
    return avt_guard("avt_bgsub_run_depth", [&]() -> int { return run_impl(bg, background_index, depth, intrin, true, nn_rel, neighb_rel, mask_out, masked_depth_out, info); });
}

int avt_bgsub_set_background_depth(avt_bgsub* bg, int index, const float* depth, const float* intrin) {
    return avt_guard("avt_bgsub_set_background_depth", [&]() -> int { return set_background_impl(bg, index, depth, intrin, true); });
}

int avt_bgsub_xyz_download(avt_bgsub* bg, int image, float* xyz_out) {
    return avt_guard("avt_bgsub_xyz_download", [&]() -> int { return xyz_download_impl(bg, image, xyz_out); });
}

int avt_bgsub_sync(avt_bgsub* bg) {
    if (!bg) { avt_set_error("avt_bgsub_sync: null handle"); return 1; }
    return avt_guard("avt_bgsub_sync", [&]() -> int { return check_fault(bg); });
}
}  // extern "C"
