// avt_post.hip — RTree::postProcess (RTree.cpp:3422-3449) for a batch of label images on gfx950, restated as connected
// components per part on the interval grid.  At interval 1 that is the reference's result bit for bit; above it
// it is the reference with its downward probe reading row r + interval instead of r + 1 (a deliberate difference).
//
// The grid of image i is the pixels (tl.y + a interval, tl.x + b interval) inside its box; a grid pixel's index is
// a GW + b with GW the grid width of the WHOLE image, so one launch shape serves boxes the host has not seen.
//
// Launch sequence per call, every kernel batched over the images on a grid dimension, no host wait in between:
//   k_post_local    32x32 grid tile per 256-thread workgroup: labels loaded at stride `interval`, union-find over equal labels
//                   in LDS; writes the tile-local root per grid pixel (-1: background), zeroes the statistics, raises the
//                   bad-label bit of the image
//   k_post_border   one lane per edge across a tile border: lock-free union in global memory, larger root under smaller, so
//                   a root is the smallest raster index of its component (what the tie rule needs)
//   k_post_flatten  every grid pixel to its root; 1, b and a added to the root's count (32 bit) and sums (64 bit), one set of
//                   integer atomics per (wave, root)
//   k_post_score    per root the score in IEEE double, operation by operation; 64-bit atomicMax of its bit pattern per
//                   (image, part): positive doubles order as unsigned integers
//   k_post_pick     atomicMin of the root index among the roots that hold that maximum
//   k_post_commit   one lane per (image, part): the centre-of-mass memory of the slot
//   k_post_relabel  a grid pixel whose root lost becomes 255, and its cell is written by upscaleGrid's rule (RTree.cpp:70-99)
// Every loop over parent chains is bounded; a bound that runs out raises the image's fault bit (AVT_STATUS_DEVICE_FAULT).
// The number of components is not capped: on a checkerboard every grid pixel is a root.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/avt.h"
#include "avt_post.h"

#define PP_TILE 32

namespace {

struct PostGeo { int tlx, tly, brx, bry, gh, gw; };

// the box of an image and its grid extents; false: the box is empty or does not lie inside the image (nothing is touched)
__device__ __forceinline__ bool post_geo(const int* __restrict__ boxes, int box_stride, int img, int rows, int cols, int iv, PostGeo& g) {
    const int* b = boxes + (size_t)img * box_stride;
    g.tlx = b[0]; g.tly = b[1]; g.brx = b[2]; g.bry = b[3];
    if (!(0 <= g.tlx && g.tlx <= g.brx && g.brx < cols && 0 <= g.tly && g.tly <= g.bry && g.bry < rows)) return false;
    g.gh = (g.bry - g.tly) / iv + 1;           // <= ceil(rows / iv)
    g.gw = (g.brx - g.tlx) / iv + 1;
    return true;
}

__device__ __forceinline__ int ld_rel(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_wg(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// parents always point to a smaller index, so a chain is strictly decreasing; the bounds only guard against a broken invariant
__device__ int find_lds(const int* L, int x, bool& ok) {
    for (int i = 0; i < PP_TILE * PP_TILE; ++i) {
        const int y = ld_wg(&L[x]);
        if (y == x) return x;
        x = y;
    }
    ok = false;
    return x;
}

__device__ void union_lds(int* L, int a, int b, bool& ok) {
    for (int it = 0; it < 4 * PP_TILE * PP_TILE; ++it) {
        a = find_lds(L, a, ok); b = find_lds(L, b, ok);
        if (!ok || a == b) return;
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
        if (y < 0 || y > x) break;               // not a parent: the invariant is broken
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

__global__ __launch_bounds__(256) void k_post_local(const unsigned char* __restrict__ labels, const int* __restrict__ boxes, int box_stride,
                                                    int* __restrict__ parent, int* __restrict__ count, unsigned long long* __restrict__ sums,
                                                    unsigned* __restrict__ status, int rows, int cols, int iv, int GH, int GW, int num_parts) {
    __shared__ int s_L[PP_TILE * PP_TILE];
    __shared__ unsigned char s_lab[PP_TILE * PP_TILE];
    const int img = blockIdx.z, t = threadIdx.x;
    PostGeo g;
    if (!post_geo(boxes, box_stride, img, rows, cols, iv, g)) return;
    const int i0 = blockIdx.y * PP_TILE, j0 = blockIdx.x * PP_TILE;
    if (i0 >= g.gh || j0 >= g.gw) return;                    // the whole workgroup: no barrier is left behind
    const unsigned char* im = labels + (size_t)img * rows * cols;
    bool bad = false;
    for (int k = t; k < PP_TILE * PP_TILE; k += 256) {
        const int i = i0 + (k >> 5), j = j0 + (k & 31);
        unsigned char v = 255;
        if (i < g.gh && j < g.gw) {
            v = im[(size_t)(g.tly + i * iv) * cols + g.tlx + j * iv];      // row <= br.y, column <= br.x
            if (v != 255 && v >= num_parts) { bad = true; v = 255; }
        }
        s_lab[k] = v;
        s_L[k] = v == 255 ? -1 : k;
    }
    __syncthreads();
    bool ok = true;
    for (int k = t; k < PP_TILE * PP_TILE; k += 256) {
        if (s_L[k] < 0) continue;
        const unsigned char v = s_lab[k];
        if ((k & 31) > 0 && s_lab[k - 1] == v) union_lds(s_L, k, k - 1, ok);
        if ((k >> 5) > 0 && s_lab[k - PP_TILE] == v) union_lds(s_L, k, k - PP_TILE, ok);
    }
    __syncthreads();
    const size_t base = (size_t)img * GH * GW;
    for (int k = t; k < PP_TILE * PP_TILE; k += 256) {
        const int i = i0 + (k >> 5), j = j0 + (k & 31);
        if (i >= g.gh || j >= g.gw) continue;
        int r = -1;
        if (s_L[k] >= 0) {
            const int root = find_lds(s_L, k, ok);
            r = (i0 + (root >> 5)) * GW + j0 + (root & 31);
        }
        const size_t o = base + (size_t)i * GW + j;
        parent[o] = r;
        count[o] = 0;
        sums[2 * o] = 0; sums[2 * o + 1] = 0;
    }
    if (bad) atomicOr(&status[img], AVT_POST_BAD_LABEL);
    if (!ok) atomicOr(&status[img], AVT_POST_FAULT);
}

__global__ __launch_bounds__(256) void k_post_border(const unsigned char* __restrict__ labels, const int* __restrict__ boxes, int box_stride,
                                                     int* __restrict__ parent, unsigned* __restrict__ status, int rows, int cols, int iv, int GH,
                                                     int GW, int nvb, int nhb) {
    const int img = blockIdx.y;
    PostGeo g;
    if (!post_geo(boxes, box_stride, img, rows, cols, iv, g)) return;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nv = (long long)nvb * GH;
    if (e >= nv + (long long)nhb * GW) return;
    int i, j, di, dj;
    if (e < nv) {                                 // across the vertical border k: (i, 32(k+1) - 1) - (i, 32(k+1))
        const int k = (int)(e / GH);
        i = (int)(e % GH); j = PP_TILE * (k + 1) - 1; di = 0; dj = 1;
    } else {                                      // across the horizontal border k
        const long long e2 = e - nv;
        const int k = (int)(e2 / GW);
        j = (int)(e2 % GW); i = PP_TILE * (k + 1) - 1; di = 1; dj = 0;
    }
    if (i + di >= g.gh || j + dj >= g.gw) return;
    const int p = i * GW + j, q = (i + di) * GW + j + dj;
    int* L = parent + (size_t)img * GH * GW;
    if (L[p] < 0 || L[q] < 0) return;
    const unsigned char* im = labels + (size_t)img * rows * cols;
    if (im[(size_t)(g.tly + i * iv) * cols + g.tlx + j * iv] != im[(size_t)(g.tly + (i + di) * iv) * cols + g.tlx + (j + dj) * iv]) return;
    bool ok = true;
    union_g(L, p, q, GH * GW, ok);
    if (!ok) atomicOr(&status[img], AVT_POST_FAULT);
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_post_flatten(const int* __restrict__ boxes, int box_stride, int* __restrict__ parent, int* __restrict__ count,
                                                      unsigned long long* __restrict__ sums, unsigned* __restrict__ status, int rows, int cols, int iv,
                                                      int GH, int GW) {
    const int img = blockIdx.y;
    PostGeo g;
    if (!post_geo(boxes, box_stride, img, rows, cols, iv, g)) return;
    const int G = GH * GW;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int i = p / GW, j = p - i * GW;
    const size_t base = (size_t)img * G;
    int* L = parent + base;
    int root = -1;
    bool ok = true;
    if (p < G && i < g.gh && j < g.gw && ld_rel(&L[p]) >= 0) {
        root = find_g(L, p, G, ok);
        __hip_atomic_store(&L[p], root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!ok) { atomicOr(&status[img], AVT_POST_FAULT); root = -1; }
    // one set of atomics per distinct root of the wave (64 consecutive grid pixels: mostly one root or none)
    bool live = root >= 0;
    for (int it = 0; it < 64; ++it) {
        const unsigned long long m = __ballot(live);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const int lr = __shfl(root, leader, 64);
        const bool match = live && root == lr;
        const unsigned long long same = __ballot(match);
        int sj = match ? j : 0, si = match ? i : 0;
        if (__popcll(same) > 1) { sj = wave_sum(sj); si = wave_sum(si); }      // wave-uniform branch; 64 x 32767 fits an int
        if ((int)(threadIdx.x & 63) == leader) {
            atomicAdd(&count[base + lr], __popcll(same));
            atomicAdd(&sums[2 * (base + lr)], (unsigned long long)sj);
            atomicAdd(&sums[2 * (base + lr) + 1], (unsigned long long)si);
        }
        if (match) live = false;
    }
}

// The score of a component (suppressPartNonMax, RTree.cpp:125-237): size minus weight times the squared distance of its centre
// of mass to the part's previous one.  The coordinate sums are exact integers; every double operation is rounded on its own, in
// the order the host code evaluates them.
__device__ __forceinline__ double post_score(int n, unsigned long long sj, unsigned long long si, const PostGeo& g, int iv, double cpx, double cpy,
                                             double w, double& cx, double& cy) {
    const long long sx = (long long)n * g.tlx + (long long)iv * (long long)sj, sy = (long long)n * g.tly + (long long)iv * (long long)si;
    const double dn = (double)n;
    cx = __ddiv_rn((double)sx, dn); cy = __ddiv_rn((double)sy, dn);
    double score = dn;
    if (cpx >= 0.) {
        const double dx = __dsub_rn(cx, cpx), dy = __dsub_rn(cy, cpy);
        score = __dsub_rn(score, __dmul_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), w));
    }
    return score;
}

// pick == 0: the maximum of the scores > 0 per (image, part); pick == 1: the smallest root among those that hold it
__global__ __launch_bounds__(256) void k_post_score(const unsigned char* __restrict__ labels, const int* __restrict__ boxes, int box_stride,
                                                    const int* __restrict__ parent, const int* __restrict__ count,
                                                    const unsigned long long* __restrict__ sums, const unsigned* __restrict__ status,
                                                    const double* __restrict__ com, const int* __restrict__ valid,
                                                    unsigned long long* __restrict__ best, int* __restrict__ win, int rows, int cols, int iv, int GH,
                                                    int GW, int num_parts, double w, int pick) {
    const int img = blockIdx.y;
    if (status[img] & AVT_POST_BAD_LABEL) return;
    PostGeo g;
    if (!post_geo(boxes, box_stride, img, rows, cols, iv, g)) return;
    const int G = GH * GW;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int i = p / GW, j = p - i * GW;
    if (p >= G || i >= g.gh || j >= g.gw) return;
    const size_t o = (size_t)img * G + p;
    if (parent[o] != p) return;
    const int part = labels[(size_t)img * rows * cols + (size_t)(g.tly + i * iv) * cols + g.tlx + j * iv];   // < num_parts: a root of a good image
    const size_t slot = (size_t)img * num_parts + part;
    const bool sized = valid[img] != 0;
    double cx, cy;
    const double score = post_score(count[o], sums[2 * o], sums[2 * o + 1], g, iv, sized ? com[2 * slot] : -1., sized ? com[2 * slot + 1] : 0., w, cx, cy);
    if (!(score > 0.)) return;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(score);
    if (!pick) atomicMax(&best[slot], bits);
    else if (best[slot] == bits) atomicMin(&win[slot], p);
}

__global__ __launch_bounds__(256) void k_post_commit(const int* __restrict__ boxes, int box_stride, const int* __restrict__ count,
                                                     const unsigned long long* __restrict__ sums, const unsigned* __restrict__ status,
                                                     double* __restrict__ com, const int* __restrict__ valid, const int* __restrict__ win, int n,
                                                     int rows, int cols, int iv, int GH, int GW, int num_parts, int type) {
    const int tid = blockIdx.x * 256 + threadIdx.x;
    if (tid >= n * num_parts) return;
    const int img = tid / num_parts;
    if (status[img] & AVT_POST_BAD_LABEL) return;
    double* c = com + 2 * (size_t)tid;
    if (!valid[img]) { c[0] = -1.; c[1] = 0.; }               // the resize branch of RTree.cpp:3431-3435
    if (type != 0) return;                                    // a disjoint part map only sizes the memory
    PostGeo g;
    const int root = post_geo(boxes, box_stride, img, rows, cols, iv, g) ? win[tid] : AVT_POST_NONE;
    if (root == AVT_POST_NONE) { c[0] = -1.; return; }        // y stays
    const size_t o = (size_t)img * GH * GW + root;
    double cx, cy;
    post_score(count[o], sums[2 * o], sums[2 * o + 1], g, iv, -1., 0., 0., cx, cy);
    c[0] = cx; c[1] = cy;
}

__global__ __launch_bounds__(256) void k_post_relabel(unsigned char* __restrict__ labels, const int* __restrict__ boxes, int box_stride,
                                                      const int* __restrict__ parent, const int* __restrict__ count,
                                                      const unsigned* __restrict__ status, int* __restrict__ valid, const int* __restrict__ win,
                                                      int rows, int cols, int iv, int GH, int GW, int num_parts, int type,
                                                      unsigned long long min_size) {
    const int img = blockIdx.y;
    if (status[img] & AVT_POST_BAD_LABEL) return;             // that image is not written, and neither is its memory
    if (blockIdx.x == 0 && threadIdx.x == 0) valid[img] = 1;  // k_post_commit has sized the slot
    PostGeo g;
    if (!post_geo(boxes, box_stride, img, rows, cols, iv, g)) return;
    const int G = GH * GW;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int i = p / GW, j = p - i * GW;
    if (p >= G || i >= g.gh || j >= g.gw) return;
    unsigned char* im = labels + (size_t)img * rows * cols;
    const int r = g.tly + i * iv, c = g.tlx + j * iv;          // r <= br.y < rows, c <= br.x < cols
    const unsigned char lab = im[(size_t)r * cols + c];
    unsigned char out = lab;
    if (lab != 255) {
        const size_t base = (size_t)img * G;
        const int root = parent[base + p];
        const bool keep = type == 0 ? win[(size_t)img * num_parts + lab] == root : (unsigned long long)count[base + root] >= min_size;
        if (!keep) out = 255;
    }
    if (iv == 1 || i == 0) {                                   // grid row tl.y is not up-scaled
        if (out != lab) im[(size_t)r * cols + c] = out;
        return;
    }
    const int r1 = min(r + iv - 1, g.bry), c1 = min(c + iv - 1, cols - 1);    // the fill may pass br.x, never the image
    for (int rr = r; rr <= r1; ++rr)
        for (int cc = c; cc <= c1; ++cc) im[(size_t)rr * cols + cc] = out;
}

int reserve_slots(AvtPostState* ps, hipStream_t stream, int num_parts, int slots) {
    if (slots <= ps->slots) return 0;
    const size_t old = (size_t)ps->slots;
    if (ps->com.grow((size_t)slots * num_parts * 2, old * num_parts * 2, stream, false)) return 1;
    if (ps->valid.grow((size_t)slots, old, stream, false)) return 1;
    AVT_HIP(hipMemsetAsync(ps->valid + old, 0, (slots - old) * sizeof(int), stream));     // not sized yet
    ps->slots = slots;
    return 0;
}

}  // namespace

int avt_post_launch(AvtPostState* ps, hipStream_t stream, unsigned char* d_labels, int n, int rows, int cols, const int* d_boxes, int box_stride,
                    int interval, int num_parts, int part_map_type, double dist_to_pre_weight) {
    if (n <= 0 || n > 65535) { avt_set_error("post-process: 1 to 65535 images per call"); return 1; }
    if (rows <= 0 || cols <= 0 || rows >= 32768 || cols >= 32768 || interval <= 0 || num_parts <= 0 || num_parts > 127) {
        avt_set_error("post-process: bad image size, interval or number of parts");
        return 1;
    }
    const int GH = (rows + interval - 1) / interval, GW = (cols + interval - 1) / interval;
    const size_t G = (size_t)GH * GW, total = (size_t)n * G, np = (size_t)n * num_parts;       // G < 2^30
    if (ps->parent.reserve(total) || ps->count.reserve(total) || ps->sums.reserve(2 * total) || ps->best.reserve(np) || ps->win.reserve(np) ||
        ps->status.reserve(n) || reserve_slots(ps, stream, num_parts, n))
        return 1;
    AVT_HIP(hipMemsetAsync(ps->status, 0, n * sizeof(unsigned), stream));
    AVT_HIP(hipMemsetAsync(ps->best, 0, np * sizeof(unsigned long long), stream));
    AVT_HIP(hipMemsetAsync(ps->win, 0x7f, np * sizeof(int), stream));                      // AVT_POST_NONE
    const int tx = (GW + PP_TILE - 1) / PP_TILE, ty = (GH + PP_TILE - 1) / PP_TILE;
    hipLaunchKernelGGL(k_post_local, dim3(tx, ty, n), dim3(256), 0, stream, d_labels, d_boxes, box_stride, ps->parent, ps->count, ps->sums, ps->status,
                       rows, cols, interval, GH, GW, num_parts);
    const long long edges = (long long)(tx - 1) * GH + (long long)(ty - 1) * GW;
    if (edges > 0)
        hipLaunchKernelGGL(k_post_border, dim3((unsigned)((edges + 255) / 256), n), dim3(256), 0, stream, d_labels, d_boxes, box_stride, ps->parent,
                           ps->status, rows, cols, interval, GH, GW, tx - 1, ty - 1);
    const dim3 g1((unsigned)((G + 255) / 256), n);
    hipLaunchKernelGGL(k_post_flatten, g1, dim3(256), 0, stream, d_boxes, box_stride, ps->parent, ps->count, ps->sums, ps->status, rows, cols, interval,
                       GH, GW);
    if (part_map_type == 0)
        for (int pick = 0; pick < 2; ++pick)
            hipLaunchKernelGGL(k_post_score, g1, dim3(256), 0, stream, d_labels, d_boxes, box_stride, ps->parent, ps->count, ps->sums, ps->status,
                               ps->com, ps->valid, ps->best, ps->win, rows, cols, interval, GH, GW, num_parts, dist_to_pre_weight, pick);
    hipLaunchKernelGGL(k_post_commit, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream, d_boxes, box_stride, ps->count, ps->sums, ps->status,
                       ps->com, ps->valid, ps->win, n, rows, cols, interval, GH, GW, num_parts, part_map_type);
    // removeSmallPieces' threshold (RTree.cpp:239-323): the integer division first, as the host code has it
    const unsigned long long min_size = (unsigned long long)((long long)rows * cols / ((long long)interval * interval) * 0.0005);
    hipLaunchKernelGGL(k_post_relabel, g1, dim3(256), 0, stream, d_labels, d_boxes, box_stride, ps->parent, ps->count, ps->status, ps->valid, ps->win,
                       rows, cols, interval, GH, GW, num_parts, part_map_type, min_size);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { avt_set_error(std::string("post-process: launch failed: ") + hipGetErrorString(e)); return 1; }
    return 0;
}

int avt_post_finish(AvtPostState* ps, hipStream_t stream, int n, const char* who) {
    ps->h_status.assign(n, 0u);
    AVT_HIP(hipMemcpyAsync(ps->h_status.data(), ps->status, n * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    AVT_HIP(hipStreamSynchronize(stream));
    int bad = -1, fault = -1;
    for (int i = n - 1; i >= 0; --i) {
        if (ps->h_status[i] & AVT_POST_BAD_LABEL) bad = i;
        if (ps->h_status[i] & AVT_POST_FAULT) fault = i;
    }
    if (fault >= 0) {
        avt_set_error(std::string(who) + ": a kernel ran out of a bounded retry on image " + std::to_string(fault) + "; the result is not valid");
        return AVT_STATUS_DEVICE_FAULT;
    }
    if (bad >= 0) {
        avt_set_error(std::string(who) + ": label out of range (neither 255 nor < num_parts) in image " + std::to_string(bad) +
                      "; that image and its memory were left as they were");
        return 1;
    }
    return 0;
}

int avt_post_com_set(AvtPostState* ps, hipStream_t stream, int num_parts, int first, int n, const double* com, const unsigned char* valid) {
    if (!com || first < 0 || n <= 0 || first > 65535 - n) { avt_set_error("com_pre_set: bad arguments (slots 0 to 65534)"); return 1; }
    if (reserve_slots(ps, stream, num_parts, first + n)) return 1;
    std::vector<int> v(n, 1);
    if (valid) for (int i = 0; i < n; ++i) v[i] = valid[i] ? 1 : 0;
    AVT_HIP(hipMemcpyAsync(ps->com + (size_t)first * num_parts * 2, com, (size_t)n * num_parts * 2 * sizeof(double), hipMemcpyHostToDevice, stream));
    AVT_HIP(hipMemcpyAsync(ps->valid + first, v.data(), n * sizeof(int), hipMemcpyHostToDevice, stream));
    AVT_HIP(hipStreamSynchronize(stream));             // `v` is on this stack frame
    return 0;
}

int avt_post_com_get(AvtPostState* ps, hipStream_t stream, int num_parts, int first, int n, double* com, unsigned char* valid) {
    if (!com || first < 0 || n <= 0 || first > 65535 - n) { avt_set_error("com_pre_get: bad arguments (slots 0 to 65534)"); return 1; }
    const int have = std::max(0, std::min(n, ps->slots - first));      // the slots behind these were never set
    std::vector<int> v(n, 0);
    if (have > 0) {
        AVT_HIP(hipMemcpyAsync(com, ps->com + (size_t)first * num_parts * 2, (size_t)have * num_parts * 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
        AVT_HIP(hipMemcpyAsync(v.data(), ps->valid + first, have * sizeof(int), hipMemcpyDeviceToHost, stream));
        AVT_HIP(hipStreamSynchronize(stream));
    }
    for (int i = 0; i < n; ++i) {
        if (valid) valid[i] = v[i] ? 1 : 0;
        if (!v[i])                                     // not sized: what the resize branch would make of it
            for (int k = 0; k < num_parts; ++k) { com[((size_t)i * num_parts + k) * 2] = -1.; com[((size_t)i * num_parts + k) * 2 + 1] = 0.; }
    }
    return 0;
}
