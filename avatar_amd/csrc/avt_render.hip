// avt_render.hip — synthetic depth-frame generator on the GPU: depth + body-part render of posed
// avatars and back-projection into (data_cloud, data_part_labels), written straight into the context's resident frame
// buffers so that batched benchmarks need no host rasteriser.
// The second half of the file is ark::AvatarRenderer on the GPU (include/avt_render.h): the same painter's-order fills applied
// to avatars that are already posed, with the renderer's own buffers.
//
// Behavioural counterpart of AvatarRenderer::renderDepth / renderPartMask (AvatarRenderer.cpp:72-101, :174-202), the
// projection of AvatarRenderer.cpp:11-24, CameraIntrin::to3D (Calibration.cpp:68-74, float arithmetic) and the y flip of
// optim.cpp:116-119.  Like the host generator (synth_render.cpp) it resolves visibility with a z-buffer instead of the
// reference's painter's algorithm; the two generators are bit-identical to each other (tests/test_gpu_render.py,
// tests/test_gpu_raster_edges.py):
// this translation unit is built with -ffp-contract=off and uses the same float expressions, and depth ties go to the
// lowest face index (64-bit atomicMin on (depth bits, face id)) exactly like the host's in-order strict '<' test.
#include <algorithm>
#include <string>
#include <vector>

#include "avt_device.h"
#include "avt_bucket.h"
#include "../../include/avt_render.h"

__device__ __forceinline__ void project(const double* p, double fx, double fy, double cx, double cy, float* px, float* py) {
    *px = (float)(p[0] * fx / p[2] + cx);
    *py = (float)(-p[1] * fy / p[2] + cy);
}

__global__ __launch_bounds__(256) void k_raster_clear(unsigned long long* zkey, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) zkey[i] = 0xFFFFFFFFFFFFFFFFull;
}

// one lane per face
__global__ __launch_bounds__(256) void k_raster(DeviceModel dm, FrameBuffers fb, unsigned long long* zkey, double fx, double fy, double cx,
                                                double cy, int width, int height) {
    const int F = dm.d.F, V = dm.d.V;
    const int f = blockIdx.y + fb.f0;
    const int face = blockIdx.x * 256 + threadIdx.x;
    if (face >= F) return;
    const int ia = dm.mesh[face], ib = dm.mesh[(size_t)F + face], ic = dm.mesh[2 * (size_t)F + face];
    const double* cl = fb.cloud + (size_t)f * 3 * V;
    const double* a = cl + 3 * ia; const double* b = cl + 3 * ib; const double* c = cl + 3 * ic;
    const double ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2], ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
    const double n0 = ab1 * ac2 - ab2 * ac1, n1 = ab2 * ac0 - ab0 * ac2, n2 = ab0 * ac1 - ab1 * ac0;
    const double nn = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    if (!(nn > 0.0) || fabs(n2 / nn) < 0.1) return;             // edge-on faces carry no depth
    if (a[2] <= 0.0 || b[2] <= 0.0 || c[2] <= 0.0) return;
    float ax, ay, bx, by, cxx, cyy;
    project(a, fx, fy, cx, cy, &ax, &ay); project(b, fx, fy, cx, cy, &bx, &by); project(c, fx, fy, cx, cy, &cxx, &cyy);
    const float denom = (by - cyy) * (ax - cxx) + (cxx - bx) * (ay - cyy);
    if (denom == 0.0f) return;
    const float inv = 1.0f / denom;
    // clamped in float before the conversion, as in synth_render.cpp (a projected coordinate may lie beyond the range of int)
    const int x0 = (int)fminf(fmaxf(floorf(fminf(ax, fminf(bx, cxx))), 0.0f), (float)width);
    const int x1 = (int)fminf(fmaxf(ceilf(fmaxf(ax, fmaxf(bx, cxx))), -1.0f), (float)(width - 1));
    const int y0 = (int)fminf(fmaxf(floorf(fminf(ay, fminf(by, cyy))), 0.0f), (float)height);
    const int y1 = (int)fminf(fmaxf(ceilf(fmaxf(ay, fmaxf(by, cyy))), -1.0f), (float)(height - 1));
    const float az = (float)a[2], bz = (float)b[2], cz = (float)c[2];
    unsigned long long* zk = zkey + (size_t)(f - fb.f0) * width * height;
    for (int r = y0; r <= y1; ++r)
        for (int col = x0; col <= x1; ++col) {
            const float w1 = ((by - cyy) * (col - cxx) + (cxx - bx) * (r - cyy)) * inv;
            const float w2 = ((cyy - ay) * (col - cxx) + (ax - cxx) * (r - cyy)) * inv;
            const float w3 = 1.0f - w1 - w2;
            if (w1 < 0.0f || w2 < 0.0f || w3 < 0.0f) continue;
            const float z = w1 * az + w2 * bz + w3 * cz;
            if (!(z > 0.0f)) continue;
            const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)face;
            atomicMin(zk + (size_t)r * width + col, key);
        }
}

// per pixel: winning face -> part label of its nearest projected vertex; count foreground pixels per 256-pixel block
__global__ __launch_bounds__(256) void k_raster_label(DeviceModel dm, FrameBuffers fb, const unsigned long long* zkey, const int* vertex_part,
                                                      unsigned char* label, int* block_count, double fx, double fy, double cx, double cy,
                                                      int width, int height) {
    const int F = dm.d.F, V = dm.d.V;
    const int fl = blockIdx.y, f = fl + fb.f0;
    const size_t npix = (size_t)width * height;
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    int fg = 0;
    if (o < npix) {
        const unsigned long long key = zkey[(size_t)fl * npix + o];
        unsigned char lab = 255;
        if (key != 0xFFFFFFFFFFFFFFFFull) {
            const int face = (int)(key & 0xFFFFFFFFull);
            const int r = (int)(o / width), col = (int)(o % width);
            const int ia = dm.mesh[face], ib = dm.mesh[(size_t)F + face], ic = dm.mesh[2 * (size_t)F + face];
            const double* cl = fb.cloud + (size_t)f * 3 * V;
            float ax, ay, bx, by, cxx, cyy;
            project(cl + 3 * ia, fx, fy, cx, cy, &ax, &ay); project(cl + 3 * ib, fx, fy, cx, cy, &bx, &by);
            project(cl + 3 * ic, fx, fy, cx, cy, &cxx, &cyy);
            const float da = (ax - col) * (ax - col) + (ay - r) * (ay - r);
            const float db = (bx - col) * (bx - col) + (by - r) * (by - r);
            const float dc = (cxx - col) * (cxx - col) + (cyy - r) * (cyy - r);
            lab = (unsigned char)((da < db && da < dc) ? vertex_part[ia] : (db < dc ? vertex_part[ib] : vertex_part[ic]));
            fg = 1;
        }
        label[(size_t)fl * npix + o] = lab;
    }
    const unsigned long long bal = __ballot(fg);
    __shared__ int s_c[4];
    if (lane_id() == 0) s_c[wave_id()] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) block_count[(size_t)fl * gridDim.x + blockIdx.x] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
}

// exclusive scan of the per-block counts, one workgroup per frame; also publishes N
__global__ __launch_bounds__(1024) void k_raster_scan(FrameBuffers fb, int* block_count, int nblocks) {
    const int fl = blockIdx.x, t = threadIdx.x;
    int* bc = block_count + (size_t)fl * nblocks;
    __shared__ int s_w[16];
    __shared__ int s_run;
    if (t == 0) s_run = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblocks; b0 += 1024) {
        const int i = b0 + t;
        const int v = (i < nblocks) ? bc[i] : 0;
        const int incl = wave_incl_scan(v);
        if (lane_id() == 63) s_w[wave_id()] = incl;
        __syncthreads();
        int off = s_run;
        for (int w = 0; w < wave_id(); ++w) off += s_w[w];
        if (i < nblocks) bc[i] = off + incl - v;
        __syncthreads();
        if (t == 1023) s_run = off + incl;
        __syncthreads();
    }
    if (t == 0) {
        const int N = min(s_run, fb.max_points);
        fb.ctl[fl + fb.f0].N = N;
        fb.ctl[fl + fb.f0].T = s_run;       // total foreground pixels (reported even when truncated to max_points)
    }
}

// ordered back-projection of the foreground pixels (row-major pixel order, as the host loop at optim.cpp:100-120)
__global__ __launch_bounds__(256) void k_raster_emit(FrameBuffers fb, const unsigned long long* zkey, const unsigned char* label,
                                                     const int* block_off, float ffx, float ffy, float fcx, float fcy, int width, int height) {
    const int fl = blockIdx.y, f = fl + fb.f0;
    const size_t npix = (size_t)width * height;
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool fg = false;
    unsigned long long key = 0;
    if (o < npix) { key = zkey[(size_t)fl * npix + o]; fg = key != 0xFFFFFFFFFFFFFFFFull; }
    const unsigned long long bal = __ballot(fg);
    __shared__ int s_c[4];
    if (lane_id() == 0) s_c[wave_id()] = __popcll(bal);
    __syncthreads();
    if (!fg) return;
    int pos = block_off[(size_t)fl * gridDim.x + blockIdx.x] + __popcll(bal & ((1ull << lane_id()) - 1ull));
    for (int w = 0; w < wave_id(); ++w) pos += s_c[w];
    if (pos >= fb.max_points) return;
    const int r = (int)(o / width), col = (int)(o % width);
    const float depth = __uint_as_float((unsigned)(key >> 32));
    const float X = ((float)col - fcx) * depth / ffx;       // CameraIntrin::to3D (Calibration.cpp:68-74)
    const float Y = ((float)r - fcy) * depth / ffy;
    double* d = fb.data_raw + 3 * ((size_t)f * fb.max_points + pos);
    d[0] = (double)X; d[1] = -(double)Y; d[2] = (double)depth;  // y negated (optim.cpp:116-119)
    fb.labels_raw[(size_t)f * fb.max_points + pos] = (int)label[(size_t)fl * npix + o];
}

// =====================================================================================================================
// Painter's-order mode: the REFERENCE's renderer, pixel for pixel (oracle/render_oracle.cpp restates the same lines).
//   * faces painted in order of decreasing mean depth, later faces overwrite earlier ones, no depth test
//     (AvatarRenderer.cpp:39-70, :72-101, :174-202)
//   * renderDepth: scanline fill over rows, barycentric depth from the FLOORED first / CEILED last vertex
//     (paintTriangleBary, AvatarHelpers.cpp:61-139); edge-on faces (|n_z| < 0.1) paint 0 with the end-EXCLUSIVE row fill of
//     paintTriangleSingleColor (AvatarHelpers.cpp:247-303)
//   * renderPartMask: scanline fill over COLUMNS, label of the nearest projected vertex by int-truncated squared distances
//     (paintPartsTriangleNN, AvatarHelpers.cpp:153-245); edge-on faces paint 255
// A pixel's final value is the value painted by the LAST covering face of the painter's order, and what a face paints at a
// pixel is a pure function of (face, row, column).  So instead of painting 13 776 faces one after the other, every face
// marks its coverage with atomicMax(order position << 32 | face) - one key image per output, because the two fills cover
// different pixel sets - and a resolve pass evaluates the winner's value with the reference's float / double expression
// order (this translation unit is built with -ffp-contract=off).  Equal sort keys: the reference's std::sort leaves their order
// unspecified; here ties go by ascending face id (a stable sort) - tests assert the fixtures are insensitive to it.
// =====================================================================================================================

// float / double -> int as the reference's x86-64 build converts them (cvttss2si / cvttsd2si: NaN and out-of-range values
// give INT_MIN; the GPU's own conversion saturates instead)
__device__ __forceinline__ int cvt_x86(float v) { return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000; }
__device__ __forceinline__ int cvt_x86(double v) { return (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : (int)0x80000000; }

struct PaintTri { float ax, ay, bx, by, cx, cy; int ia, ib, ic; };   // sorted vertices (a floored / c ceiled by the caller), sorted slots

// std::sort of three (double(coordinate), slot) pairs, lexicographic like std::pair's operator<
__device__ __forceinline__ void sort3(const float k[3], int o[3]) {
    o[0] = 0; o[1] = 1; o[2] = 2;
    auto less = [&](int x, int y) { return (double)k[x] < (double)k[y] || (!((double)k[y] < (double)k[x]) && x < y); };
    if (less(o[1], o[0])) { const int t = o[0]; o[0] = o[1]; o[1] = t; }
    if (less(o[2], o[1])) { const int t = o[1]; o[1] = o[2]; o[2] = t; }
    if (less(o[1], o[0])) { const int t = o[0]; o[0] = o[1]; o[1] = t; }
}

__device__ __forceinline__ void face_projection(const DeviceModel& dm, const double* cl, int face, double fx, double fy, double cx, double cy,
                                                float px[3], float py[3], int vid[3]) {
    const int F = dm.d.F;
    vid[0] = dm.mesh[face]; vid[1] = dm.mesh[(size_t)F + face]; vid[2] = dm.mesh[2 * (size_t)F + face];
    for (int k = 0; k < 3; ++k) project(cl + 3 * (size_t)vid[k], fx, fy, cx, cy, &px[k], &py[k]);
}

// ---- per-face and per-pixel expressions shared by the two painter modes (the generator's AVT_RENDER_PAINTER and the renderer)

// the face's sort key (AvatarRenderer.cpp:62-66) and its normal (b - a) x (c - a) through Eigen 3.3's normalized(): a zero
// vector is returned unchanged (both painter modes use it)
__device__ __forceinline__ float face_key(const double* a, const double* b, const double* c) { return (float)((a[2] + b[2] + c[2]) / 3.f); }

__device__ __forceinline__ float face_key_normal(const double* a, const double* b, const double* c, double n[3]) {
    const double ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2], ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
    const double n0 = ab1 * ac2 - ab2 * ac1, n1 = ab2 * ac0 - ab0 * ac2, n2 = ab0 * ac1 - ab1 * ac0;
    const double z = n0 * n0 + n1 * n1 + n2 * n2;
    if (z > 0.0) { const double s = sqrt(z); n[0] = n0 / s; n[1] = n1 / s; n[2] = n2 / s; }
    else { n[0] = n0; n[1] = n1; n[2] = n2; }
    return face_key(a, b, c);
}

// paintTriangleBary's value at (row i, column j) of the face (AvatarHelpers.cpp:61-139): vertices sorted by y, the first
// floored and the last ceiled, attribute zv of the face's vertex slots; std::min(std::max(v, 0.f), 255.f) (NaN stays NaN)
__device__ __forceinline__ float bary_value(const float px[3], const float py[3], const float zv[3], int i, int j) {
    int s[3];
    sort3(py, s);
    const float ax = px[s[0]], ay = floorf(py[s[0]]), bx = px[s[1]], by = py[s[1]], cxx = px[s[2]], cyy = ceilf(py[s[2]]);
    const float az = zv[s[0]], bz = zv[s[1]], cz = zv[s[2]];
    const float denom = 1.0f / ((bx - cxx) * (ay - cyy) + (cyy - by) * (ax - cxx));
    const float w1v = (bx - cxx) * ((float)i - cyy), w2v = (cxx - ax) * ((float)i - cyy);
    const float w1 = (w1v + (cyy - by) * ((float)j - cxx)) * denom, w2 = (w2v + (ay - cyy) * ((float)j - cxx)) * denom;
    const float v = w1 * az + w2 * bz + (1.f - w1 - w2) * cz;
    const float lo = (v < 0.0f) ? 0.0f : v;
    return (255.0f < lo) ? 255.0f : lo;
}

// paintPartsTriangleNN's label at (row i, column j) of the face (AvatarHelpers.cpp:153-245): vertices sorted by x, the first
// floored and the last ceiled, the part of the nearest one by int-truncated squared distances
__device__ __forceinline__ unsigned char part_label(const float px[3], const float py[3], const int vid[3], const int* vertex_part, int i, int j) {
    int s[3];
    sort3(px, s);
    const float ax = floorf(px[s[0]]), ay = py[s[0]], bx = px[s[1]], by = py[s[1]], cxx = ceilf(px[s[2]]), cyy = py[s[2]];
    const int dista = cvt_x86((ax - (float)j) * (ax - (float)j) + (ay - (float)i) * (ay - (float)i));
    const int distb = cvt_x86((bx - (float)j) * (bx - (float)j) + (by - (float)i) * (by - (float)i));
    const int distc = cvt_x86((cxx - (float)j) * (cxx - (float)j) + (cyy - (float)i) * (cyy - (float)i));
    return (unsigned char)((dista < distb && dista < distc) ? vertex_part[vid[s[0]]] : (distb < distc ? vertex_part[vid[s[1]]] : vertex_part[vid[s[2]]]));
}

// sort key (AvatarRenderer.cpp:62-66: doubles summed, divided by 3.f, stored as float) and the edge-on flag
// (AvatarRenderer.cpp:88-90 with Eigen 3.3's normalized(): a zero vector is returned unchanged, so a degenerate face is edge-on)
__global__ __launch_bounds__(256) void k_paint_keys(DeviceModel dm, FrameBuffers fb, float* fkey, unsigned char* fedge) {
    const int F = dm.d.F, V = dm.d.V;
    const int fl = blockIdx.y, f = fl + fb.f0;
    const int face = blockIdx.x * 256 + threadIdx.x;
    if (face >= F) return;
    const int ia = dm.mesh[face], ib = dm.mesh[(size_t)F + face], ic = dm.mesh[2 * (size_t)F + face];
    const double* cl = fb.cloud + (size_t)f * 3 * V;
    const double* a = cl + 3 * (size_t)ia; const double* b = cl + 3 * (size_t)ib; const double* c = cl + 3 * (size_t)ic;
    double n[3];
    fkey[(size_t)fl * F + face] = face_key_normal(a, b, c, n);
    fedge[(size_t)fl * F + face] = fabs(n[2]) < 0.1 ? 1 : 0;
}

// a sort key as 32 bits whose ascending unsigned order is the painter's order (decreasing float): -0 folded onto +0, which
// compare equal; sign-fold (ascending unsigned = ascending float), complement.  A total order on every bit pattern, so NaN keys
// have a place too, where the reference's std::sort is undefined: positive NaN before +inf, negative NaN
// after -inf.  k_paint_rank and k_rend_sort both order by it.
__device__ __forceinline__ unsigned painter_key_bits(float k) {
    unsigned u = __float_as_uint(k == 0.0f ? 0.0f : k);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

// position of every face in the painter's order = number of faces painted before it: those with a larger key, and those
// with an equal key and a smaller face id (keys compared as painter_key_bits: the float order on every key that is not NaN).
// All lanes read the same key at the same time (scalar loads), 13 776 steps.
__global__ __launch_bounds__(256) void k_paint_rank(int F, const float* __restrict__ fkey, int* __restrict__ frank) {
    const int fl = blockIdx.y;
    const int face = blockIdx.x * 256 + threadIdx.x;
    const float* key = fkey + (size_t)fl * F;
    const unsigned mine = painter_key_bits(face < F ? key[face] : 0.f);
    int before = 0;
    for (int g = 0; g < F; ++g) {
        const unsigned k = painter_key_bits(key[g]);
        before += (k < mine || (k == mine && g < face)) ? 1 : 0;
    }
    if (face < F) frank[(size_t)fl * F + face] = before;
}

// coverage of the row fills (paintTriangleBary when bary, paintTriangleSingleColor otherwise): calls mark(row, col)
template <bool BARY, class Mark>
__device__ __forceinline__ void cover_rows(const float px[3], const float py[3], int W, int H, Mark mark) {
    int o[3];
    sort3(py, o);
    float ax = px[o[0]], ay = floorf(py[o[0]]), bx = px[o[1]], by = py[o[1]], cx = px[o[2]], cy = ceilf(py[o[2]]);
    if (ay == cy) return;
    const int minyi = max(cvt_x86(ay), 0), maxyi = min(cvt_x86(cy), H - 1), midyi = cvt_x86(floorf(by));
    for (int half = 0; half < 2; ++half) {
        if (half == 0 ? !(ay != by) : !(by != cy)) continue;
        int i0, i1;
        if (half == 0) { i0 = minyi; i1 = min(midyi, H - 1); }
        else { i0 = max(midyi, 0) + (BARY ? (ay != by ? 1 : 0) : 1); i1 = maxyi; }
        if (BARY) {
            float mhi = (cx - ax) / (cy - ay), bhi = ax - ay * mhi, mlo, blo;
            if (half == 0) { mlo = (bx - ax) / (by - ay); blo = ax - ay * mlo; }
            else { mlo = (cx - bx) / (cy - by); blo = bx - by * mlo; }
            if (half == 0 ? bx > cx : bx > ax) { float t = mlo; mlo = mhi; mhi = t; t = blo; blo = bhi; bhi = t; }
            for (int i = i0; i <= i1; ++i) {
                const int minxi = max(cvt_x86(floorf(mlo * (float)i + blo)), 0), maxxi = min(cvt_x86(ceilf(mhi * (float)i + bhi)), W - 1);
                for (int j = minxi; j <= maxxi; ++j) mark(i, j);
            }
        } else {
            double mhi = (double)((cx - ax) / (cy - ay)), bhi = (double)ax - (double)ay * mhi, mlo, blo;
            if (half == 0) { mlo = (double)((bx - ax) / (by - ay)); blo = (double)ax - (double)ay * mlo; }
            else { mlo = (double)((cx - bx) / (cy - by)); blo = (double)bx - (double)by * mlo; }
            if (half == 0 ? bx > cx : bx > ax) { double t = mlo; mlo = mhi; mhi = t; t = blo; blo = bhi; bhi = t; }
            for (int i = i0; i <= i1; ++i) {
                const int minxi = max(cvt_x86(floor(mlo * (double)i + blo)), 0), maxxi = min(cvt_x86(ceil(mhi * (double)i + bhi)), W - 1);
                for (int j = minxi; j < maxxi; ++j) mark(i, j);          // std::fill(ptr + minxi, ptr + maxxi): end exclusive
            }
        }
    }
}

// coverage of the column fill of paintPartsTriangleNN: calls mark(row, col)
template <class Mark>
__device__ __forceinline__ void cover_cols(const float px[3], const float py[3], int W, int H, Mark mark) {
    int o[3];
    sort3(px, o);
    float ax = floorf(px[o[0]]), ay = py[o[0]], bx = px[o[1]], by = py[o[1]], cx = ceilf(px[o[2]]), cy = py[o[2]];
    if (ax == cx) return;
    const int minxi = max(cvt_x86(ax), 0), maxxi = min(cvt_x86(cx), W - 1), midxi = cvt_x86(floorf(bx));
    for (int half = 0; half < 2; ++half) {
        if (half == 0 ? !(ax != bx) : !(bx != cx)) continue;
        const int i0 = half == 0 ? minxi : max(midxi, 0) + 1, i1 = half == 0 ? min(midxi, W - 1) : maxxi;
        double mhi = (double)((cy - ay) / (cx - ax)), bhi = (double)ay - (double)ax * mhi, mlo, blo;
        if (half == 0) { mlo = (double)((by - ay) / (bx - ax)); blo = (double)ay - (double)ax * mlo; }
        else { mlo = (double)((cy - by) / (cx - bx)); blo = (double)by - (double)bx * mlo; }
        if (half == 0 ? by > cy : by > ay) { double t = mlo; mlo = mhi; mhi = t; t = blo; blo = bhi; bhi = t; }
        for (int i = i0; i <= i1; ++i) {
            const int minyi = max(cvt_x86(floor(mlo * (double)i + blo)), 0), maxyi = min(cvt_x86(ceil(mhi * (double)i + bhi)), H - 1);
            for (int j = minyi; j <= maxyi; ++j) mark(j, i);
        }
    }
}

// one lane per face: marks its coverage in both key images
__global__ __launch_bounds__(256) void k_paint_cover(DeviceModel dm, FrameBuffers fb, const int* __restrict__ frank, const unsigned char* __restrict__ fedge,
                                                     unsigned long long* dkey, unsigned long long* mkey, double fx, double fy, double cx,
                                                     double cy, int width, int height) {
    const int F = dm.d.F, V = dm.d.V;
    const int fl = blockIdx.y, f = fl + fb.f0;
    const int face = blockIdx.x * 256 + threadIdx.x;
    if (face >= F) return;
    float px[3], py[3]; int vid[3];
    face_projection(dm, fb.cloud + (size_t)f * 3 * V, face, fx, fy, cx, cy, px, py, vid);
    const size_t npix = (size_t)width * height;
    const unsigned long long key = ((unsigned long long)(unsigned)(frank[(size_t)fl * F + face] + 1) << 32) | (unsigned)face;
    unsigned long long* dk = dkey + (size_t)fl * npix;
    unsigned long long* mk = mkey + (size_t)fl * npix;
    const bool eo = fedge[(size_t)fl * F + face] != 0;
    auto mark_d = [&](int r, int c) { atomicMax(dk + (size_t)r * width + c, key); };
    auto mark_m = [&](int r, int c) { atomicMax(mk + (size_t)r * width + c, key); };
    if (eo) {
        cover_rows<false>(px, py, width, height, mark_d);
        cover_rows<false>(px, py, width, height, mark_m);
    } else {
        cover_rows<true>(px, py, width, height, mark_d);
        cover_cols(px, py, width, height, mark_m);
    }
}

// per pixel: what the winning faces painted.  Writes the two reference images (float depth, 0 = background; uint8 part mask,
// 255 = background), rewrites the depth key into the z-buffer generator's format (depth bits << 32, all ones = background) so
// that k_raster_scan / k_raster_emit back-project it unchanged, and counts the pixels with depth > 0 per 256-pixel block.
__global__ __launch_bounds__(256) void k_paint_resolve(DeviceModel dm, FrameBuffers fb, unsigned long long* dkey, const unsigned long long* mkey,
                                                       const unsigned char* __restrict__ fedge, const int* vertex_part, float* depth_img,
                                                       unsigned char* label, int* block_count, double fx, double fy, double cx, double cy,
                                                       int width, int height) {
    const int F = dm.d.F, V = dm.d.V;
    const int fl = blockIdx.y, f = fl + fb.f0;
    const size_t npix = (size_t)width * height;
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    const double* cl = fb.cloud + (size_t)f * 3 * V;
    int fg = 0;
    if (o < npix) {
        const int i = (int)(o / width), j = (int)(o % width);          // row, column
        float depth = 0.f;
        const unsigned long long kd = dkey[(size_t)fl * npix + o];
        if (kd != 0ull) {
            const int face = (int)(kd & 0xFFFFFFFFull);
            if (!fedge[(size_t)fl * F + face]) {
                float px[3], py[3]; int vid[3];
                face_projection(dm, cl, face, fx, fy, cx, cy, px, py, vid);
                const float zv[3] = {(float)cl[3 * (size_t)vid[0] + 2], (float)cl[3 * (size_t)vid[1] + 2], (float)cl[3 * (size_t)vid[2] + 2]};
                depth = bary_value(px, py, zv, i, j);
            }
        }
        unsigned char lab = 255;
        const unsigned long long km = mkey[(size_t)fl * npix + o];
        if (km != 0ull) {
            const int face = (int)(km & 0xFFFFFFFFull);
            if (!fedge[(size_t)fl * F + face]) {
                float px[3], py[3]; int vid[3];
                face_projection(dm, cl, face, fx, fy, cx, cy, px, py, vid);
                lab = part_label(px, py, vid, vertex_part, i, j);
            }
        }
        depth_img[(size_t)fl * npix + o] = depth;
        label[(size_t)fl * npix + o] = lab;
        fg = !(depth <= 0.0f);                                         // optim.cpp:110: `if (ptr[c] <= 0.0) continue;`
        dkey[(size_t)fl * npix + o] = fg ? ((unsigned long long)__float_as_uint(depth) << 32) : 0xFFFFFFFFFFFFFFFFull;
    }
    const unsigned long long bal = __ballot(fg);
    __shared__ int s_c[4];
    if (lane_id() == 0) s_c[wave_id()] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) block_count[(size_t)fl * gridDim.x + blockIdx.x] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
}

__global__ __launch_bounds__(256) void k_paint_clear(unsigned long long* a, unsigned long long* b, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { a[i] = 0ull; b[i] = 0ull; }
}

int avt_paint_enqueue(avt_ctx* c, int nframes, const int* d_vertex_part, unsigned long long* d_dkey, unsigned long long* d_mkey, float* d_fkey,
                      int* d_frank, unsigned char* d_fedge, float* d_depth, unsigned char* d_label, int* d_block, double fx, double fy, double cx,
                      double cy, int width, int height) {
    const size_t npix = (size_t)width * height;
    const int nb = (int)((npix + 255) / 256), F = c->dm.d.F, fb = (F + 255) / 256;
    hipStream_t s = c->cur_stream;
    // the reference's intrinsics are floats (Calibration.h:13); the projection promotes them to double
    fx = (double)(float)fx; fy = (double)(float)fy; cx = (double)(float)cx; cy = (double)(float)cy;
    hipLaunchKernelGGL(k_paint_clear, dim3((unsigned)((npix * nframes + 255) / 256)), dim3(256), 0, s, d_dkey, d_mkey, npix * nframes);
    hipLaunchKernelGGL(k_paint_keys, dim3(fb, nframes), dim3(256), 0, s, c->dm, c->fb, d_fkey, d_fedge);
    hipLaunchKernelGGL(k_paint_rank, dim3(fb, nframes), dim3(256), 0, s, F, d_fkey, d_frank);
    hipLaunchKernelGGL(k_paint_cover, dim3(fb, nframes), dim3(256), 0, s, c->dm, c->fb, d_frank, d_fedge, d_dkey, d_mkey, fx, fy, cx, cy, width, height);
    hipLaunchKernelGGL(k_paint_resolve, dim3(nb, nframes), dim3(256), 0, s, c->dm, c->fb, d_dkey, d_mkey, d_fedge, d_vertex_part, d_depth, d_label,
                       d_block, fx, fy, cx, cy, width, height);
    hipLaunchKernelGGL(k_raster_scan, dim3(nframes), dim3(1024), 0, s, c->fb, d_block, nb);
    hipLaunchKernelGGL(k_raster_emit, dim3(nb, nframes), dim3(256), 0, s, c->fb, d_dkey, d_label, d_block, (float)fx, (float)fy, (float)cx,
                       (float)cy, width, height);
    return hipGetLastError() != hipSuccess;
}

int avt_render_enqueue(avt_ctx* c, int nframes, const int* d_vertex_part, unsigned long long* d_zkey, unsigned char* d_label, int* d_block,
                       double fx, double fy, double cx, double cy, int width, int height) {
    const size_t npix = (size_t)width * height;
    const int nb = (int)((npix + 255) / 256);
    hipStream_t s = c->cur_stream;
    hipLaunchKernelGGL(k_raster_clear, dim3((unsigned)((npix * nframes + 255) / 256)), dim3(256), 0, s, d_zkey, npix * nframes);
    hipLaunchKernelGGL(k_raster, dim3((c->dm.d.F + 255) / 256, nframes), dim3(256), 0, s, c->dm, c->fb, d_zkey, fx, fy, cx, cy, width, height);
    hipLaunchKernelGGL(k_raster_label, dim3(nb, nframes), dim3(256), 0, s, c->dm, c->fb, d_zkey, d_vertex_part, d_label, d_block, fx, fy, cx, cy,
                       width, height);
    hipLaunchKernelGGL(k_raster_scan, dim3(nframes), dim3(1024), 0, s, c->fb, d_block, nb);
    hipLaunchKernelGGL(k_raster_emit, dim3(nb, nframes), dim3(256), 0, s, c->fb, d_zkey, d_label, d_block, (float)fx, (float)fy, (float)cx,
                       (float)cy, width, height);
    return hipGetLastError() != hipSuccess;
}

// =====================================================================================================================
// ark::AvatarRenderer on the GPU (include/avt_render.h): the painter's-order machinery above applied to avatars that are
// already posed, with the reference's four outputs (AvatarRenderer.cpp:11-224).  The handle owns its clouds, its key
// images and its outputs, so nothing here writes to a context.  Launch sequence of a run, every kernel batched over the
// images on a grid dimension:
//   k_rend_project  projected vertices and joints (float pairs, what getProjectedPoints / getProjectedJoints return)
//   k_rend_faces    per face: the mean-depth key, the edge-on flag of renderDepth / renderPartMask (|n_z| < 0.1), the
//                   normalized face normal and the visibility flag of renderLambert (|n_z| > 1e-2)
//   k_rend_sort     one workgroup per image sorts its (key, face id) pairs in LDS: painter position <-> face
//                   (or k_paint_rank + k_rend_scatter, the O(F^2) count; same positions)
//   k_rend_vnormal  per vertex: the normals of its incident faces summed in painter order, divided by their norm (no zero
//                   guard), turned to face the camera; the Lambert value of the two lights
//   k_rend_cover    per face: its coverage marked in the selected key images with atomicMax(position + 1) (a position is
//                   unique, so the key needs no face id); renderFaces' image is the key image itself (atomicMax(position)
//                   over -1)
//   k_rend_resolve  per pixel: what the winning face painted, with the reference's float expression order
// =====================================================================================================================

namespace {

constexpr int REND_SORT_CAP = 16384;           // faces one workgroup sorts in LDS (128 KiB of (key, id) pairs)

__global__ __launch_bounds__(256) void k_rend_project(const double* __restrict__ cloud, const double* __restrict__ joints, float2* proj,
                                                      float2* jproj, int V, int J, double fx, double fy, double cx, double cy) {
    const int img = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    float x, y;
    if (i < V) {
        project(cloud + ((size_t)img * V + i) * 3, fx, fy, cx, cy, &x, &y);
        proj[(size_t)img * V + i] = make_float2(x, y);
    }
    if (i < J) {
        project(joints + ((size_t)img * J + i) * 3, fx, fy, cx, cy, &x, &y);
        jproj[(size_t)img * J + i] = make_float2(x, y);
    }
}

// fflag bit 0: edge-on for renderDepth / renderPartMask (fabs(n_z) < 0.1); bit 1: visible for renderLambert
// (fabs(n_z) > 1e-2: AvatarRenderer.cpp:131's abs() read as the double overload)
__global__ __launch_bounds__(256) void k_rend_faces(const double* __restrict__ cloud, const int* __restrict__ mesh, int V, int F, float* fkey,
                                                    unsigned char* fflag, double* fnorm) {
    const int img = blockIdx.y, face = blockIdx.x * 256 + threadIdx.x;
    if (face >= F) return;
    const double* cl = cloud + (size_t)img * 3 * V;
    const double* a = cl + 3 * (size_t)mesh[face];
    const double* b = cl + 3 * (size_t)mesh[(size_t)F + face];
    const double* c = cl + 3 * (size_t)mesh[2 * (size_t)F + face];
    double n[3];
    const size_t o = (size_t)img * F + face;
    fkey[o] = face_key_normal(a, b, c, n);
    fflag[o] = (fabs(n[2]) < 0.1 ? 1 : 0) | (fabs(n[2]) > 1e-2 ? 2 : 0);
    fnorm[3 * o] = n[0]; fnorm[3 * o + 1] = n[1]; fnorm[3 * o + 2] = n[2];
}

// painter order of one image: (key, face id) pairs sorted in LDS, decreasing key, ties by ascending face id.  The pair is one
// 64-bit word whose ascending order is that order: the high half is the key's bits mapped so that unsigned order is
// decreasing float order (-0 folded onto +0, which compare equal), the low half the face id.  Bitonic sort over the next power
// of two (padding all ones sorts last).
__global__ __launch_bounds__(1024) void k_rend_sort(int F, const float* __restrict__ fkey, int* __restrict__ order, int* __restrict__ rank) {
    __shared__ unsigned long long s[REND_SORT_CAP];
    const int img = blockIdx.x, t = threadIdx.x;
    int P = 1;
    while (P < F) P <<= 1;
    const float* key = fkey + (size_t)img * F;
    for (int i = t; i < P; i += 1024) {
        unsigned long long v = ~0ull;
        if (i < F) v = ((unsigned long long)painter_key_bits(key[i]) << 32) | (unsigned)i;
        s[i] = v;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += 1024) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long x = s[i], y = s[l];
                    const bool up = (i & k) == 0;
                    if (up ? x > y : x < y) { s[i] = y; s[l] = x; }
                }
            }
            __syncthreads();
        }
    for (int i = t; i < F; i += 1024) {
        const int face = (int)(s[i] & 0xFFFFFFFFull);
        order[(size_t)img * F + i] = face;
        rank[(size_t)img * F + face] = i;
    }
}

__global__ __launch_bounds__(256) void k_rend_scatter(int F, const int* __restrict__ rank, int* __restrict__ order) {
    const int img = blockIdx.y, face = blockIdx.x * 256 + threadIdx.x;
    if (face < F) order[(size_t)img * F + rank[(size_t)img * F + face]] = face;
}

// per vertex (AvatarRenderer.cpp:113-166): vertNormal.col(v) += normal for every incident face in painter order (a face that
// names v twice adds twice), colwise().normalize() (VectorwiseOp: division by the column norm, no zero guard, so a zero sum is
// NaN), negated if z > 0; then the Lambert value std::max(float(main . n * 0.8 + back . n * 0.2) * 255, 0.f) with the light
// vectors (light - vertex).normalized().  Sums of 3 terms go left to right.
__global__ __launch_bounds__(256) void k_rend_vnormal(const double* __restrict__ cloud, const int* __restrict__ vf_start, const int* __restrict__ vf,
                                                      const int* __restrict__ rank, const double* __restrict__ fnorm, int V, int F, double* vnorm,
                                                      float* lam) {
    const int img = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int* rk = rank + (size_t)img * F;
    const double* fn = fnorm + (size_t)img * F * 3;
    const int s0 = vf_start[v], s1 = vf_start[v + 1];
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    // selection in (position, slot) order: valences are small, and a slot with a position already taken is skipped by the
    // strict lexicographic step
    int last_pos = -1, last_slot = -1;
    for (int step = s0; step < s1; ++step) {
        int best_pos = 0x7FFFFFFF, best_slot = -1;
        for (int sl = s0; sl < s1; ++sl) {
            const int p = rk[vf[sl]];
            const bool after = p > last_pos || (p == last_pos && sl > last_slot);
            if (after && (p < best_pos || (p == best_pos && sl < best_slot))) { best_pos = p; best_slot = sl; }
        }
        const double* n = fn + 3 * (size_t)vf[best_slot];
        n0 += n[0]; n1 += n[1]; n2 += n[2];
        last_pos = best_pos; last_slot = best_slot;
    }
    const double nrm = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    n0 = n0 / nrm; n1 = n1 / nrm; n2 = n2 / nrm;
    if (n2 > 0) { n0 = -n0; n1 = -n1; n2 = -n2; }
    double* vn = vnorm + ((size_t)img * V + v) * 3;
    vn[0] = n0; vn[1] = n1; vn[2] = n2;
    const double* a = cloud + ((size_t)img * V + v) * 3;
    double m0 = 0.8 - a[0], m1 = 1.5 - a[1], m2 = -1.2 - a[2];
    double b0 = -0.2 - a[0], b1 = -1.5 - a[1], b2 = 0.4 - a[2];
    const double mz = m0 * m0 + m1 * m1 + m2 * m2, bz = b0 * b0 + b1 * b1 + b2 * b2;
    if (mz > 0.0) { const double q = sqrt(mz); m0 = m0 / q; m1 = m1 / q; m2 = m2 / q; }
    if (bz > 0.0) { const double q = sqrt(bz); b0 = b0 / q; b1 = b1 / q; b2 = b2 / q; }
    const double dm = m0 * n0 + m1 * n1 + m2 * n2, db = b0 * n0 + b1 * n1 + b2 * n2;
    const float val = (float)(dm * 0.8 + db * 0.2) * 255.f;
    lam[(size_t)img * V + v] = (val < 0.f) ? 0.f : val;
}

struct RendImgs {
    unsigned* dkey; unsigned* mkey; unsigned* lkey; int* faces;   // [images][npix] each, NULL when not selected
};

// one lane per face: its coverage in every selected image (renderDepth and renderPartMask as k_paint_cover; renderLambert's
// visible faces with the barycentric row fill; renderFaces' end-exclusive row fill for every face)
__global__ __launch_bounds__(256) void k_rend_cover(const float2* __restrict__ proj, const int* __restrict__ mesh, const int* __restrict__ rank,
                                                    const unsigned char* __restrict__ fflag, RendImgs im, int V, int F, int width, int height) {
    const int img = blockIdx.y, face = blockIdx.x * 256 + threadIdx.x;
    if (face >= F) return;
    float px[3], py[3];
    for (int k = 0; k < 3; ++k) {
        const float2 q = proj[(size_t)img * V + mesh[(size_t)k * F + face]];
        px[k] = q.x; py[k] = q.y;
    }
    const size_t npix = (size_t)width * height, base = (size_t)img * npix;
    const int pos = rank[(size_t)img * F + face];
    const unsigned key = (unsigned)pos + 1u;
    const unsigned char fl = fflag[(size_t)img * F + face];
    const bool eo = (fl & 1) != 0;
    if (im.dkey) {
        unsigned* k = im.dkey + base;
        auto mark = [&](int r, int c) { atomicMax(k + (size_t)r * width + c, key); };
        if (eo) cover_rows<false>(px, py, width, height, mark); else cover_rows<true>(px, py, width, height, mark);
    }
    if (im.mkey) {
        unsigned* k = im.mkey + base;
        auto mark = [&](int r, int c) { atomicMax(k + (size_t)r * width + c, key); };
        if (eo) cover_rows<false>(px, py, width, height, mark); else cover_cols(px, py, width, height, mark);
    }
    if (im.lkey && (fl & 2)) {
        unsigned* k = im.lkey + base;
        cover_rows<true>(px, py, width, height, [&](int r, int c) { atomicMax(k + (size_t)r * width + c, key); });
    }
    if (im.faces) {
        int* k = im.faces + base;
        cover_rows<false>(px, py, width, height, [&](int r, int c) { atomicMax(k + (size_t)r * width + c, pos); });
    }
}

__device__ __forceinline__ void face_points(const float2* pr, const int* mesh, int F, int face, float px[3], float py[3], int vid[3]) {
    for (int k = 0; k < 3; ++k) {
        vid[k] = mesh[(size_t)k * F + face];
        const float2 q = pr[vid[k]];
        px[k] = q.x; py[k] = q.y;
    }
}

__global__ __launch_bounds__(256) void k_rend_resolve(const double* __restrict__ cloud, const float2* __restrict__ proj, const int* __restrict__ mesh,
                                                      const int* __restrict__ order, const unsigned char* __restrict__ fflag, const float* __restrict__ lam,
                                                      const int* __restrict__ vertex_part, RendImgs im, float* depth_img, unsigned char* mask_img,
                                                      unsigned char* lam_img, int V, int F, int width, int height) {
    const int img = blockIdx.y;
    const size_t npix = (size_t)width * height;
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= npix) return;
    const size_t po = (size_t)img * npix + o;
    const int i = (int)(o / width), j = (int)(o % width);          // row, column
    const float2* pr = proj + (size_t)img * V;
    const int* ord = order + (size_t)img * F;
    const unsigned char* ff = fflag + (size_t)img * F;
    float px[3], py[3]; int vid[3];
    if (im.dkey) {
        float depth = 0.f;
        const unsigned k = im.dkey[po];
        if (k != 0u) {
            const int face = ord[k - 1];
            if (!(ff[face] & 1)) {
                face_points(pr, mesh, F, face, px, py, vid);
                const double* cl = cloud + (size_t)img * 3 * V;
                const float zv[3] = {(float)cl[3 * (size_t)vid[0] + 2], (float)cl[3 * (size_t)vid[1] + 2], (float)cl[3 * (size_t)vid[2] + 2]};
                depth = bary_value(px, py, zv, i, j);
            }
        }
        depth_img[po] = depth;
    }
    if (im.mkey) {
        unsigned char lab = 255;
        const unsigned k = im.mkey[po];
        if (k != 0u) {
            const int face = ord[k - 1];
            if (!(ff[face] & 1)) {
                face_points(pr, mesh, F, face, px, py, vid);
                lab = part_label(px, py, vid, vertex_part, i, j);
            }
        }
        mask_img[po] = lab;
    }
    if (im.lkey) {
        unsigned char g = 0;
        const unsigned k = im.lkey[po];
        if (k != 0u) {
            const int face = ord[k - 1];
            face_points(pr, mesh, F, face, px, py, vid);
            const float* lm = lam + (size_t)img * V;
            const float zv[3] = {lm[vid[0]], lm[vid[1]], lm[vid[2]]};
            g = (unsigned char)cvt_x86(bary_value(px, py, zv, i, j));   // uint8_t(float) on x86: truncation, NaN -> 0
        }
        lam_img[po] = g;
    }
}

}  // namespace

// =====================================================================================================================
// Self-occlusion visibility inside optimize() (avt_set_occlusion_render, include/avt.h; the block the reference left commented
// out at AvatarOptimizer.cpp:1369-1385): a vertex is visible iff one of its faces passes the back-face test of k_visibility
// AND owns a pixel of renderFaces of the frame's current cloud.  The face image is the renderer's, made by the renderer's
// kernels on fb.cloud where it lies (3 x V interleaved doubles per frame: the renderer's own layout); launch sequence, every
// kernel batched over the launch's frames (which start at fb.f0; the scratch is indexed by absolute frame):
//   memset          the frames' face images to -1
//   k_rend_project  projected vertices
//   k_occ_faces     per face: the sort key (face_key: k_rend_faces' expression without its normal) and the back-face flag;
//                   few frames, first ICP iteration: the scatter pass of the data bucketing in trailing workgroups, as in
//                   k_visibility (frame batches: it rides in k_compact, as behind k_visibility_frame)
//   k_rend_sort     painter order (k_paint_rank + k_rend_scatter above REND_SORT_CAP faces)
//   k_rend_cover    renderFaces' coverage: atomicMax of the painter position
//   k_occ_mark      per pixel: painter position -> face -> the three vertices of a front-facing face, in fb.visible and, through
//                   dm.part_pos, in fb.vis_sorted (same-value byte stores, like k_visibility's).  A pixel that equals its left
//                   neighbour or the pixel above it has nothing new to say: by induction over (row, column) some pixel of the
//                   same value with neither is reached, so a face's stores are issued once per run of rows it starts, not per pixel.
//                   (Measured against the alternative - pixels set a per-face seen byte, a per-face pass marks the vertices - the
//                   two are equal within the noise, 0.318 ms per frame and 1.06 ms per 64 frames at 1280 x 720 either way: this
//                   one is a launch and a memset fewer.)
// No allocation, no host wait, no memset whose size depends on data: the sequence is capturable.
// =====================================================================================================================
__global__ __launch_bounds__(256) void k_occ_faces(DeviceModel dm, FrameBuffers fb, float* __restrict__ fkey, unsigned char* __restrict__ front, int nfb) {
    const int F = dm.d.F, V = dm.d.V;
    const int fl = blockIdx.y, f = fl + fb.f0;
    if ((int)blockIdx.x >= nfb) { bucket_scatter_block<false>(dm, fb, f, (int)blockIdx.x - nfb); return; }
    const int face = blockIdx.x * 256 + threadIdx.x;
    if (face >= F) return;
    const double* cl = fb.cloud + (size_t)f * 3 * V;
    const double* p1 = cl + 3 * (size_t)dm.mesh[face];
    const double* p2 = cl + 3 * (size_t)dm.mesh[(size_t)F + face];
    const double* p3 = cl + 3 * (size_t)dm.mesh[2 * (size_t)F + face];
    const double ax = p2[0] - p1[0], ay = p2[1] - p1[1], bx = p1[0] - p3[0], by = p1[1] - p3[1];
    const double z = __dsub_rn(__dmul_rn(ax, by), __dmul_rn(ay, bx));  // k_visibility's test: no FMA
    const size_t o = (size_t)fl * F + face;
    fkey[o] = face_key(p1, p2, p3);
    front[o] = z > 1e-4 ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_occ_mark(DeviceModel dm, FrameBuffers fb, const int* __restrict__ faces, const int* __restrict__ order,
                                                  const unsigned char* __restrict__ front, int width, int height) {
    const int F = dm.d.F, V = dm.d.V;
    const int fl = blockIdx.y, f = fl + fb.f0;
    const size_t npix = (size_t)width * height;
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= npix) return;
    const int* im = faces + (size_t)fl * npix;
    const int pos = im[o];
    if (pos < 0 || pos >= F) return;                                  // background
    if (o % width != 0 && im[o - 1] == pos) return;
    if (o >= (size_t)width && im[o - width] == pos) return;
    const int face = order[(size_t)fl * F + pos];
    if (!front[(size_t)fl * F + face]) return;                        // a back-facing winner marks nothing and hides what lies behind it
    const int i1 = dm.mesh[face], i2 = dm.mesh[(size_t)F + face], i3 = dm.mesh[2 * (size_t)F + face];
    unsigned char* vis = fb.visible + (size_t)f * V;
    vis[i1] = 1; vis[i2] = 1; vis[i3] = 1;
    if (dm.part_pos) {
        unsigned char* vs = fb.vis_sorted + (size_t)f * V;
        vs[dm.part_pos[i1]] = 1; vs[dm.part_pos[i2]] = 1; vs[dm.part_pos[i3]] = 1;
    }
}

void launch_visibility_render(avt_ctx* c, int nframes, bool with_bucket_scatter) {
    const int V = c->dm.d.V, F = c->dm.d.F, W = c->occ_w, H = c->occ_h, f0 = c->fb.f0;
    const size_t npix = (size_t)W * H;
    hipStream_t s = c->cur_stream;
    int* faces = c->occ_faces + (size_t)f0 * npix;
    int* order = c->occ_order + (size_t)f0 * F;
    int* rank = c->occ_rank + (size_t)f0 * F;
    float* fkey = c->occ_fkey + (size_t)f0 * F;
    float2* proj = (float2*)c->occ_proj.p + (size_t)f0 * V;
    unsigned char* front = c->occ_front + (size_t)f0 * F;
    const bool few = avt_nn_few(c, nframes);
    const int nfb = (F + 255) / 256, vb = (V + 255) / 256;
    const int nb = (with_bucket_scatter && few) ? std::max(1, (c->launch_maxN + BUCKET_TILE - 1) / BUCKET_TILE) : 0;
    c->scatter_in_compact = with_bucket_scatter && !few;              // frame batches: k_compact follows and takes the scatter workgroups
    const double fx = c->occ_fx, fy = c->occ_fy, cx = c->occ_cx, cy = c->occ_cy;   // float intrinsics promoted (AvatarRenderer.cpp:16-19)
    (void)hipMemsetAsync(faces, 0xFF, (size_t)nframes * npix * sizeof(int), s);   // -1
    hipLaunchKernelGGL(k_rend_project, dim3(vb, nframes), dim3(256), 0, s, c->fb.cloud + (size_t)f0 * 3 * V, (const double*)nullptr, proj, (float2*)nullptr, V, 0,
                       fx, fy, cx, cy);
    hipLaunchKernelGGL(k_occ_faces, dim3(nfb + nb, nframes), dim3(256), 0, s, c->dm, c->fb, fkey, front, nfb);
    if (F <= REND_SORT_CAP) {      // (the rank count instead, measured: 0.89 against 0.32 ms for one frame, 4.1 against 1.1 ms for 64)
        hipLaunchKernelGGL(k_rend_sort, dim3(nframes), dim3(1024), 0, s, F, fkey, order, rank);
    } else {
        hipLaunchKernelGGL(k_paint_rank, dim3(nfb, nframes), dim3(256), 0, s, F, fkey, rank);
        hipLaunchKernelGGL(k_rend_scatter, dim3(nfb, nframes), dim3(256), 0, s, F, rank, order);
    }
    RendImgs im{nullptr, nullptr, nullptr, faces};
    hipLaunchKernelGGL(k_rend_cover, dim3(nfb, nframes), dim3(256), 0, s, proj, c->dm.mesh, rank, front, im, V, F, W, H);
    hipLaunchKernelGGL(k_occ_mark, dim3((unsigned)((npix + 255) / 256), nframes), dim3(256), 0, s, c->dm, c->fb, faces, order, front, W, H);
}

struct avt_renderer {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    int V = 0, F = 0, J = 0, W = 0, H = 0, cap = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    int ordering = 0;
    int n_images = 0, rendered = 0;                 // resident avatars; AVT_RENDER_* bits of the last run
    std::vector<int> mesh_soa, main_joint;
    std::vector<char> has_joints;
    DevBuf<int> d_mesh, d_vf_start, d_vf, d_vpart;
    DevBuf<double> d_cloud, d_joints, d_fnorm, d_vnorm;
    DevBuf<float2> d_proj, d_jproj;
    DevBuf<float> d_fkey, d_lam;
    DevBuf<unsigned char> d_fflag;
    DevBuf<int> d_order, d_rank;
    DevBuf<unsigned> d_dkey, d_mkey, d_lkey;
    DevBuf<int> d_faces;
    DevBuf<float> d_depth;
    DevBuf<unsigned char> d_mask, d_lambert;
};

namespace {

// every buffer is allocated once, at its full size for max_images.  No kernel in this file is known to read the 16 bytes of
// slack behind each (none uses vector loads); they stay so that the byte counts handed to hipMalloc do not change
template <class T>
int rd_alloc(DevBuf<T>& b, size_t n) { return b.reserve(n, 16); }

int rd_create(int device, const avt_model* m, int W, int H, float fx, float fy, float cx, float cy, int cap, avt_renderer** out) {
    if (!m || !out || W <= 0 || H <= 0 || cap <= 0 || (long long)W * H >= (1ll << 31) || (long long)W * H * cap >= (1ll << 40)) {
        avt_set_error("avt_renderer_create: bad arguments (model, width, height, max_images > 0)");
        return 1;
    }
    const int V = m->d.V, F = m->d.F, J = m->d.J;
    if (F <= 0 || V <= 0 || F >= (1 << 30)) { avt_set_error("avt_renderer_create: the model has no faces"); return 1; }
    AVT_HIP(hipSetDevice(device));
    avt_renderer* r = new avt_renderer();
    r->device = device; r->V = V; r->F = F; r->J = J; r->W = W; r->H = H; r->cap = cap;
    r->fx = fx; r->fy = fy; r->cx = cx; r->cy = cy;
    r->mesh_soa = m->mesh_soa; r->main_joint = m->main_joint;
    r->has_joints.assign((size_t)cap, 0);
    // vertex -> incident faces, one entry per face slot (counting sort by vertex, faces ascending within a vertex)
    std::vector<int> start((size_t)V + 1, 0), vf((size_t)3 * F);
    for (int k = 0; k < 3; ++k) for (int f = 0; f < F; ++f) ++start[(size_t)r->mesh_soa[(size_t)k * F + f] + 1];
    for (int v = 0; v < V; ++v) start[(size_t)v + 1] += start[(size_t)v];
    {
        std::vector<int> fill(start.begin(), start.end() - 1);
        for (int f = 0; f < F; ++f) for (int k = 0; k < 3; ++k) vf[(size_t)fill[(size_t)r->mesh_soa[(size_t)k * F + f]]++] = f;
    }
    auto fail = [&]() { avt_renderer_destroy(r); return 1; };
    if (hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&r->ev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&r->ev_out, hipEventDisableTiming) != hipSuccess) {
        avt_set_error("avt_renderer_create: stream creation failed");
        return fail();
    }
    const size_t ci = (size_t)cap;
    if (rd_alloc(r->d_mesh, (size_t)3 * F) || rd_alloc(r->d_vf_start, (size_t)V + 1) || rd_alloc(r->d_vf, (size_t)3 * F) ||
        rd_alloc(r->d_vpart, (size_t)V) || rd_alloc(r->d_cloud, ci * 3 * V) || rd_alloc(r->d_joints, ci * 3 * (J > 0 ? J : 1)) ||
        rd_alloc(r->d_fnorm, ci * 3 * F) || rd_alloc(r->d_proj, ci * V) || rd_alloc(r->d_jproj, ci * (J > 0 ? J : 1)) ||
        rd_alloc(r->d_fkey, ci * F) || rd_alloc(r->d_lam, ci * V) || rd_alloc(r->d_vnorm, ci * 3 * V) || rd_alloc(r->d_fflag, ci * F) || rd_alloc(r->d_order, ci * F) ||
        rd_alloc(r->d_rank, ci * F))
        return fail();
    hipError_t e = hipMemcpyAsync(r->d_mesh, r->mesh_soa.data(), (size_t)3 * F * sizeof(int), hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_vf_start, start.data(), ((size_t)V + 1) * sizeof(int), hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_vf, vf.data(), (size_t)3 * F * sizeof(int), hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_vpart, r->main_joint.data(), (size_t)V * sizeof(int), hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) e = hipMemsetAsync(r->d_joints, 0, ci * 3 * (J > 0 ? J : 1) * sizeof(double), r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);            // the host tables are on this stack frame
    if (e != hipSuccess) { avt_set_error(std::string("avt_renderer_create: ") + hipGetErrorString(e)); return fail(); }
    *out = r;
    return 0;
}

int rd_set_part_map(avt_renderer* r, int n, const int* map) {
    if (!r || n < 0) { avt_set_error("avt_renderer_set_part_map: bad arguments"); return 1; }
    std::vector<int> vp((size_t)r->V);
    for (int v = 0; v < r->V; ++v) {
        const int j = r->main_joint[(size_t)v];
        if (map && n > 0 && (j < 0 || j >= n)) { avt_set_error("avt_renderer_set_part_map: the part map has fewer entries than the model's joints"); return 1; }
        vp[(size_t)v] = (map && n > 0) ? map[j] : j;
    }
    AVT_HIP(hipSetDevice(r->device));
    AVT_HIP(hipMemcpyAsync(r->d_vpart, vp.data(), (size_t)r->V * sizeof(int), hipMemcpyHostToDevice, r->stream));
    AVT_HIP(hipStreamSynchronize(r->stream));
    return 0;
}

int rd_upload(avt_renderer* r, int n, const double* clouds, const double* joints) {
    if (!r || !clouds || n <= 0 || n > r->cap) { avt_set_error("avt_renderer_upload: bad arguments (1 <= n_images <= max_images)"); return 1; }
    AVT_HIP(hipSetDevice(r->device));
    AVT_HIP(hipMemcpyAsync(r->d_cloud, clouds, (size_t)n * 3 * r->V * sizeof(double), hipMemcpyHostToDevice, r->stream));
    if (joints && r->J > 0) AVT_HIP(hipMemcpyAsync(r->d_joints, joints, (size_t)n * 3 * r->J * sizeof(double), hipMemcpyHostToDevice, r->stream));
    AVT_HIP(hipStreamSynchronize(r->stream));
    for (int i = 0; i < n; ++i) r->has_joints[(size_t)i] = joints ? 1 : 0;
    r->n_images = n; r->rendered = -1;
    return 0;
}

int rd_from_ctx(avt_renderer* r, avt_ctx* c, int n, const int* frames) {
    if (!r || !c || n <= 0 || n > r->cap) { avt_set_error("avt_renderer_from_ctx: bad arguments (1 <= n_images <= max_images)"); return 1; }
    if (c->dm.d.V != r->V || c->dm.d.F != r->F || c->dm.d.J != r->J || c->device != r->device) {
        avt_set_error("avt_renderer_from_ctx: the context's model or device is not the renderer's");
        return 1;
    }
    for (int i = 0; i < n; ++i) {
        const int f = frames ? frames[i] : i;
        if (f < 0 || f >= c->fb.max_frames) { avt_set_error("avt_renderer_from_ctx: frame index out of range"); return 1; }
    }
    AVT_HIP(hipSetDevice(r->device));
    // after everything queued on the context (its side streams join its main stream), and before anything queued on it later
    AVT_HIP(hipEventRecord(r->ev_in, c->stream));
    AVT_HIP(hipStreamWaitEvent(r->stream, r->ev_in, 0));
    const size_t cb = (size_t)3 * r->V * sizeof(double), jb = (size_t)3 * r->J * sizeof(double);
    for (int i = 0; i < n;) {
        const int f = frames ? frames[i] : i;
        int run = 1;                                                   // consecutive frames go in one copy
        while (i + run < n && (frames ? frames[i + run] : i + run) == f + run) ++run;
        AVT_HIP(hipMemcpyAsync(r->d_cloud + (size_t)i * 3 * r->V, c->fb.cloud + (size_t)f * 3 * r->V, run * cb, hipMemcpyDeviceToDevice, r->stream));
        if (r->J > 0)
            AVT_HIP(hipMemcpyAsync(r->d_joints + (size_t)i * 3 * r->J, c->fb.jointpos + (size_t)f * 3 * r->J, run * jb, hipMemcpyDeviceToDevice, r->stream));
        i += run;
    }
    AVT_HIP(hipEventRecord(r->ev_out, r->stream));
    AVT_HIP(hipStreamWaitEvent(c->stream, r->ev_out, 0));
    for (int i = 0; i < n; ++i) r->has_joints[(size_t)i] = 1;
    r->n_images = n; r->rendered = -1;
    return 0;
}

int rd_run(avt_renderer* r, int what) {
    if (!r || r->n_images <= 0) { avt_set_error("avt_renderer_run: no avatars resident"); return 1; }
    if (what & ~(AVT_RENDER_DEPTH | AVT_RENDER_PART_MASK | AVT_RENDER_LAMBERT | AVT_RENDER_FACES)) { avt_set_error("avt_renderer_run: unknown output bits"); return 1; }
    AVT_HIP(hipSetDevice(r->device));
    const int n = r->n_images, V = r->V, F = r->F, J = r->J, W = r->W, H = r->H;
    const size_t npix = (size_t)W * H, tot = npix * n, ci = (size_t)r->cap * npix;
    RendImgs im{nullptr, nullptr, nullptr, nullptr};
    if (what & AVT_RENDER_DEPTH) { if (rd_alloc(r->d_dkey, ci) || rd_alloc(r->d_depth, ci)) return 1; im.dkey = r->d_dkey; }
    if (what & AVT_RENDER_PART_MASK) { if (rd_alloc(r->d_mkey, ci) || rd_alloc(r->d_mask, ci)) return 1; im.mkey = r->d_mkey; }
    if (what & AVT_RENDER_LAMBERT) { if (rd_alloc(r->d_lkey, ci) || rd_alloc(r->d_lambert, ci)) return 1; im.lkey = r->d_lkey; }
    if (what & AVT_RENDER_FACES) { if (rd_alloc(r->d_faces, ci)) return 1; im.faces = r->d_faces; }
    hipStream_t s = r->stream;
    if (im.dkey) AVT_HIP(hipMemsetAsync(im.dkey, 0, tot * sizeof(unsigned), s));
    if (im.mkey) AVT_HIP(hipMemsetAsync(im.mkey, 0, tot * sizeof(unsigned), s));
    if (im.lkey) AVT_HIP(hipMemsetAsync(im.lkey, 0, tot * sizeof(unsigned), s));
    if (im.faces) AVT_HIP(hipMemsetAsync(im.faces, 0xFF, tot * sizeof(int), s));            // -1
    const double fx = r->fx, fy = r->fy, cx = r->cx, cy = r->cy;                           // float intrinsics promoted (AvatarRenderer.cpp:16-19)
    const int vb = (std::max(V, J) + 255) / 256, fb = (F + 255) / 256;
    hipLaunchKernelGGL(k_rend_project, dim3(vb, n), dim3(256), 0, s, r->d_cloud, r->d_joints, r->d_proj, r->d_jproj, V, J, fx, fy, cx, cy);
    hipLaunchKernelGGL(k_rend_faces, dim3(fb, n), dim3(256), 0, s, r->d_cloud, r->d_mesh, V, F, r->d_fkey, r->d_fflag, r->d_fnorm);
    if (r->ordering == 0 && F <= REND_SORT_CAP) {
        hipLaunchKernelGGL(k_rend_sort, dim3(n), dim3(1024), 0, s, F, r->d_fkey, r->d_order, r->d_rank);
    } else {
        hipLaunchKernelGGL(k_paint_rank, dim3(fb, n), dim3(256), 0, s, F, r->d_fkey, r->d_rank);
        hipLaunchKernelGGL(k_rend_scatter, dim3(fb, n), dim3(256), 0, s, F, r->d_rank, r->d_order);
    }
    if (im.lkey)
        hipLaunchKernelGGL(k_rend_vnormal, dim3((V + 255) / 256, n), dim3(256), 0, s, r->d_cloud, r->d_vf_start, r->d_vf, r->d_rank, r->d_fnorm, V, F, r->d_vnorm, r->d_lam);
    if (what) {
        hipLaunchKernelGGL(k_rend_cover, dim3(fb, n), dim3(256), 0, s, r->d_proj, r->d_mesh, r->d_rank, r->d_fflag, im, V, F, W, H);
        if (im.dkey || im.mkey || im.lkey)
            hipLaunchKernelGGL(k_rend_resolve, dim3((unsigned)((npix + 255) / 256), n), dim3(256), 0, s, r->d_cloud, r->d_proj, r->d_mesh, r->d_order, r->d_fflag,
                               r->d_lam, r->d_vpart, im, r->d_depth, r->d_mask, r->d_lambert, V, F, W, H);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { avt_set_error(std::string("avt_renderer_run: launch failed: ") + hipGetErrorString(e)); return 1; }
    r->rendered = what;
    return 0;
}

int rd_download(avt_renderer* r, int image, float* depth, unsigned char* mask, unsigned char* lam, int* faces) {
    if (!r || image < 0 || image >= r->n_images || r->rendered < 0) { avt_set_error("avt_renderer_download: bad image, or no run since the avatars changed"); return 1; }
    if ((depth && !(r->rendered & AVT_RENDER_DEPTH)) || (mask && !(r->rendered & AVT_RENDER_PART_MASK)) || (lam && !(r->rendered & AVT_RENDER_LAMBERT)) ||
        (faces && !(r->rendered & AVT_RENDER_FACES))) {
        avt_set_error("avt_renderer_download: an image the last run did not render was asked for");
        return 1;
    }
    AVT_HIP(hipSetDevice(r->device));
    const size_t npix = (size_t)r->W * r->H, o = (size_t)image * npix;
    if (depth) AVT_HIP(hipMemcpyAsync(depth, r->d_depth + o, npix * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    if (mask) AVT_HIP(hipMemcpyAsync(mask, r->d_mask + o, npix, hipMemcpyDeviceToHost, r->stream));
    if (lam) AVT_HIP(hipMemcpyAsync(lam, r->d_lambert + o, npix, hipMemcpyDeviceToHost, r->stream));
    if (faces) AVT_HIP(hipMemcpyAsync(faces, r->d_faces + o, npix * sizeof(int), hipMemcpyDeviceToHost, r->stream));
    AVT_HIP(hipStreamSynchronize(r->stream));
    return 0;
}

int rd_projection(avt_renderer* r, int image, float* pts, float* jts, float* keys, int* faces, int* face_pos) {
    if (!r || image < 0 || image >= r->n_images || r->rendered < 0) { avt_set_error("avt_renderer_projection: bad image, or no run since the avatars changed"); return 1; }
    if (jts && !r->has_joints[(size_t)image]) { avt_set_error("avt_renderer_projection: no joints were given for this image"); return 1; }
    AVT_HIP(hipSetDevice(r->device));
    const int F = r->F;
    std::vector<int> order((size_t)F);
    std::vector<float> fk((size_t)F);
    if (pts) AVT_HIP(hipMemcpyAsync(pts, r->d_proj + (size_t)image * r->V, (size_t)r->V * sizeof(float2), hipMemcpyDeviceToHost, r->stream));
    if (jts && r->J > 0) AVT_HIP(hipMemcpyAsync(jts, r->d_jproj + (size_t)image * r->J, (size_t)r->J * sizeof(float2), hipMemcpyDeviceToHost, r->stream));
    if (face_pos) AVT_HIP(hipMemcpyAsync(face_pos, r->d_rank + (size_t)image * F, (size_t)F * sizeof(int), hipMemcpyDeviceToHost, r->stream));
    if (keys || faces) {
        AVT_HIP(hipMemcpyAsync(order.data(), r->d_order + (size_t)image * F, (size_t)F * sizeof(int), hipMemcpyDeviceToHost, r->stream));
        AVT_HIP(hipMemcpyAsync(fk.data(), r->d_fkey + (size_t)image * F, (size_t)F * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    }
    AVT_HIP(hipStreamSynchronize(r->stream));
    for (int p = 0; p < F && (keys || faces); ++p) {
        const int f = order[(size_t)p];
        if (f < 0 || f >= F) { avt_set_error("avt_renderer_projection: the painter order is not a permutation"); return AVT_STATUS_DEVICE_FAULT; }
        if (keys) keys[p] = fk[(size_t)f];
        if (faces) for (int k = 0; k < 3; ++k) faces[3 * (size_t)p + k] = r->mesh_soa[(size_t)k * F + f];
    }
    return 0;
}

int rd_shading(avt_renderer* r, int image, double* normals, float* lam) {
    if (!r || image < 0 || image >= r->n_images || r->rendered < 0 || !(r->rendered & AVT_RENDER_LAMBERT)) {
        avt_set_error("avt_renderer_vertex_shading: bad image, or the last run did not render the Lambert image");
        return 1;
    }
    AVT_HIP(hipSetDevice(r->device));
    const size_t V = (size_t)r->V;
    if (normals) AVT_HIP(hipMemcpyAsync(normals, r->d_vnorm + (size_t)image * 3 * V, 3 * V * sizeof(double), hipMemcpyDeviceToHost, r->stream));
    if (lam) AVT_HIP(hipMemcpyAsync(lam, r->d_lam + (size_t)image * V, V * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    AVT_HIP(hipStreamSynchronize(r->stream));
    return 0;
}

}  // namespace

extern "C" {
int avt_renderer_create(int device, const avt_model* m, int width, int height, float fx, float fy, float cx, float cy, int max_images,
                        avt_renderer** out) {
    return avt_guard("avt_renderer_create", [&]() -> int { return rd_create(device, m, width, height, fx, fy, cx, cy, max_images, out); });
}

void avt_renderer_destroy(avt_renderer* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    // the buffers go with `delete`, after the events and the stream: the stream has just been drained, so nothing is queued on them either way
    if (r->ev_in) (void)hipEventDestroy(r->ev_in);
    if (r->ev_out) (void)hipEventDestroy(r->ev_out);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
}

int avt_renderer_set_part_map(avt_renderer* r, int n_joints, const int* part_map) {
    return avt_guard("avt_renderer_set_part_map", [&]() -> int { return rd_set_part_map(r, n_joints, part_map); });
}
int avt_renderer_upload(avt_renderer* r, int n_images, const double* clouds, const double* joints) {
    return avt_guard("avt_renderer_upload", [&]() -> int { return rd_upload(r, n_images, clouds, joints); });
}
int avt_renderer_from_ctx(avt_renderer* r, avt_ctx* c, int n_images, const int* frames) {
    return avt_guard("avt_renderer_from_ctx", [&]() -> int { return rd_from_ctx(r, c, n_images, frames); });
}
int avt_renderer_run(avt_renderer* r, int what) { return avt_guard("avt_renderer_run", [&]() -> int { return rd_run(r, what); }); }
int avt_renderer_download(avt_renderer* r, int image, float* depth, unsigned char* part_mask, unsigned char* lambert, int* faces) {
    return avt_guard("avt_renderer_download", [&]() -> int { return rd_download(r, image, depth, part_mask, lambert, faces); });
}
int avt_renderer_projection(avt_renderer* r, int image, float* points_2xV, float* joints_2xJ, float* face_keys, int* faces_3xF, int* face_pos) {
    return avt_guard("avt_renderer_projection", [&]() -> int { return rd_projection(r, image, points_2xV, joints_2xJ, face_keys, faces_3xF, face_pos); });
}
int avt_renderer_vertex_shading(avt_renderer* r, int image, double* normals_3xV, float* lambert_v) {
    return avt_guard("avt_renderer_vertex_shading", [&]() -> int { return rd_shading(r, image, normals_3xV, lambert_v); });
}
int avt_renderer_sync(avt_renderer* r) {
    if (!r) { avt_set_error("avt_renderer_sync: null handle"); return 1; }
    const hipError_t e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) { avt_set_error(std::string("avt_renderer_sync: ") + hipGetErrorString(e)); return 1; }
    return 0;
}
int avt_renderer_set_ordering(avt_renderer* r, int ordering) {
    if (!r || (ordering != 0 && ordering != 1)) { avt_set_error("avt_renderer_set_ordering: bad arguments (0 = sort, 1 = rank count)"); return 1; }
    r->ordering = ordering;
    return 0;
}
}  // extern "C"

// The forest trainer's device-to-device path (avt_rtree_train.cpp): the last run's depth and part-mask images of all resident
// avatars, made visible to stream `s` after everything queued on the renderer.  The caller waits for its own work on `s`
// before the renderer may run again (avt_rtree_trainer_add_rendered and avt_rtree_transfer_rendered return after it).
int avt_renderer_images_for(avt_renderer* r, hipStream_t s, const float** depth, const unsigned char** mask, int* n, int* width, int* height) {
    if (!r || r->n_images <= 0 || r->rendered < 0 || !(r->rendered & AVT_RENDER_DEPTH) || !(r->rendered & AVT_RENDER_PART_MASK)) {
        avt_set_error("renderer: the last run rendered no depth and part mask (avt_renderer_run(r, AVT_RENDER_DEPTH | AVT_RENDER_PART_MASK))");
        return 1;
    }
    AVT_HIP(hipSetDevice(r->device));
    AVT_HIP(hipEventRecord(r->ev_out, r->stream));
    AVT_HIP(hipStreamWaitEvent(s, r->ev_out, 0));
    *depth = r->d_depth; *mask = r->d_mask; *n = r->n_images; *width = r->W; *height = r->H;
    return 0;
}
