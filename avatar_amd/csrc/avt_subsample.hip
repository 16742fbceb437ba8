// avt_subsample.hip — the trackers' interval subsampling (demo.cpp:216-250) for a batch of label images, from device memory
// into device memory: labels behind a forest handle, XYZ maps behind the background subtractor, frame slots of a context.
// The rule is in include/avt_subsample.h.  gfx950, wave64.
//
//   k_sub_count     one workgroup per chunk of AVT_SUBSAMPLE_CHUNK consecutive grid pixels of one image: keep flags by ballot /
//                   popcount, the chunk's count, the per-part counts through an LDS histogram, the bad-label flag
//   k_sub_scan      one workgroup per image: exclusive scan of its chunk counts, AVT_SUBSAMPLE_SCAN_WIDTH per pass; the total and
//                   the overflow flag
//   k_sub_emit      the flags again, the position inside the chunk by wave prefix, three doubles and an int per kept pixel
//   k_sub_centroid  one lane per (image, coordinate): the sum in frame order, one division
// The same ordered compaction as the synthetic frame generator's (k_raster_label / _scan / _emit, avt_render.hip), on a grid
// with a box and an interval per image.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/avt_subsample.h"
#include "avt_bgsub_internal.h"
#include "avt_host.h"
#include "avt_internal.h"
#include "avt_rforest.h"
#include "avt_rtree.h"

#define SUB_CHUNK AVT_SUBSAMPLE_CHUNK
#define SUB_SCAN AVT_SUBSAMPLE_SCAN_WIDTH
#define SUB_BAD_LABEL 1u          // a kept label >= num_parts
#define SUB_OVERFLOW 2u           // more kept pixels than a frame slot holds
static_assert(SUB_CHUNK == 256 && SUB_SCAN == 256, "both kernels' workgroups are four waves of 64");

namespace {

__device__ __forceinline__ int sub_lane() { return threadIdx.x & 63; }
__device__ __forceinline__ int sub_wave() { return threadIdx.x >> 6; }

struct SubGeo { int tlx, tly, gw, G; };      // the grid of one image: its origin, its width and its pixels (0: none)

// image img's box and interval; a box that is empty or not inside the image has no grid pixel.  G < 2^30 (rows x cols is)
__device__ __forceinline__ SubGeo sub_geo(const int* __restrict__ boxes, int box_stride, const int* __restrict__ intervals, int img, int rows, int cols,
                                          int& iv) {
    const int* b = boxes + (size_t)img * box_stride;
    const int tlx = b[0], tly = b[1], brx = b[2], bry = b[3];
    iv = intervals[img];
    SubGeo g = {tlx, tly, 0, 0};
    if (iv < 1 || tlx < 0 || tly < 0 || tlx > brx || tly > bry || brx >= cols || bry >= rows) return g;
    g.gw = (brx - tlx) / iv + 1;
    g.G = ((bry - tly) / iv + 1) * g.gw;
    return g;
}

// the label of grid pixel p of the image (p < g.G), and where it lies in the image
__device__ __forceinline__ unsigned char sub_label(const unsigned char* __restrict__ labels, const SubGeo& g, int iv, int img, int rows, int cols, int p,
                                                   size_t& pix) {
    const int i = p / g.gw, j = p - i * g.gw;
    pix = (size_t)img * rows * cols + (size_t)(g.tly + i * iv) * cols + (g.tlx + j * iv);      // row <= br.y < rows, column <= br.x < cols
    return labels[pix];
}

__global__ __launch_bounds__(SUB_CHUNK) void k_sub_count(const unsigned char* __restrict__ labels, const int* __restrict__ boxes, int box_stride,
                                                         const int* __restrict__ intervals, int rows, int cols, int num_parts,
                                                         int* __restrict__ block_count, int max_chunks, int* __restrict__ counts,
                                                         unsigned* __restrict__ status) {
    const int img = blockIdx.y, t = threadIdx.x;
    int iv;
    const SubGeo g = sub_geo(boxes, box_stride, intervals, img, rows, cols, iv);
    const int base = blockIdx.x * SUB_CHUNK;
    if (base >= g.G) return;                                   // uniform: the whole workgroup leaves
    __shared__ int s_hist[256];
    __shared__ int s_c[SUB_CHUNK / 64];
    s_hist[t] = 0;
    __syncthreads();
    const int p = base + t;
    bool keep = false;
    if (p < g.G) {
        size_t pix;
        const unsigned char lab = sub_label(labels, g, iv, img, rows, cols, p, pix);
        keep = lab != 255;
        if (keep) atomicAdd(&s_hist[lab], 1);
    }
    const unsigned long long bal = __ballot(keep);
    if (sub_lane() == 0) s_c[sub_wave()] = __popcll(bal);
    __syncthreads();
    if (t == 0) block_count[(size_t)img * max_chunks + blockIdx.x] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
    const int h = s_hist[t];
    if (h > 0 && t != 255) {
        if (t < num_parts) atomicAdd(&counts[(size_t)img * (1 + num_parts) + 1 + t], h);     // one integer atomic per (workgroup, part)
        else atomicOr(&status[img], SUB_BAD_LABEL);
    }
}

// also publishes the box it used: what the host hands back as boxes_out
__global__ __launch_bounds__(SUB_SCAN) void k_sub_scan(const int* __restrict__ boxes, int box_stride, const int* __restrict__ intervals, int rows, int cols,
                                                       int num_parts, int* __restrict__ block_count, int max_chunks, int max_points,
                                                       int* __restrict__ counts, unsigned* __restrict__ status, int* __restrict__ boxes_used) {
    const int img = blockIdx.x, t = threadIdx.x;
    int iv;
    const SubGeo g = sub_geo(boxes, box_stride, intervals, img, rows, cols, iv);
    const int nchunks = (g.G + SUB_CHUNK - 1) / SUB_CHUNK;     // <= max_chunks: the host sized it from the whole image at this interval
    int* bc = block_count + (size_t)img * max_chunks;
    __shared__ int s_w[SUB_SCAN / 64];
    __shared__ int s_run;
    if (t == 0) s_run = 0;
    if (t < 4) boxes_used[4 * (size_t)img + t] = boxes[(size_t)img * box_stride + t];
    __syncthreads();
    for (int b0 = 0; b0 < nchunks; b0 += SUB_SCAN) {
        const int i = b0 + t;
        const int v = i < nchunks ? bc[i] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(incl, d, 64);
            if (sub_lane() >= d) incl += u;
        }
        if (sub_lane() == 63) s_w[sub_wave()] = incl;
        __syncthreads();
        int off = s_run;
        for (int w = 0; w < sub_wave(); ++w) off += s_w[w];
        if (i < nchunks) bc[i] = off + incl - v;
        __syncthreads();
        if (t == SUB_SCAN - 1) s_run = off + incl;
        __syncthreads();
    }
    if (t == 0) {
        counts[(size_t)img * (1 + num_parts)] = s_run;        // <= G < 2^30
        if (s_run > max_points) atomicOr(&status[img], SUB_OVERFLOW);
    }
}

__global__ __launch_bounds__(SUB_CHUNK) void k_sub_emit(const unsigned char* __restrict__ labels, const float* __restrict__ xyz,
                                                        const int* __restrict__ boxes, int box_stride, const int* __restrict__ intervals, int rows,
                                                        int cols, const int* __restrict__ block_off, int max_chunks, int max_points,
                                                        double* __restrict__ data_raw, int* __restrict__ labels_raw) {
    const int img = blockIdx.y, t = threadIdx.x;
    int iv;
    const SubGeo g = sub_geo(boxes, box_stride, intervals, img, rows, cols, iv);
    const int base = blockIdx.x * SUB_CHUNK;
    if (base >= g.G) return;
    const int p = base + t;
    bool keep = false;
    unsigned char lab = 255;
    size_t pix = 0;
    if (p < g.G) { lab = sub_label(labels, g, iv, img, rows, cols, p, pix); keep = lab != 255; }
    const unsigned long long bal = __ballot(keep);
    __shared__ int s_c[SUB_CHUNK / 64];
    if (sub_lane() == 0) s_c[sub_wave()] = __popcll(bal);
    __syncthreads();
    if (!keep) return;
    int pos = block_off[(size_t)img * max_chunks + blockIdx.x] + __popcll(bal & ((1ull << sub_lane()) - 1ull));
    for (int w = 0; w < sub_wave(); ++w) pos += s_c[w];
    if (pos >= max_points) return;                             // never past the slot: the call fails on the overflow flag
    const float* s = xyz + 3 * pix;
    const float x = s[0], y = s[1], z = s[2];
    double* d = data_raw + 3 * ((size_t)img * max_points + pos);
    d[0] = (double)x; d[1] = -(double)y; d[2] = (double)z;     // widened, then negated (demo.cpp:245)
    labels_raw[(size_t)img * max_points + pos] = (int)lab;
}

// s = 0; for k: s += data[3 k + c]; s / n - the order is the definition (demo.cpp:253), so one lane walks one coordinate
__global__ __launch_bounds__(64) void k_sub_centroid(const int* __restrict__ want, const int* __restrict__ counts, const unsigned* __restrict__ status,
                                                     int n, int num_parts, int max_points, const double* __restrict__ data_raw,
                                                     double* __restrict__ centroid) {
    const int tid = blockIdx.x * 64 + threadIdx.x;
    if (tid >= 3 * n) return;
    const int img = tid / 3, c = tid - 3 * img;
    if (!want[img] || status[img]) return;
    const int N = counts[(size_t)img * (1 + num_parts)];
    if (N <= 0 || N > max_points) return;
    const double* d = data_raw + 3 * (size_t)img * max_points + c;
    double s = 0.0;
    int k = 0;
    for (; k + 8 <= N; k += 8) {                               // eight loads in flight, the additions in order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = d[3 * (size_t)(k + u)];
#pragma unroll
        for (int u = 0; u < 8; ++u) s = __dadd_rn(s, v[u]);
    }
    for (; k < N; ++k) s = __dadd_rn(s, d[3 * (size_t)k]);
    centroid[tid] = __ddiv_rn(s, (double)N);
}

int grow_scratch(avt_ctx* c, size_t n_block, size_t n_in, size_t n_out) {
    AvtSubState& st = c->sub;
    if (n_block <= st.block.cap && n_in <= st.in.cap && n_out <= st.out.cap) return 0;
    AVT_HIP(hipStreamSynchronize(c->stream));                  // what is queued on the old blocks drains before they go
    return st.block.reserve(n_block) || st.in.reserve(n_in) || st.out.reserve(n_out);
}

// h: the labelling handle (avt_label.h) of a tree or a forest
int subsample_impl(avt_ctx* c, AvtLabelHandle* h, avt_bgsub* bg, const char* who, const int* boxes, const int* intervals, const unsigned char* want_centroid,
                   int* counts_out, double* centroid_out, int* boxes_out) {
    const std::string w(who);
    if (!c) { avt_set_error(w + ": null context"); return 1; }
    if (!h) { avt_set_error(w + ": null forest handle"); return 1; }
    if (!bg) { avt_set_error(w + ": null background subtractor"); return 1; }
    if (!intervals || !counts_out) { avt_set_error(w + ": null argument (intervals, counts_out)"); return 1; }
    if (h->device < 0) { avt_set_error(w + ": the forest handle was created host-only (device < 0)"); return 1; }
    if (h->n_labels <= 0) { avt_set_error(w + ": no labelled images behind the handle"); return 1; }
    avt_bgsub_view v;
    if (!boxes) {
        if (avt_bgsub_last_run(bg, &v)) return 1;
    } else {
        bool ran = false;
        if (avt_bgsub_resident(bg, &v, &ran)) { avt_set_error(w + ": no XYZ maps resident behind the background subtractor (an upload first)"); return 1; }
    }
    if (v.device != h->device || v.device != c->device) { avt_set_error(w + ": the context, the handle and the background subtractor are on different devices"); return 1; }
    const int n = h->n_labels, rows = h->rows, cols = h->cols, P = c->dm.d.num_parts, max_points = c->fb.max_points;
    if (n != v.n_images || rows != v.rows || cols != v.cols) {
        avt_set_error(w + (boxes ? ": the labels behind the handle do not match the background subtractor's images in number or size"
                                 : ": the labels behind the handle are not those of the background subtractor's last run"));
        return 1;
    }
    if (n > c->fb.max_frames) { avt_set_error(w + ": more images than the context has frame slots (max_frames)"); return 1; }
    bool any_centroid = false;
    for (int i = 0; i < n; ++i) any_centroid = any_centroid || (want_centroid && want_centroid[i]);
    if (any_centroid && !centroid_out) { avt_set_error(w + ": centroids asked for without centroid_out"); return 1; }
    // what goes up: intervals | centroid flags | host boxes.  Everything is checked before anything is queued.
    AvtSubState& st = c->sub;
    std::vector<int>& in = st.h_in;
    in.assign(6 * (size_t)n, 0);
    long long max_chunks = 1;
    for (int i = 0; i < n; ++i) {
        const int iv = intervals[i];
        if (iv < 1) { avt_set_error(w + ": interval < 1 (image " + std::to_string(i) + ")"); return 1; }
        in[i] = iv;
        in[n + i] = (want_centroid && want_centroid[i]) ? 1 : 0;
        const long long whole = (long long)((rows + iv - 1) / iv) * ((cols + iv - 1) / iv);     // no box has more grid pixels
        max_chunks = std::max(max_chunks, (whole + SUB_CHUNK - 1) / SUB_CHUNK);
        if (!boxes) continue;
        int* q = &in[2 * (size_t)n + 4 * (size_t)i];
        for (int k = 0; k < 4; ++k) q[k] = boxes[4 * (size_t)i + k];
        if (q[2] == -1) { q[0] = q[1] = 0; q[2] = cols - 1; q[3] = rows - 1; }
        if (q[0] > q[2] || q[1] > q[3]) continue;              // an empty box: a frame of 0 points
        if (q[0] < 0 || q[1] < 0 || q[2] >= cols || q[3] >= rows) { avt_set_error(w + ": bad region of interest (image " + std::to_string(i) + ")"); return 1; }
    }
    if ((long long)rows * cols >= (1ll << 30) || max_chunks > 0x7fffffffll / std::max(n, 1)) { avt_set_error(w + ": images too large"); return 1; }
    AVT_HIP(hipSetDevice(c->device));
    const size_t out_ints = (size_t)n * (1 + P) + n + 4 * (size_t)n, out_doubles = 3 * (size_t)n + (out_ints + 1) / 2;
    if (grow_scratch(c, (size_t)n * max_chunks, in.size(), out_doubles)) return 1;
    if (!st.ev_labels) AVT_HIP(hipEventCreateWithFlags(&st.ev_labels, hipEventDisableTiming));
    // the slots are about to be overwritten: nothing is resident from here on, whatever happens
    if (c->frames_valid) st.prev_nframes = c->nframes;
    else if (!st.pending) st.prev_nframes = -1;
    c->frames_valid = false;
    st.pending = false;
    c->have_moments = c->have_records = false;
    c->results_fresh = false;
    hipStream_t s = c->stream;
    // the context's stream waits for the labels (the handle's stream) and for the XYZ maps and boxes (bg's stream); bg's next
    // upload / run / destroy waits for this stage.  The handle needs no such wait: this call returns after its one host wait.
    AVT_HIP(hipEventRecord(st.ev_labels, h->stream));
    AVT_HIP(hipStreamWaitEvent(s, st.ev_labels, 0));
    if (avt_bgsub_reader_begin(bg, s)) return 1;
    double* d_cent = st.out;
    int* d_counts = reinterpret_cast<int*>(d_cent + 3 * (size_t)n);
    unsigned* d_status = reinterpret_cast<unsigned*>(d_counts + (size_t)n * (1 + P));
    int* d_used = d_counts + (size_t)n * (1 + P) + n;
    const int* d_iv = st.in;
    const int* d_want = st.in + n;
    const int* d_boxes = boxes ? st.in + 2 * (size_t)n : v.d_boxes;
    const int stride = boxes ? 4 : v.box_stride;
    hipError_t e = hipMemcpyAsync(st.in, in.data(), in.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_cent, 0, out_doubles * sizeof(double), s);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)max_chunks, (unsigned)n);
        hipLaunchKernelGGL(k_sub_count, grid, dim3(SUB_CHUNK), 0, s, h->d_labels, d_boxes, stride, d_iv, rows, cols, P, st.block, (int)max_chunks, d_counts,
                           d_status);
        hipLaunchKernelGGL(k_sub_scan, dim3(n), dim3(SUB_SCAN), 0, s, d_boxes, stride, d_iv, rows, cols, P, st.block, (int)max_chunks, max_points, d_counts,
                           d_status, d_used);
        hipLaunchKernelGGL(k_sub_emit, grid, dim3(SUB_CHUNK), 0, s, h->d_labels, v.d_xyz, d_boxes, stride, d_iv, rows, cols, st.block, (int)max_chunks,
                           max_points, c->fb.data_raw, c->fb.labels_raw);
        if (any_centroid)
            hipLaunchKernelGGL(k_sub_centroid, dim3((3 * n + 63) / 64), dim3(64), 0, s, d_want, d_counts, d_status, n, P, max_points, c->fb.data_raw, d_cent);
        e = hipGetLastError();
    }
    st.h_out.assign(out_doubles, 0.0);
    if (e == hipSuccess) e = hipMemcpyAsync(st.h_out.data(), d_cent, out_doubles * sizeof(double), hipMemcpyDeviceToHost, s);
    const int rc_end = avt_bgsub_reader_end(bg, s);
    const hipError_t es = hipStreamSynchronize(s);             // the one host wait of the call
    if (e != hipSuccess || es != hipSuccess) { avt_set_error(w + ": " + hipGetErrorString(e != hipSuccess ? e : es)); return 1; }
    if (rc_end) return 1;
    const int* h_counts = reinterpret_cast<const int*>(st.h_out.data() + 3 * (size_t)n);
    const unsigned* h_status = reinterpret_cast<const unsigned*>(h_counts + (size_t)n * (1 + P));
    const int* h_used = h_counts + (size_t)n * (1 + P) + n;
    for (int i = 0; i < n; ++i) {
        if (h_status[i] & SUB_BAD_LABEL) {
            avt_set_error(w + ": body part label out of range (neither 255 nor < num_parts) in image " + std::to_string(i) + " (demo.cpp:236-243); no frame is resident");
            return 1;
        }
        if (h_status[i] & SUB_OVERFLOW) {
            avt_set_error(w + ": image " + std::to_string(i) + " keeps " + std::to_string(h_counts[(size_t)i * (1 + P)]) +
                          " points, more than max_points_per_frame; no frame is resident");
            return 1;
        }
    }
    std::memcpy(counts_out, h_counts, (size_t)n * (1 + P) * sizeof(int));
    if (boxes_out) std::memcpy(boxes_out, h_used, 4 * (size_t)n * sizeof(int));
    st.counts.resize(n);
    for (int i = 0; i < n; ++i) {
        st.counts[i] = h_counts[(size_t)i * (1 + P)];
        if (in[n + i] && st.counts[i] > 0) std::memcpy(centroid_out + 3 * (size_t)i, st.h_out.data() + 3 * (size_t)i, 3 * sizeof(double));
    }
    st.pending = true;
    return 0;
}

int commit_impl(avt_ctx* c, const unsigned char* keep) {
    if (!c) { avt_set_error("avt_frames_subsample_commit: null context"); return 1; }
    AvtSubState& st = c->sub;
    if (!st.pending || c->frames_valid) { avt_set_error("avt_frames_subsample_commit: nothing pending (a subsample call first)"); return 1; }
    AVT_HIP(hipSetDevice(c->device));
    const int n = (int)st.counts.size();
    std::vector<int> N(n);
    for (int i = 0; i < n; ++i) N[i] = (!keep || keep[i]) ? st.counts[i] : 0;
    const bool same_shape = st.prev_nframes == n;
    if (avt_internal_commit_frames(c, n, N.data(), same_shape)) return 1;      // (takes `pending` down)
    st.prev_nframes = -1;
    return 0;
}

}  // namespace

extern "C" {

int avt_frames_subsample_constants(int* chunk, int* scan_width) {
    if (chunk) *chunk = SUB_CHUNK;
    if (scan_width) *scan_width = SUB_SCAN;
    return 0;
}

int avt_frames_subsample_rtree(avt_ctx* ctx, avt_rtree* rt, avt_bgsub* bg, const int* boxes, const int* intervals, const unsigned char* want_centroid,
                               int* counts_out, double* centroid_out, int* boxes_out) {
    return avt_guard("avt_frames_subsample_rtree", [&]() -> int {
        return subsample_impl(ctx, rt, bg, "avt_frames_subsample_rtree", boxes, intervals, want_centroid, counts_out, centroid_out, boxes_out);
    });
}

int avt_frames_subsample_rforest(avt_ctx* ctx, avt_rforest* rf, avt_bgsub* bg, const int* boxes, const int* intervals, const unsigned char* want_centroid,
                                 int* counts_out, double* centroid_out, int* boxes_out) {
    return avt_guard("avt_frames_subsample_rforest", [&]() -> int {
        return subsample_impl(ctx, rf, bg, "avt_frames_subsample_rforest", boxes, intervals, want_centroid, counts_out, centroid_out, boxes_out);
    });
}

int avt_frames_subsample_commit(avt_ctx* ctx, const unsigned char* keep) {
    return avt_guard("avt_frames_subsample_commit", [&]() -> int { return commit_impl(ctx, keep); });
}

}  // extern "C"
