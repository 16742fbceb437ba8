// avt_rtree_train.hip — the forest trainer on gfx950 (include/avt_rtree_train.h): the reference's AvatarTrainerV3
// (RTree.cpp:2338-2950) level by level instead of depth first, and RTree::trainTransfer's counts (:3332-3420).
//
//   k_rt_img_scan / k_rt_crop   bounding box of non-zero depth, foreground count, label / depth checks, crop into the store
//   k_rt_select                 initTraining (:2424-2497): raster-order compaction of mask != 255, partial Fisher-Yates
//   k_rt_count                  per open node: integer part counts (LDS atomics, flushed as integers)
//   k_rt_search<BS>             per (node, chunk of features): min / max of the scores, the (parts x T) bucket histogram in
//                               LDS, the threshold scan of optimalInformationGain3 (:2782-2851), the chunk's best feature
//   k_rt_choose                 per node: the best chunk (lower feature index on bit-equal gains)
//   k_rt_partition              split (:2853-2928): stable segmented partition, score < thresh to the left
//   k_rt_transfer               every labelled pixel walks the tree; 64-bit integer atomics per (leaf, part)
//
// Built with -ffp-contract=off: scores (rt_score_by_feature, shared with k_rtree_predict), the bucket rule, thresholds and
// the feature components are the reference's float sequence; gains are double.
#include <cfloat>
#include <climits>

#include "avt_rtree_train.h"
#include "avt_rtree_score.h"

namespace {

__device__ __forceinline__ float4 rt_feature(uint64_t seed, unsigned long long key, int f, float maxp) {
    return make_float4(avt_rt_feature_component(seed, key, f, 0, maxp), avt_rt_feature_component(seed, key, f, 1, maxp),
                       avt_rt_feature_component(seed, key, f, 2, maxp), avt_rt_feature_component(seed, key, f, 3, maxp));
}

// a sample of zero depth scores 0: u / 0 is infinite, every probe leaves the image and reads BACKGROUND_DEPTH twice
__device__ __forceinline__ float rt_train_score(const float* __restrict__ store, const RtImg& m, int xy, float sd, float4 f) {
    if (sd == 0.f) return 0.f;
    return rt_score_by_feature(store + m.off, m.w, m.x0, m.y0, m.x0, m.y0, m.x0 + m.w - 1, m.y0 + m.h - 1, xy & 0xffff, xy >> 16, sd, f);
}

// -(S_L H(L) + S_R H(R)) of threshold i (RTree.cpp:2824-2847) in double, parts in ascending order; `cum` holds per part the
// count of samples in buckets 0..i (the reference's "right" set), `tot` the node's counts.  NaN: a side is empty.
__device__ double rt_gain(const int* cum, const int* tot, const int* plist, int npres, int T, int i) {
    long long ls = 0, rs = 0;
    for (int k = 0; k < npres; ++k) {
        const int p = plist[k], r = cum[p * T + i];
        rs += r;
        ls += tot[p] - r;
    }
    if (ls == 0 || rs == 0) return __longlong_as_double(0x7ff8000000000000ll);
    const double L = (double)ls, R = (double)rs;
    double hl = 0.0, hr = 0.0;
    for (int k = 0; k < npres; ++k) {       // parts with a zero count contribute nothing (p < 1e-10 is skipped, :33)
        const int p = plist[k], r = cum[p * T + i], l = tot[p] - r;
        const double pl = (double)l / L, pr = (double)r / R;
        if (!(pl < 1e-10)) hl -= pl * log2(pl);
        if (!(pr < 1e-10)) hr -= pr * log2(pr);
    }
    return -(L * hl + R * hr);
}

}  // namespace

// per image: bounding box of non-zero depth, labelled pixels, the largest label (255 excluded) and whether a depth is negative or
// not finite; out7 = x0 y0 x1 y1 count max_label bad
__global__ __launch_bounds__(256) void k_rt_img_scan(const float* __restrict__ depth, const unsigned char* __restrict__ mask, int rows, int cols,
                                                     int* __restrict__ out7) {
    __shared__ int s[7];
    if (threadIdx.x == 0) { s[0] = INT_MAX; s[1] = INT_MAX; s[2] = -1; s[3] = -1; s[4] = 0; s[5] = -1; s[6] = 0; }
    __syncthreads();
    const size_t npix = (size_t)rows * cols;
    const float* d = depth + blockIdx.x * npix;
    const unsigned char* m = mask + blockIdx.x * npix;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1, cnt = 0, ml = -1, bad = 0;
    for (size_t p = threadIdx.x; p < npix; p += 256) {
        const int r = (int)(p / cols), c = (int)(p - (size_t)r * cols);
        const float z = d[p];
        if (z != 0.f) { x0 = min(x0, c); y0 = min(y0, r); x1 = max(x1, c); y1 = max(y1, r); }
        bad |= !(z >= 0.f) || isinf(z);
        const int l = m[p];
        if (l != 255) { ++cnt; ml = max(ml, l); }
    }
    atomicMin(&s[0], x0); atomicMin(&s[1], y0); atomicMax(&s[2], x1); atomicMax(&s[3], y1); atomicAdd(&s[4], cnt);
    atomicMax(&s[5], ml); atomicOr(&s[6], bad);
    __syncthreads();
    if (threadIdx.x < 7) out7[blockIdx.x * 7 + threadIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_rt_crop(const float* __restrict__ depth, int rows, int cols, const RtImg* __restrict__ imgs, float* __restrict__ store) {
    const RtImg m = imgs[blockIdx.x];
    const float* d = depth + blockIdx.x * (size_t)rows * cols;
    const int tot = m.w * m.h;
    for (int i = threadIdx.x; i < tot; i += 256) {
        const int y = i / m.w, x = i - y * m.w;
        store[m.off + i] = d[(size_t)(m.y0 + y) * cols + (m.x0 + x)];
    }
}

// one wave per image: the candidates in raster order by ballot compaction, then random_util::choose's partial Fisher-Yates
// (Util.h:242-250) by lane 0, or every candidate in raster order when there are no more than k
__global__ __launch_bounds__(64) void k_rt_select(const float* __restrict__ depth, const unsigned char* __restrict__ mask, int rows, int cols, int k,
                                                  uint64_t seed, int img_base, const long long* __restrict__ out_off, int* __restrict__ scratch, RtSamples s) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const size_t npix = (size_t)rows * cols;
    const unsigned char* m = mask + i * npix;
    const float* d = depth + i * npix;
    int* cand = scratch + i * npix;
    int cnt = 0;
    for (size_t base = 0; base < npix; base += 64) {
        const size_t p = base + lane;
        const bool fg = p < npix && m[p] != 255;
        const unsigned long long bal = __ballot(fg);
        if (fg) cand[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = (int)p;
        cnt += __popcll(bal);
    }
    __syncthreads();                                    // lane 0 reads what every lane wrote
    const long long o = out_off[i];
    const int img = img_base + i;
    if (cnt <= k) {
        for (int j = lane; j < cnt; j += 64) {
            const int p = cand[j], r = p / cols;
            s.img[o + j] = img; s.xy[o + j] = (p - r * cols) | (r << 16); s.d[o + j] = d[p]; s.lab[o + j] = m[p];
        }
        return;
    }
    if (lane != 0) return;
    const uint64_t sk = seed ^ AVT_RT_TAG_SAMPLE;
    for (int j = 0; j < k; ++j) {
        const int r = j + (int)(avt_rt_hash(sk, (uint64_t)img, (uint64_t)j) % (uint64_t)(cnt - j));
        const int p = cand[r], row = p / cols;
        s.img[o + j] = img; s.xy[o + j] = (p - row * cols) | (row << 16); s.d[o + j] = d[p]; s.lab[o + j] = m[p];
        cand[r] = cand[j];                              // std::swap(source[j], source[r]); source[j] is never read again
    }
}

__global__ __launch_bounds__(256) void k_rt_count(const RtNode* __restrict__ nodes, const unsigned char* __restrict__ lab, int P, int* __restrict__ counts) {
    __shared__ int c[128];
    for (int p = threadIdx.x; p < P; p += 256) c[p] = 0;
    __syncthreads();
    const RtNode nd = nodes[blockIdx.x];
    for (int i = nd.start + threadIdx.x; i < nd.end; i += 256) atomicAdd(&c[lab[i]], 1);
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += 256) counts[(size_t)blockIdx.x * P + p] = c[p];
}

// LDS of k_rt_search, in ints: hist P*T | tot P | plist P | btot T | pad | gains T doubles | min, max per wave | misc 4
__host__ __device__ inline size_t rt_search_lds_ints(int P, int T, int BS) {
    size_t n = (size_t)P * T + 2 * (size_t)P + (size_t)T;
    n += n & 1;
    return n + 2 * (size_t)T + 2 * (size_t)(BS / 64) + 4;
}

// One workgroup per (node, chunk of features).  Per feature: pass 1 the scores' min / max, pass 2 the bucket histogram
// (LDS integer atomics: the result does not depend on their order), then per part the cumulative counts and per threshold
// the gain; a bucket that holds no sample repeats the partition of the threshold before it (an equal gain is never
// chosen: the reference takes the FIRST maximum), so it is skipped.
template <int BS>
__global__ __launch_bounds__(BS) void k_rt_search(const int* __restrict__ list, int nchunks, int fchunk, const RtNode* __restrict__ nodes,
                                                  const int* __restrict__ counts, RtSamples s, const RtImg* __restrict__ imgs,
                                                  const float* __restrict__ store, RtTrainArgs a, RtChunk* __restrict__ out, int* __restrict__ tap_hist,
                                                  float* __restrict__ tap_minmax) {
    extern __shared__ int lds[];
    const int P = a.P, T = a.T, tid = threadIdx.x;
    int* hist = lds;
    int* tot = hist + P * T;
    int* plist = tot + P;
    int* btot = plist + P;
    size_t goff = (size_t)P * T + 2 * (size_t)P + (size_t)T;
    goff += goff & 1;
    double* gains = (double*)(lds + goff);
    float* rmin = (float*)(lds + goff + 2 * (size_t)T);
    float* rmax = rmin + BS / 64;
    int* misc = (int*)(rmax + BS / 64);

    const int pos = blockIdx.x / nchunks, chunk = blockIdx.x - pos * nchunks;
    const int m = list[pos];
    const RtNode nd = nodes[m];
    for (int p = tid; p < P; p += BS) tot[p] = counts[(size_t)m * P + p];
    __syncthreads();
    if (tid == 0) {
        int k = 0;
        for (int p = 0; p < P; ++p)
            if (tot[p]) plist[k++] = p;
        misc[0] = k;
    }
    __syncthreads();
    const int npres = misc[0];
    const int f0 = chunk * fchunk, f1 = min(a.F, f0 + fchunk);
    double best = -INFINITY;
    float best_t = 0.f;
    int best_f = -1;
    for (int f = f0; f < f1; ++f) {
        const float4 uv = rt_feature(a.seed, nd.key, f, a.maxp);
        float mn = FLT_MAX, mx = -FLT_MAX;
        for (int i = nd.start + tid; i < nd.end; i += BS) {
            const float sc = rt_train_score(store, imgs[s.img[i]], s.xy[i], s.d[i], uv);
            mn = fminf(mn, sc);
            mx = fmaxf(mx, sc);
        }
        for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
        if ((tid & 63) == 0) { rmin[tid >> 6] = mn; rmax[tid >> 6] = mx; }
        for (int j = tid; j < P * T; j += BS) hist[j] = 0;
        for (int j = tid; j < T; j += BS) btot[j] = 0;
        __syncthreads();
        mn = rmin[0]; mx = rmax[0];
        for (int w = 1; w < BS / 64; ++w) { mn = fminf(mn, rmin[w]); mx = fmaxf(mx, rmax[w]); }
        const float step = (mx - mn + FLT_EPSILON) / ((float)T + 1.f);
        for (int i = nd.start + tid; i < nd.end; i += BS) {
            const float sc = rt_train_score(store, imgs[s.img[i]], s.xy[i], s.d[i], uv);
            const float q = (sc - mn) / step;             // (size_t)q < T  <=>  q < T  (q >= 0)
            if (q < (float)T) {
                const int b = (int)q;
                atomicAdd(&hist[(int)s.lab[i] * T + b], 1);
                atomicAdd(&btot[b], 1);
            }
        }
        __syncthreads();
        if (tap_hist) {                                   // avt_rtree_trainer_root_histograms: the integer histogram as counted
            for (int j = tid; j < P * T; j += BS) tap_hist[(size_t)f * P * T + j] = hist[j];
            if (tid == 0) { tap_minmax[2 * f] = mn; tap_minmax[2 * f + 1] = mx; }
            __syncthreads();                              // the rows are summed in place below: every wave's copy is done first
        }
        for (int k = tid; k < npres; k += BS) {
            int* h = hist + plist[k] * T;
            int acc = 0;
            for (int b = 0; b < T; ++b) { acc += h[b]; h[b] = acc; }
        }
        __syncthreads();
        for (int i = tid; i < T; i += BS) gains[i] = btot[i] ? rt_gain(hist, tot, plist, npres, T, i) : __longlong_as_double(0x7ff8000000000000ll);
        __syncthreads();
        if (tid == 0) {
            double g = -INFINITY;
            int bi = -1;
            for (int i = 0; i < T; ++i)
                if (gains[i] > g) { g = gains[i]; bi = i; }
            if (bi >= 0 && g > best) { best = g; best_t = mn + (float)(bi + 1) * step; best_f = f; }
        }
        __syncthreads();                                  // hist, btot and the min / max slots are rewritten by the next feature
    }
    if (tid == 0) out[blockIdx.x] = RtChunk{best, best_t, best_f};
}

__global__ __launch_bounds__(256) void k_rt_choose(const int* __restrict__ list, int nlist, int nchunks, const RtNode* __restrict__ nodes,
                                                   const RtChunk* __restrict__ chunks, RtTrainArgs a, RtRes* __restrict__ res) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nlist) return;
    const RtChunk* c = chunks + (size_t)j * nchunks;
    double g = -INFINITY;
    float t = 0.f;
    int f = -1;
    for (int k = 0; k < nchunks; ++k)
        if (c[k].f >= 0 && c[k].gain > g) { g = c[k].gain; t = c[k].thresh; f = c[k].f; }
    const int m = list[j];
    RtRes r{};
    r.f = f; r.gain = g; r.nleft = -1;
    if (f >= 0) {
        const float4 uv = rt_feature(a.seed, nodes[m].key, f, a.maxp);
        r.feat[0] = uv.x; r.feat[1] = uv.y; r.feat[2] = uv.z; r.feat[3] = uv.w; r.feat[4] = t;
    }
    res[m] = r;
}

// one workgroup per searched node: count the left side, then tiles of 256 in order, ballot + wave offsets
__global__ __launch_bounds__(256) void k_rt_partition(const int* __restrict__ list, const RtNode* __restrict__ nodes, RtRes* __restrict__ res, RtSamples in,
                                                      RtSamples out, const RtImg* __restrict__ imgs, const float* __restrict__ store) {
    __shared__ int wsum[4];
    const int m = list[blockIdx.x];
    if (res[m].f < 0) return;
    const RtNode nd = nodes[m];
    const float4 uv = make_float4(res[m].feat[0], res[m].feat[1], res[m].feat[2], res[m].feat[3]);
    const float th = res[m].feat[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cl = 0;
    for (int i = nd.start + tid; i < nd.end; i += 256) cl += rt_train_score(store, imgs[in.img[i]], in.xy[i], in.d[i], uv) < th;
    for (int o = 32; o > 0; o >>= 1) cl += __shfl_xor(cl, o);
    if (lane == 0) wsum[wave] = cl;
    __syncthreads();
    const int nl = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    int lbase = 0;
    for (int t0 = nd.start; t0 < nd.end; t0 += 256) {
        const int i = t0 + tid;
        const bool act = i < nd.end;
        int img = 0, xy = 0;
        float d = 0.f;
        unsigned char lab = 0;
        bool left = false;
        if (act) {
            img = in.img[i]; xy = in.xy[i]; d = in.d[i]; lab = in.lab[i];
            left = rt_train_score(store, imgs[img], xy, d, uv) < th;
        }
        const unsigned long long bal = __ballot(left);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        const int tl = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (act) {
            const int lpos = lbase + before + __popcll(bal & ((1ull << lane) - 1ull));     // lefts before sample i
            const int dst = left ? nd.start + lpos : nd.start + nl + (i - nd.start - lpos);
            out.img[dst] = img; out.xy[dst] = xy; out.d[dst] = d; out.lab[dst] = lab;
        }
        lbase += tl;
        __syncthreads();
    }
    if (tid == 0) res[m].nleft = nl;
}

__global__ __launch_bounds__(256) void k_rt_transfer(const RtNodeDev* __restrict__ nodes, const float* __restrict__ depth, const unsigned char* __restrict__ mask,
                                                     int rows, int cols, long long total, int P, unsigned long long* __restrict__ counts,
                                                     int* __restrict__ bad) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int lab = mask[g];
    if (lab == 255) return;
    if (lab >= P) { atomicOr(bad, 1); return; }   // refused by the host: the batch's counts are dropped
    const long long npix = (long long)rows * cols, img = g / npix;
    const int p = (int)(g - img * npix), r = p / cols, c = p - r * cols;
    const float* d = depth + img * npix;
    const float sd = d[p];
    const float4* nv = (const float4*)nodes;
    int nodeid = 0, leaf;
    for (;;) {
        const float4 a = nv[2 * nodeid], b = nv[2 * nodeid + 1];
        if (__float_as_int(b.w)) { leaf = __float_as_int(b.z); break; }
        const float sc = sd == 0.f ? 0.f : rt_score_by_feature(d, cols, 0, 0, 0, 0, cols - 1, rows - 1, c, r, sd, a);
        nodeid = sc < b.x ? __float_as_int(b.y) : __float_as_int(b.z);
    }
    atomicAdd(&counts[(size_t)leaf * P + lab], 1ull);
}

// ---- launches ----------------------------------------------------------------------------------------------------
static int rt_ok() { return hipGetLastError() != hipSuccess; }

int rt_launch_img_scan(hipStream_t s, const float* depth, const unsigned char* mask, int n, int rows, int cols, int* out7) {
    hipLaunchKernelGGL(k_rt_img_scan, dim3(n), dim3(256), 0, s, depth, mask, rows, cols, out7);
    return rt_ok();
}
int rt_launch_crop(hipStream_t s, const float* depth, int n, int rows, int cols, const RtImg* imgs, float* store) {
    hipLaunchKernelGGL(k_rt_crop, dim3(n), dim3(256), 0, s, depth, rows, cols, imgs, store);
    return rt_ok();
}
int rt_launch_select(hipStream_t s, const float* depth, const unsigned char* mask, int n, int rows, int cols, int k, uint64_t seed, int img_base,
                     const long long* out_off, int* scratch, RtSamples out) {
    hipLaunchKernelGGL(k_rt_select, dim3(n), dim3(64), 0, s, depth, mask, rows, cols, k, seed, img_base, out_off, scratch, out);
    return rt_ok();
}
int rt_launch_count(hipStream_t s, const RtNode* nodes, int m, const unsigned char* lab, int P, int* counts) {
    hipLaunchKernelGGL(k_rt_count, dim3(m), dim3(256), 0, s, nodes, lab, P, counts);
    return rt_ok();
}
size_t rt_search_lds_bytes(int P, int T, bool large) { return 4 * rt_search_lds_ints(P, T, large ? 256 : 64); }
// both forms of k_rt_search may be launched with up to `bytes` of dynamic LDS (above 64 KiB for three of the accepted shapes)
int rt_search_set_attributes(size_t bytes) {
    return hipFuncSetAttribute((const void*)k_rt_search<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess ||
           hipFuncSetAttribute((const void*)k_rt_search<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess;
}
int rt_launch_search(hipStream_t s, bool large, const int* list, int nlist, int nchunks, int fchunk, const RtNode* nodes, const int* counts, RtSamples in,
                     const RtImg* imgs, const float* store, RtTrainArgs a, RtChunk* out, int* tap_hist, float* tap_minmax) {
    const unsigned grid = (unsigned)nlist * (unsigned)nchunks;
    if (large)
        hipLaunchKernelGGL(k_rt_search<256>, dim3(grid), dim3(256), rt_search_lds_bytes(a.P, a.T, true), s, list, nchunks, fchunk, nodes, counts, in,
                           imgs, store, a, out, tap_hist, tap_minmax);
    else
        hipLaunchKernelGGL(k_rt_search<64>, dim3(grid), dim3(64), rt_search_lds_bytes(a.P, a.T, false), s, list, nchunks, fchunk, nodes, counts, in,
                           imgs, store, a, out, tap_hist, tap_minmax);
    return rt_ok();
}
int rt_launch_choose(hipStream_t s, const int* list, int nlist, int nchunks, const RtNode* nodes, const RtChunk* chunks, RtTrainArgs a, RtRes* res) {
    hipLaunchKernelGGL(k_rt_choose, dim3((nlist + 255) / 256), dim3(256), 0, s, list, nlist, nchunks, nodes, chunks, a, res);
    return rt_ok();
}
int rt_launch_partition(hipStream_t s, const int* list, int nlist, const RtNode* nodes, RtRes* res, RtSamples in, RtSamples out, const RtImg* imgs,
                        const float* store) {
    hipLaunchKernelGGL(k_rt_partition, dim3(nlist), dim3(256), 0, s, list, nodes, res, in, out, imgs, store);
    return rt_ok();
}
int rt_launch_transfer(hipStream_t s, const RtNodeDev* nodes, const float* depth, const unsigned char* mask, int n, int rows, int cols, int P,
                       unsigned long long* counts, int* bad) {
    const long long total = (long long)n * rows * cols;
    hipLaunchKernelGGL(k_rt_transfer, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, nodes, depth, mask, rows, cols, total, P, counts, bad);
    return rt_ok();
}
