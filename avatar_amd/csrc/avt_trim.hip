// avt_trim.hip — trimmed ICP (avt_set_corr_trim): one stage between the correspondence search and k_finalize that
// takes back the matches that are far RELATIVE to the distribution of this frame's own match distances, per part.
//
// THIS TRANSLATION UNIT IS COMPILED WITH -ffp-contract=off.  The squared distance of a match is the search's own expression on the same
// values (avt_nn.hip: r = d0*d0; r += d1*d1; r += d2*d2 of query minus matched model point, each operation rounded; k_lbs stores one
// value to the cloud and to its part-sorted copy, k_compact gathers from either), and the fixed-point term that is taken back from the
// sums is the one nn_record added: a contracted multiply-add would change both.
//
// grid (num_parts, frames), one workgroup of TRIM_THREADS threads per (part, frame) - the walks are chains of dependent loads (query ->
// matched vertex -> its position), so what a workgroup has in flight per turn is what it runs at:
//   1. count the matched queries of the part's range [part_off[q], part_off[q + 1]) of the part-sorted arrays, n, and keep their keys
//      in LDS while they fit
//   2. n == 0 or n < min_matches: T = +inf, nothing dropped.  Else k = ceil(rho n) clamped to [1, n], and t = the k-th smallest squared
//      distance by an exact radix select on the 64-bit patterns (non-negative doubles: the unsigned order of the patterns is the
//      numeric order), most significant byte first: eight rounds of one 256-bin LDS histogram over the keys that share the bytes
//      found so far.  A part with more than TRIM_KEYS matches recomputes its keys in every round (no scratch memory: eight more
//      walks over the part's range, exact either way).
//   3. T = max(k2 t, f2); a second walk takes back every match with d2 > T: -1 in corr and corr_sorted, the negative of nn_record's
//      integer terms on cnt and fsum (integer atomics: exact modulo 2^64, order-independent).
// Every loop is counted.  A state the workgroup cannot vouch for (a range outside the frame, a matched vertex outside the model, a
// histogram that does not hold the wanted rank) raises AVT_FAULT_TRIM in the frame's fault word and ends; nothing waits for anything.
#include "avt_device.h"

#define TRIM_KEYS 4096                // matched keys of one (part, frame) kept in LDS (32 KB)
#define TRIM_THREADS 1024

// one more key in the round's histogram.  Early rounds see one digit for almost every key (distances of one magnitude): a wave whose
// active lanes agree adds its popcount once instead of queueing up to 64 atomics on one LDS address.
__device__ __forceinline__ void trim_hist_add(int* hist, bool on, int digit) {
    const unsigned long long act = __ballot(on);
    if (act == 0ull) return;
    const int first = __shfl(digit, (int)__ffsll((long long)act) - 1, 64);
    const unsigned long long same = __ballot(on && digit == first);
    if (same == act) {
        if (lane_id() == (int)__ffsll((long long)act) - 1) atomicAdd(hist + first, __popcll(act));
    } else if (on) {
        atomicAdd(hist + digit, 1);
    }
}

__global__ __launch_bounds__(TRIM_THREADS) void k_trim(AvtTrimArgs a) {
    const int q = blockIdx.x, f = blockIdx.y + a.f0, t = threadIdx.x;
    const int np = a.num_parts, V = a.V;
    int* out_n = a.trimmed + (size_t)f * np + q;
    double* out_T = a.thr + (size_t)f * np + q;
    const double rho = a.set[q], k2 = a.set[np + q], f2 = a.set[2 * np + q];
    const int min_matches = (int)a.set[3 * np];
    if (!(k2 < AVT_INF)) {              // this part is not trimmed
        if (t == 0) { *out_n = 0; *out_T = AVT_INF; }
        return;
    }
    const int* po = a.part_off + (size_t)f * (np + 1);
    const int b = po[q], e = po[q + 1];
    const size_t base = (size_t)f * a.max_points;
    const double* cloud = a.cloud + (size_t)f * 3 * V;

    __shared__ unsigned long long s_key[TRIM_KEYS];
    __shared__ int s_hist[256], s_wtot[4], s_bin[8], s_krem[8];
    __shared__ int s_bad, s_fill, s_drop;
    if (t == 0) { s_bad = 0; s_fill = 0; s_drop = 0; }
    if (t < 8) { s_bin[t] = -1; s_krem[t] = 0; }
    __syncthreads();
    auto give_up = [&]() {
        if (t == 0) { atomicOr(a.fault + f, AVT_FAULT_TRIM); *out_n = 0; *out_T = AVT_INF; }
    };
    if (b < 0 || e < b || e > a.max_points) { give_up(); return; }
    const int nwalk = (e - b + TRIM_THREADS - 1) / TRIM_THREADS;      // turns of a walk over the part's range, the same for every thread

    // the squared distance of sorted query s to model vertex m: the search's expression on the search's values
    auto d2_of = [&](int s, int m) {
        const double* cl = cloud + 3 * (size_t)m;
        const double d0 = a.dx[base + s] - cl[0], d1 = a.dy[base + s] - cl[1], d2 = a.dz[base + s] - cl[2];
        double r = d0 * d0;
        r = r + d1 * d1;
        r = r + d2 * d2;
        return r;
    };

    // ---- 1. the matched queries of the part; their keys go to LDS while they fit (any order: a selection does not look at positions) ----
    {
        int bad = 0;
        for (int i = 0; i < nwalk; ++i) {
            const int s = b + i * TRIM_THREADS + t;
            const int m = s < e ? a.corr_sorted[base + s] : -1;
            if (m >= V || m < -1) bad = 1;
            const bool on = m >= 0 && m < V;
            const unsigned long long bal = __ballot(on);
            if (bal == 0ull) continue;                               // (wave-uniform)
            const int leader = (int)__ffsll((long long)bal) - 1;
            int slot0 = 0;
            if (lane_id() == leader) slot0 = atomicAdd(&s_fill, __popcll(bal));
            const int slot = __shfl(slot0, leader, 64) + __popcll(bal & ((1ull << lane_id()) - 1ull));
            if (on && slot < TRIM_KEYS) s_key[slot] = (unsigned long long)__double_as_longlong(d2_of(s, m));
        }
        if (bad) atomicOr(&s_bad, 1);
    }
    __syncthreads();
    if (s_bad) { give_up(); return; }
    const int n = s_fill;
    if (n == 0 || n < min_matches) {
        if (t == 0) { *out_n = 0; *out_T = AVT_INF; }
        return;
    }
    int k = (int)ceil(rho * (double)n);
    k = max(1, min(k, n));

    // ---- 2. the k-th smallest key ----
    const bool in_lds = n <= TRIM_KEYS;
    unsigned long long prefix = 0ull;
    int krem = k;
#pragma unroll 1
    for (int r = 0; r < 8; ++r) {
        const int shift = 56 - 8 * r;
        const unsigned long long himask = r == 0 ? 0ull : ~0ull << (shift + 8);      // the bytes found so far
        if (t < 256) s_hist[t] = 0;
        __syncthreads();
        if (in_lds) {
            const int nk = (n + TRIM_THREADS - 1) / TRIM_THREADS;
            for (int i = 0; i < nk; ++i) {
                const int j = i * TRIM_THREADS + t;
                const unsigned long long key = j < n ? s_key[j] : 0ull;
                trim_hist_add(s_hist, j < n && (key & himask) == prefix, (int)((key >> shift) & 255ull));
            }
        } else {
            for (int i = 0; i < nwalk; ++i) {
                const int s = b + i * TRIM_THREADS + t;
                const int m = s < e ? a.corr_sorted[base + s] : -1;
                const unsigned long long key = m >= 0 ? (unsigned long long)__double_as_longlong(d2_of(s, m)) : 0ull;
                trim_hist_add(s_hist, m >= 0 && (key & himask) == prefix, (int)((key >> shift) & 255ull));
            }
        }
        __syncthreads();
        // the bin that holds rank krem among the keys of this round: a prefix sum over the 256 bins, one bin per thread of the first four waves
        int c = 0, incl = 0;
        if (t < 256) {
            c = s_hist[t];
            incl = wave_incl_scan(c);
            if (lane_id() == 63) s_wtot[wave_id()] = incl;
        }
        __syncthreads();
        if (t < 256) {
            for (int w = 0; w < wave_id(); ++w) incl += s_wtot[w];
            if (c > 0 && incl - c < krem && krem <= incl) { s_bin[r] = t; s_krem[r] = krem - (incl - c); }
        }
        __syncthreads();
        const int bin = s_bin[r];
        if (bin < 0) { give_up(); return; }      // the histogram does not hold the rank: the range changed under the walk
        prefix |= (unsigned long long)bin << shift;
        krem = s_krem[r];
    }
    const double tk = __longlong_as_double((long long)prefix);
    const double kt = k2 * tk;
    const double T = kt > f2 ? kt : f2;

    // ---- 3. take back the matches beyond T ----
    const AvtFrameCtl& ctl = a.ctl[f];
    const double c0 = ctl.centre[0], c1 = ctl.centre[1], c2 = ctl.centre[2];
    unsigned long long* fs = (unsigned long long*)(a.fsum + (size_t)f * 3 * V);
    for (int i = 0; i < nwalk; ++i) {
        const int s = b + i * TRIM_THREADS + t;
        const int m = s < e ? a.corr_sorted[base + s] : -1;
        bool drop = false;
        if (m >= 0) drop = d2_of(s, m) > T;
        if (drop) {
            a.corr_sorted[base + s] = -1;
            a.corr[base + a.dorig[base + s]] = -1;
            atomicAdd(a.cnt + (size_t)f * V + m, -1);
            atomicAdd(fs + m, 0ull - (unsigned long long)rint_to_ll((a.dx[base + s] - c0) * AVT_FIX_SCALE));
            atomicAdd(fs + (size_t)V + m, 0ull - (unsigned long long)rint_to_ll((a.dy[base + s] - c1) * AVT_FIX_SCALE));
            atomicAdd(fs + 2 * (size_t)V + m, 0ull - (unsigned long long)rint_to_ll((a.dz[base + s] - c2) * AVT_FIX_SCALE));
        }
        const unsigned long long bal = __ballot(drop);
        if (bal != 0ull && lane_id() == (int)__ffsll((long long)bal) - 1) atomicAdd(&s_drop, __popcll(bal));
    }
    __syncthreads();
    if (t == 0) { *out_n = s_drop; *out_T = T; }
}

void launch_trim(avt_ctx* c, int nframes) {
    const FrameBuffers& fb = c->fb;
    AvtTrimArgs a;
    a.part_off = fb.part_off; a.dorig = fb.dorig; a.dx = fb.dx; a.dy = fb.dy; a.dz = fb.dz; a.cloud = fb.cloud;
    a.corr = fb.corr; a.corr_sorted = fb.corr_sorted; a.cnt = fb.cnt; a.fsum = fb.fsum; a.ctl = fb.ctl; a.fault = fb.fault;
    a.set = c->trim_set; a.trimmed = c->trim_count; a.thr = c->trim_thr;
    a.f0 = fb.f0; a.num_parts = c->dm.d.num_parts; a.V = c->dm.d.V; a.max_points = fb.max_points;
    hipLaunchKernelGGL(k_trim, dim3(c->dm.d.num_parts, nframes), dim3(TRIM_THREADS), 0, c->cur_stream, a);
}
