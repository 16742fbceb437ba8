// avt_poseerr.hip — the pose error on gfx950 (include/avt_poseerr.h, THE RULE): PVE, MPJPE and their Procrustes-aligned forms of
// n (estimate, truth) pairs, one workgroup of four waves per pair.
//
// A pair's two clouds are 330 KB at SMPL's size and are read three times (errors and centroids; centred cross-covariance; aligned
// errors), the second and third time from L2.  A point is three interleaved doubles, so a lane that read its own point would
// fetch 24-byte pieces at a 24-byte stride; instead the workgroup copies a tile of 256 points of both sides into LDS as flat,
// consecutive doubles (every wave reads 512 contiguous bytes per load) and each lane then takes its point from LDS.  The joints
// go through the same code, so J is not bounded by a wave.  Every sum is a lane's serial sum over its points in ascending order,
// a shuffle tree inside the wave and a serial sum over the four waves through LDS: a fixed order, no atomics.  The 4 x 4
// eigenproblem is solved by every lane redundantly (no divergence, nothing to broadcast).  The d_v go to global scratch and come
// back for the per-part sums: wave w takes parts w, w + 4, ... over the part-sorted vertex list.  Built with -ffp-contract=off.
#include <climits>

#include "avt_poseerr.h"

#define PE_LANES 256
#define PE_WAVES (PE_LANES / 64)
#define PE_NSUM 10            // the widest block sum: nine cross-covariance entries and the estimate's variance

namespace {

struct PeSet {                // what one point set of a pair gives
    double sum, sq, mx, rr, pa_sum, pa_sq, scale;
    int arg;
    unsigned status;
};

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                 // lane 0 holds the sum
}

// v[0 .. K) summed over the workgroup, the result in every lane.  s_red: PE_WAVES x PE_NSUM doubles.
template <int K>
__device__ inline void block_sum(double* v, double* s_red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double w = wave_sum(v[k]);
        if (lane == 0) s_red[wave * PE_NSUM + k] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = s_red[k];
#pragma unroll
        for (int w = 1; w < PE_WAVES; ++w) t += s_red[w * PE_NSUM + k];
        v[k] = t;
    }
    __syncthreads();          // s_red is free again
}

__device__ inline void arg_better(double& m, int& a, double om, int oa) {
    if (om > m || (om == m && oa < a)) { m = om; a = oa; }
}

// tile `base` of X and Y (n points each, 3 interleaved doubles) into LDS; the caller's lane t then owns point base + t
__device__ inline int load_tile(const double* __restrict__ X, const double* __restrict__ Y, int n, int base, double* s_x, double* s_y) {
    const int cnt = min(PE_LANES, n - base);
    __syncthreads();          // the previous tile has been read
    for (int i = threadIdx.x; i < 3 * cnt; i += PE_LANES) {
        s_x[i] = X[(size_t)3 * base + i];
        s_y[i] = Y[(size_t)3 * base + i];
    }
    __syncthreads();
    return cnt;
}

// One point set: X the estimate's n points, Y the truth's.  raw[n] receives the errors, pa[n] the aligned ones unless null.
// ROOT: also the root-relative sum.  Every lane returns the same PeSet.
template <bool ROOT>
__device__ void pe_set(const double* __restrict__ X, const double* __restrict__ Y, int n, double* __restrict__ raw, double* __restrict__ pa,
                       double* s_x, double* s_y, double* s_red, int* s_arg, PeSet& o) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double x0[3] = {X[0], X[1], X[2]}, y0[3] = {Y[0], Y[1], Y[2]};
    // ---- pass 1: errors, the two centroids, the flags
    double acc[PE_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // sum d, sum q, sum r, sum x (3), sum y (3)
    double mx = -1.0;
    int arg = INT_MAX;
    bool bad = false, spread = false;
    for (int base = 0; base < n; base += PE_LANES) {
        const int cnt = load_tile(X, Y, n, base, s_x, s_y);
        if (t < cnt) {
            const double x[3] = {s_x[3 * t], s_x[3 * t + 1], s_x[3 * t + 2]}, y[3] = {s_y[3 * t], s_y[3 * t + 1], s_y[3 * t + 2]};
            const double dx = x[0] - y[0], dy = x[1] - y[1], dz = x[2] - y[2];
            const double q = (dx * dx + dy * dy) + dz * dz, d = sqrt(q);
            raw[base + t] = d;
            acc[0] += d; acc[1] += q;
            if (d > mx) { mx = d; arg = base + t; }
            if (ROOT) {
                const double rx = (x[0] - x0[0]) - (y[0] - y0[0]), ry = (x[1] - x0[1]) - (y[1] - y0[1]), rz = (x[2] - x0[2]) - (y[2] - y0[2]);
                acc[2] += sqrt((rx * rx + ry * ry) + rz * rz);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                acc[3 + k] += x[k]; acc[6 + k] += y[k];
                bad |= !isfinite(x[k]) || !isfinite(y[k]);
                spread |= x[k] != x0[k];
            }
        }
    }
    block_sum<9>(acc, s_red);
    // the maximum and the lowest index that attains it
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double om = __shfl_down(mx, off);
        const int oa = __shfl_down(arg, off);
        arg_better(mx, arg, om, oa);
    }
    if (lane == 0) { s_red[wave] = mx; s_arg[wave] = arg; }
    __syncthreads();
    mx = s_red[0]; arg = s_arg[0];
#pragma unroll
    for (int w = 1; w < PE_WAVES; ++w) arg_better(mx, arg, s_red[w], s_arg[w]);
    o.status = __syncthreads_or(bad) ? AVT_POSEERR_BAD_INPUT : 0u;          // also the barrier that frees s_red
    const bool coincident = !__syncthreads_or(spread);
    o.sum = acc[0]; o.sq = acc[1]; o.rr = acc[2]; o.mx = mx; o.arg = arg;
    const double mux[3] = {acc[3] / n, acc[4] / n, acc[5] / n}, muy[3] = {acc[6] / n, acc[7] / n, acc[8] / n};
    // ---- pass 2: the centred cross-covariance S[3 a + b] = sum x'_a y'_b and the estimate's variance; then (s, R)
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, s = 0.0;
    if (!coincident && !o.status) {                                         // uniform over the workgroup; a non-finite set is not aligned
        double S[PE_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int base = 0; base < n; base += PE_LANES) {
            const int cnt = load_tile(X, Y, n, base, s_x, s_y);
            if (t < cnt) {
                const double x[3] = {s_x[3 * t] - mux[0], s_x[3 * t + 1] - mux[1], s_x[3 * t + 2] - mux[2]};
                const double y[3] = {s_y[3 * t] - muy[0], s_y[3 * t + 1] - muy[1], s_y[3 * t + 2] - muy[2]};
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) S[3 * a + b] += x[a] * y[b];
                S[9] += (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
            }
        }
        block_sum<PE_NSUM>(S, s_red);
        double lambda;
        o.status |= pe_horn(S, R, &lambda);
        s = lambda > 0.0 && S[9] > 0.0 ? lambda / S[9] : 0.0;
    }
    o.scale = s;
    // ---- pass 3: the aligned errors a_k = |s R x'_k - y'_k|
    double al[2] = {0.0, 0.0};
    for (int base = 0; base < n; base += PE_LANES) {
        const int cnt = load_tile(X, Y, n, base, s_x, s_y);
        if (t < cnt) {
            const double x[3] = {s_x[3 * t] - mux[0], s_x[3 * t + 1] - mux[1], s_x[3 * t + 2] - mux[2]};
            const double ax = s * ((R[0] * x[0] + R[1] * x[1]) + R[2] * x[2]) - (s_y[3 * t] - muy[0]);
            const double ay = s * ((R[3] * x[0] + R[4] * x[1]) + R[5] * x[2]) - (s_y[3 * t + 1] - muy[1]);
            const double az = s * ((R[6] * x[0] + R[7] * x[1]) + R[8] * x[2]) - (s_y[3 * t + 2] - muy[2]);
            const double q = (ax * ax + ay * ay) + az * az, e = sqrt(q);
            al[0] += e; al[1] += q;
            if (pa) pa[base + t] = e;
        }
    }
    block_sum<2>(al, s_red);
    o.pa_sum = al[0]; o.pa_sq = al[1];
}

__global__ __launch_bounds__(PE_LANES) void k_pose_err(const double* __restrict__ cloud_e, const double* __restrict__ cloud_t,
                                                       const double* __restrict__ joints_e, const double* __restrict__ joints_t, int V, int J, int P,
                                                       const int* __restrict__ perm, const int* __restrict__ pstart, double* __restrict__ dist,
                                                       double* __restrict__ summary, double* __restrict__ per_joint, double* __restrict__ per_part,
                                                       int* __restrict__ argmax, unsigned* __restrict__ status) {
    __shared__ double s_x[3 * PE_LANES], s_y[3 * PE_LANES], s_red[PE_WAVES * PE_NSUM];
    __shared__ int s_arg[PE_WAVES];
    const size_t pair = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double* d = dist + pair * V;
    PeSet vs, js;
    pe_set<false>(cloud_e + pair * 3 * V, cloud_t + pair * 3 * V, V, d, nullptr, s_x, s_y, s_red, s_arg, vs);
    // the per-part sums: the workgroup's own stores to d are visible behind the barriers of pass 2 and 3
    for (int q = wave; q < P; q += PE_WAVES) {
        double sum = 0.0, mx = 0.0;
        for (int i = pstart[q] + lane; i < pstart[q + 1]; i += 64) {
            const double e = d[perm[i]];
            sum += e;
            mx = e > mx ? e : mx;
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double om = __shfl_down(mx, off);
            mx = om > mx ? om : mx;
        }
        if (lane == 0) {
            per_part[pair * 2 * P + q] = sum;
            per_part[pair * 2 * P + P + q] = mx;
        }
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    js.sum = js.mx = js.rr = js.pa_sum = js.pa_sq = js.scale = nan;
    js.arg = -1;
    js.status = 0;
    if (J > 0)
        pe_set<true>(joints_e + pair * 3 * J, joints_t + pair * 3 * J, J, per_joint + pair * 2 * J, per_joint + pair * 2 * J + J, s_x, s_y, s_red, s_arg, js);
    if (t == 0) {
        double* o = summary + pair * AVT_POSEERR_COLS;
        o[AVT_POSEERR_V_SUM] = vs.sum; o[AVT_POSEERR_V_SQ] = vs.sq; o[AVT_POSEERR_V_MAX] = vs.mx;
        o[AVT_POSEERR_VPA_SUM] = vs.pa_sum; o[AVT_POSEERR_VPA_SQ] = vs.pa_sq; o[AVT_POSEERR_VPA_SCALE] = vs.scale;
        o[AVT_POSEERR_J_SUM] = js.sum; o[AVT_POSEERR_J_MAX] = js.mx; o[AVT_POSEERR_JR_SUM] = js.rr;
        o[AVT_POSEERR_JPA_SUM] = js.pa_sum; o[AVT_POSEERR_JPA_SQ] = js.pa_sq; o[AVT_POSEERR_JPA_SCALE] = js.scale;
        argmax[pair * 2 + AVT_POSEERR_V_ARGMAX] = vs.arg;
        argmax[pair * 2 + AVT_POSEERR_J_ARGMAX] = js.arg;
        status[pair] = vs.status | js.status;
    }
}

}  // namespace

int avt_poseerr_launch(avt_poseerr* pe, int n) {
    hipLaunchKernelGGL(k_pose_err, dim3((unsigned)n), dim3(PE_LANES), 0, pe->stream, (const double*)pe->d_cloud[0], (const double*)pe->d_cloud[1],
                       (const double*)pe->d_joints[0], (const double*)pe->d_joints[1], pe->V, pe->J, pe->P, (const int*)pe->d_perm, (const int*)pe->d_pstart,
                       (double*)pe->d_dist, (double*)pe->d_summary, (double*)pe->d_per_joint, (double*)pe->d_per_part, (int*)pe->d_argmax, (unsigned*)pe->d_status);
    return hipGetLastError() != hipSuccess;
}
