// avt_poseerr.h (private) — the handle of include/avt_poseerr.h, the launch of its one kernel, and the 4 x 4 eigenproblem of
// the alignment (host and device: the kernel solves it in every lane, a host program can check it without a GPU)
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/avt_poseerr.h"
#include "avt_host.h"

struct avt_poseerr {
    int device = 0, V = 0, J = 0, P = 0, max_pairs = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    std::vector<int> part_size;               // n_q
    // sized at creation.  d_perm: the vertices sorted by part (ascending inside a part), d_pstart[q] .. d_pstart[q + 1] part q's
    DevBuf<int> d_perm, d_pstart;
    DevBuf<double> d_cloud[2], d_joints[2];   // per side: max_pairs x 3V, max_pairs x 3J
    DevBuf<double> d_dist;                    // max_pairs x V: the d_v of a run, read back by its per-part sums
    DevBuf<double> d_summary, d_per_joint, d_per_part;
    DevBuf<int> d_argmax;
    DevBuf<unsigned> d_status;
    int n_side[2] = {0, 0};                   // pairs resident per side
    int n_result = 0;                         // pairs of the last run; 0: no result
};

// scores pairs 0 .. n - 1 of the resident sides on pe->stream: one workgroup per pair
int avt_poseerr_launch(avt_poseerr* pe, int n);

// Horn's matrix N of the centred cross-covariance S (S[3 a + b] = sum x'_a y'_b), its largest eigenvalue and the rotation of
// that eigenvalue's eigenvector (row-major R: y ~ R x), by cyclic Jacobi: at most AVT_POSEERR_MAX_SWEEPS sweeps of the six
// rotations, done when the off-diagonal squares are below 1e-34 of the whole.  Returns 0, or AVT_POSEERR_NO_CONVERGENCE with
// the last iterate.  Every loop is bounded, whatever S holds.
__host__ __device__ inline unsigned pe_horn(const double* S, double* R, double* lambda) {
    double a[4][4], v[4][4];
    a[0][0] = S[0] + S[4] + S[8];
    a[1][1] = S[0] - S[4] - S[8];
    a[2][2] = -S[0] + S[4] - S[8];
    a[3][3] = -S[0] - S[4] + S[8];
    a[0][1] = a[1][0] = S[5] - S[7];
    a[0][2] = a[2][0] = S[6] - S[2];
    a[0][3] = a[3][0] = S[1] - S[3];
    a[1][2] = a[2][1] = S[1] + S[3];
    a[1][3] = a[3][1] = S[6] + S[2];
    a[2][3] = a[3][2] = S[5] + S[7];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    unsigned status = AVT_POSEERR_NO_CONVERGENCE;
    for (int sweep = 0; sweep <= AVT_POSEERR_MAX_SWEEPS; ++sweep) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            diag += a[p][p] * a[p][p];
#pragma unroll
            for (int q = p + 1; q < 4; ++q) off += a[p][q] * a[p][q];
        }
        if (off <= (diag + 2.0 * off) * 1e-34) { status = 0; break; }      // also the zero matrix; false for a NaN
        if (sweep == AVT_POSEERR_MAX_SWEEPS) break;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {                                // A <- A G
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {                                // A <- G^T A
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
                a[p][q] = a[q][p] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {                                // V <- V G: the columns are the eigenvectors
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
        }
    }
    double w = v[0][0], x = v[1][0], y = v[2][0], z = v[3][0], lam = a[0][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)                                              // selects, not indices: the arrays stay in registers
        if (a[i][i] > lam) { w = v[0][i]; x = v[1][i]; y = v[2][i]; z = v[3][i]; lam = a[i][i]; }
    const double nrm = sqrt((w * w + x * x) + (y * y + z * z));
    if (nrm > 0.0) { w /= nrm; x /= nrm; y /= nrm; z /= nrm; } else { w = 1.0; x = y = z = 0.0; }
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
    *lambda = lam;
    return status;
}
