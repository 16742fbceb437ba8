// ark/PoseError.h — the pose error over the C ABI of avt_poseerr.h: how far fitted avatars are from the avatars that made the
// data, as the field's standard figures (PVE, MPJPE, root-relative MPJPE, PA-MPJPE, PA-PVE), in metres.  ark::PoseErrorResult is
// one pair's figures as the device left them, with derive(); ark::PoseError is the handle that scores pairs on the GPU.
// Header-only.
//
// avt_poseerr.h states the rule.  No threshold on any figure is offered, no per-vertex error comes down, the alignment always
// includes the scale, and nothing in the trackers calls this by default.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../avt.h"
#include "../avt_poseerr.h"

namespace ark {

/** The derived figures of one pair: host arithmetic, one division each (and one root); NaN where the denominator is 0. */
struct PoseErrorFigures {
    double pve, pveRms, pveMax, paPve, paPveScale;
    double mpjpe, mpjpeMax, mpjpeRoot, paMpjpe, paMpjpeScale;
    std::vector<double> pvePart;              // numParts entries, NaN for an empty part
};

/** One pair as avt_poseerr_get returns it. */
struct PoseErrorResult {
    int V = 0, J = 0, numParts = 0;
    double summary[AVT_POSEERR_COLS] = {};
    std::vector<double> jointErr, jointErrAligned;      // J each
    std::vector<double> partSum, partMax;               // numParts each
    std::vector<int> partSize;                          // n_q
    int vArgmax = -1, jArgmax = -1;
    unsigned status = 0;                                // AVT_POSEERR_BAD_INPUT | AVT_POSEERR_NO_CONVERGENCE

    PoseErrorFigures derive() const {
        PoseErrorFigures f;
        f.pve = summary[AVT_POSEERR_V_SUM] / (double)V;
        f.pveRms = std::sqrt(summary[AVT_POSEERR_V_SQ] / (double)V);
        f.pveMax = summary[AVT_POSEERR_V_MAX];
        f.paPve = summary[AVT_POSEERR_VPA_SUM] / (double)V;
        f.paPveScale = summary[AVT_POSEERR_VPA_SCALE];
        f.mpjpe = summary[AVT_POSEERR_J_SUM] / (double)J;
        f.mpjpeMax = summary[AVT_POSEERR_J_MAX];
        f.mpjpeRoot = summary[AVT_POSEERR_JR_SUM] / (double)J;
        f.paMpjpe = summary[AVT_POSEERR_JPA_SUM] / (double)J;
        f.paMpjpeScale = summary[AVT_POSEERR_JPA_SCALE];
        f.pvePart.resize((size_t)numParts);
        for (int q = 0; q < numParts; ++q)
            f.pvePart[(size_t)q] = partSize[(size_t)q] == 0 ? std::numeric_limits<double>::quiet_NaN() : partSum[(size_t)q] / (double)partSize[(size_t)q];
        return f;
    }
};

/** The handle: up to max_pairs (estimate, truth) pairs per run.  A failure is fatal, like every failure of this facade. */
class PoseError {
   public:
    /** V vertices, J joints, vertex_part empty: one part */
    PoseError(int V, int J, int num_parts, const std::vector<int>& vertex_part, int max_pairs = 64, int device = 0) {
        if (!vertex_part.empty() && (int)vertex_part.size() != V) fatal("PoseError", "vertex_part needs V entries (or none)");
        if (avt_poseerr_create(device, V, J, num_parts, vertex_part.empty() ? nullptr : vertex_part.data(), max_pairs, &h_) != 0) die("PoseError");
        dims();
    }
    /** the model's V and J, vertex_part[v] = part_map[main joint of v] (empty: the joint itself) */
    PoseError(const avt_model* model, int num_parts, const std::vector<int>& part_map = {}, int max_pairs = 64, int device = 0) {
        if (avt_poseerr_create_for_model(device, model, num_parts, part_map.empty() ? nullptr : part_map.data(), max_pairs, &h_) != 0) die("PoseError");
        dims();
    }
    ~PoseError() { avt_poseerr_destroy(h_); }
    PoseError(const PoseError&) = delete;
    PoseError& operator=(const PoseError&) = delete;

    /** one side of n pairs from the host: clouds n x 3V, joints n x 3J (ignored when J == 0) */
    void upload(int side, int n, const double* clouds, const double* joints) {
        if (avt_poseerr_upload(h_, side, n, clouds, joints) != 0) die("upload");
    }
    /** one side from a context's frames (empty: 0 .. n - 1), copied on the device */
    void fromContext(int side, avt_ctx* ctx, int n, const std::vector<int>& frames = {}) {
        if (!frames.empty() && (int)frames.size() != n) fatal("fromContext", "one frame index per pair");
        if (avt_poseerr_from_ctx(h_, side, ctx, n, frames.empty() ? nullptr : frames.data()) != 0) die("fromContext");
    }
    void run() { if (avt_poseerr_run(h_) != 0) die("run"); }

    /** the result of the last run, one entry per pair */
    std::vector<PoseErrorResult> get() {
        int n = 0;
        if (avt_poseerr_get(h_, nullptr, nullptr, nullptr, nullptr, nullptr, &n) != 0) die("get");
        const size_t N = (size_t)n, Js = (size_t)J, Ps = (size_t)numParts;
        std::vector<double> sum(N * AVT_POSEERR_COLS), pj(N * 2 * Js), pp(N * 2 * Ps);
        std::vector<int> am(N * 2);
        std::vector<unsigned> st(N);
        if (avt_poseerr_get(h_, sum.data(), pj.data(), pp.data(), am.data(), st.data(), nullptr) != 0) die("get");
        std::vector<PoseErrorResult> out(N);
        for (size_t i = 0; i < N; ++i) {
            PoseErrorResult& r = out[i];
            r.V = V; r.J = J; r.numParts = numParts; r.partSize = partSize;
            for (int k = 0; k < AVT_POSEERR_COLS; ++k) r.summary[k] = sum[i * AVT_POSEERR_COLS + (size_t)k];
            r.jointErr.assign(pj.begin() + (long)(i * 2 * Js), pj.begin() + (long)(i * 2 * Js + Js));
            r.jointErrAligned.assign(pj.begin() + (long)(i * 2 * Js + Js), pj.begin() + (long)((i + 1) * 2 * Js));
            r.partSum.assign(pp.begin() + (long)(i * 2 * Ps), pp.begin() + (long)(i * 2 * Ps + Ps));
            r.partMax.assign(pp.begin() + (long)(i * 2 * Ps + Ps), pp.begin() + (long)((i + 1) * 2 * Ps));
            r.vArgmax = am[2 * i + AVT_POSEERR_V_ARGMAX]; r.jArgmax = am[2 * i + AVT_POSEERR_J_ARGMAX];
            r.status = st[i];
        }
        return out;
    }

    avt_poseerr* handle() const { return h_; }
    int V = 0, J = 0, numParts = 0;
    std::vector<int> partSize;

   private:
    void dims() {
        if (avt_poseerr_part_sizes(h_, nullptr, &V, &J, &numParts) != 0) die("PoseError");
        partSize.resize((size_t)numParts);
        if (avt_poseerr_part_sizes(h_, partSize.data(), nullptr, nullptr, nullptr) != 0) die("PoseError");
    }
    [[noreturn]] static void die(const char* what) { std::fprintf(stderr, "FATAL: PoseError::%s: %s\n", what, avt_last_error()); std::exit(1); }
    [[noreturn]] static void fatal(const char* what, const char* why) { std::fprintf(stderr, "FATAL: PoseError::%s: %s\n", what, why); std::exit(1); }
    avt_poseerr* h_ = nullptr;
};

}  // namespace ark
