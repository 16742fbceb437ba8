// ark/AvatarOptimizer.h — the reference's `ark::AvatarOptimizer` (include/AvatarOptimizer.h:11-61) on top of the C ABI.
#pragma once
#include <limits>
#include <vector>

#include "Avatar.h"

namespace ark {
/** Optimize avatar to fit a point cloud */
class AvatarOptimizer {
   public:
    /** Same signature as the reference.  `intrin` and `image_size` do not influence optimize() there (renderer constructed but
     *  unused, AvatarOptimizer.cpp:1271,:1369-1385); here they are the camera and image size of `renderOcclusion`.  `part_map`
     *  must have >= numJoints entries (AvatarOptimizer.cpp:1229) and is kept by reference, like the reference does. */
    AvatarOptimizer(Avatar& ava, const CameraIntrin& intrin, const Size& image_size, int num_parts, const std::vector<int>& part_map)
        : ava(ava), intrin(intrin), imageSize(image_size), numParts(num_parts), partMap(part_map) {
        r.resize(ava.model.numJoints());
    }
    ~AvatarOptimizer() { if (ctx) avt_ctx_destroy(ctx); }
    // holds references (ava, intrin, partMap) and owns a device context: not copyable (the reference's class holds the same
    // references; copying it would alias the avatar it optimises)
    AvatarOptimizer(const AvatarOptimizer&) = delete;
    AvatarOptimizer& operator=(const AvatarOptimizer&) = delete;

    /** Begin full optimization on the target data cloud (AvatarOptimizer.cpp:1246-1517).  Precondition as in the
     *  reference: ava.update() has been called; postcondition: ava.p, ava.w, ava.r updated and ava.update()d. */
    void optimize(const CloudType& data_cloud, const VectorXi& data_part_labels, int icp_iters = 1, int num_threads = 4) {
        const int N = (int)data_cloud.cols(), J = ava.model.numJoints();
        if ((int)data_part_labels.size() != N) { std::fprintf(stderr, "avatar (MI355X): labels/cloud size mismatch\n"); std::exit(1); }
        if (!ctx || N > capacity) {
            if (ctx) avt_ctx_destroy(ctx);
            capacity = N > 65536 ? N : 65536;
            ARK_AVT_CHECK(avt_ctx_create(ava.device, ava.model.handle, numParts, partMap.data(), capacity, 1, &ctx));
            occlusionRenderSet = false;
            gateSet.clear();
            trimSet.clear();
        }
        if (renderOcclusion != occlusionRenderSet) {       // the context follows the member (a new context starts with the mode off)
            ARK_AVT_CHECK(avt_set_occlusion_render(ctx, renderOcclusion ? imageSize.width : 0, imageSize.height, intrin.fx, intrin.fy, intrin.cx, intrin.cy));
            occlusionRenderSet = renderOcclusion;
        }
        {   // the correspondence gate: per-part values when given, else the one member for every part (a new context starts with it off)
            const std::vector<double> want = partGates.empty() ? std::vector<double>(1, maxCorrespondenceDist) : partGates;
            if (want != gateSet && !(gateSet.empty() && want.size() == 1 && want[0] == std::numeric_limits<double>::infinity())) {
                ARK_AVT_CHECK(avt_set_corr_gate(ctx, (int)want.size(), want.data()));
                gateSet = want;
            }
        }
        {   // trimmed ICP: the four members for every part (a new context starts with it off)
            const std::vector<double> want = {trimQuantile, trimFactor, trimFloor, (double)trimMinMatches};
            if (want != trimSet && !(trimSet.empty() && trimFactor == std::numeric_limits<double>::infinity())) {
                if (trimFactor == std::numeric_limits<double>::infinity()) ARK_AVT_CHECK(avt_set_corr_trim(ctx, 0, nullptr, nullptr, nullptr, 1));
                else ARK_AVT_CHECK(avt_set_corr_trim(ctx, 1, &trimQuantile, &trimFactor, &trimFloor, trimMinMatches));
                trimSet = want;
            }
        }
        for (int i = 0; i < J; ++i) r[i] = rotationToQuaternion(ava.r[i]);       // :1250-1254
        avt_options o;
        avt_options_default(&o);
        o.beta_pose = betaPose; o.beta_shape = betaShape; o.nn_step = nnStep; o.max_iters_per_icp = maxItersPerICP;
        o.enable_occlusion = enableOcclusion ? 1 : 0; o.icp_iters = icp_iters; o.num_threads = num_threads;
        o.function_tolerance = functionTolerance;
        std::vector<double> q(4 * (size_t)J);
        for (int i = 0; i < J; ++i) for (int c = 0; c < 4; ++c) q[4 * i + c] = r[i].c[c];
        // :1497 ava.update(): the launch sequence ends with exactly that update; its outputs come back with the fit, in the call's one synchronisation
        ava.cloud.resize(3, ava.model.numPoints());
        ava.jointPos.resize(3, J);
        ava.jointTrans.resize(12, J);
        if (icp_iters >= 1) {
            ARK_AVT_CHECK(avt_optimize_posed(ctx, data_cloud.data(), data_part_labels.data(), N, &o, ava.p.data(), q.data(), ava.w.data(), &lastStats,
                                             ava.cloud.data(), ava.jointPos.data(), ava.jointTrans.data()));
        } else {      // (no ICP iteration: no closing update in the sequence)
            ARK_AVT_CHECK(avt_optimize(ctx, data_cloud.data(), data_part_labels.data(), N, &o, ava.p.data(), q.data(), ava.w.data(), &lastStats));
            ARK_AVT_CHECK(avt_get_posed(ctx, 0, ava.cloud.data(), ava.jointPos.data(), ava.jointTrans.data()));
        }
        for (int i = 0; i < J; ++i) {
            for (int c = 0; c < 4; ++c) r[i].c[c] = q[4 * i + c];
            ava.r[i] = quaternionToRotation(r[i]);                               // :1494-1496
        }
    }

    /** The visibility flags (numPoints bytes, 0 / 1) of the last ICP iteration of the last optimize() (avt_get_visibility) */
    std::vector<unsigned char> visibility() const {
        std::vector<unsigned char> v((size_t)ava.model.numPoints());
        ARK_AVT_CHECK(avt_get_visibility(ctx, 0, v.data()));
        return v;
    }

    /** Per-part correspondence gates (numParts distances, +inf = off for that part); an empty vector returns to maxCorrespondenceDist */
    void setCorrespondenceGate(const std::vector<double>& gates) { partGates = gates; }
    /** Data points the last search of the last optimize() dropped at the gate (avt_get_gated) */
    int lastGated() const {
        int n = 0;
        ARK_AVT_CHECK(avt_get_gated(ctx, 0, &n));
        return n;
    }

    /** Matches the last search of the last optimize() lost to the trim (avt_get_trimmed) */
    int lastTrimmed() const {
        int n = 0;
        ARK_AVT_CHECK(avt_get_trimmed(ctx, 0, &n, nullptr));
        return n;
    }

    /** Rotation representation size */
    static const int ROT_SIZE = 4;
    /** Optimization parameter r */
    std::vector<Quaterniond> r;
    /** Cost function component weights */
    double betaPose = 0.1, betaShape = 1.0;
    /** NN matching step size (unused in the inverted NN mode the reference runs) */
    int nnStep = 20;
    /** maximum inner iterations per ICP */
    int maxItersPerICP = 10;
    /** Whether to elimiate occluded points before NN matching */
    bool enableOcclusion = true;
    /** NOT a member of the reference's class: the true-occlusion block its author left commented out as too slow
     *  (AvatarOptimizer.cpp:1369-1385).  With enableOcclusion, a point is visible iff one of its front-facing faces owns a pixel
     *  of renderFaces(imageSize) of the current cloud at `intrin` (include/avt.h, avt_set_occlusion_render): a body part in front
     *  of another hides it.  Off by default; takes effect at the next optimize(). */
    bool renderOcclusion = false;
    /** NOT a member of the reference's class, whose findNN keeps the nearest visible model point of a data point's part however far
     *  away it is: a data point further than this (metres) from that model point gets no correspondence in any ICP iteration, as if
     *  its part had no visible model point (include/avt.h, avt_set_corr_gate).  +inf (default) = off; no value is offered.  Followed
     *  before every optimize(); setCorrespondenceGate gives per-part values. */
    double maxCorrespondenceDist = std::numeric_limits<double>::infinity();
    /** NOT members of the reference's class: trimmed ICP (include/avt.h, avt_set_corr_trim).  After every search, per part, a match is
     *  kept iff its squared distance d2 <= max(trimFactor^2 * t, trimFloor^2), t the ceil(trimQuantile * n)-th smallest d2 of the part's
     *  n matches in this frame; a part with fewer than trimMinMatches matches is left alone.  trimFactor +inf (default) = off; no value
     *  is offered.  Followed before every optimize(). */
    double trimQuantile = 1.0;
    double trimFactor = std::numeric_limits<double>::infinity();
    double trimFloor = 0.0;
    int trimMinMatches = 1;
    /** Not a member of the reference's class: the value its optimize() hard-codes as options.function_tolerance
     *  (AvatarOptimizer.cpp:1333) - a step that lowers the objective by no more than this fraction ends the inner iterations
     *  of the ICP iteration; 0 = always maxItersPerICP iterations (include/avt.h, avt_options::function_tolerance) */
    double functionTolerance = 1e-4;

    Avatar& ava;
    const CameraIntrin& intrin;
    Size imageSize;
    int numParts;
    const std::vector<int>& partMap;

    /** final cost / #correspondences of the last call, so a caller can implement the reference's tracking-loss
     *  reinit policy (demo.cpp:225,251-266) */
    avt_stats lastStats{};

   private:
    avt_ctx* ctx = nullptr;
    int capacity = 0;
    bool occlusionRenderSet = false;   // what ctx was last told
    std::vector<double> partGates;     // setCorrespondenceGate (empty: maxCorrespondenceDist for every part)
    std::vector<double> gateSet;       // the gate ctx was last told (empty: never told, i.e. off)
    std::vector<double> trimSet;       // the trim settings ctx was last told (empty: never told, i.e. off)
};
}  // namespace ark
