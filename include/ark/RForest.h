// ark/RForest.h — several trained ark::RTree run as one forest, over the C ABI of avt_rforest.h: what the reference's tools do
// with any number of models (rtree-run-dataset.cpp:98-159): RTree::predict per model, the distributions added in model order
// in float32, the arg-max per pixel (the first part whose sum exceeds a running best that starts at 0; 255 when none does).
// The members are ark::RTree's inference side (LabelHandle's predictBest, predictBestBatch, predictBestFromBGSub, predict and the
// device postProcess; postProcess, numParts, partMap, partMapType), so a forest stands where a tree stands
// (MultiFrameTracker::attachFrontEnd).  As with ark::RTree a failure is fatal (message + exit).
//
// The score (avt_rforest.h, THE SCORE) is what rtree-run-dataset leaves to the eye: the forest's arg-max against ground-truth
// part masks as a (numParts + 1)^2 confusion matrix of 64-bit counts, accumulated on the GPU (scoreReset, score, scoreRendered,
// scoreGet), and scoreFromAvatar, the held-out counterpart of RTree::trainFromAvatar.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../avt.h"
#include "../avt_rforest.h"
#include "AvatarRenderer.h"
#include "BGSubtractor.h"
#include "RTree.h"

namespace ark {

/** What RForest::scoreGet returns: the counts and the figures derived from them on the host, in double from the integers.  A
 *  figure with a zero denominator is NaN; meanIoU is over the parts whose IoU is not NaN. */
struct ForestScore {
    int numParts = 0;
    std::vector<long long> confusion;          // (numParts + 1)^2, row-major conf[truth][predicted]; index numParts = none (255)
    long long numImages = 0, numPixels = 0;    // numPixels: those the stride selected
    double accuracy = 0, meanIoU = 0;
    std::vector<double> recall, precision, iou;
    long long missed = 0, spurious = 0;        // labelled pixels left unlabelled; background pixels the forest labels

    long long at(int truth, int predicted) const { return confusion[(size_t)truth * (numParts + 1) + predicted]; }
    /** Fills the derived figures from confusion */
    void derive() {
        const int P = numParts;
        const double nan = std::nan("");
        auto ratio = [nan](long long a, long long b) { return b ? (double)a / (double)b : nan; };
        std::vector<long long> row(P, 0), col(P, 0);
        long long trace = 0, labelled = 0;
        missed = spurious = 0;
        for (int t = 0; t <= P; ++t)
            for (int q = 0; q <= P; ++q) {
                if (t < P) row[t] += at(t, q);
                if (q < P) col[q] += at(t, q);
            }
        recall.assign(P, nan); precision.assign(P, nan); iou.assign(P, nan);
        double iouSum = 0;
        int iouCount = 0;
        for (int p = 0; p < P; ++p) {
            trace += at(p, p); labelled += row[p]; missed += at(p, P); spurious += at(P, p);
            recall[p] = ratio(at(p, p), row[p]);
            precision[p] = ratio(at(p, p), col[p]);
            iou[p] = ratio(at(p, p), row[p] + col[p] - at(p, p));
            if (!std::isnan(iou[p])) { iouSum += iou[p]; ++iouCount; }
        }
        accuracy = ratio(trace, labelled);
        meanIoU = iouCount ? iouSum / iouCount : nan;
    }
};

/** The C handle's type, the class name of the FATAL lines and the entry points of a forest, for LabelHandle */
struct RForestApi {
    typedef avt_rforest Handle;
    static constexpr const char* name = "RForest";
    static constexpr auto predict_best = avt_rforest_predict_best;
    static constexpr auto predict = avt_rforest_predict;
    static constexpr auto images_upload = avt_rforest_images_upload;
    static constexpr auto predict_best_resident_boxes = avt_rforest_predict_best_resident_boxes;
    static constexpr auto predict_best_from_bgsub = avt_rforest_predict_best_from_bgsub;
    static constexpr auto labels_download_all = avt_rforest_labels_download_all;
    static constexpr auto labels_upload = avt_rforest_labels_upload;
    static constexpr auto post_process_resident = avt_rforest_post_process_resident;
    static constexpr auto post_process_from_bgsub = avt_rforest_post_process_from_bgsub;
    static constexpr auto com_pre_get = avt_rforest_com_pre_get;
    static constexpr auto com_pre_set = avt_rforest_com_pre_set;
};

class RForest : public LabelHandle<RForest, RForestApi> {
    friend class LabelHandle<RForest, RForestApi>;      // ensure()

public:
    /** Load the trees from files, in forest order (rtree-run-dataset.cpp:98-104) */
    explicit RForest(const std::vector<std::string>& paths, int device = 0) : device_(device) {
        std::vector<std::unique_ptr<RTree>> owned;
        std::vector<RTree*> trees;
        for (const std::string& p : paths) {
            owned.emplace_back(new RTree(p, -1));          // members only: the forest holds the device image
            trees.push_back(owned.back().get());
        }
        build(trees);
    }
    /** From trees in memory; the forest copies them, they may go away afterwards */
    explicit RForest(const std::vector<RTree*>& trees, int device = 0) : device_(device) { build(trees); }
    ~RForest() { avt_rforest_destroy(h_); }
    RForest(const RForest&) = delete;
    RForest& operator=(const RForest&) = delete;

    /** RTree::postProcess (RTree.h:150-166) through the first member tree: host code that reads numParts and the part-map type */
    void postProcess(Image8& image, MatrixNX<2>& com_pre, int interval = 1, int num_threads = 1, Point top_left = Point(0, 0),
                     Point bot_right = Point(-1, -1), double dist_to_pre_weight = 0.001) {
        first_->postProcess(image, com_pre, interval, num_threads, top_left, bot_right, dist_to_pre_weight);
    }

    // ---- the score: a confusion matrix against ground-truth part masks (avt_rforest.h, THE SCORE)
    /** Puts the totals back to zero */
    void scoreReset() {
        if (avt_rforest_score_reset(h_) != 0) die("scoreReset");
    }

    /** Adds same-size depth images and their part masks (255 = none) to the totals: every pixel of the stride grid */
    void score(const std::vector<ImageF>& depth, const std::vector<Image8>& part_mask, int stride = 1) {
        if (depth.empty() || depth.size() != part_mask.size()) fatal("score", "need as many part masks as depth images, at least one");
        const int rows = depth[0].rows, cols = depth[0].cols;
        std::vector<float> d;
        std::vector<uint8_t> m;
        for (size_t i = 0; i < depth.size(); ++i) {
            if (depth[i].rows != rows || depth[i].cols != cols || part_mask[i].rows != rows || part_mask[i].cols != cols)
                fatal("score", "the images must share one size");
            d.insert(d.end(), depth[i].a.begin(), depth[i].a.end());
            m.insert(m.end(), part_mask[i].a.begin(), part_mask[i].a.end());
        }
        if (avt_rforest_score_images(h_, (int)depth.size(), rows, cols, d.data(), m.data(), stride) != 0) die("score");
    }

    /** Adds what `renderer` left on the device (AvatarRenderer::renderDepthAndPartMaskOnDevice), read where it lies */
    void scoreRendered(AvatarRenderer& renderer, int stride = 1) {
        if (avt_rforest_score_rendered(h_, renderer.handle(), stride) != 0) die("scoreRendered");
    }

    /** The totals since the last reset and the figures derived from them */
    ForestScore scoreGet() {
        ForestScore s;
        s.numParts = numParts;
        s.confusion.assign((size_t)(numParts + 1) * (numParts + 1), 0);
        if (avt_rforest_score_get(h_, s.confusion.data(), &s.numImages, &s.numPixels) != 0) die("scoreGet");
        s.derive();
        return s;
    }

    /** The held-out loop, RTree::trainFromAvatar's with the score in the trainer's place: image idx in [first_image, first_image
     *  + num_images) is avatar_model posed by Avatar::randomize(true, true, true, idx ^ xorKey) (xorKey = avt_rt_xor_key(seed)),
     *  skinned by avt_lbs_update into a context of this call, rendered by the GPU renderer with part_map (empty: the joint id
     *  itself) and scored device to device, `batch` images at a time; no image crosses to the host.  With the training run's
     *  seed and first_image = its num_images the poses are ones the forest never saw, from the same distribution.  Starts from a
     *  reset; the result does not depend on `batch`. */
    ForestScore scoreFromAvatar(AvatarModel& avatar_model, const CameraIntrin& intrin, const Size& image_size, int num_images, int first_image = 0,
                                const std::vector<int>& part_map = {}, uint64_t seed = 0, int batch = 64, int stride = 1) {
        const int J = avatar_model.numJoints(), K = avatar_model.numShapeKeys();
        std::vector<int> pm(part_map);
        if (pm.empty()) for (int j = 0; j < J; ++j) pm.push_back(j);
        if ((int)pm.size() < J || num_images < 1 || batch < 1 || first_image < 0)
            fatal("scoreFromAvatar", "part_map needs one entry per joint; num_images, batch >= 1; first_image >= 0");
        int np = 0;
        for (int v : pm) np = v + 1 > np ? v + 1 : np;
        avt_ctx* ctx = nullptr;
        avt_renderer* rend = nullptr;
        if (avt_ctx_create(device_, avatar_model.handle, np, pm.data(), 64, batch, &ctx) != 0 ||
            avt_renderer_create(device_, avatar_model.handle, image_size.width, image_size.height, intrin.fx, intrin.fy, intrin.cx, intrin.cy, batch,
                                &rend) != 0 ||
            avt_renderer_set_part_map(rend, (int)pm.size(), pm.data()) != 0)
            die("scoreFromAvatar");
        const uint32_t xorKey = avt_rt_xor_key(seed);
        Avatar ava(avatar_model);
        std::vector<double> w, p, R;
        scoreReset();
        for (int i0 = first_image; i0 < first_image + num_images; i0 += batch) {
            const int k = first_image + num_images - i0 < batch ? first_image + num_images - i0 : batch;
            w.assign((size_t)K * k, 0.0); p.assign((size_t)3 * k, 0.0); R.assign((size_t)9 * J * k, 0.0);
            for (int i = 0; i < k; ++i) {
                ava.randomize(true, true, true, (uint32_t)(i0 + i) ^ xorKey);
                for (int c = 0; c < K; ++c) w[(size_t)i * K + c] = ava.w[c];
                for (int c = 0; c < 3; ++c) p[(size_t)i * 3 + c] = ava.p(c);
                for (int j = 0; j < J; ++j)
                    for (int c = 0; c < 9; ++c) R[((size_t)i * J + j) * 9 + c] = ava.r[j].data()[c];
            }
            if (avt_lbs_update(ctx, k, w.data(), p.data(), R.data(), nullptr, nullptr, nullptr) != 0 || avt_renderer_from_ctx(rend, ctx, k, nullptr) != 0 ||
                avt_renderer_run(rend, AVT_RENDER_DEPTH | AVT_RENDER_PART_MASK) != 0 || avt_rforest_score_rendered(h_, rend, stride) != 0)
                die("scoreFromAvatar");
        }
        avt_renderer_destroy(rend);
        avt_ctx_destroy(ctx);
        return scoreGet();
    }

    int numTrees = 0;
    int numParts = 0;
    std::vector<int> partMap;
    int partMapType = 0;
    int totalNodes = 0, totalLeafs = 0;

    /** The C handle (MultiFrameTracker's device subsampling, avt_subsample.h) */
    avt_rforest* handle() const { return h_; }

private:
    void build(const std::vector<RTree*>& trees) {
        std::vector<const avt_rtree*> hs;
        for (RTree* t : trees) hs.push_back(t ? t->handle() : nullptr);
        if (avt_rforest_create(hs.data(), (int)hs.size(), device_, &h_) != 0) die("RForest");
        int pml = 0;
        avt_rforest_info(h_, &numTrees, &numParts, &pml, &partMapType, &totalNodes, &totalLeafs);
        partMap = trees[0]->partMap;
        // a host-only copy of the first tree's members for postProcess
        first_.reset(new RTree(numParts, -1));
        first_->nodes = trees[0]->nodes; first_->leafData = trees[0]->leafData; first_->partMap = partMap; first_->partMapType = partMapType;
    }
    bool ensure() { return true; }      // the constructors made the handle
    std::unique_ptr<RTree> first_;
    int device_ = 0;
};

}  // namespace ark
