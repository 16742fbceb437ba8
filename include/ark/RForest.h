// ark/RForest.h — several trained ark::RTree run as one forest, over the C ABI of avt_rforest.h: what the reference's tools do
// with any number of models (rtree-run-dataset.cpp:98-159): RTree::predict per model, the distributions added in model order
// in float32, the arg-max per pixel (the first part whose sum exceeds a running best that starts at 0; 255 when none does).
// The members are ark::RTree's inference side (predictBest, predictBestBatch, predictBestFromBGSub, predict, postProcess,
// numParts, partMap, partMapType), so a forest stands where a tree stands (MultiFrameTracker::attachFrontEnd).  As with
// ark::RTree a failure is fatal (message + exit).
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

class RForest {
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

    /** RTree::predictBest's walk per tree (RTree.cpp:3184-3262), labels from the summed distributions; num_threads is ignored */
    Image8 predictBest(const ImageF& depth, int /*num_threads*/, int interval = 1, Point top_left = Point(0, 0), Point bot_right = Point(-1, -1),
                       bool fill_in_gaps = true) {
        Image8 result(depth.rows, depth.cols, 255);
        if (avt_rforest_predict_best(h_, depth.data(), depth.rows, depth.cols, interval, top_left.x, top_left.y, bot_right.x, bot_right.y,
                                     fill_in_gaps ? 1 : 0, result.data()) != 0)
            die("predictBest");
        return result;
    }

    /** predictBest for a batch of same-size images, image i inside boxes[i] = {tl.x, tl.y, br.x, br.y} (RTree::predictBestBatch) */
    std::vector<Image8> predictBestBatch(const std::vector<ImageF>& depths, int interval, const std::vector<std::array<int, 4>>& boxes,
                                         bool fill_in_gaps = true) {
        if (depths.empty() || depths.size() != boxes.size()) fatal("predictBestBatch", "need one box per depth image, at least one");
        const int rows = depths[0].rows, cols = depths[0].cols;
        std::vector<float> d;
        for (const ImageF& im : depths) {
            if (im.rows != rows || im.cols != cols) fatal("predictBestBatch", "the images must share one size");
            d.insert(d.end(), im.a.begin(), im.a.end());
        }
        if (avt_rforest_images_upload(h_, (int)depths.size(), rows, cols, d.data()) != 0 ||
            avt_rforest_predict_best_resident_boxes(h_, interval, boxes[0].data(), fill_in_gaps ? 1 : 0) != 0)
            die("predictBestBatch");
        return downloadAll((int)depths.size(), rows, cols, "predictBestBatch");
    }

    /** The labels of every image of bgsub's last runBatch, each inside the box that run found, read from the masked depth on the
     *  device (avt_rforest_predict_best_from_bgsub) */
    std::vector<Image8> predictBestFromBGSub(BGSubtractor& bgsub, int interval = 1, bool fill_in_gaps = true, bool download = true) {
        if (bgsub.batchSize() <= 0) fatal("predictBestFromBGSub", "the background subtractor has no batch run behind it");
        if (avt_rforest_predict_best_from_bgsub(h_, bgsub.handle(), interval, fill_in_gaps ? 1 : 0) != 0) die("predictBestFromBGSub");
        if (!download) return {};          // the labels stay on the device (for postProcessFromBGSub)
        return downloadAll(bgsub.batchSize(), bgsub.rows(), bgsub.cols(), "predictBestFromBGSub");
    }

    /** numParts planes of summed distributions, not divided by the number of trees (rtree-run-dataset.cpp:124-138) */
    std::vector<ImageF> predict(const ImageF& depth) {
        const size_t px = (size_t)depth.rows * depth.cols;
        std::vector<float> all((size_t)numParts * px);
        if (avt_rforest_predict(h_, depth.data(), depth.rows, depth.cols, all.data()) != 0) die("predict");
        std::vector<ImageF> result(numParts, ImageF(depth.rows, depth.cols));
        for (int i = 0; i < numParts; ++i) result[i].a.assign(all.begin() + (size_t)i * px, all.begin() + (size_t)(i + 1) * px);
        return result;
    }

    /** RTree::postProcess (RTree.h:150-166) through the first member tree: host code that reads numParts and the part-map type */
    void postProcess(Image8& image, MatrixNX<2>& com_pre, int interval = 1, int num_threads = 1, Point top_left = Point(0, 0),
                     Point bot_right = Point(-1, -1), double dist_to_pre_weight = 0.001) {
        first_->postProcess(image, com_pre, interval, num_threads, top_left, bot_right, dist_to_pre_weight);
    }

    // ---- postProcess for a batch on the device (avt_rforest.h: connected components per part on the interval grid; RTree::postProcess
    // bit for bit at interval 1, a documented difference above it).  Image i of a batch uses memory slot i.
    /** Label images of one size that another classifier made become the images of the last labelling call */
    void uploadLabels(const std::vector<Image8>& labels) {
        if (labels.empty()) fatal("uploadLabels", "need at least one image");
        const int rows = labels[0].rows, cols = labels[0].cols;
        std::vector<uint8_t> all;
        for (const Image8& im : labels) {
            if (im.rows != rows || im.cols != cols) fatal("uploadLabels", "the images must share one size");
            all.insert(all.end(), im.a.begin(), im.a.end());
        }
        if (avt_rforest_labels_upload(h_, (int)labels.size(), rows, cols, all.data()) != 0) die("uploadLabels");
        lastN_ = (int)labels.size(); lastRows_ = rows; lastCols_ = cols;
    }

    /** postProcess on the device, in place on the images of the last labelling call (predictBestBatch, predictBestFromBGSub,
     *  uploadLabels), image i inside boxes[i] = {tl.x, tl.y, br.x, br.y} (none: whole images; tl > br: nothing to do); returns them */
    std::vector<Image8> postProcessResident(int interval = 1, const std::vector<std::array<int, 4>>& boxes = {}, double dist_to_pre_weight = 0.001) {
        if (lastN_ <= 0) fatal("postProcessResident", "no labelled images behind the handle");
        if (!boxes.empty() && (int)boxes.size() != lastN_) fatal("postProcessResident", "need one box per image, or none");
        if (avt_rforest_post_process_resident(h_, interval, boxes.empty() ? nullptr : boxes[0].data(), dist_to_pre_weight) != 0) die("postProcessResident");
        return downloadAll(lastN_, lastRows_, lastCols_, "postProcessResident");
    }

    /** postProcessResident behind predictBestFromBGSub(bgsub, ...): every image inside the box bgsub's last runBatch left on the
     *  device */
    std::vector<Image8> postProcessFromBGSub(BGSubtractor& bgsub, int interval = 1, double dist_to_pre_weight = 0.001) {
        if (bgsub.batchSize() <= 0) fatal("postProcessFromBGSub", "the background subtractor has no batch run behind it");
        if (avt_rforest_post_process_from_bgsub(h_, bgsub.handle(), interval, dist_to_pre_weight) != 0) die("postProcessFromBGSub");
        return downloadAll(bgsub.batchSize(), bgsub.rows(), bgsub.cols(), "postProcessFromBGSub");
    }

    /** com_pre of memory slot `slot` as postProcess keeps it (2 x numParts); a slot that is not sized yet comes back empty */
    MatrixNX<2> comPre(int slot) {
        MatrixNX<2> com;
        com.resize(2, numParts);
        unsigned char valid = 0;
        if (avt_rforest_com_pre_get(h_, slot, 1, com.data(), &valid) != 0) die("comPre");
        if (!valid) com.a.clear();
        return com;
    }
    /** Installs com_pre into memory slot `slot`; one that is not 2 x numParts makes the slot "not sized yet" */
    void setComPre(int slot, const MatrixNX<2>& com_pre) {
        const unsigned char valid = (int)com_pre.cols() == numParts ? 1 : 0;
        std::vector<double> zero(2 * (size_t)numParts, 0.0);
        if (avt_rforest_com_pre_set(h_, slot, 1, valid ? com_pre.data() : zero.data(), &valid) != 0) die("setComPre");
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
    std::vector<Image8> downloadAll(int n, int rows, int cols, const char* what) {
        std::vector<uint8_t> all((size_t)n * rows * cols);
        if (avt_rforest_labels_download_all(h_, all.data()) != 0) die(what);
        lastN_ = n; lastRows_ = rows; lastCols_ = cols;
        std::vector<Image8> result((size_t)n, Image8(rows, cols));
        for (int i = 0; i < n; ++i) result[(size_t)i].a.assign(all.begin() + (size_t)i * rows * cols, all.begin() + (size_t)(i + 1) * rows * cols);
        return result;
    }
    [[noreturn]] void fatal(const char* what, const char* why) {
        std::fprintf(stderr, "FATAL: RForest::%s: %s\n", what, why);
        std::exit(1);
    }
    [[noreturn]] void die(const char* what) {
        std::fprintf(stderr, "FATAL: RForest::%s: %s\n", what, avt_last_error());
        std::exit(1);
    }
    avt_rforest* h_ = nullptr;
    std::unique_ptr<RTree> first_;
    int device_ = 0;
    int lastN_ = 0, lastRows_ = 0, lastCols_ = 0;   // the images of the last labelling call
};

}  // namespace ark
