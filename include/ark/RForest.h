// ark/RForest.h — several trained ark::RTree run as one forest, over the C ABI of avt_rforest.h: what the reference's tools do
// with any number of models (rtree-run-dataset.cpp:98-159): RTree::predict per model, the distributions added in model order
// in float32, the arg-max per pixel (the first part whose sum exceeds a running best that starts at 0; 255 when none does).
// The members are ark::RTree's inference side (predictBest, predictBestBatch, predictBestFromBGSub, predict, postProcess,
// numParts, partMap, partMapType), so a forest stands where a tree stands (MultiFrameTracker::attachFrontEnd).  As with
// ark::RTree a failure is fatal (message + exit).
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../avt.h"
#include "../avt_rforest.h"
#include "BGSubtractor.h"
#include "RTree.h"

namespace ark {

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
    std::vector<Image8> predictBestFromBGSub(BGSubtractor& bgsub, int interval = 1, bool fill_in_gaps = true) {
        if (bgsub.batchSize() <= 0) fatal("predictBestFromBGSub", "the background subtractor has no batch run behind it");
        if (avt_rforest_predict_best_from_bgsub(h_, bgsub.handle(), interval, fill_in_gaps ? 1 : 0) != 0) die("predictBestFromBGSub");
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

    int numTrees = 0;
    int numParts = 0;
    std::vector<int> partMap;
    int partMapType = 0;
    int totalNodes = 0, totalLeafs = 0;

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
};

}  // namespace ark
