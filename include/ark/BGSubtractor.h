// ark/BGSubtractor.h — the reference's `ark::BGSubtractor` (include/BGSubtractor.h, BGSubtractor.cpp:10-163) re-created
// over the C ABI of avt_bgsub.h: same class name, member names, defaults and call protocol (run, nnDistThreshRel,
// neighbThreshRel, numThreads, background, topLeft, botRight), computed on the GPU with the reference's result bit for bit.
// cv::Mat is replaced by the row-major images of ark/RTree.h (Image8 for the mask) and of ark/Types.h (ImageXYZ for the
// CV_32FC3 XYZ maps, ImageDepth for CV_32FC1 depth images), cv::Point by ark::Point.  The handle is created on the first run() and again when `background` changes size.
// Beyond the reference: runBatch() runs many streams' images in one launch sequence, image i against backgrounds[i], and
// leaves the masked depth and the boxes on the device for RTree::predictBestFromBGSub.  runDepth(), runBatchDepth() and
// setBackgroundDepth() take depth images and their cameras in place of XYZ maps (the recorded-data path, demo.cpp:126,166): the
// depth crosses the bus and CameraIntrin::depthToXYZ runs on the device; xyz() fetches a resident map.
#pragma once
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../avt_bgsub.h"
#include "RTree.h"

namespace ark {

class BGSubtractor {
public:
    /** Create background subtractor with given background image */
    explicit BGSubtractor(ImageXYZ background, int device = 0) : background(std::move(background)), device_(device) {}
    /** One background per stream (the batch form); `background` is the first of them */
    explicit BGSubtractor(std::vector<ImageXYZ> backgrounds_, int device = 0)
        : background(backgrounds_.empty() ? ImageXYZ() : backgrounds_[0]), backgrounds(std::move(backgrounds_)), device_(device) {}
    ~BGSubtractor() { avt_bgsub_destroy(h_); }
    BGSubtractor(const BGSubtractor&) = delete;
    BGSubtractor& operator=(const BGSubtractor&) = delete;

    /** Run background subtraction on image and return a mask: 0..253 component ids, 254 / 255 background
     *  (BGSubtractor.cpp:159-163).  Optionally fills comps_by_size with (pixels in component, component id). */
    Image8 run(const ImageXYZ& image, std::vector<std::array<int, 2>>* comps_by_size = nullptr) {
        return runAny(image.rows, image.cols, image.data(), nullptr, comps_by_size);
    }
    /** run() on a depth image and its camera: the XYZ map is CameraIntrin::depthToXYZ's, built on the device */
    Image8 runDepth(const ImageDepth& depth, const CameraIntrin& intrin, std::vector<std::array<int, 2>>* comps_by_size = nullptr) {
        return runAny(depth.rows, depth.cols, depth.data(), &intrin, comps_by_size);
    }

private:
    static std::array<float, 4> camera(const CameraIntrin& k) { return {k.fx, k.fy, k.cx, k.cy}; }
    Image8 runAny(int rows, int cols, const float* src, const CameraIntrin* intrin, std::vector<std::array<int, 2>>* comps_by_size) {
        const char* who = intrin ? "runDepth" : "run";
        Image8 mask(rows, cols, 255);
        if (!ensure(rows, cols)) die(who);
        maskedDepth_ = ImageF(rows, cols);
        avt_bgsub_frame f;
        f.top_left[0] = topLeft.x; f.top_left[1] = topLeft.y; f.bot_right[0] = botRight.x; f.bot_right[1] = botRight.y;
        if ((intrin ? avt_bgsub_run_depth(h_, 0, src, camera(*intrin).data(), nnDistThreshRel, neighbThreshRel, mask.data(), maskedDepth_.data(), &f)
                    : avt_bgsub_run(h_, 0, src, nnDistThreshRel, neighbThreshRel, mask.data(), maskedDepth_.data(), &f)) != 0) die(who);
        batch_ = 0;                                   // slot 0 now holds this image: no batch run behind the handle
        topLeft = Point(f.top_left[0], f.top_left[1]);
        botRight = Point(f.bot_right[0], f.bot_right[1]);
        fgCount_ = f.fg_count;
        if (comps_by_size) {
            comps_by_size->clear();
            for (int i = 0; i < f.n_comps; ++i) comps_by_size->push_back({f.comps[i][0], f.comps[i][1]});
        }
        return mask;
    }

public:
    /** bgsub.background = ... (live-demo.cpp:207) from a depth image: `background` (index 0) or backgrounds[index] becomes
     *  intrin.depthToXYZ(depth) (the members are the reference's, a caller may read them, so the host expands too); with a handle
     *  of that size alive the depth is what crosses the bus and the device expands it for itself */
    void setBackgroundDepth(const ImageDepth& depth, const CameraIntrin& intrin, int index = 0) {
        const int nbg = backgrounds.empty() ? 1 : (int)backgrounds.size();
        if (index < 0 || index >= nbg || depth.empty()) { fprintf(stderr, "FATAL: BGSubtractor::setBackgroundDepth: no background %d, or an empty image\n", index); std::exit(1); }
        const bool live = h_ && ensure(depth.rows, depth.cols);     // (brings the device up to date with any other edit first)
        ImageXYZ xyz = intrin.depthToXYZ(depth);
        if (live) {
            if (avt_bgsub_set_background_depth(h_, index, depth.data(), camera(intrin).data()) != 0) die("setBackgroundDepth");
            std::copy(xyz.a.begin(), xyz.a.end(), uploaded_.begin() + (size_t)index * xyz.a.size());
        }
        if (index == 0) background = xyz;
        if (!backgrounds.empty()) backgrounds[(size_t)index] = std::move(xyz);
    }

    /** One image's record of a batch run */
    struct BatchInfo {
        Point topLeft, botRight;
        bool capped = false;
        int fgCount = 0;
    };

    /** Batch form: image i against background i of `backgrounds` (or bg_index[i]).  prev_boxes: {tl.x, tl.y, br.x, br.y} per image,
     *  null: every slot keeps the box of its previous batch run ((0,0),(0,0) at first).  Queues the run; batchInfo / batchMask /
     *  batchMaskedDepth wait for it and fetch one image's part. */
    void runBatch(const std::vector<ImageXYZ>& images, const std::vector<int>& bg_index = {}, const std::vector<std::array<int, 4>>* prev_boxes = nullptr) {
        runBatchAny(images, nullptr, bg_index, prev_boxes);
    }
    /** runBatch() on depth images; intrins: one camera per image, or one for all of them */
    void runBatchDepth(const std::vector<ImageDepth>& depths, const std::vector<CameraIntrin>& intrins, const std::vector<int>& bg_index = {},
                       const std::vector<std::array<int, 4>>* prev_boxes = nullptr) {
        if (intrins.size() != depths.size() && intrins.size() != 1) die("runBatchDepth");
        runBatchAny(depths, &intrins, bg_index, prev_boxes);
    }
    /** The resident XYZ map of image i of the last run, runBatch or their depth forms */
    ImageXYZ xyz(int i) {
        ImageXYZ m(rows_, cols_);
        if (!h_ || avt_bgsub_xyz_download(h_, i, m.data()) != 0) die("xyz");
        return m;
    }

private:
    template <class Img>
    void runBatchAny(const std::vector<Img>& images, const std::vector<CameraIntrin>* intrins, const std::vector<int>& bg_index,
                     const std::vector<std::array<int, 4>>* prev_boxes) {
        const char* who = intrins ? "runBatchDepth" : "runBatch";
        if (images.empty() || !ensure(images[0].rows, images[0].cols) || (!bg_index.empty() && bg_index.size() != images.size()) ||
            (prev_boxes && prev_boxes->size() != images.size())) die(who);
        std::vector<float> all, cams;
        for (size_t i = 0; i < images.size(); ++i) {
            if (images[i].rows != rows_ || images[i].cols != cols_) die(who);
            all.insert(all.end(), images[i].a.begin(), images[i].a.end());
            if (intrins) { const std::array<float, 4> k = camera((*intrins)[intrins->size() == 1 ? 0 : i]); cams.insert(cams.end(), k.begin(), k.end()); }
        }
        const int* bi = bg_index.empty() ? nullptr : bg_index.data();
        const int* pb = prev_boxes ? (*prev_boxes)[0].data() : nullptr;
        if ((intrins ? avt_bgsub_depth_upload(h_, (int)images.size(), all.data(), cams.data(), bi, pb)
                     : avt_bgsub_images_upload(h_, (int)images.size(), all.data(), bi, pb)) != 0 ||
            avt_bgsub_run_resident(h_, nnDistThreshRel, neighbThreshRel) != 0)
            die(who);
        batch_ = (int)images.size();
    }

public:
    int batchSize() const { return batch_; }
    BatchInfo batchInfo(int i) {
        avt_bgsub_frame f;
        if (avt_bgsub_download(h_, i, nullptr, nullptr, &f) != 0) die("batchInfo");
        BatchInfo b;
        b.topLeft = Point(f.top_left[0], f.top_left[1]); b.botRight = Point(f.bot_right[0], f.bot_right[1]);
        b.capped = f.capped != 0; b.fgCount = f.fg_count;
        return b;
    }
    Image8 batchMask(int i) {
        Image8 m(rows_, cols_, 255);
        if (avt_bgsub_download(h_, i, m.data(), nullptr, nullptr) != 0) die("batchMask");
        return m;
    }
    ImageF batchMaskedDepth(int i) {
        ImageF d(rows_, cols_);
        if (avt_bgsub_download(h_, i, nullptr, d.data(), nullptr) != 0) die("batchMaskedDepth");
        return d;
    }
    /** The C handle and the image size (RTree::predictBestFromBGSub) */
    avt_bgsub* handle() const { return h_; }
    int rows() const { return rows_; }
    int cols() const { return cols_; }

    /** Channel 2 of the last image with 0 inside [topLeft, botRight] where the mask is >= 254 (demo.cpp:183-192) */
    const ImageF& maskedDepth() const { return maskedDepth_; }
    /** Pixels with mask < 254 inside [topLeft, botRight] of the last run (live-demo.cpp:318-332's subCnz) */
    int foregroundCount() const { return fgCount_; }

    /** Minimum distance to neighbor in background image to consider a point foreground */
    float nnDistThreshRel = 0.005;
    /** Max squared distance to a neighbor, for flood fill */
    float neighbThreshRel = 0.005;
    /** Max allowed number of threads for background subtractor (accepted, unused: the GPU runs it) */
    int numThreads = 1;
    /** The background image */
    ImageXYZ background;
    /** The batch form's backgrounds, one per stream; empty: `background` alone */
    std::vector<ImageXYZ> backgrounds;
    /** Current top left and bottom right points of foreground */
    Point topLeft, botRight;

private:
    // (re)creates the handle when the background's size changed, uploads the background when its contents did
    bool ensure(int rows, int cols) {
        if (rows != background.rows || cols != background.cols || background.empty()) return false;
        // background 0 is `background` (the reference's member); the batch form's further backgrounds follow it
        const int nbg = backgrounds.empty() ? 1 : (int)backgrounds.size();
        std::vector<float> all(background.a);
        for (int i = 1; i < nbg; ++i) {
            if (backgrounds[(size_t)i].rows != background.rows || backgrounds[(size_t)i].cols != background.cols) return false;
            all.insert(all.end(), backgrounds[(size_t)i].a.begin(), backgrounds[(size_t)i].a.end());
        }
        if (!h_ || rows_ != background.rows || cols_ != background.cols || nbg_ != nbg) {
            avt_bgsub_destroy(h_);
            h_ = nullptr;
            batch_ = 0;
            if (avt_bgsub_create(device_, nbg, background.rows, background.cols, all.data(), &h_) != 0) return false;
            rows_ = background.rows; cols_ = background.cols; nbg_ = nbg; uploaded_ = all;
        } else if (uploaded_ != all) {
            const size_t n = (size_t)rows_ * cols_ * 3;
            for (int i = 0; i < nbg; ++i)
                if (!std::equal(all.begin() + i * n, all.begin() + (i + 1) * n, uploaded_.begin() + i * n) &&
                    avt_bgsub_set_background(h_, i, all.data() + i * n) != 0) return false;
            uploaded_ = all;
        }
        return true;
    }
    [[noreturn]] void die(const char* what) {
        fprintf(stderr, "FATAL: BGSubtractor::%s: %s\n", what, avt_last_error());
        std::exit(1);
    }
    avt_bgsub* h_ = nullptr;
    int device_ = 0, rows_ = 0, cols_ = 0, fgCount_ = 0, nbg_ = 0, batch_ = 0;
    std::vector<float> uploaded_;
    ImageF maskedDepth_;
};

template <class D, class Api>
inline std::vector<Image8> LabelHandle<D, Api>::predictBestFromBGSub(BGSubtractor& bgsub, int interval, bool fill_in_gaps, bool download) {
    if (bgsub.batchSize() <= 0) fatal("predictBestFromBGSub", "the background subtractor has no batch run behind it");
    if (!self().ensure() || Api::predict_best_from_bgsub(h_, bgsub.handle(), interval, fill_in_gaps ? 1 : 0) != 0) die("predictBestFromBGSub");
    if (!download) return {};
    return downloadAll(bgsub.batchSize(), bgsub.rows(), bgsub.cols(), "predictBestFromBGSub");
}

template <class D, class Api>
inline std::vector<Image8> LabelHandle<D, Api>::postProcessFromBGSub(BGSubtractor& bgsub, int interval, double dist_to_pre_weight) {
    if (bgsub.batchSize() <= 0) fatal("postProcessFromBGSub", "the background subtractor has no batch run behind it");
    if (!self().ensure() || Api::post_process_from_bgsub(h_, bgsub.handle(), interval, dist_to_pre_weight) != 0) die("postProcessFromBGSub");
    return downloadAll(bgsub.batchSize(), bgsub.rows(), bgsub.cols(), "postProcessFromBGSub");
}

}  // namespace ark
