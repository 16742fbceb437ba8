// ark/BGSubtractor.h — the reference's `ark::BGSubtractor` (include/BGSubtractor.h, BGSubtractor.cpp:10-163) re-created
// over the C ABI of avt_bgsub.h: same class name, member names, defaults and call protocol (run, nnDistThreshRel,
// neighbThreshRel, numThreads, background, topLeft, botRight), computed on the GPU with the reference's result bit for bit.
// cv::Mat is replaced by the row-major images of ark/RTree.h (Image8 for the mask) and ImageXYZ below for the CV_32FC3
// XYZ maps, cv::Point by ark::Point.  The handle is created on the first run() and again when `background` changes size.
// Beyond the reference: runBatch() runs many streams' images in one launch sequence, image i against backgrounds[i], and
// leaves the masked depth and the boxes on the device for RTree::predictBestFromBGSub.
#pragma once
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../avt_bgsub.h"
#include "RTree.h"

namespace ark {

struct ImageXYZ {  // row-major rows x cols x 3 float32, the layout of a continuous CV_32FC3 cv::Mat (cv::Vec3f per pixel)
    int rows = 0, cols = 0;
    std::vector<float> a;
    ImageXYZ() {}
    ImageXYZ(int r, int c, float fill = 0.f) : rows(r), cols(c), a((size_t)r * c * 3, fill) {}
    float* at(int r, int c) { return a.data() + ((size_t)r * cols + c) * 3; }
    const float* at(int r, int c) const { return a.data() + ((size_t)r * cols + c) * 3; }
    float* data() { return a.data(); }
    const float* data() const { return a.data(); }
    bool empty() const { return a.empty(); }
};

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
        Image8 mask(image.rows, image.cols, 255);
        if (!ensure(image)) die("run");
        maskedDepth_ = ImageF(image.rows, image.cols);
        avt_bgsub_frame f;
        f.top_left[0] = topLeft.x; f.top_left[1] = topLeft.y; f.bot_right[0] = botRight.x; f.bot_right[1] = botRight.y;
        if (avt_bgsub_run(h_, 0, image.data(), nnDistThreshRel, neighbThreshRel, mask.data(), maskedDepth_.data(), &f) != 0) die("run");
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
        if (images.empty() || !ensure(images[0]) || (!bg_index.empty() && bg_index.size() != images.size()) ||
            (prev_boxes && prev_boxes->size() != images.size())) die("runBatch");
        std::vector<float> all;
        for (const ImageXYZ& im : images) {
            if (im.rows != rows_ || im.cols != cols_) die("runBatch");
            all.insert(all.end(), im.a.begin(), im.a.end());
        }
        if (avt_bgsub_images_upload(h_, (int)images.size(), all.data(), bg_index.empty() ? nullptr : bg_index.data(),
                                    prev_boxes ? (*prev_boxes)[0].data() : nullptr) != 0 ||
            avt_bgsub_run_resident(h_, nnDistThreshRel, neighbThreshRel) != 0)
            die("runBatch");
        batch_ = (int)images.size();
    }
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
    bool ensure(const ImageXYZ& image) {
        if (image.rows != background.rows || image.cols != background.cols || background.empty()) return false;
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

inline std::vector<Image8> RTree::predictBestFromBGSub(BGSubtractor& bgsub, int interval, bool fill_in_gaps) {
    if (bgsub.batchSize() <= 0) fatal("predictBestFromBGSub", "the background subtractor has no batch run behind it");
    if (!ensure() || avt_rtree_predict_best_from_bgsub(h_, bgsub.handle(), interval, fill_in_gaps ? 1 : 0) != 0) die("predictBestFromBGSub");
    return downloadAll(bgsub.batchSize(), bgsub.rows(), bgsub.cols(), "predictBestFromBGSub");
}

}  // namespace ark
