// ark/BGSubtractor.h — the reference's `ark::BGSubtractor` (include/BGSubtractor.h, BGSubtractor.cpp:10-163) re-created
// over the C ABI of avt_bgsub.h: same class name, member names, defaults and call protocol (run, nnDistThreshRel,
// neighbThreshRel, numThreads, background, topLeft, botRight), computed on the GPU with the reference's result bit for bit.
// cv::Mat is replaced by the row-major images of ark/RTree.h (Image8 for the mask) and ImageXYZ below for the CV_32FC3
// XYZ maps, cv::Point by ark::Point.  The handle is created on the first run() and again when `background` changes size.
#pragma once
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
        topLeft = Point(f.top_left[0], f.top_left[1]);
        botRight = Point(f.bot_right[0], f.bot_right[1]);
        fgCount_ = f.fg_count;
        if (comps_by_size) {
            comps_by_size->clear();
            for (int i = 0; i < f.n_comps; ++i) comps_by_size->push_back({f.comps[i][0], f.comps[i][1]});
        }
        return mask;
    }

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
    /** Current top left and bottom right points of foreground */
    Point topLeft, botRight;

private:
    // (re)creates the handle when the background's size changed, uploads the background when its contents did
    bool ensure(const ImageXYZ& image) {
        if (image.rows != background.rows || image.cols != background.cols || background.empty()) return false;
        if (!h_ || rows_ != background.rows || cols_ != background.cols) {
            avt_bgsub_destroy(h_);
            h_ = nullptr;
            if (avt_bgsub_create(device_, 1, background.rows, background.cols, background.data(), &h_) != 0) return false;
            rows_ = background.rows; cols_ = background.cols; uploaded_ = background.a;
        } else if (uploaded_ != background.a) {
            if (avt_bgsub_set_background(h_, 0, background.data()) != 0) return false;
            uploaded_ = background.a;
        }
        return true;
    }
    [[noreturn]] void die(const char* what) {
        fprintf(stderr, "FATAL: BGSubtractor::%s: %s\n", what, avt_last_error());
        std::exit(1);
    }
    avt_bgsub* h_ = nullptr;
    int device_ = 0, rows_ = 0, cols_ = 0, fgCount_ = 0;
    std::vector<float> uploaded_;
    ImageF maskedDepth_;
};

}  // namespace ark
