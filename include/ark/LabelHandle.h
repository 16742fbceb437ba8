// ark/LabelHandle.h — what ark::RTree and ark::RForest share: the image side of a labelling handle over the C ABI (avt_rtree.h,
// avt_rforest.h name the same entry points for the two kinds).  predictBest and predict, the batch with one box per image, the
// hand-over from the background subtractor, postProcess for a batch on the device with its per-slot memory.  cv::Mat is
// replaced by the two plain row-major images below, cv::Point by ark::Point, Eigen::Matrix<double,2,Dynamic> by MatrixNX<2>
// (same column-major layout).  As in the reference a failure is fatal (message + exit, RTree.cpp:2984-2996).
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../avt.h"
#include "Types.h"

namespace ark {

struct Point {  // cv::Point stand-in
    int x = 0, y = 0;
    Point() {}
    Point(int x_, int y_) : x(x_), y(y_) {}
};

template <class T>
struct Image {  // row-major rows x cols, the layout of a continuous single-channel cv::Mat
    int rows = 0, cols = 0;
    std::vector<T> a;
    Image() {}
    Image(int r, int c, T fill = T()) : rows(r), cols(c), a((size_t)r * c, fill) {}
    T& at(int r, int c) { return a[(size_t)r * cols + c]; }
    T at(int r, int c) const { return a[(size_t)r * cols + c]; }
    T* ptr(int r) { return a.data() + (size_t)r * cols; }
    const T* ptr(int r) const { return a.data() + (size_t)r * cols; }
    T* data() { return a.data(); }
    const T* data() const { return a.data(); }
};
using ImageF = Image<float>;      // CV_32F depth, metres, 0 = background
using Image8 = Image<uint8_t>;    // CV_8U part labels, 255 = none

class BGSubtractor;   // ark/BGSubtractor.h, which defines the two members that take one

/** D: the class itself (it has numParts and bool ensure(), which makes the C handle h_ exist or says there is none).  Api: the
 *  C handle's type, the class name of the FATAL lines, and the kind's entry points. */
template <class D, class Api>
class LabelHandle {
public:
    /** Predict best match for each pixel in image (RTree.h:63-81; a forest: RTree::predictBest's walk per tree, RTree.cpp:3184-3262,
     *  labels from the summed distributions); num_threads is accepted and ignored (GPU). */
    Image8 predictBest(const ImageF& depth, int /*num_threads*/, int interval = 1, Point top_left = Point(0, 0), Point bot_right = Point(-1, -1),
                       bool fill_in_gaps = true) {
        Image8 result(depth.rows, depth.cols, 255);
        if (!self().ensure() || Api::predict_best(h_, depth.data(), depth.rows, depth.cols, interval, top_left.x, top_left.y, bot_right.x, bot_right.y,
                                                  fill_in_gaps ? 1 : 0, result.data()) != 0)
            die("predictBest");
        return result;
    }

    /** predictBest for a batch of same-size images, image i inside boxes[i] = {tl.x, tl.y, br.x, br.y} (the labelling of
     *  demo.cpp:179-204 for many streams in one launch): br.x == -1 is the whole image, an empty box (tl > br) leaves its image
     *  all 255.  One upload, one launch sequence, one download. */
    std::vector<Image8> predictBestBatch(const std::vector<ImageF>& depths, int interval, const std::vector<std::array<int, 4>>& boxes,
                                         bool fill_in_gaps = true) {
        if (depths.empty() || depths.size() != boxes.size()) fatal("predictBestBatch", "need one box per depth image, at least one");
        const int rows = depths[0].rows, cols = depths[0].cols;
        std::vector<float> d;
        for (const ImageF& im : depths) {
            if (im.rows != rows || im.cols != cols) fatal("predictBestBatch", "the images must share one size");
            d.insert(d.end(), im.a.begin(), im.a.end());
        }
        if (!self().ensure() || Api::images_upload(h_, (int)depths.size(), rows, cols, d.data()) != 0 ||
            Api::predict_best_resident_boxes(h_, interval, boxes[0].data(), fill_in_gaps ? 1 : 0) != 0)
            die("predictBestBatch");
        return downloadAll((int)depths.size(), rows, cols, "predictBestBatch");
    }

    /** The labels of every image of bgsub's last runBatch, each inside the box that run found, read from the masked depth on the
     *  device (demo.cpp:179-204 without the host in between; avt_*_predict_best_from_bgsub).  download = false leaves them
     *  there (for postProcessFromBGSub) and returns nothing.  Defined in ark/BGSubtractor.h. */
    std::vector<Image8> predictBestFromBGSub(BGSubtractor& bgsub, int interval = 1, bool fill_in_gaps = true, bool download = true);

    /** Predict distribution for all of image: numParts planes of CV_32F (RTree.h:59-61); a forest's are its trees' added in tree
     *  order, not divided by their number (rtree-run-dataset.cpp:124-138) */
    std::vector<ImageF> predict(const ImageF& depth) {
        const int np = self().numParts;
        const size_t px = (size_t)depth.rows * depth.cols;
        std::vector<float> all((size_t)np * px);
        if (!self().ensure() || Api::predict(h_, depth.data(), depth.rows, depth.cols, all.data()) != 0) die("predict");
        std::vector<ImageF> result(np, ImageF(depth.rows, depth.cols));
        for (int i = 0; i < np; ++i) result[i].a.assign(all.begin() + (size_t)i * px, all.begin() + (size_t)(i + 1) * px);
        return result;
    }

    // ---- postProcess for a batch on the device (avt_rtree.h: connected components per part on the interval grid; RTree::postProcess
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
        if (!self().ensure() || Api::labels_upload(h_, (int)labels.size(), rows, cols, all.data()) != 0) die("uploadLabels");
        lastN_ = (int)labels.size(); lastRows_ = rows; lastCols_ = cols;
    }

    /** postProcess on the device, in place on the images of the last labelling call (predictBestBatch, predictBestFromBGSub,
     *  uploadLabels), image i inside boxes[i] = {tl.x, tl.y, br.x, br.y} (none: whole images; tl > br: nothing to do); returns them */
    std::vector<Image8> postProcessResident(int interval = 1, const std::vector<std::array<int, 4>>& boxes = {}, double dist_to_pre_weight = 0.001) {
        if (lastN_ <= 0) fatal("postProcessResident", "no labelled images behind the handle");
        if (!boxes.empty() && (int)boxes.size() != lastN_) fatal("postProcessResident", "need one box per image, or none");
        if (Api::post_process_resident(h_, interval, boxes.empty() ? nullptr : boxes[0].data(), dist_to_pre_weight) != 0) die("postProcessResident");
        return downloadAll(lastN_, lastRows_, lastCols_, "postProcessResident");
    }

    /** postProcessResident behind predictBestFromBGSub(bgsub, ...): every image inside the box bgsub's last runBatch left on the
     *  device.  Defined in ark/BGSubtractor.h. */
    std::vector<Image8> postProcessFromBGSub(BGSubtractor& bgsub, int interval = 1, double dist_to_pre_weight = 0.001);

    /** com_pre of memory slot `slot` as postProcess keeps it (2 x numParts); a slot that is not sized yet comes back empty */
    MatrixNX<2> comPre(int slot) {
        MatrixNX<2> com;
        com.resize(2, self().numParts);
        unsigned char valid = 0;
        if (!self().ensure() || Api::com_pre_get(h_, slot, 1, com.data(), &valid) != 0) die("comPre");
        if (!valid) com.a.clear();
        return com;
    }
    /** Installs com_pre into memory slot `slot`; one that is not 2 x numParts makes the slot "not sized yet" */
    void setComPre(int slot, const MatrixNX<2>& com_pre) {
        const unsigned char valid = (int)com_pre.cols() == self().numParts ? 1 : 0;
        std::vector<double> zero(2 * (size_t)self().numParts, 0.0);
        if (!self().ensure() || Api::com_pre_set(h_, slot, 1, valid ? com_pre.data() : zero.data(), &valid) != 0) die("setComPre");
    }

protected:
    std::vector<Image8> downloadAll(int n, int rows, int cols, const char* what) {
        std::vector<uint8_t> all((size_t)n * rows * cols);
        if (Api::labels_download_all(h_, all.data()) != 0) die(what);
        lastN_ = n; lastRows_ = rows; lastCols_ = cols;
        std::vector<Image8> result((size_t)n, Image8(rows, cols));
        for (int i = 0; i < n; ++i) result[(size_t)i].a.assign(all.begin() + (size_t)i * rows * cols, all.begin() + (size_t)(i + 1) * rows * cols);
        return result;
    }
    [[noreturn]] void fatal(const char* what, const char* why) {
        fprintf(stderr, "FATAL: %s::%s: %s\n", Api::name, what, why);
        std::exit(1);
    }
    [[noreturn]] void die(const char* what) { fatal(what, avt_last_error()); }
    typename Api::Handle* h_ = nullptr;
    int lastN_ = 0, lastRows_ = 0, lastCols_ = 0;   // the images of the last labelling call

private:
    D& self() { return *static_cast<D*>(this); }
};

}  // namespace ark
