// ark/FitScore.h — the fit score over the C ABI of avt_fitscore.h: what the reference leaves to the eye (live-demo.cpp:428-445
// renders the avatar over the camera image) as integers.  ark::FitScore is one image's (numParts + 1) x 7 table with the figures
// derived from it; ark::FitScorer is the handle that counts the tables on the GPU.  Header-only, no OpenCV: images are the
// row-major ImageF / Image8 of ark/RTree.h.
//
// avt_fitscore.h states the rule.  No threshold on any figure is offered: nobody has measured what a good or a bad fit scores on
// real data.  The default tolerance is a choice, not a measurement.
#pragma once
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../avt.h"
#include "../avt_bgsub.h"
#include "../avt_fitscore.h"
#include "../avt_render.h"
#include "RTree.h"

namespace ark {

/** The figures derived from a table row or from the column sums: integer sums first, each converted to double once, then one
 *  division (and for the errors one multiplication by 1e-6); NaN on a zero denominator.  iou and unexplained are NaN for a row:
 *  DATA_ONLY has no part. */
struct FitFigures {
    double iou, agree, violation, unexplained, meanAbsErr, meanAbsErrAgree;
};

/** One image's table: at(p, AVT_FITSCORE_*) for part p, row numParts for pixels without a part. */
struct FitScore {
    static constexpr float kDefaultTol = 0.05f;      // metres; a choice, not a measurement
    int numParts = 0;
    std::vector<long long> table;                    // (numParts + 1) x AVT_FITSCORE_COLS, row-major

    long long at(int row, int col) const { return table[(size_t)row * AVT_FITSCORE_COLS + col]; }
    /** the column sum over all rows */
    long long total(int col) const {
        long long s = 0;
        for (int p = 0; p <= numParts; ++p) s += at(p, col);
        return s;
    }
    /** the figures of the whole image */
    FitFigures derive() const {
        std::array<long long, AVT_FITSCORE_COLS> c;
        for (int k = 0; k < AVT_FITSCORE_COLS; ++k) c[(size_t)k] = total(k);
        return figures(c.data(), true);
    }
    /** the figures of one row: part p, or numParts for the pixels without a part */
    FitFigures derive(int row) const { return figures(&table[(size_t)row * AVT_FITSCORE_COLS], false); }
    // per part: which limb is off
    double agree(int part) const { return derive(part).agree; }
    double violation(int part) const { return derive(part).violation; }
    double meanAbsErr(int part) const { return derive(part).meanAbsErr; }
    double meanAbsErrAgree(int part) const { return derive(part).meanAbsErrAgree; }

   private:
    static double ratio(long long a, long long b) { return b == 0 ? std::numeric_limits<double>::quiet_NaN() : (double)a / (double)b; }
    static FitFigures figures(const long long* c, bool whole) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const long long both = c[AVT_FITSCORE_AGREE] + c[AVT_FITSCORE_IN_FRONT] + c[AVT_FITSCORE_BEHIND];
        FitFigures f;
        f.iou = whole ? ratio(both, both + c[AVT_FITSCORE_MODEL_ONLY] + c[AVT_FITSCORE_DATA_ONLY]) : nan;
        f.agree = ratio(c[AVT_FITSCORE_AGREE], both);
        f.violation = ratio(c[AVT_FITSCORE_IN_FRONT] + c[AVT_FITSCORE_MODEL_ONLY], both + c[AVT_FITSCORE_MODEL_ONLY]);
        f.unexplained = whole ? ratio(c[AVT_FITSCORE_BEHIND] + c[AVT_FITSCORE_DATA_ONLY], both + c[AVT_FITSCORE_DATA_ONLY]) : nan;
        f.meanAbsErr = ratio(c[AVT_FITSCORE_ABS_UM], both) * 1e-6;
        f.meanAbsErrAgree = ratio(c[AVT_FITSCORE_ABS_UM_AGREE], c[AVT_FITSCORE_AGREE]) * 1e-6;
        return f;
    }
};

/** The handle: tables of up to max_images images per call.  Every scoring call returns one FitScore per image and replaces the
 *  previous result.  A failure (a part-mask byte >= num_parts that is not 255 at a selected pixel among them) is fatal, like
 *  every failure of this facade. */
class FitScorer {
   public:
    FitScorer(int num_parts, int max_images = 64, int device = 0) : numParts(num_parts) {
        if (avt_fitscore_create(device, num_parts, max_images, &h_) != 0) die("FitScorer");
    }
    ~FitScorer() { avt_fitscore_destroy(h_); }
    FitScorer(const FitScorer&) = delete;
    FitScorer& operator=(const FitScorer&) = delete;

    /** Host images (live-demo.cpp:428-445 in numbers): renderDepth, renderPartMask and the observed depth of every image; boxes
     *  {tl.x, tl.y, br.x, br.y} inclusive, br.x == -1 the whole image, empty: whole images. */
    std::vector<FitScore> score(const std::vector<ImageF>& model_depth, const std::vector<Image8>& model_mask, const std::vector<ImageF>& observed,
                                const std::vector<std::array<int, 4>>& boxes = {}, float tol = FitScore::kDefaultTol, int stride = 1) {
        const size_t n = model_depth.size();
        if (n == 0 || model_mask.size() != n || observed.size() != n || (!boxes.empty() && boxes.size() != n))
            fatal("score", "need as many part masks, observed images and boxes as model depth images, at least one");
        const int rows = model_depth[0].rows, cols = model_depth[0].cols;
        std::vector<float> r, d;
        std::vector<unsigned char> m;
        for (size_t i = 0; i < n; ++i) {
            if (model_depth[i].rows != rows || model_depth[i].cols != cols || model_mask[i].rows != rows || model_mask[i].cols != cols ||
                observed[i].rows != rows || observed[i].cols != cols)
                fatal("score", "the images must share one size");
            r.insert(r.end(), model_depth[i].a.begin(), model_depth[i].a.end());
            m.insert(m.end(), model_mask[i].a.begin(), model_mask[i].a.end());
            d.insert(d.end(), observed[i].a.begin(), observed[i].a.end());
        }
        if (avt_fitscore_images(h_, (int)n, rows, cols, r.data(), m.data(), d.data(), boxes.empty() ? nullptr : boxes[0].data(), tol, stride) != 0) die("score");
        return get();
    }

    /** The model side read where the renderer's last AVT_RENDER_DEPTH | AVT_RENDER_PART_MASK run left it; observed and boxes on
     *  the host, one per rendered image. */
    std::vector<FitScore> scoreRendered(avt_renderer* renderer, const std::vector<ImageF>& observed, const std::vector<std::array<int, 4>>& boxes = {},
                                        float tol = FitScore::kDefaultTol, int stride = 1) {
        if (observed.empty() || (!boxes.empty() && boxes.size() != observed.size())) fatal("scoreRendered", "need one observed image and one box per rendered image");
        std::vector<float> d;
        for (const ImageF& im : observed) {
            if (im.rows != observed[0].rows || im.cols != observed[0].cols) fatal("scoreRendered", "the images must share one size");
            d.insert(d.end(), im.a.begin(), im.a.end());
        }
        if (avt_fitscore_rendered(h_, renderer, d.data(), boxes.empty() ? nullptr : boxes[0].data(), tol, stride) != 0) die("scoreRendered");
        const std::vector<FitScore> out = get();
        if (out.size() != observed.size()) fatal("scoreRendered", "the renderer's last run holds another number of images than were given");
        return out;
    }

    /** Both sides where they lie: image i of the renderer's last run against image obs_index[i] (empty: i) of the background
     *  subtractor's last batch run, its masked depth inside the box that run found.  No image is copied. */
    std::vector<FitScore> scoreRenderedFromBGSub(avt_renderer* renderer, avt_bgsub* bgsub, const std::vector<int>& obs_index = {},
                                                 float tol = FitScore::kDefaultTol, int stride = 1) {
        if (avt_fitscore_rendered_from_bgsub(h_, renderer, bgsub, obs_index.empty() ? nullptr : obs_index.data(), tol, stride) != 0) die("scoreRenderedFromBGSub");
        const std::vector<FitScore> out = get();
        if (!obs_index.empty() && out.size() != obs_index.size()) fatal("scoreRenderedFromBGSub", "one index per rendered image");
        return out;
    }

    /** The result of the last call again. */
    std::vector<FitScore> get() {
        int n = 0;
        if (avt_fitscore_get(h_, nullptr, &n) != 0) die("get");
        const size_t cells = (size_t)(numParts + 1) * AVT_FITSCORE_COLS;
        std::vector<long long> all(cells * (size_t)n);
        if (avt_fitscore_get(h_, all.data(), nullptr) != 0) die("get");
        std::vector<FitScore> out((size_t)n);
        for (size_t i = 0; i < (size_t)n; ++i) {
            out[i].numParts = numParts;
            out[i].table.assign(all.begin() + (long)(cells * i), all.begin() + (long)(cells * (i + 1)));
        }
        return out;
    }

    avt_fitscore* handle() const { return h_; }
    const int numParts;

   private:
    [[noreturn]] static void die(const char* what) { std::fprintf(stderr, "FATAL: FitScorer::%s: %s\n", what, avt_last_error()); std::exit(1); }
    [[noreturn]] static void fatal(const char* what, const char* why) { std::fprintf(stderr, "FATAL: FitScorer::%s: %s\n", what, why); std::exit(1); }
    avt_fitscore* h_ = nullptr;
};

}  // namespace ark
