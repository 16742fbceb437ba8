// ark/FrameTracker.h — the per-frame protocol of the reference's trackers (demo.cpp:215-290, live-demo.cpp:335-432) over
// ark::AvatarOptimizer: interval subsampling of the labelled XYZ map inside the foreground bounding box, the
// tracking-loss / reinitialisation policy, the per-frame ICP budgets and the temporal warm start (the avatar state simply
// carries over between frames).  SURVEY.md §8 row f3.  Header-only, no OpenCV: images are plain row-major buffers.
//
// Inputs per frame are what the reference's front end produces (ark::BGSubtractor, then ark::RTree): an XYZ map (height x width x 3
// float, camera coordinates, cv::Vec3f layout) and a per-pixel body-part mask (height x width uint8, 255 = background), plus
// the foreground bounding box (bgsub.topLeft / bgsub.botRight, inclusive).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "AvatarOptimizer.h"
#include "TrackerPolicy.h"

namespace ark {

class FrameTracker {
   public:
    using Rect = TrackRect;   // inclusive, like bgsub.topLeft / botRight

    explicit FrameTracker(AvatarOptimizer& ava_opt) : avaOpt(ava_opt), ava(ava_opt.ava) {}

    /** Every `interval`-th pixel of the bounding box that carries a body-part label (demo.cpp:216-250); y negated (:245).
     *  Returns the number of points; a label >= numParts is fatal exactly like demo.cpp:236-243. */
    size_t subsample(const float* xyz, const std::uint8_t* part_mask, int width, const Rect& box, CloudType& dataCloud,
                     VectorXi& dataPartLabels) const {
        return subsampleFrame(xyz, part_mask, width, box, interval, avaOpt.numParts, dataCloud, dataPartLabels);
    }

    /** One tracked frame.  Returns true if the avatar was fitted, false if tracking was declared lost (too few body
     *  pixels; the next fitted frame reinitialises: live-demo.cpp:335-340, :379-383).  The decision: ark::frameDecision. */
    bool process(const float* xyz, const std::uint8_t* part_mask, int width, int height, const Rect& box) {
        (void)height;
        return fit(subsample(xyz, part_mask, width, box, dataCloud, dataPartLabels));
    }

    /** process() on a depth image (height x width float) and its camera: no XYZ map is needed, the kept pixels alone are
     *  back-projected (ark::subsampleFrameDepth). */
    bool processDepthImage(const float* depth, const CameraIntrin& intrin, const std::uint8_t* part_mask, int width, int height, const Rect& box) {
        (void)height;
        return fit(subsampleFrameDepth(depth, intrin, part_mask, width, box, interval, avaOpt.numParts, dataCloud, dataPartLabels));
    }

   private:
    /** process() behind the subsampling, on dataCloud / dataPartLabels */
    bool fit(size_t cnz) {
        int icpIters = 0;
        bool reinitNow = false;
        if (!frameDecision(*this, dataPartLabels, cnz, avaOpt.numParts, icpIters, reinitNow)) return false;
        if (reinitNow) {                                                // demo.cpp:252-265
            reinitState(dataCloud, cnz, ava.p.data(), ava.w, ava.r);
            ava.update();
        }
        if (renderOcclusion >= 0) avaOpt.renderOcclusion = renderOcclusion != 0;
        if (maxCorrespondenceDist >= 0) avaOpt.maxCorrespondenceDist = maxCorrespondenceDist;
        if (trimFactor >= 0) { avaOpt.trimQuantile = trimQuantile; avaOpt.trimFactor = trimFactor; avaOpt.trimFloor = trimFloor; avaOpt.trimMinMatches = trimMinMatches; }
        avaOpt.optimize(dataCloud, dataPartLabels, icpIters, numThreads);
        ++framesFitted;
        return true;
    }

   public:

    int interval = 12;            // demo.cpp:58   --data-interval
    int frameICPIters = 3;        // demo.cpp:63   --frame-icp-iters
    int reinitICPIters = 6;       // demo.cpp:66   --reinit-icp-iters
    int initialICPIters = 6;      // live-demo.cpp:80 (demo.cpp has one budget for both)
    int reinitCnz = 1000;         // demo.cpp:71   --min-points
    int initialPerPartCnz = 0;    // live-demo.cpp:89-90 --initial-per-part-thresh (80 there); 0 = demo.cpp, which has no per-part check
    int numThreads = 4;
    bool reinit = true;           // demo.cpp:151
    bool firstTime = true;        // live-demo.cpp:256
    long framesFitted = 0;
    /** not a reference member: 1 / 0 sets avaOpt.renderOcclusion before every fit (self-occlusion from a face-id render with the
     *  optimizer's own intrin and imageSize, AvatarOptimizer.cpp:1369-1385); -1 (default) leaves the optimizer's member alone */
    int renderOcclusion = -1;
    /** not a reference member: a value >= 0 (+inf = off) sets avaOpt.maxCorrespondenceDist before every fit (the correspondence gate,
     *  include/avt.h avt_set_corr_gate); negative (default) leaves the optimizer's member alone */
    double maxCorrespondenceDist = -1.0;
    /** not reference members: a trimFactor >= 0 (+inf = off) sets avaOpt.trimQuantile / trimFactor / trimFloor / trimMinMatches before
     *  every fit (trimmed ICP, include/avt.h avt_set_corr_trim); negative (default) leaves the optimizer's members alone */
    double trimQuantile = 1.0, trimFactor = -1.0, trimFloor = 0.0;
    int trimMinMatches = 1;

    AvatarOptimizer& avaOpt;
    Avatar& ava;

   private:
    CloudType dataCloud;
    VectorXi dataPartLabels;
};

}  // namespace ark
