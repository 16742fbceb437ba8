// ark/TrackerPolicy.h — the per-frame protocol pieces of the reference's trackers (demo.cpp:215-290, live-demo.cpp:376-418) that
// ark::FrameTracker and ark::MultiFrameTracker share: interval subsampling of a labelled XYZ map, the tracking-loss /
// reinitialisation decision of one stream, the start state of a reinitialisation, and fitLost, an optional loss test on the fit
// score.  Header-only, no OpenCV.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "Avatar.h"
#include "FitScore.h"

namespace ark {

struct TrackRect { int top = 0, left = 0, bottom = 0, right = 0; };   // inclusive, like bgsub.topLeft / botRight

/** The grid walk of demo.cpp:216-250 behind subsampleFrame and subsampleFrameDepth: `point_at(r, c, out)` gives the three float
 *  coordinates of a kept pixel. */
template <class PointAt>
size_t subsampleGrid(PointAt point_at, const std::uint8_t* part_mask, int width, const TrackRect& box, int interval, int numParts,
                     CloudType& dataCloud, VectorXi& dataPartLabels) {
    size_t cnz = 0;
    for (int r = box.top; r <= box.bottom; r += interval) {
        const std::uint8_t* partptr = part_mask + (size_t)r * width;
        for (int c = box.left; c <= box.right; c += interval) cnz += partptr[c] != 255;
    }
    dataCloud.resize(3, cnz);
    dataPartLabels.assign(cnz, 0);
    size_t i = 0;
    for (int r = box.top; r <= box.bottom; r += interval) {
        const std::uint8_t* partptr = part_mask + (size_t)r * width;
        for (int c = box.left; c <= box.right; c += interval) {
            if (partptr[c] == 255) continue;
            if (partptr[c] >= numParts) {
                std::fprintf(stderr, "FATAL: body part prediction %d is invalid, since there are only %d body parts\n", (int)partptr[c], numParts);
                std::exit(1);
            }
            float pt[3];
            point_at(r, c, pt);
            dataCloud(0, i) = pt[0];
            dataCloud(1, i) = -pt[1];
            dataCloud(2, i) = pt[2];
            dataPartLabels[i] = partptr[c];
            ++i;
        }
    }
    return cnz;
}

/** Every `interval`-th pixel of the box that carries a body-part label (demo.cpp:216-250); y negated (:245).  Returns the number
 *  of points; a label >= numParts is fatal exactly like demo.cpp:236-243. */
inline size_t subsampleFrame(const float* xyz, const std::uint8_t* part_mask, int width, const TrackRect& box, int interval, int numParts,
                             CloudType& dataCloud, VectorXi& dataPartLabels) {
    return subsampleGrid([&](int r, int c, float* out) { const float* p = xyz + ((size_t)r * width + c) * 3; out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; },
                         part_mask, width, box, interval, numParts, dataCloud, dataPartLabels);
}

/** subsampleFrame without an XYZ map: the kept pixels alone are back-projected from the depth image (height x width float) by
 *  CameraIntrin::depthToXYZ's expression, so the result is subsampleFrame's on intrin.depthToXYZ(depth), bit for bit. */
inline size_t subsampleFrameDepth(const float* depth, const CameraIntrin& intrin, const std::uint8_t* part_mask, int width, const TrackRect& box,
                                  int interval, int numParts, CloudType& dataCloud, VectorXi& dataPartLabels) {
    return subsampleGrid([&](int r, int c, float* out) { intrin.pixelToXYZ(r, c, depth[(size_t)r * width + c], out); },
                         part_mask, width, box, interval, numParts, dataCloud, dataPartLabels);
}

/** The decision of one stream on its subsampled frame.  `T` carries the stream's policy and state under FrameTracker's member names
 *  (interval, frameICPIters, reinitICPIters, initialICPIters, reinitCnz, initialPerPartCnz, reinit, firstTime); reinit / firstTime
 *  are updated.  Returns false when tracking is lost (nothing is fitted; the next fitted frame reinitialises: live-demo.cpp:335-340,
 *  :379-383 - demo.cpp:225 only skips the frame, the documented deviation FrameTracker keeps); else sets the ICP iterations and
 *  whether the stream reinitialises (demo.cpp:252-265, live-demo.cpp:417-418). */
template <class T>
bool frameDecision(T& tr, const int* countRow, int numParts, int& icpIters, bool& reinitNow);

template <class T>
bool frameDecision(T& tr, const VectorXi& labels, size_t cnz, int numParts, int& icpIters, bool& reinitNow) {
    std::vector<int> row((size_t)numParts + 1, 0);
    row[0] = (int)cnz;
    if (tr.firstTime && tr.initialPerPartCnz > 0)      // the only reader of the per-part counts
        for (size_t i = 0; i < cnz; ++i) ++row[1 + (size_t)labels[i]];
    return frameDecision(tr, row.data(), numParts, icpIters, reinitNow);
}

/** The same decision on the frame's row of the device subsampling's table (avt_subsample.h): countRow[0] points in all,
 *  countRow[1 + q] of part q - the policy reads nothing else of a frame. */
template <class T>
bool frameDecision(T& tr, const int* countRow, int numParts, int& icpIters, bool& reinitNow) {
    const size_t cnz = (size_t)countRow[0];
    // An EMPTY frame is never fitted whatever reinitCnz says: the reinitialisation centroid divides by cnz.
    bool part_missing = false;       // live-demo.cpp:376-380: the FIRST fit wants every body part seen (initialPerPartCnz pixels at interval 1)
    if (tr.firstTime && tr.initialPerPartCnz > 0) {
        size_t mn = numParts > 0 ? (size_t)countRow[1] : 0;
        for (int q = 0; q < numParts; ++q) mn = (size_t)countRow[1 + q] < mn ? (size_t)countRow[1 + q] : mn;
        const int need = tr.initialPerPartCnz / (tr.interval * tr.interval);
        part_missing = mn < (size_t)(need > 1 ? need : 1);
    }
    reinitNow = false;
    icpIters = 0;
    if (cnz == 0 || part_missing || cnz < (size_t)(tr.reinitCnz / (tr.interval * tr.interval))) {
        tr.reinit = true;
        return false;
    }
    icpIters = tr.frameICPIters;
    if (tr.reinit) {
        icpIters = tr.firstTime ? tr.initialICPIters : tr.reinitICPIters;
        tr.reinit = false;
        tr.firstTime = false;
        reinitNow = true;
    }
    return true;
}

/** Start state of a reinitialisation (demo.cpp:252-265): p = centroid of the data, w = 0, identity joints, root AngleAxis(pi, y). */
inline void reinitState(const CloudType& dataCloud, size_t cnz, double p[3], std::vector<double>& w, std::vector<Matrix3d>& r) {
    double cen[3] = {0, 0, 0};
    for (size_t i = 0; i < cnz; ++i) for (int c = 0; c < 3; ++c) cen[c] += dataCloud(c, i);
    for (int c = 0; c < 3; ++c) p[c] = cen[c] / (double)cnz;
    w.assign(w.size(), 0.0);
    for (size_t i = 1; i < r.size(); ++i) r[i].setIdentity();
    // AngleAxis(pi, (0, 1, 0)).toRotationMatrix(): written out (cos(pi) and sin(pi) leave rounding residue)
    Matrix3d r0;
    r0(0, 0) = -1.0; r0(2, 2) = -1.0;
    r[0] = r0;
}

/** A loss test on the fit score (ark/FitScore.h, MultiFrameTracker::fitScore): true when the image's IoU is below minIoU or its
 *  violation above maxViolation; a NaN figure (nothing to compare) counts as lost.  Nothing calls it by default and there are no
 *  default bounds: nobody has measured what a good or a bad fit scores on real data.  A caller who has bounds sets
 *  `streams[s].reinit = true` on it, which makes the stream's next fitted frame reinitialise, as frameDecision's own loss does. */
inline bool fitLost(const FitScore& score, double minIoU, double maxViolation) {
    const FitFigures f = score.derive();
    return !(f.iou >= minIoU) || !(f.violation <= maxViolation);
}

}  // namespace ark
