// ark/MultiFrameTracker.h — S independent tracking streams (each the protocol of ark::FrameTracker) fitted together: one batched
// fit per step over one resident frame per stream, every stream with its own ICP budget (avt_optimize_resident_budgets).
// Header-only, over the C ABI, with a device context of its own sized for S frames.
//
// A step: subsample every stream's frame on the host; avt_frames_upload of the S frames (the same count keeps the warm states
// resident; a lost stream rides as an empty frame); avt_state_upload_frames for the streams that reinitialise (the first step
// installs all S with avt_state_upload); avt_optimize_resident_budgets with icp_iters = the largest budget of the step; one
// avt_state_download.  Per-stream p, r, w and stats are always there; posed clouds are fetched on request (posed()).
//
// processDepth() puts the front end of demo.cpp:179-204 in front of a step for all streams at once: BGSubtractor::runBatch, then
// RTree::predictBestFromBGSub on the masked depth where it lies on the device, one download of all labels, postProcess per stream
// on the host (a sequential flood fill, as in the reference), then process() with the caller's XYZ maps.  processDepthImages() is
// the same from depth images and one camera per stream (BGSubtractor::runBatchDepth, ark::subsampleFrameDepth): no XYZ map on the host.
//
// With deviceSubsample (attachFrontEnd; needs devicePostProcess) both run everything up to the fit on the device: the labels are
// post-processed where they lie, avt_frames_subsample_* writes every stream's kept points into the context's frame slots and brings
// back a table of counts (and the centroids of the streams that may reinitialise), the policy runs on the counts, and
// avt_frames_subsample_commit makes the frames resident, a lost stream as an empty frame.  No label image comes down and no cloud
// goes up; frames, budgets and states are those of the host path, bit for bit.  partMasks stays empty: downloadPartMasks() fetches.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../avt_render.h"
#include "../avt_subsample.h"
#include "AvatarOptimizer.h"
#include "BGSubtractor.h"
#include "FitScore.h"
#include "PoseError.h"
#include "RForest.h"
#include "RTree.h"
#include "TrackerPolicy.h"

namespace ark {

class MultiFrameTracker {
   public:
    using Rect = TrackRect;
    /** policy and state of one stream: FrameTracker's members of the same names */
    struct Stream {
        int interval = 12, frameICPIters = 3, reinitICPIters = 6, initialICPIters = 6, reinitCnz = 1000, initialPerPartCnz = 0;
        bool reinit = true, firstTime = true;
        long framesFitted = 0;
    };
    /** one stream's input of a step: XYZ map (height x width x 3 float), part mask (uint8, 255 = background), box */
    struct Frame { const float* xyz; const std::uint8_t* mask; int width, height; Rect box; };

    MultiFrameTracker(const AvatarModel& model, int num_streams, int num_parts, const std::vector<int>& part_map, int max_points_per_frame,
                      int device = 0)
        : model(model), S(num_streams), numParts(num_parts), J(model.numJoints()), K(model.numShapeKeys()), streams((size_t)num_streams),
          p(3 * (size_t)num_streams, 0.0), q(4 * (size_t)J * num_streams, 0.0), w((size_t)K * num_streams, 0.0),
          stats((size_t)num_streams), clouds((size_t)num_streams), labels((size_t)num_streams), cnz((size_t)num_streams) {
        for (int s = 0; s < S; ++s) for (int j = 0; j < J; ++j) q[((size_t)s * J + j) * 4 + 3] = 1.0;
        ARK_AVT_CHECK(avt_ctx_create(device, model.handle, num_parts, part_map.data(), max_points_per_frame, num_streams, &ctx));
        device_ = device;
        partMap_ = part_map;
    }
    ~MultiFrameTracker() {
        delete poseScorer;
        delete scorer;
        avt_renderer_destroy(rend);
        if (ctx) avt_ctx_destroy(ctx);
    }
    MultiFrameTracker(const MultiFrameTracker&) = delete;
    MultiFrameTracker& operator=(const MultiFrameTracker&) = delete;

    /** Not a reference behaviour: self-occlusion visibility from a face-id render of every stream's current cloud at this camera
     *  (include/avt.h, avt_set_occlusion_render; AvatarOptimizer.cpp:1369-1385 is the block the reference left commented out).
     *  on = false turns it off again.  Takes effect for the following steps; `renderOcclusion` tells what is in force. */
    void setRenderOcclusion(bool on, const Size& image_size = Size(), const CameraIntrin& intrin = CameraIntrin()) {
        ARK_AVT_CHECK(avt_set_occlusion_render(ctx, on ? image_size.width : 0, image_size.height, intrin.fx, intrin.fy, intrin.cx, intrin.cy));
        renderOcclusion = on;
        if (on) { occlusionSize = image_size; occlusionIntrin = intrin; }
    }
    /** Not a reference behaviour: the correspondence gate of every stream (include/avt.h, avt_set_corr_gate) - one distance for every
     *  part, or numParts distances; +inf / an empty vector = off.  Takes effect for the following steps; `correspondenceGate` tells
     *  what is in force (empty: off). */
    void setCorrespondenceGate(double max_dist) { setCorrespondenceGate(std::vector<double>(1, max_dist)); }
    void setCorrespondenceGate(const std::vector<double>& gates) {
        ARK_AVT_CHECK(avt_set_corr_gate(ctx, (int)gates.size(), gates.data()));
        correspondenceGate = gates;
    }
    /** Not a reference behaviour: trimmed ICP on every stream (include/avt.h, avt_set_corr_trim), every part alike; a factor of +inf
     *  turns it off.  Takes effect for the following steps. */
    void setCorrespondenceTrim(double quantile, double factor, double floor_dist = 0.0, int min_matches = 1) {
        if (factor == std::numeric_limits<double>::infinity()) ARK_AVT_CHECK(avt_set_corr_trim(ctx, 0, nullptr, nullptr, nullptr, 1));
        else ARK_AVT_CHECK(avt_set_corr_trim(ctx, 1, &quantile, &factor, &floor_dist, min_matches));
    }
    /** matches the last search of the last step lost to the trim on stream s (avt_get_trimmed) */
    int lastTrimmed(int s) const {
        int n = 0;
        ARK_AVT_CHECK(avt_get_trimmed(ctx, s, &n, nullptr));
        return n;
    }
    /** queries the last search of the last step dropped at the gate on stream s (avt_get_gated) */
    int lastGated(int s) const {
        int n = 0;
        ARK_AVT_CHECK(avt_get_gated(ctx, s, &n));
        return n;
    }
    /** the visibility flags (numPoints bytes) of the last ICP iteration of the last step on stream s (avt_get_visibility) */
    std::vector<unsigned char> visibility(int s) const {
        std::vector<unsigned char> v((size_t)model.numPoints());
        ARK_AVT_CHECK(avt_get_visibility(ctx, s, v.data()));
        return v;
    }

    /** One step, one frame per stream.  fitted[s] = 1 if stream s was fitted, 0 if its tracking was declared lost. */
    void process(const std::vector<Frame>& frames, std::vector<int>& fitted) {
        if ((int)frames.size() != S) { std::fprintf(stderr, "MultiFrameTracker: %d frames for %d streams\n", (int)frames.size(), S); std::exit(1); }
        fit([&](int s, int interval) {
            const Frame& f = frames[(size_t)s];
            return subsampleFrame(f.xyz, f.mask, f.width, f.box, interval, numParts, clouds[(size_t)s], labels[(size_t)s]);
        }, fitted);
    }

   private:
    /** process() around the subsampling: `subsampleStream(s, interval)` fills clouds[s], labels[s] and returns the point count */
    template <class Sub>
    void fit(Sub subsampleStream, std::vector<int>& fitted) {
        fitted.assign((size_t)S, 0);
        budgets.assign((size_t)S, 0);
        reinitStreams.clear();
        std::vector<Matrix3d> r((size_t)J);
        std::vector<double> wz((size_t)K, 0.0);
        for (int s = 0; s < S; ++s) {
            Stream& st = streams[(size_t)s];
            cnz[(size_t)s] = subsampleStream(s, st.interval);
            int icp = 0;
            bool re = false;
            if (!frameDecision(st, labels[(size_t)s], cnz[(size_t)s], numParts, icp, re)) {
                cnz[(size_t)s] = 0;                    // nothing of a lost stream's frame is needed: it rides as an empty frame
                continue;
            }
            fitted[(size_t)s] = 1;
            budgets[(size_t)s] = icp;
            if (re) {
                reinitStreams.push_back(s);
                reinitState(clouds[(size_t)s], cnz[(size_t)s], &p[3 * (size_t)s], wz, r);
                std::copy(wz.begin(), wz.end(), w.begin() + (size_t)K * s);
                for (int j = 0; j < J; ++j) {
                    const Quaterniond qq = rotationToQuaternion(r[(size_t)j]);
                    for (int c = 0; c < 4; ++c) q[((size_t)s * J + j) * 4 + c] = qq.c[c];
                }
            }
        }
        if (std::find(fitted.begin(), fitted.end(), 1) == fitted.end()) return;
        // the frames back to back
        std::vector<int> offs((size_t)S + 1, 0);
        for (int s = 0; s < S; ++s) offs[(size_t)s + 1] = offs[(size_t)s] + (int)cnz[(size_t)s];
        data.resize(3 * (size_t)offs[(size_t)S]);
        lab.resize((size_t)offs[(size_t)S]);
        for (int s = 0; s < S; ++s) {
            std::copy(clouds[(size_t)s].data(), clouds[(size_t)s].data() + 3 * cnz[(size_t)s], data.begin() + 3 * (size_t)offs[(size_t)s]);
            std::copy(labels[(size_t)s].begin(), labels[(size_t)s].begin() + (long)cnz[(size_t)s], lab.begin() + offs[(size_t)s]);
        }
        ARK_AVT_CHECK(avt_frames_upload(ctx, S, data.data(), lab.data(), offs.data()));
        fitResident(fitted);
    }

    /** fit() behind the frame install: start states, the batched fit, one download of all states */
    void fitResident(const std::vector<int>& fitted) {
        if (!stateResident) {
            ARK_AVT_CHECK(avt_state_upload(ctx, S, p.data(), q.data(), w.data()));
            stateResident = true;
        } else if (!reinitStreams.empty()) {
            const size_t n = reinitStreams.size();
            std::vector<double> pp(3 * n), qq(4 * (size_t)J * n), ww((size_t)K * n);
            for (size_t i = 0; i < n; ++i) {
                const size_t s = (size_t)reinitStreams[i];
                std::copy(&p[3 * s], &p[3 * s] + 3, &pp[3 * i]);
                std::copy(&q[4 * (size_t)J * s], &q[4 * (size_t)J * s] + 4 * J, &qq[4 * (size_t)J * i]);
                std::copy(&w[(size_t)K * s], &w[(size_t)K * s] + K, &ww[(size_t)K * i]);
            }
            ARK_AVT_CHECK(avt_state_upload_frames(ctx, (int)n, reinitStreams.data(), pp.data(), qq.data(), ww.data()));
        }
        avt_options o;
        avt_options_default(&o);
        o.beta_pose = betaPose; o.beta_shape = betaShape; o.max_iters_per_icp = maxItersPerICP;
        o.enable_occlusion = enableOcclusion ? 1 : 0; o.function_tolerance = functionTolerance;
        o.icp_iters = *std::max_element(budgets.begin(), budgets.end());
        ARK_AVT_CHECK(avt_optimize_resident_budgets(ctx, &o, budgets.data()));
        std::vector<avt_stats> st((size_t)S);
        ARK_AVT_CHECK(avt_state_download(ctx, p.data(), q.data(), w.data(), st.data()));
        for (int s = 0; s < S; ++s)
            if (fitted[(size_t)s]) { stats[(size_t)s] = st[(size_t)s]; ++streams[(size_t)s].framesFitted; }
    }

   public:

    /** The front end of processDepth: a BGSubtractor holding one background per stream and a forest on the same device (both
     *  outlive the tracker's use of them); the interval of predictBest / postProcess (demo.cpp:198) and postProcess's weight. */
    /** devicePostProcess: postProcess runs on the device for all streams at once (RTree::postProcessFromBGSub: connected components
     *  on the interval grid, the reference's result at rtree_interval 1 and a documented difference above it); comPre[s] is then the
     *  forest's resident memory of slot s.  Off, postProcess runs per stream on the host as ever.
     *  deviceSubsample (needs devicePostProcess): the subsampling and the frame install run on the device too (avt_subsample.h). */
    void attachFrontEnd(BGSubtractor& bgsub, RTree& rtree, int rtree_interval = 2, double dist_to_pre_weight = 0.001, bool devicePostProcess = false,
                        bool deviceSubsample = false) {
        if (deviceSubsample && !devicePostProcess) { std::fprintf(stderr, "MultiFrameTracker::attachFrontEnd: deviceSubsample needs devicePostProcess\n"); std::exit(1); }
        deviceSub = deviceSubsample;
        frontBG = &bgsub; frontTree = &rtree; frontForest = nullptr;
        rtreeInterval = rtree_interval; distToPreWeight = dist_to_pre_weight; devicePost = devicePostProcess;
        comPre.assign((size_t)S, MatrixNX<2>());
        boxes.assign((size_t)S, {0, 0, 0, 0});
        partMasks.clear();
    }

    /** The same front end with a forest of several trees in the tree's place (ark/RForest.h). */
    void attachFrontEnd(BGSubtractor& bgsub, RForest& rforest, int rtree_interval = 2, double dist_to_pre_weight = 0.001, bool devicePostProcess = false,
                        bool deviceSubsample = false) {
        if (deviceSubsample && !devicePostProcess) { std::fprintf(stderr, "MultiFrameTracker::attachFrontEnd: deviceSubsample needs devicePostProcess\n"); std::exit(1); }
        deviceSub = deviceSubsample;
        frontBG = &bgsub; frontTree = nullptr; frontForest = &rforest;
        rtreeInterval = rtree_interval; distToPreWeight = dist_to_pre_weight; devicePost = devicePostProcess;
        comPre.assign((size_t)S, MatrixNX<2>());
        boxes.assign((size_t)S, {0, 0, 0, 0});
        partMasks.clear();
    }

    /** One step from S XYZ maps: image s against background s (every slot keeps the box of its previous run), labelled inside its
     *  box without leaving the device, post-processed on the host with stream s's comPre, then process().  A stream whose box is
     *  empty or not inside the image has an all-255 mask: it goes through postProcess on the whole image (every comPre x becomes
     *  -1) and is lost in process().  Afterwards partMasks[s] and boxes[s] (tl.x tl.y br.x br.y) hold the step's labels and boxes. */
    void processDepth(const std::vector<ImageXYZ>& images, std::vector<int>& fitted) {
        if (!frontBG || (!frontTree && !frontForest)) { std::fprintf(stderr, "MultiFrameTracker::processDepth: no front end attached\n"); std::exit(1); }
        if ((int)images.size() != S) { std::fprintf(stderr, "MultiFrameTracker: %d images for %d streams\n", (int)images.size(), S); std::exit(1); }
        frontBG->runBatch(images);
        if (deviceSub) { fitDevice(fitted); return; }
        const std::vector<Rect> box = labelBatch();
        std::vector<Frame> frames((size_t)S);
        for (int s = 0; s < S; ++s) frames[(size_t)s] = {images[(size_t)s].data(), partMasks[(size_t)s].data(), partMasks[(size_t)s].cols, partMasks[(size_t)s].rows, box[(size_t)s]};
        process(frames, fitted);
    }

    /** processDepth() from S depth images and their cameras (one per stream, or one for all): the depth is what is uploaded
     *  (BGSubtractor::runBatchDepth), and the subsampling back-projects the kept pixels alone. */
    void processDepthImages(const std::vector<ImageDepth>& depths, const std::vector<CameraIntrin>& intrins, std::vector<int>& fitted) {
        if (!frontBG || (!frontTree && !frontForest)) { std::fprintf(stderr, "MultiFrameTracker::processDepthImages: no front end attached\n"); std::exit(1); }
        if ((int)depths.size() != S || ((int)intrins.size() != S && intrins.size() != 1)) {
            std::fprintf(stderr, "MultiFrameTracker: %d depth images, %d cameras for %d streams\n", (int)depths.size(), (int)intrins.size(), S);
            std::exit(1);
        }
        frontBG->runBatchDepth(depths, intrins);
        if (deviceSub) { fitDevice(fitted); return; }
        const std::vector<Rect> box = labelBatch();
        fit([&](int s, int interval) {
            return subsampleFrameDepth(depths[(size_t)s].data(), intrins[intrins.size() == 1 ? 0 : (size_t)s], partMasks[(size_t)s].data(),
                                       partMasks[(size_t)s].cols, box[(size_t)s], interval, numParts, clouds[(size_t)s], labels[(size_t)s]);
        }, fitted);
    }

   private:
    /** A depth-in step behind the batch run with everything up to the fit on the device (demo.cpp:196-265 for all streams) */
    void fitDevice(std::vector<int>& fitted) {
        if (frontTree) {
            frontTree->predictBestFromBGSub(*frontBG, rtreeInterval, true, false);
            ARK_AVT_CHECK(avt_rtree_post_process_from_bgsub(frontTree->handle(), frontBG->handle(), rtreeInterval, distToPreWeight));
        } else {
            frontForest->predictBestFromBGSub(*frontBG, rtreeInterval, true, false);
            ARK_AVT_CHECK(avt_rforest_post_process_from_bgsub(frontForest->handle(), frontBG->handle(), rtreeInterval, distToPreWeight));
        }
        (void)frontBG->batchInfo(0);                   // the one read of the subtractor's fault word
        std::vector<int> iv((size_t)S), counts((size_t)S * (1 + (size_t)numParts)), used(4 * (size_t)S);
        std::vector<unsigned char> want((size_t)S), keep((size_t)S, 0);
        std::vector<double> cen(3 * (size_t)S, 0.0);
        for (int s = 0; s < S; ++s) { iv[(size_t)s] = streams[(size_t)s].interval; want[(size_t)s] = streams[(size_t)s].reinit ? 1 : 0; }
        if (frontTree)
            ARK_AVT_CHECK(avt_frames_subsample_rtree(ctx, frontTree->handle(), frontBG->handle(), nullptr, iv.data(), want.data(), counts.data(), cen.data(), used.data()));
        else
            ARK_AVT_CHECK(avt_frames_subsample_rforest(ctx, frontForest->handle(), frontBG->handle(), nullptr, iv.data(), want.data(), counts.data(), cen.data(), used.data()));
        partMasks.clear();
        fitted.assign((size_t)S, 0);
        budgets.assign((size_t)S, 0);
        reinitStreams.clear();
        std::vector<Matrix3d> r((size_t)J);
        std::vector<double> wz((size_t)K, 0.0);
        CloudType one;
        one.resize(3, 1);
        for (int s = 0; s < S; ++s) {
            for (int c = 0; c < 4; ++c) boxes[(size_t)s][(size_t)c] = used[4 * (size_t)s + c];
            comPre[(size_t)s] = frontTree ? frontTree->comPre(s) : frontForest->comPre(s);
            int icp = 0;
            bool re = false;
            if (!frameDecision(streams[(size_t)s], &counts[(size_t)s * (1 + (size_t)numParts)], numParts, icp, re)) continue;
            fitted[(size_t)s] = keep[(size_t)s] = 1;
            budgets[(size_t)s] = icp;
            if (re) {
                reinitStreams.push_back(s);
                for (int c = 0; c < 3; ++c) one(c, 0) = cen[3 * (size_t)s + c];      // (the centroid of one point is the point)
                reinitState(one, 1, &p[3 * (size_t)s], wz, r);
                std::copy(wz.begin(), wz.end(), w.begin() + (size_t)K * s);
                for (int j = 0; j < J; ++j) {
                    const Quaterniond qq = rotationToQuaternion(r[(size_t)j]);
                    for (int c = 0; c < 4; ++c) q[((size_t)s * J + j) * 4 + c] = qq.c[c];
                }
            }
        }
        if (std::find(fitted.begin(), fitted.end(), 1) == fitted.end()) return;
        ARK_AVT_CHECK(avt_frames_subsample_commit(ctx, keep.data()));
        fitResident(fitted);
    }

    /** The front end behind the batch run, whatever its source: labels on the device, postProcess per stream; fills partMasks and
     *  boxes and returns every stream's box to subsample. */
    std::vector<Rect> labelBatch() {
        partMasks = frontTree ? frontTree->predictBestFromBGSub(*frontBG, rtreeInterval, true, !devicePost)
                              : frontForest->predictBestFromBGSub(*frontBG, rtreeInterval, true, !devicePost);
        if (devicePost)       // in place on the device, all streams in one launch sequence; the labels come down once, after it
            partMasks = frontTree ? frontTree->postProcessFromBGSub(*frontBG, rtreeInterval, distToPreWeight)
                                  : frontForest->postProcessFromBGSub(*frontBG, rtreeInterval, distToPreWeight);
        auto postProcess = [&](Image8& m, MatrixNX<2>& com, Point tl, Point br) {
            if (devicePost) return;
            if (frontTree) frontTree->postProcess(m, com, rtreeInterval, 1, tl, br, distToPreWeight);
            else frontForest->postProcess(m, com, rtreeInterval, 1, tl, br, distToPreWeight);
        };
        std::vector<Rect> out((size_t)S);
        for (int s = 0; s < S; ++s) {
            const BGSubtractor::BatchInfo b = frontBG->batchInfo(s);
            boxes[(size_t)s] = {b.topLeft.x, b.topLeft.y, b.botRight.x, b.botRight.y};
            Image8& m = partMasks[(size_t)s];
            Rect& box = out[(size_t)s];
            if (0 <= b.topLeft.x && b.topLeft.x <= b.botRight.x && b.botRight.x < m.cols && 0 <= b.topLeft.y && b.topLeft.y <= b.botRight.y &&
                b.botRight.y < m.rows) {
                postProcess(m, comPre[(size_t)s], b.topLeft, b.botRight);
                box.top = b.topLeft.y; box.left = b.topLeft.x; box.bottom = b.botRight.y; box.right = b.botRight.x;
            } else {
                postProcess(m, comPre[(size_t)s], Point(0, 0), Point(-1, -1));
                box.top = m.rows - 1; box.left = m.cols - 1; box.bottom = 0; box.right = 0;       // nothing to subsample
            }
            if (devicePost) comPre[(size_t)s] = frontTree ? frontTree->comPre(s) : frontForest->comPre(s);
        }
        return out;
    }

   public:
    /** The post-processed part masks of the last depth-in step: partMasks where the step brought them down, one download where
     *  it did not (deviceSubsample); partMasks holds them afterwards. */
    const std::vector<Image8>& downloadPartMasks() {
        if (!partMasks.empty() || !frontBG || frontBG->batchSize() <= 0) return partMasks;
        const int n = frontBG->batchSize(), rows = frontBG->rows(), cols = frontBG->cols();
        std::vector<std::uint8_t> all((size_t)n * rows * cols);
        if (frontTree) ARK_AVT_CHECK(avt_rtree_labels_download_all(frontTree->handle(), all.data()));
        else ARK_AVT_CHECK(avt_rforest_labels_download_all(frontForest->handle(), all.data()));
        partMasks.assign((size_t)n, Image8(rows, cols));
        for (int i = 0; i < n; ++i) std::copy(all.begin() + (size_t)i * rows * cols, all.begin() + (size_t)(i + 1) * rows * cols, partMasks[(size_t)i].data());
        return partMasks;
    }

    /** ava.cloud (3 x V), jointPos (3 x J), jointTrans (12 x J) of stream s's last fit; any pointer may be null (avt_get_posed) */
    void posed(int s, double* cloud_3xV, double* joint_pos_3xJ = nullptr, double* joint_trans_12xJ = nullptr) {
        ARK_AVT_CHECK(avt_get_posed(ctx, s, cloud_3xV, joint_pos_3xJ, joint_trans_12xJ));
    }
    /** Renders the last fit of the given streams on the device in one run (avt_render.h): the posed clouds are read from the
     *  context, not downloaded.  what: AVT_RENDER_* bits; part_map as AvatarRenderer::renderPartMask.  Image i of the run
     *  belongs to streams[i]: fetch it with renderedDepth / renderedPartMask / renderedLambert / renderedFaces. */
    void render(const std::vector<int>& stream_ids, const Size& image_size, const CameraIntrin& intrin, int what = AVT_RENDER_LAMBERT,
                const std::vector<int>& part_map = {}) {
        if (!rend || image_size.width != rendW || image_size.height != rendH || intrin.fx != rendIntrin.fx || intrin.fy != rendIntrin.fy ||
            intrin.cx != rendIntrin.cx || intrin.cy != rendIntrin.cy) {
            avt_renderer_destroy(rend);
            rend = nullptr;
            ARK_AVT_CHECK(avt_renderer_create(device_, model.handle, image_size.width, image_size.height, intrin.fx, intrin.fy, intrin.cx,
                                              intrin.cy, S, &rend));
            rendW = image_size.width; rendH = image_size.height; rendIntrin = intrin;
        }
        if (what & AVT_RENDER_PART_MASK)
            ARK_AVT_CHECK(avt_renderer_set_part_map(rend, (int)part_map.size(), part_map.empty() ? nullptr : part_map.data()));
        ARK_AVT_CHECK(avt_renderer_from_ctx(rend, ctx, (int)stream_ids.size(), stream_ids.data()));
        ARK_AVT_CHECK(avt_renderer_run(rend, what));
    }
    ImageF renderedDepth(int i) const { ImageF o(rendH, rendW); ARK_AVT_CHECK(avt_renderer_download(rend, i, o.data(), nullptr, nullptr, nullptr)); return o; }
    Image8 renderedPartMask(int i) const { Image8 o(rendH, rendW); ARK_AVT_CHECK(avt_renderer_download(rend, i, nullptr, o.data(), nullptr, nullptr)); return o; }
    Image8 renderedLambert(int i) const { Image8 o(rendH, rendW); ARK_AVT_CHECK(avt_renderer_download(rend, i, nullptr, nullptr, o.data(), nullptr)); return o; }
    Image<int32_t> renderedFaces(int i) const {
        Image<int32_t> o(rendH, rendW);
        ARK_AVT_CHECK(avt_renderer_download(rend, i, nullptr, nullptr, nullptr, o.data()));
        return o;
    }

    /** How well the last fit of the given streams explains the depth images of the last step (ark/FitScore.h, the numbers behind
     *  the overlay of live-demo.cpp:428-445): depth and part mask of the streams' fit are rendered from the context with the
     *  tracker's own renderer and scored on the device against the attached front end's last batch, image stream_ids[i] of it,
     *  inside the box that run found.  One FitScore per stream.  Refused without a front end or before a step.  Nothing calls this
     *  by default; see fitLost (ark/TrackerPolicy.h) for the idiom. */
    std::vector<FitScore> fitScore(const std::vector<int>& stream_ids, const Size& image_size, const CameraIntrin& intrin,
                                   float tol = FitScore::kDefaultTol, int stride = 1, const std::vector<int>& part_map = {}) {
        if (!frontBG || frontBG->batchSize() <= 0 || !stateResident) {
            std::fprintf(stderr, "MultiFrameTracker::fitScore: needs an attached front end and a fitted step behind it\n");
            std::exit(1);
        }
        render(stream_ids, image_size, intrin, AVT_RENDER_DEPTH | AVT_RENDER_PART_MASK, part_map);
        if (!scorer) scorer = new FitScorer(numParts, S, device_);
        return scorer->scoreRenderedFromBGSub(rend, frontBG->handle(), stream_ids, tol, stride);
    }

    /** How far the last fit of the given streams is from the truth (ark/PoseError.h: PVE, MPJPE and the Procrustes-aligned
     *  forms): the estimate side is read from the context on the device, the truth side is given, one cloud (3 x V) and one set
     *  of joints (3 x J) per stream of stream_ids, back to back.  Parts are the tracker's own (its part map over the main joints).
     *  One PoseErrorResult per stream; derive() gives the figures.  Nothing calls this by default and no threshold is offered. */
    std::vector<PoseErrorResult> poseError(const std::vector<int>& stream_ids, const std::vector<double>& truth_clouds, const std::vector<double>& truth_joints) {
        const size_t n = stream_ids.size();
        if (n == 0 || truth_clouds.size() != n * 3 * (size_t)model.numPoints() || truth_joints.size() != n * 3 * (size_t)J || !stateResident) {
            std::fprintf(stderr, "MultiFrameTracker::poseError: needs a fitted step and one truth cloud (3 x V) and joint set (3 x J) per stream\n");
            std::exit(1);
        }
        if (!poseScorer) poseScorer = new PoseError(model.handle, numParts, partMap_, S, device_);
        poseScorer->fromContext(AVT_POSEERR_ESTIMATE, ctx, (int)n, stream_ids);
        poseScorer->upload(AVT_POSEERR_TRUTH, (int)n, truth_clouds.data(), truth_joints.data());
        poseScorer->run();
        return poseScorer->get();
    }

    const double* pos(int s) const { return &p[3 * (size_t)s]; }
    const double* shape(int s) const { return &w[(size_t)K * s]; }
    const double* quats(int s) const { return &q[4 * (size_t)J * s]; }           // J quaternions (x, y, z, w)
    Matrix3d rotation(int s, int j) const {
        Quaterniond qq;
        for (int c = 0; c < 4; ++c) qq.c[c] = q[((size_t)s * J + j) * 4 + c];
        return quaternionToRotation(qq);
    }

    const AvatarModel& model;
    const int S, numParts, J, K;
    std::vector<Stream> streams;
    double betaPose = 0.1, betaShape = 1.0, functionTolerance = 1e-4;
    int maxItersPerICP = 10;
    bool enableOcclusion = true;
    bool renderOcclusion = false;                  // read-only: set by setRenderOcclusion, with the camera below
    Size occlusionSize;
    CameraIntrin occlusionIntrin;
    std::vector<double> correspondenceGate;        // read-only: set by setCorrespondenceGate (empty: off)
    std::vector<int> budgets, reinitStreams;       // of the last step (0 = not fitted)
    // processDepth: per stream the previous centres of mass (demo.cpp:148), the last step's box and post-processed labels
    std::vector<MatrixNX<2>> comPre;
    std::vector<std::array<int, 4>> boxes;
    std::vector<Image8> partMasks;
    int rtreeInterval = 2;
    double distToPreWeight = 0.001;
    bool devicePost = false;
    bool deviceSub = false;                        // read-only: set by attachFrontEnd

   private:
    std::vector<double> p, q, w;

   public:
    std::vector<avt_stats> stats;                  // avt_stats of every stream's last fit

   private:
    avt_ctx* ctx = nullptr;
    BGSubtractor* frontBG = nullptr;
    RTree* frontTree = nullptr;
    RForest* frontForest = nullptr;   // in frontTree's place when a forest was attached
    int device_ = 0;
    avt_renderer* rend = nullptr;                  // render(): created on first use, again when the size or the intrinsics change
    int rendW = 0, rendH = 0;
    CameraIntrin rendIntrin;
    FitScorer* scorer = nullptr;                   // fitScore(): created on first use
    PoseError* poseScorer = nullptr;               // poseError(): created on first use
    std::vector<int> partMap_;
    bool stateResident = false;
    std::vector<CloudType> clouds;
    std::vector<VectorXi> labels;
    std::vector<size_t> cnz;
    std::vector<double> data;
    std::vector<int> lab;
};

}  // namespace ark
