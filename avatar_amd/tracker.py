"""Frame protocol of the reference's trackers (demo.cpp:215-290, live-demo.cpp:364-426) on top of AvatarOptimizer:
interval subsampling of the labelled depth image, the reinitialisation policy, per-frame ICP budgets and the temporal
warm start (the avatar state simply carries over between frames).  SURVEY.md §8 row f3.

Inputs per frame are what the reference's front end produces (bgsub.BGSubtractor, then rtree.RTree): an XYZ map (H,W,3)
float32 in camera coordinates and a per-pixel body-part mask (H,W) uint8 with 255 = background, plus the foreground
bounding box (top, left, bottom, right), inclusive.
"""
from __future__ import annotations

import numpy as np

from . import api
from .depth import CameraIntrin, intrin_array


def _subsample(points_at, part_mask, bbox, interval, num_parts):
    """The grid and the label checks of demo.cpp:216-250; `points_at(rows, cols, keep)` gives the kept pixels' (n,3) float32."""
    H, W = part_mask.shape
    top, left, bottom, right = bbox if bbox is not None else (0, 0, H - 1, W - 1)
    rows = np.arange(top, bottom + 1, interval)
    cols = np.arange(left, right + 1, interval)
    sub_mask = part_mask[np.ix_(rows, cols)]
    keep = sub_mask != 255
    if (sub_mask[keep] >= num_parts).any():
        raise ValueError("body part prediction out of range (demo.cpp:236-243)")
    pts = points_at(rows, cols, keep).astype(np.float64)
    pts[:, 1] = -pts[:, 1]
    return pts, sub_mask[keep].astype(np.int32)


def subsample(xyz, part_mask, bbox, interval, num_parts):
    """Every `interval`-th pixel of the bounding box (top, left, bottom, right; inclusive; None = the whole image) that carries a
    body-part label (demo.cpp:216-250); y is negated (:245).  Returns (data_cloud (n,3) float64, labels (n,) int32)."""
    return _subsample(lambda rows, cols, keep: xyz[np.ix_(rows, cols)][keep], part_mask, bbox, interval, num_parts)


def subsample_depth(depth, intrin, part_mask, bbox, interval, num_parts):
    """subsample() without an XYZ map: the three coordinates of the kept pixels alone, from the depth image (H,W) and the
    camera by CameraIntrin::depthToXYZ's float32 expression (Calibration.cpp:91), so the result is exactly
    subsample(depth.depth_to_xyz(depth, intrin), ...)."""
    k = CameraIntrin.of(intrin)

    def points_at(rows, cols, keep):
        ri, ci = np.nonzero(keep)
        r, c = rows[ri].astype(np.int32), cols[ci].astype(np.int32)
        z = np.asarray(depth, np.float32)[r, c]
        with np.errstate(all="ignore"):
            return np.stack([(c.astype(np.float32) - k.cx) * z / k.fx, (r.astype(np.float32) - k.cy) * z / k.fy, z], 1).astype(np.float32)

    return _subsample(points_at, part_mask, bbox, interval, num_parts)


def frame_decision(tr, labels, num_parts=None, counts=None):
    """The per-frame policy of one stream (demo.cpp:225-265, live-demo.cpp:376-418) on the subsampled labels: returns
    (fit, ICP iterations, reinitialise); fit False means tracking is lost (nothing is fitted, the next fitted frame reinitialises).
    `tr` carries the stream's policy and state under FrameTracker's attribute names; reinit / firstTime are updated.
    counts: instead of the labels (then None), the frame's row of the device subsampling's table (api.Context.frames_subsample):
    [points, points of part 0, points of part 1, ...] - the policy reads nothing else of a frame."""
    if counts is not None:
        n, part_counts = int(counts[0]), (lambda: np.asarray(counts[1:]))
    else:
        n, part_counts = len(labels), (lambda: np.bincount(labels, minlength=num_parts))
    part_missing = False                          # live-demo.cpp:376-380: the first fit wants every body part seen
    if tr.firstTime and tr.initialPerPartCnz > 0:
        part_missing = part_counts().min() < max(1, tr.initialPerPartCnz // (tr.interval * tr.interval))
    if n == 0 or part_missing or n < tr.reinitCnz // (tr.interval * tr.interval):   # an empty frame is never fitted
        tr.reinit = True
        return False, 0, False
    if not tr.reinit:
        return True, tr.frameICPIters, False
    icp_iters = tr.initialICPIters if tr.firstTime else tr.reinitICPIters     # live-demo.cpp:417-418
    tr.reinit = False
    tr.firstTime = False
    return True, icp_iters, True


def reinit_state(data, num_joints, num_shape_keys):
    """The start state of a (re)initialisation (demo.cpp:252-265): the data centroid, zero shape, identity joints and the root
    turned by AngleAxis(pi, y).  Returns (p (3,), r (J,3,3), w (K,))."""
    r = np.tile(np.eye(3), (num_joints, 1, 1))
    r[0] = np.array([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]])   # AngleAxis(pi, y)
    return data.mean(0), r, np.zeros(num_shape_keys)


class FrameTracker:
    def __init__(self, ava_opt: "api.AvatarOptimizer", interval=12, frame_icp_iters=3, reinit_icp_iters=6, reinit_cnz=1000,
                 num_threads=4, rtree=None, rtree_interval=2, dist_to_pre_weight=0.001, initial_per_part_cnz=0, initial_icp_iters=None,
                 render_occlusion=None, max_corr_dist=None, corr_trim=None):
        """render_occlusion: True / False sets ava_opt.renderOcclusion (self-occlusion from a face-id render at the optimizer's own
        intrin and imageSize; not a reference behaviour); None leaves it as it is.
        max_corr_dist: a distance or numParts distances sets ava_opt.max_corr_dist (the correspondence gate, api.Context.set_corr_gate;
        not a reference behaviour); None leaves it as it is.
        corr_trim: (quantile, factor, floor, min_matches) sets ava_opt.trimQuantile / trimFactor / trimFloor / trimMinMatches (trimmed
        ICP, api.Context.set_corr_trim; not a reference behaviour); None leaves them as they are."""
        self.opt = ava_opt
        if corr_trim is not None:
            ava_opt.trimQuantile, ava_opt.trimFactor, ava_opt.trimFloor, ava_opt.trimMinMatches = corr_trim
        if max_corr_dist is not None:
            ava_opt.max_corr_dist = max_corr_dist
        if render_occlusion is not None:
            ava_opt.renderOcclusion = bool(render_occlusion)
        self.ava = ava_opt.ava
        self.interval = interval                      # demo.cpp:58  --data-interval
        self.frameICPIters = frame_icp_iters          # demo.cpp:63  --frame-icp-iters
        self.reinitICPIters = reinit_icp_iters        # demo.cpp:66  --reinit-icp-iters
        self.reinitCnz = reinit_cnz                   # demo.cpp:71  --min-points
        self.num_threads = num_threads
        self.initialPerPartCnz = initial_per_part_cnz # live-demo.cpp:89-90 --initial-per-part-thresh (80 there); 0 = demo.cpp: no per-part check
        self.initialICPIters = reinit_icp_iters if initial_icp_iters is None else initial_icp_iters   # live-demo.cpp:80
        self.firstTime = True                         # live-demo.cpp:256
        self.reinit = True                            # demo.cpp:151
        self.rtree = rtree                            # avatar_amd.rtree.RTree or None (labels supplied by the caller)
        self.rtreeInterval = rtree_interval           # demo.cpp:198 (predictBest / postProcess interval)
        self.distToPreWeight = dist_to_pre_weight     # live-demo.cpp:104-108
        self.comPre = None                            # demo.cpp:148: previous centres of mass for the post-processor

    def subsample(self, xyz, part_mask, bbox=None):
        """Every `interval`-th pixel of the bounding box that carries a body-part label (demo.cpp:216-250);
        y is negated (:245).  Returns (data_cloud (n,3) float64, labels (n,) int32)."""
        return subsample(xyz, part_mask, bbox, self.interval, self.opt.numParts)

    def process(self, xyz, part_mask, bbox=None):
        """One tracked frame.  Returns True if the avatar was fitted, False if tracking was declared lost
        (too few body pixels: the next frame reinitialises, demo.cpp:225,283-285)."""
        return self._fit(*self.subsample(xyz, part_mask, bbox))

    def _fit(self, data, labels):
        fit, icp_iters, reinit = frame_decision(self, labels, self.opt.numParts)
        if not fit:
            return False
        ava = self.ava
        if reinit:                                    # demo.cpp:252-265
            ava.p, ava.r, ava.w = reinit_state(data, ava.model.numJoints(), len(ava.w))
            ava.update()
        self.opt.optimize(data, labels, icp_iters, self.num_threads)
        return True

    def label(self, xyz, bbox):
        """Per-pixel body parts of a foreground XYZ map with the forest (demo.cpp:196-204): predictBest on the GPU at
        `rtree_interval` inside the bounding box, then postProcess.  bbox = (top, left, bottom, right) inclusive."""
        return self.label_depth(np.ascontiguousarray(xyz[:, :, 2], np.float32), bbox)

    def label_depth(self, depth, bbox):
        """label() on the foreground depth image (H,W) itself."""
        if self.rtree is None:
            raise RuntimeError("FrameTracker.label: no RTree attached")
        top, left, bottom, right = bbox
        mask = self.rtree.predictBest(depth, 0, self.rtreeInterval, (left, top), (right, bottom))
        self.comPre = self.rtree.postProcess(mask, self.comPre, self.rtreeInterval, 1, (left, top), (right, bottom), self.distToPreWeight)
        return mask

    def process_depth(self, xyz, bbox):
        """One tracked frame from depth alone: label() then process()."""
        return self.process(xyz, self.label(xyz, bbox), bbox)

    def process_depth_image(self, depth, intrin, bbox):
        """process_depth() from the foreground depth image (H,W) float32 and its camera (a depth.CameraIntrin or fx, fy, cx, cy):
        no XYZ map is built, the kept pixels alone are back-projected (subsample_depth)."""
        depth = np.ascontiguousarray(depth, np.float32)
        mask = self.label_depth(depth, bbox)
        return self._fit(*subsample_depth(depth, intrin, mask, bbox, self.interval, self.opt.numParts))


class _Stream:
    """Policy and state of one stream of a MultiFrameTracker, under FrameTracker's attribute names (frame_decision reads them)."""

    def __init__(self, interval, frame_icp_iters, reinit_icp_iters, reinit_cnz, initial_per_part_cnz, initial_icp_iters):
        self.interval = interval
        self.frameICPIters = frame_icp_iters
        self.reinitICPIters = reinit_icp_iters
        self.reinitCnz = reinit_cnz
        self.initialPerPartCnz = initial_per_part_cnz
        self.initialICPIters = reinit_icp_iters if initial_icp_iters is None else initial_icp_iters
        self.firstTime = True
        self.reinit = True
        self.framesFitted = 0


class MultiFrameTracker:
    """S independent FrameTracker streams fitted together: one batched fit per step over one resident frame per stream.

    Every stream has exactly FrameTracker's policy and state (`streams[s]`: reinit, firstTime, interval, the three ICP budgets,
    reinitCnz, initialPerPartCnz).  A step subsamples every stream's frame on the host, makes the S frames resident (the warm
    states stay resident), installs the start state of the streams that reinitialise (avt_state_upload_frames; the first step
    installs all S with avt_state_upload), fits every stream with its own ICP budget in ONE call (avt_optimize_resident_budgets;
    a lost stream has budget 0 and keeps its state) and downloads all states once.  Posed clouds are fetched on request (posed()).

    `ctx` is an api.Context with room for S frames of `max_points` points (create() makes one)."""

    def __init__(self, ctx, num_streams, interval=12, frame_icp_iters=3, reinit_icp_iters=6, reinit_cnz=1000, initial_per_part_cnz=0,
                 initial_icp_iters=None, beta_pose=0.1, beta_shape=1.0, max_iters_per_icp=10, enable_occlusion=True,
                 function_tolerance=1e-4, render_occlusion=None, max_corr_dist=None, corr_trim=None):
        """render_occlusion: None (off), or (intrin, (width, height)): self-occlusion visibility from a face-id render with that camera
        (api.Context.set_occlusion_render; not a reference behaviour).  `renderOcclusion` holds it; set_render_occlusion changes it.
        max_corr_dist: None (the context's gate is left as it is), or a distance / numParts distances: the correspondence gate of every
        stream (api.Context.set_corr_gate; not a reference behaviour).  set_corr_gate changes it; ctx.corr_gate() tells what is in force.
        corr_trim: None (the context's trim settings are left as they are), or (quantile, factor, floor, min_matches): trimmed ICP on
        every stream (api.Context.set_corr_trim; not a reference behaviour).  set_corr_trim changes it; ctx.corr_trim() tells what is
        in force."""
        self.ctx = ctx
        if corr_trim is not None:
            self.set_corr_trim(*corr_trim)
        if max_corr_dist is not None:
            self.set_corr_gate(max_corr_dist)
        self.renderOcclusion = None
        if render_occlusion:
            self.set_render_occlusion(render_occlusion)
        self.S = int(num_streams)
        self.numParts = ctx.num_parts
        self.J, self.K = ctx.model.numJoints(), ctx.model.numShapeKeys()
        self.streams = [_Stream(interval, frame_icp_iters, reinit_icp_iters, reinit_cnz, initial_per_part_cnz, initial_icp_iters)
                        for _ in range(self.S)]
        self.betaPose, self.betaShape = beta_pose, beta_shape
        self.maxItersPerICP, self.enableOcclusion, self.functionTolerance = max_iters_per_icp, enable_occlusion, function_tolerance
        self.p = np.zeros((self.S, 3))
        self.q = np.zeros((self.S, self.J, 4)); self.q[:, :, 3] = 1.0
        self.w = np.zeros((self.S, self.K))
        self.stats = [None] * self.S                  # avt_stats of every stream's last fit
        self.state_resident = False
        self.last_budgets = None                      # the budget vector of the last step (0 = not fitted)
        self.last_reinit = []                         # the streams re-installed by the last step

    @classmethod
    def create(cls, model: "api.AvatarModel", num_streams, num_parts=None, part_map=None, max_points=200000, device=None, **kw):
        J = model.numJoints()
        pm = np.arange(J, dtype=np.int32) if part_map is None else np.asarray(part_map, np.int32)
        ctx = api.Context(model, J if num_parts is None else num_parts, pm, max_points, num_streams, device)
        return cls(ctx, num_streams, **kw)

    def set_render_occlusion(self, render_occlusion):
        """None / False: off; (intrin, (width, height)): on with that camera.  Takes effect for the following steps."""
        if not render_occlusion:
            self.ctx.set_occlusion_render(None)
            self.renderOcclusion = None
        else:
            intrin, size = render_occlusion
            self.ctx.set_occlusion_render(size, intrin)
            self.renderOcclusion = (intrin, tuple(size))

    def set_corr_gate(self, max_corr_dist):
        """None: off; a distance or numParts distances: one gate for all streams.  Takes effect for the following steps."""
        self.ctx.set_corr_gate(max_corr_dist)

    def set_corr_trim(self, quantile=None, factor=1.0, floor=0.0, min_matches=1):
        """quantile None: off; else one setting for all streams (api.Context.set_corr_trim).  Takes effect for the following steps."""
        self.ctx.set_corr_trim(quantile, factor, floor, min_matches)

    def options(self, icp_iters):
        o = api.Options.reference_defaults()
        o.beta_pose, o.beta_shape = self.betaPose, self.betaShape
        o.max_iters_per_icp, o.enable_occlusion, o.icp_iters = self.maxItersPerICP, int(self.enableOcclusion), icp_iters
        o.function_tolerance = self.functionTolerance
        return o

    def process(self, frames):
        """One step: `frames` holds one (xyz (H,W,3), part mask (H,W) uint8, bbox or None) per stream.  Returns the list of
        per-stream fitted flags (False: tracking lost, the stream's next fitted frame reinitialises)."""
        if len(frames) != self.S:
            raise ValueError(f"MultiFrameTracker.process: {len(frames)} frames for {self.S} streams")
        return self._fit([subsample(xyz, mask, bbox, self.streams[s].interval, self.numParts) for s, (xyz, mask, bbox) in enumerate(frames)])

    def _fit(self, clouds):
        """process() behind the subsampling: `clouds` holds every stream's (data_cloud, labels)."""
        datas, labels, budgets, reinit, fitted = [], [], np.zeros(self.S, np.int32), [], []
        for s, (d, l) in enumerate(clouds):
            fit, icp_iters, re = frame_decision(self.streams[s], l, self.numParts)
            fitted.append(fit)
            if not fit:                               # nothing of a lost stream's frame is needed: it rides as an empty frame
                d, l = d[:0], l[:0]
            budgets[s] = icp_iters if fit else 0
            if re:
                reinit.append(s)
                p, r, w = reinit_state(d, self.J, self.K)
                self.p[s], self.q[s], self.w[s] = p, api.rot_to_quat(r), w
            datas.append(d); labels.append(l)
        self.last_budgets, self.last_reinit = budgets.copy(), list(reinit)
        if not any(fitted):
            return fitted
        self.ctx.frames_upload(datas, labels)
        return self._fit_resident(fitted, budgets, reinit)

    def _fit_resident(self, fitted, budgets, reinit):
        """_fit behind the frame install: start states, the batched fit, one download of all states."""
        ctx = self.ctx
        if not self.state_resident:
            ctx.state_upload(self.p, self.q, self.w)
            self.state_resident = True
        elif reinit:
            ctx.state_upload_frames(reinit, self.p[reinit], self.q[reinit], self.w[reinit])
        ctx.optimize_resident_budgets(self.options(int(budgets.max())), budgets)
        p, q, w, st = ctx.state_download()
        for s in range(self.S):
            if fitted[s]:
                self.p[s], self.q[s], self.w[s], self.stats[s] = p[s], q[s], w[s], st[s]
                self.streams[s].framesFitted += 1
        return fitted

    # ---- depth in: the front end of demo.cpp:179-204 for all streams at once ----
    def attach_front_end(self, bgsub, rtree, rtree_interval=2, dist_to_pre_weight=0.001, device_post_process=False, device_subsample=False):
        """`bgsub`: a bgsub.BGSubtractor holding one background per stream; `rtree`: an rtree.RTree on the same device.
        device_post_process: postProcess runs on the device for all streams at once (rtree.post_process_from_bgsub: connected
        components on the interval grid; the reference's result at rtree_interval 1, a documented difference above it) and
        comPre is the forest's resident memory, slot s for stream s.  Off, postProcess runs per stream on the host as ever.
        device_subsample (needs device_post_process): the subsampling and the frame install run on the device too
        (api.Context.frames_subsample / frames_commit): no label image comes down and no cloud goes up; the same frames, budgets
        and states as without it.  `labels` is then None after a step and download_labels() fetches the masks on request."""
        if device_subsample and not device_post_process:
            raise ValueError("MultiFrameTracker.attach_front_end: device_subsample needs device_post_process=True")
        self.bgsub, self.rtree = bgsub, rtree
        self.devicePostProcess = bool(device_post_process)
        self.deviceSubsample = bool(device_subsample)
        self._stepped = False                         # a depth-in step has run: the front end holds its batch (fit_score)
        self.rtreeInterval, self.distToPreWeight = rtree_interval, dist_to_pre_weight
        self.comPre = [None] * self.S                 # demo.cpp:148, per stream
        self.boxes = [None] * self.S                  # ((tl.x, tl.y), (br.x, br.y)) of every stream's last background subtraction
        self.labels = None

    def process_depth(self, images):
        """One step from S XYZ maps (S, H, W, 3): background subtraction of image s against background s (every slot keeps the box
        of its previous run), the forest on the masked depth inside every image's box, both without leaving the device; one
        download of all labels and of the S boxes; postProcess per stream on the host (a sequential flood fill, as in the
        reference); then process() with the caller's XYZ.  A stream whose box is empty, or not inside the image, has an all-255
        mask: it goes through postProcess on the whole image (every comPre x becomes -1) and is lost in process()."""
        self._front_end("process_depth", len(images))
        self.bgsub.upload(images)
        if self.deviceSubsample:
            return self._fit_device()
        return self.process([(images[s], mask, bbox) for s, (mask, bbox) in enumerate(self._label_resident())])

    def process_depth_images(self, depths, intrins):
        """process_depth() from S depth images (S, H, W) float32 and `intrins`, one camera for all streams or (S, 4) fx fy cx cy:
        the depth is what crosses the bus, the XYZ maps are built on the device (BGSubtractor.upload_depth) and never come back;
        the subsampling back-projects the kept pixels alone (subsample_depth)."""
        self._front_end("process_depth_images", len(depths))
        k = intrin_array(intrins, self.S)
        self.bgsub.upload_depth(depths, k)
        if self.deviceSubsample:
            return self._fit_device()
        return self._fit([subsample_depth(depths[s], k[s], mask, bbox, self.streams[s].interval, self.numParts)
                          for s, (mask, bbox) in enumerate(self._label_resident())])

    def _front_end(self, who, n):
        if getattr(self, "bgsub", None) is None:
            raise RuntimeError(f"MultiFrameTracker.{who}: no front end attached (attach_front_end)")
        if n != self.S:
            raise ValueError(f"MultiFrameTracker.{who}: {n} images for {self.S} streams")

    def _label_resident(self):
        """The front end behind the upload, whatever its kind: per stream the post-processed part mask and the box to subsample."""
        self.bgsub.run_resident()
        self.rtree.predict_from_bgsub(self.bgsub, self.rtreeInterval)
        if getattr(self, "devicePostProcess", False):
            return self._label_resident_device()
        labels = self.rtree.download_all_labels()
        out = []
        for s in range(self.S):
            res = self.bgsub.info(s)
            tl, br = res.topLeft, res.botRight
            self.boxes[s] = (tl, br)
            H, W = labels[s].shape
            if 0 <= tl[0] <= br[0] < W and 0 <= tl[1] <= br[1] < H:
                self.comPre[s] = self.rtree.postProcess(labels[s], self.comPre[s], self.rtreeInterval, 1, tl, br, self.distToPreWeight)
                bbox = (tl[1], tl[0], br[1], br[0])
            else:
                self.comPre[s] = self.rtree.postProcess(labels[s], self.comPre[s], self.rtreeInterval, 1, (0, 0), (-1, -1), self.distToPreWeight)
                bbox = (H - 1, W - 1, 0, 0)           # nothing to subsample
            out.append((labels[s], bbox))
        self.labels = labels                          # the step's post-processed part masks (S, H, W)
        self._stepped = True
        return out

    def _label_resident_device(self):
        """_label_resident with the post-processing on the device: nothing per stream on the host but the box."""
        self.rtree.post_process_from_bgsub(self.bgsub, self.rtreeInterval, self.distToPreWeight)
        labels = self.rtree.download_all_labels()
        com, _ = self.rtree.com_pre_get(0, self.S)
        out = []
        for s in range(self.S):
            res = self.bgsub.info(s)
            tl, br = res.topLeft, res.botRight
            self.boxes[s] = (tl, br)
            self.comPre[s] = com[s]
            H, W = labels[s].shape
            inside = 0 <= tl[0] <= br[0] < W and 0 <= tl[1] <= br[1] < H
            out.append((labels[s], (tl[1], tl[0], br[1], br[0]) if inside else (H - 1, W - 1, 0, 0)))
        self.labels = labels
        self._stepped = True
        return out

    def _fit_device(self):
        """A depth-in step behind the upload with everything up to the fit on the device: labelling, post-processing,
        subsampling into the context's frame slots (the centroids of the streams that may reinitialise come back with the
        counts), the policy on the counts, the commit with the lost streams as empty frames, then _fit's tail."""
        self.bgsub.run_resident()
        self.rtree.predict_from_bgsub(self.bgsub, self.rtreeInterval)
        self.rtree.post_process_from_bgsub(self.bgsub, self.rtreeInterval, self.distToPreWeight)
        self.bgsub.info(0)                            # the one read of the subtractor's fault word (bgsub.info raises on it)
        ctx = self.ctx
        counts, centroid, boxes = ctx.frames_subsample(self.bgsub, self.rtree, [st.interval for st in self.streams], None,
                                                       [st.reinit for st in self.streams])
        com, _ = self.rtree.com_pre_get(0, self.S)
        self.labels, self._stepped = None, True
        budgets, reinit, fitted = np.zeros(self.S, np.int32), [], []
        for s in range(self.S):
            self.boxes[s] = ((int(boxes[s, 0]), int(boxes[s, 1])), (int(boxes[s, 2]), int(boxes[s, 3])))
            self.comPre[s] = com[s]
            fit, icp_iters, re = frame_decision(self.streams[s], None, self.numParts, counts=counts[s])
            fitted.append(fit)
            budgets[s] = icp_iters if fit else 0
            if re:
                reinit.append(s)
                p, r, w = reinit_state(centroid[s][None], self.J, self.K)     # (the mean of one row is the row)
                self.p[s], self.q[s], self.w[s] = p, api.rot_to_quat(r), w
        self.last_budgets, self.last_reinit = budgets.copy(), list(reinit)
        if not any(fitted):
            return fitted
        ctx.frames_commit(fitted)
        return self._fit_resident(fitted, budgets, reinit)

    def download_labels(self):
        """The post-processed part masks (S, H, W) of the last depth-in step: `labels` where the step brought them down, one
        download where it did not (device_subsample)."""
        if not getattr(self, "_stepped", False):
            raise RuntimeError("MultiFrameTracker.download_labels: no step behind the front end (process_depth or process_depth_images)")
        return self.labels if self.labels is not None else self.rtree.download_all_labels()

    def posed(self, stream):
        """(cloud (V,3), jointPos (J,3), jointTrans (J,12)) of the stream's last fit (one download; avt_get_posed)."""
        return self.ctx.posed(stream)

    def render(self, streams, size, intrin, what=None, part_map=None):
        """The last fit of the given streams rendered on the device in one run, read straight from the context (no cloud download;
        avatar_amd.render): a list of dicts as render.Renderer.download returns them.  `what`: render.* bits, Lambert by default."""
        from . import render
        return render.render_streams(self, streams, size, intrin, render.LAMBERT if what is None else what, part_map)

    def fit_score(self, streams, size, intrin, tol=None, stride=1, part_map=None):
        """How well the last fit of the given streams explains the depth images of the last step (avatar_amd.fitscore, the numbers
        behind the overlay of live-demo.cpp:428-445): depth and part mask of the streams' fit are rendered from the context with
        the tracker's own renderer and scored on the device against the attached front end's last batch, image streams[i] of it,
        inside the box that run found.  Returns the (len(streams), numParts + 1, 7) int64 tables (fitscore.metrics derives the
        figures).  `tol` defaults to fitscore.DEFAULT_TOL, a choice and not a measurement; `part_map` as in render().  Nothing
        calls this by default and no threshold is offered: a caller who trusts one sets streams[s].reinit = True on it."""
        from . import fitscore, render
        if getattr(self, "bgsub", None) is None:
            raise RuntimeError("MultiFrameTracker.fit_score: no front end attached (attach_front_end)")
        if not getattr(self, "_stepped", False):
            raise RuntimeError("MultiFrameTracker.fit_score: no step behind the front end (process_depth or process_depth_images)")
        if not self.state_resident:
            raise RuntimeError("MultiFrameTracker.fit_score: no stream has been fitted yet")
        streams = [int(s) for s in streams]
        sc = getattr(self, "_fit_scorer", None)
        if sc is None or sc.max_images < len(streams):
            sc = self._fit_scorer = fitscore.FitScorer(self.numParts, max(self.S, len(streams)), getattr(self.ctx, "device", 0))
        r = render.render_streams(self, streams, size, intrin, render.DEPTH | render.PART_MASK, part_map, download=False)
        return sc.score_rendered_from_bgsub(r, self.bgsub, streams, fitscore.DEFAULT_TOL if tol is None else tol, stride)

    def pose_error(self, streams, truth_clouds, truth_joints, part_map=None):
        """How far the last fit of the given streams is from the truth (avatar_amd.poseerror: PVE, MPJPE and the Procrustes-aligned
        forms, in metres): the estimate side is read from the context on the device, the truth side is given, truth_clouds
        (len(streams), V, 3) and truth_joints (len(streams), J, 3).  Parts are numParts parts over the main joints through
        `part_map` (None: the joint itself, which needs numParts >= J).  Returns what poseerror.PoseError.get returns, with the
        figures of poseerror.metrics under "metrics".  Nothing calls this by default and no threshold is offered."""
        from . import poseerror
        if not self.state_resident:
            raise RuntimeError("MultiFrameTracker.pose_error: no stream has been fitted yet")
        streams = [int(s) for s in streams]
        key = None if part_map is None else tuple(int(x) for x in part_map)
        pe = getattr(self, "_pose_scorer", None)
        if pe is None or pe.max_pairs < len(streams) or self._pose_scorer_key != key:
            pe = self._pose_scorer = poseerror.PoseError.for_model(self.ctx.model, self.numParts, part_map, max(self.S, len(streams)),
                                                                   getattr(self.ctx, "device", 0))
            self._pose_scorer_key = key
        pe.from_context(poseerror.ESTIMATE, self.ctx, streams)
        pe.upload(poseerror.TRUTH, truth_clouds, truth_joints)
        pe.run()
        out = pe.get()
        out["metrics"] = pe.metrics(out)
        return out

    def rotations(self, stream):
        """The stream's joint rotations (J,3,3), as FrameTracker's Avatar.r holds them."""
        return api.quat_to_rot(self.q[stream])
