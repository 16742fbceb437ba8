"""The contract of a context (avatar_amd/csrc/avt_capi.cpp) as a caller sees it, on the smallest inputs at which its host paths can go
wrong: the models (9, 4, "star") - which has the moment form - and (5, 16, "star") - which has not - of tests/fit_models.py, a context of
max_frames = 8 and max_points = 512, frames of fit_frame.

  a  every refusal of the staging calls, the read-backs and the settings, with its text; through raw ctypes where the Python wrapper
     would check first
  b  the state machine: a refused setter changes nothing, a setting that is set, unset and set again fits like a fresh context
  c  the graph cache: more launch shapes than it holds, then the first again; a change of tuning drops what was captured
  d  the staged calls (frames_upload, state_upload, optimize_resident, state_download) and the host-pointer call (optimize_batch) give the
     same bits at 1, 2, 3 and 8 frames in both forms of the data term, with one empty frame in the batch"""
import ctypes as C

import numpy as np
import pytest

import fit_models as fm

pytestmark = pytest.mark.gpu

MAX_FRAMES, MAX_POINTS = 8, 512
MOM, ROWS_ONLY = (9, 4, "star"), (5, 16, "star")
NEITHER = ": neither a stand-alone avt_nn (frame 0) nor an optimize call with an ICP iteration has run last"
NO_RUN = ": no optimize call has run on the resident frames"
NO_RUN_VIS = "avt_get_visibility: no optimize call with an ICP iteration has run on the resident frames"


class Rig:
    """a model on the device, its oracle, eight frames of it and what the raw calls need"""

    def __init__(self, key):
        from avatar_amd import api, capi
        from oracle import oracle as orc
        self.m = fm.fit_model(*key)
        self.gm = api.AvatarModel(self.m)
        self.om = orc.OracleModel(self.m)
        self.frs = [fm.fit_frame(self.m, self.om, seed) for seed in range(MAX_FRAMES)]
        self.lib = capi.load_library()
        self.V, self.J, self.K = self.om.V, self.om.J, self.om.K

    def ctx(self, form=None, **tuning):
        from avatar_amd import api
        fr = self.frs[0]
        c = api.Context(self.gm, fr["num_parts"], fr["part_map"], MAX_POINTS, MAX_FRAMES, device=0)
        if tuning:
            c.set_tuning(**tuning)
        if form is not None:
            c.set_data_term(form)
        return c

    def opt(self, icp_iters=2, max_iters_per_icp=3):
        return fm.options(self.frs[0], icp_iters=icp_iters, max_iters_per_icp=max_iters_per_icp)

    def start(self, frs):
        return tuple(np.stack([fr["start"][k] for fr in frs]) for k in range(3))

    def err(self):
        return self.lib.avt_last_error().decode()


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(key):
        if key not in made:
            made[key] = Rig(key)
        return made[key]
    return get


def _empty(fr):
    return dict(fr, data=np.zeros((0, 3)), labels=np.zeros(0, np.int32))


def _bits(ctx, frs, p, q, w, st):
    """everything a fit leaves that a caller can read, per frame (the posed cloud only where the frame has points)"""
    stats = np.array([[s.initial_cost, s.final_cost, s.lambda_, s.num_correspondences, s.matched_model_points, s.gn_iterations, s.accepted_steps] for s in st])
    out = dict(p=p, q=q, w=w, stats=stats)
    for f, fr in enumerate(frs):
        out[f"corr{f}"] = ctx.correspondences(f, len(fr["labels"]))
        if len(fr["labels"]):
            out[f"cloud{f}"] = ctx.cloud(f)
    return out


def _host(rig, ctx, frs, opt):
    p0, q0, w0 = rig.start(frs)
    return _bits(ctx, frs, *ctx.optimize_batch([fr["data"] for fr in frs], [fr["labels"] for fr in frs], opt, p0, q0, w0))


def _staged(rig, ctx, frs, opt, budgets=None):
    ctx.frames_upload([fr["data"] for fr in frs], [fr["labels"] for fr in frs])
    ctx.state_upload(*rig.start(frs))
    if budgets is None:
        ctx.optimize_resident(opt)
    else:
        ctx.optimize_resident_budgets(opt, budgets)
    return _bits(ctx, frs, *ctx.state_download())


def _differ(a, b):
    """the entries in which two _bits differ (NaN equals NaN: the same bits are wanted, not the same numbers)"""
    return [k for k in a if k not in b or not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")] + [k for k in b if k not in a]


def _refused(rig, rc, text):
    assert rc == 1 and rig.err() == text, f"returned {rc} with {rig.err()!r}, wanted 1 with {text!r}"


def _last_search_calls(rig, ctx, frame):
    """{name: status} of the four read-backs of what the last search left"""
    from avatar_amd.capi import dptr, iptr
    lib, h, np_ = rig.lib, ctx.h, ctx.num_parts
    n, pp, T = C.c_int(), np.zeros(np_, np.int32), np.zeros(np_)
    cnt, fsum, centre = np.zeros(rig.V, np.int32), np.zeros((3, rig.V), np.int64), np.zeros(3)
    calls = {}
    for name, call in (("avt_debug_nn_sums", lambda: lib.avt_debug_nn_sums(h, frame, iptr(cnt), fsum.ctypes.data_as(C.POINTER(C.c_longlong)), dptr(centre))),
                       ("avt_get_gated", lambda: lib.avt_get_gated(h, frame, C.byref(n))),
                       ("avt_get_trimmed", lambda: lib.avt_get_trimmed(h, frame, C.byref(n), iptr(pp))),
                       ("avt_get_trim_thresholds", lambda: lib.avt_get_trim_thresholds(h, frame, dptr(T)))):
        rc = call()
        calls[name] = (rc, rig.err() if rc else "")
    return calls


def _fit_reads(rig, ctx, frame):
    """{name: (status, text)} of the three read-backs that need an optimize call on the resident frames"""
    from avatar_amd.capi import bptr, dptr
    lib, h, P = rig.lib, ctx.h, 3 + 3 * rig.J + rig.K
    H, g, cost, vis = np.zeros((P, P)), np.zeros(P), C.c_double(), np.zeros(rig.V, np.uint8)
    a, b, c = C.c_longlong(), C.c_longlong(), C.c_longlong()
    calls = {}
    for name, call in (("avt_get_normal_equations", lambda: lib.avt_get_normal_equations(h, frame, dptr(H), dptr(g), C.byref(cost))),
                       ("avt_debug_mfma_count", lambda: lib.avt_debug_mfma_count(h, frame, C.byref(a), C.byref(b), C.byref(c))),
                       ("avt_get_visibility", lambda: lib.avt_get_visibility(h, frame, bptr(vis)))):
        rc = call()
        calls[name] = (rc, rig.err() if rc else "")
    return calls


def test_what_the_last_search_left_is_refused_until_there_is_one(rigs):
    """a: "no optimize call has run" and "neither a stand-alone avt_nn" on a fresh context, after avt_nn, after a fit without an ICP
    iteration and after a frames upload; granted after a fit with one."""
    rig = rigs(MOM)
    fr = rig.frs[0]
    ctx = rig.ctx()
    # before any call: nothing resident, so the reads that take a resident frame refuse the frame
    assert _last_search_calls(rig, ctx, 0) == {n: (1, n + NEITHER) for n in ("avt_debug_nn_sums", "avt_get_gated", "avt_get_trimmed", "avt_get_trim_thresholds")}
    assert _fit_reads(rig, ctx, 0) == {n: (1, n + ": bad argument") for n in ("avt_get_normal_equations", "avt_debug_mfma_count", "avt_get_visibility")}
    # after a stand-alone search: frame 0 holds its counts, no other frame does, and no fit has run
    ctx.nn(rig.om.points(*fr["start"]), np.ones(rig.V, np.uint8), fr["data"], fr["labels"])
    assert _last_search_calls(rig, ctx, 0) == {n: (0, "") for n in ("avt_debug_nn_sums", "avt_get_gated", "avt_get_trimmed", "avt_get_trim_thresholds")}
    assert ctx.gated(0) == 0 and ctx.trimmed(0) == 0 and np.isinf(ctx.trim_thresholds(0)).all()
    assert _last_search_calls(rig, ctx, 1) == {n: (1, n + NEITHER) for n in ("avt_debug_nn_sums", "avt_get_gated", "avt_get_trimmed", "avt_get_trim_thresholds")}
    want = {"avt_get_normal_equations": (1, "avt_get_normal_equations" + NO_RUN), "avt_debug_mfma_count": (1, "avt_debug_mfma_count" + NO_RUN),
            "avt_get_visibility": (1, NO_RUN_VIS)}
    assert _fit_reads(rig, ctx, 0) == want
    # after a fit without an ICP iteration
    _host(rig, ctx, rig.frs[:2], rig.opt(icp_iters=0))
    for f in (0, 1):
        assert _last_search_calls(rig, ctx, f) == {n: (1, n + NEITHER) for n in ("avt_debug_nn_sums", "avt_get_gated", "avt_get_trimmed", "avt_get_trim_thresholds")}
        assert _fit_reads(rig, ctx, f) == want
    # after a fit with one, everything is granted for the resident frames and refused behind them
    _host(rig, ctx, rig.frs[:2], rig.opt(icp_iters=1))
    for f in (0, 1):
        assert _last_search_calls(rig, ctx, f) == {n: (0, "") for n in ("avt_debug_nn_sums", "avt_get_gated", "avt_get_trimmed", "avt_get_trim_thresholds")}
        assert _fit_reads(rig, ctx, f) == {n: (0, "") for n in ("avt_get_normal_equations", "avt_debug_mfma_count", "avt_get_visibility")}
    assert _last_search_calls(rig, ctx, 2) == {n: (1, n + NEITHER) for n in ("avt_debug_nn_sums", "avt_get_gated", "avt_get_trimmed", "avt_get_trim_thresholds")}
    assert _fit_reads(rig, ctx, 2) == {n: (1, n + ": bad argument") for n in ("avt_get_normal_equations", "avt_debug_mfma_count", "avt_get_visibility")}
    # a frames upload on a fresh context: frames resident, nothing searched, no state
    ctx = rig.ctx()
    ctx.frames_upload([fr["data"]], [fr["labels"]])
    assert _last_search_calls(rig, ctx, 0) == {n: (1, n + NEITHER) for n in ("avt_debug_nn_sums", "avt_get_gated", "avt_get_trimmed", "avt_get_trim_thresholds")}
    assert _fit_reads(rig, ctx, 0) == want


def test_null_arguments_and_frames_out_of_range(rigs):
    """a: the null and range checks of the staging calls and the read-backs, on a context that has fitted two frames."""
    from avatar_amd.capi import Stats, bptr, dptr, iptr
    rig = rigs(MOM)
    lib, frs, opt = rig.lib, rig.frs[:2], rig.opt(icp_iters=1)
    ctx = rig.ctx()
    _staged(rig, ctx, frs, opt)
    h, V, J = ctx.h, rig.V, rig.J
    d, i, b = dptr(np.zeros(3 * 4 * max(V, MAX_POINTS))), iptr(np.zeros(MAX_POINTS + 16, np.int32)), bptr(np.zeros(V, np.uint8))
    n, o = C.c_int(), C.byref(opt)
    for f in (-1, 2):       # two frames resident
        _refused(rig, lib.avt_get_correspondences(h, f, i), "avt_get_correspondences: bad argument")
        _refused(rig, lib.avt_get_visibility(h, f, b), "avt_get_visibility: bad argument")
        _refused(rig, lib.avt_frames_download(h, f, d, i), "avt_frames_download: bad argument")
        _refused(rig, lib.avt_get_normal_equations(h, f, d, d, None), "avt_get_normal_equations: bad argument")
        _refused(rig, lib.avt_debug_mfma_count(h, f, None, None, None), "avt_debug_mfma_count: bad argument")
    for f in (-1, MAX_FRAMES):      # the reads of a frame slot
        _refused(rig, lib.avt_get_cloud(h, f, d), "avt_get_cloud: bad argument")
        _refused(rig, lib.avt_get_posed(h, f, d, None, None), "avt_get_posed: bad argument")
        _refused(rig, lib.avt_debug_trace(h, f, d), "avt_debug_trace: bad argument")
        _refused(rig, lib.avt_debug_nn_sums(h, f, None, None, None), "avt_debug_nn_sums: bad argument")
        _refused(rig, lib.avt_get_gated(h, f, C.byref(n)), "avt_get_gated: bad argument")
        _refused(rig, lib.avt_get_trimmed(h, f, C.byref(n), None), "avt_get_trimmed: bad argument")
        _refused(rig, lib.avt_get_trim_thresholds(h, f, d), "avt_get_trim_thresholds: bad argument")
    for call, text in ((lambda: lib.avt_get_correspondences(h, 0, None), "avt_get_correspondences: bad argument"),
                       (lambda: lib.avt_get_correspondences(None, 0, i), "avt_get_correspondences: bad argument"),
                       (lambda: lib.avt_get_cloud(h, 0, None), "avt_get_cloud: bad argument"),
                       (lambda: lib.avt_get_cloud(None, 0, d), "avt_get_cloud: bad argument"),
                       (lambda: lib.avt_get_posed(None, 0, d, None, None), "avt_get_posed: bad argument"),
                       (lambda: lib.avt_get_visibility(h, 0, None), "avt_get_visibility: bad argument"),
                       (lambda: lib.avt_get_visibility(None, 0, b), "avt_get_visibility: bad argument"),
                       (lambda: lib.avt_debug_trace(h, 0, None), "avt_debug_trace: bad argument"),
                       (lambda: lib.avt_debug_nn_sums(None, 0, None, None, None), "avt_debug_nn_sums: bad argument"),
                       (lambda: lib.avt_get_gated(h, 0, None), "avt_get_gated: bad argument"),
                       (lambda: lib.avt_get_gated(None, 0, C.byref(n)), "avt_get_gated: bad argument"),
                       (lambda: lib.avt_get_trimmed(h, 0, None, None), "avt_get_trimmed: null argument"),
                       (lambda: lib.avt_get_trimmed(None, 0, C.byref(n), None), "avt_get_trimmed: null argument"),
                       (lambda: lib.avt_get_trim_thresholds(h, 0, None), "avt_get_trim_thresholds: null argument"),
                       (lambda: lib.avt_get_trim_thresholds(None, 0, d), "avt_get_trim_thresholds: null argument"),
                       (lambda: lib.avt_get_normal_equations(None, 0, d, d, None), "avt_get_normal_equations: bad argument"),
                       (lambda: lib.avt_debug_mfma_count(None, 0, None, None, None), "avt_debug_mfma_count: bad argument"),
                       (lambda: lib.avt_frames_download(None, 0, d, i), "avt_frames_download: bad argument"),
                       (lambda: lib.avt_frames_upload(h, 1, None, i, i), "avt_frames_upload: null argument"),
                       (lambda: lib.avt_frames_upload(h, 1, d, None, i), "avt_frames_upload: null argument"),
                       (lambda: lib.avt_frames_upload(h, 1, d, i, None), "avt_frames_upload: null argument"),
                       (lambda: lib.avt_frames_upload(None, 1, d, i, i), "avt_frames_upload: null argument"),
                       (lambda: lib.avt_state_upload(h, 2, None, d, d), "avt_state_upload: null argument"),
                       (lambda: lib.avt_state_upload(None, 2, d, d, d), "avt_state_upload: null argument"),
                       (lambda: lib.avt_state_download(None, d, d, d, None), "avt_state_download: null context"),
                       (lambda: lib.avt_state_reset(None), "avt_state_reset: no state resident"),
                       (lambda: lib.avt_optimize_resident(h, None), "avt_optimize_resident: null argument"),
                       (lambda: lib.avt_optimize_resident(None, o), "avt_optimize_resident: null argument"),
                       (lambda: lib.avt_optimize_resident_budgets(h, o, None), "avt_optimize_resident_budgets: null argument"),
                       (lambda: lib.avt_optimize_batch(h, 1, d, i, i, o, d, d, None, None), "avt_optimize_batch: null argument"),
                       (lambda: lib.avt_optimize_batch(None, 1, d, i, i, o, d, d, d, None), "avt_optimize_batch: null argument"),
                       (lambda: lib.avt_optimize(h, None, i, 4, o, d, d, d, None), "avt_optimize_batch: null argument"),
                       (lambda: lib.avt_optimize_posed(h, d, i, 4, None, d, d, d, None, None, None, None), "avt_optimize_posed: null argument"),
                       (lambda: lib.avt_lbs_update(h, 1, None, d, d, None, None, None), "avt_lbs_update: null argument"),
                       (lambda: lib.avt_lbs_update(h, MAX_FRAMES + 1, d, d, d, None, None, None), "avt_lbs_update: nframes out of range"),
                       (lambda: lib.avt_visibility(h, None, 1, b), "avt_visibility: null argument"),
                       (lambda: lib.avt_nn(h, d, b, d, None, 4, i), "avt_nn: null argument"),
                       (lambda: lib.avt_set_corr_gate(None, 0, None), "avt_set_corr_gate: null context"),
                       (lambda: lib.avt_get_corr_gate(h, None), "avt_get_corr_gate: null argument"),
                       (lambda: lib.avt_set_corr_trim(None, 0, None, None, None, 1), "avt_set_corr_trim: null context"),
                       (lambda: lib.avt_get_corr_trim(None, d, d, d, None), "avt_get_corr_trim: null context"),
                       (lambda: lib.avt_set_data_term(None, 0), "avt_set_data_term: bad argument"),
                       (lambda: lib.avt_set_data_term(h, 7), "avt_set_data_term: bad argument"),
                       (lambda: lib.avt_ctx_set_tuning(h, None), "avt_ctx_set_tuning: null argument"),
                       (lambda: lib.avt_ctx_get_tuning(h, None), "avt_ctx_get_tuning: null argument"),
                       (lambda: lib.avt_set_occlusion_render(None, 0, 0, 0, 0, 0, 0), "avt_set_occlusion_render: null context"),
                       (lambda: lib.avt_launch_shape(None, None, None, None), "avt_launch_shape: no frames resident"),
                       (lambda: lib.avt_profile_end(h, None), "avt_profile_end: null argument")):
        _refused(rig, call(), text)
    assert lib.avt_get_data_term(None) == -1
    # the frames of a batch, staged or through host pointers: count, sizes, order
    offs9, big, back = np.arange(10, dtype=np.int32), np.array([0, MAX_POINTS + 1], np.int32), np.array([0, 8, 4], np.int32)
    p, q, w = (dptr(np.zeros((MAX_FRAMES + 1) * k)) for k in (3, 4 * J, rig.K))
    st = (Stats * (MAX_FRAMES + 1))()
    for nf, offs, text in ((MAX_FRAMES + 1, offs9, "frames: nframes out of range for this context"), (0, offs9, "frames: nframes out of range for this context"),
                           (1, big, "frames: a frame has more points than max_points_per_frame"),
                           (2, back, "frames: negative point count (frame_offsets must be non-decreasing)")):
        _refused(rig, lib.avt_frames_upload(h, nf, d, i, iptr(offs)), text)
        _refused(rig, lib.avt_optimize_batch(h, nf, d, i, iptr(offs), o, p, q, w, st), text)
    # a refused install changes nothing: the two frames are still resident and fit as before
    ctx.state_reset()
    ctx.optimize_resident(opt)
    assert not _differ(_bits(ctx, frs, *ctx.state_download()), _host(rig, rig.ctx(), frs, opt))


def test_states_and_fits_that_are_not_there(rigs):
    """a: avt_state_upload with the wrong frame count, avt_state_reset without a state, a fit without frames or without a state, budgets out
    of range."""
    from avatar_amd.capi import dptr, iptr
    rig = rigs(MOM)
    lib, opt = rig.lib, rig.opt()
    ctx = rig.ctx()
    h, o = ctx.h, C.byref(opt)
    p, q, w = (np.ascontiguousarray(a) for a in rig.start(rig.frs[:3]))
    no_frames = "avt_optimize: no frames resident (upload frames first; the stand-alone entry points avt_nn / avt_visibility / avt_lbs_update invalidate them)"
    _refused(rig, lib.avt_state_reset(h), "avt_state_reset: no state resident")
    _refused(rig, lib.avt_state_upload(h, 1, dptr(p), dptr(q), dptr(w)), "state: nframes differs from the resident frames")
    _refused(rig, lib.avt_optimize_resident(h, o), no_frames)
    _refused(rig, lib.avt_optimize_resident_budgets(h, o, iptr(np.zeros(8, np.int32))), no_frames)
    ctx.frames_upload([fr["data"] for fr in rig.frs[:2]], [fr["labels"] for fr in rig.frs[:2]])
    _refused(rig, lib.avt_state_reset(h), "avt_state_reset: no state resident")
    for nf in (1, 3):
        _refused(rig, lib.avt_state_upload(h, nf, dptr(p), dptr(q), dptr(w)), "state: nframes differs from the resident frames")
    _refused(rig, lib.avt_optimize_resident(h, o), "avt_optimize: no start state resident for these frames (avt_state_upload)")
    ctx.state_upload(p[:2], q[:2], w[:2])
    _refused(rig, lib.avt_optimize_resident_budgets(h, o, iptr(np.array([1, 3], np.int32))), "avt_optimize_resident_budgets: frame 1 has budget 3, outside [0, icp_iters = 2]")
    _refused(rig, lib.avt_optimize_resident_budgets(h, o, iptr(np.array([-1, 2], np.int32))), "avt_optimize_resident_budgets: frame 0 has budget -1, outside [0, icp_iters = 2]")
    bad = rig.opt()
    bad.max_iters_per_icp = 63
    _refused(rig, lib.avt_optimize_resident(h, C.byref(bad)), "avt_optimize: bad iteration counts")
    # a different number of frames takes the state away, the same number keeps it (the warm start)
    ctx.frames_upload([fr["data"] for fr in rig.frs[2:4]], [fr["labels"] for fr in rig.frs[2:4]])
    ctx.optimize_resident(opt)
    ctx.frames_upload([rig.frs[0]["data"]], [rig.frs[0]["labels"]])
    _refused(rig, lib.avt_optimize_resident(h, o), "avt_optimize: no start state resident for these frames (avt_state_upload)")
    # after the stand-alone entry points nothing is resident
    ctx.nn(rig.om.points(*rig.frs[0]["start"]), np.ones(rig.V, np.uint8), rig.frs[0]["data"], rig.frs[0]["labels"])
    _refused(rig, lib.avt_optimize_resident(h, o), no_frames)
    _refused(rig, lib.avt_state_upload(h, 1, dptr(p), dptr(q), dptr(w)), "state: nframes differs from the resident frames")


def _gates(rig):
    """per part, the median distance of the frame's points from the model at the start state: about half of them lie behind it"""
    fr = rig.frs[0]
    model = rig.om.points(*fr["start"])
    dist = np.sqrt(((fr["data"][:, None, :] - model[None, :, :]) ** 2).sum(2)).min(1)
    return np.full(fr["num_parts"], float(np.median(dist))) * np.linspace(0.9, 1.1, fr["num_parts"])


def test_refused_settings_change_nothing(rigs):
    """a, b: the refusals of the gate, the trim, the data term, the tuning and the occlusion render; after each, every getter returns what
    was set before, and the fit is the fit of a fresh context with those settings."""
    from avatar_amd.capi import dptr
    rig, nomom = rigs(MOM), rigs(ROWS_ONLY)
    lib, opt, frs = rig.lib, rig.opt(icp_iters=1), rig.frs[:2]
    npart = frs[0]["num_parts"]
    assert npart == 9
    gate = _gates(rig)
    rho, kap, flo = np.linspace(0.5, 0.9, npart), np.linspace(1.0, 2.0, npart), np.linspace(0.0, 0.01, npart)
    kap[4] = np.inf

    def settings(c):
        return [c.corr_gate()] + list(c.corr_trim()) + [c.data_term()] + [sorted(c.tuning().as_dict().items())]

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    ctx = rig.ctx()
    fresh = settings(ctx)
    assert np.isinf(fresh[0]).all() and (fresh[1] == 1.0).all() and np.isinf(fresh[2]).all() and (fresh[3] == 0.0).all() and fresh[4] == 1 and fresh[5] == ctx.DATA_TERM_AUTO
    h = ctx.h
    nan9, neg9, two = np.ones(npart), np.ones(npart), np.array([0.1, 0.2])
    nan9[3], neg9[8] = np.nan, -1e-300
    one = np.ones(npart)
    gate_n = "avt_set_corr_gate: 2 values; 0 (off), 1 (every part) or num_parts = 9 wanted"
    gate_v = "avt_set_corr_gate: value %d is negative or not a number (each of the 1 or num_parts = 9 gates is a distance >= 0, +inf allowed)"
    trim_n = "avt_set_corr_trim: 2 values; 0 (off), 1 (every part) or num_parts = 9 wanted"
    trim_v = "avt_set_corr_trim: value %d of the 1 or num_parts = 9 is refused (quantile in (0, 1]; factor >= 0 with a finite square, or +inf; floor_dist >= 0 and finite; no NaN)"
    refusals = [(lambda: lib.avt_set_corr_gate(h, 2, dptr(two)), gate_n),
                (lambda: lib.avt_set_corr_gate(h, npart, dptr(nan9)), gate_v % 3),
                (lambda: lib.avt_set_corr_gate(h, npart, dptr(neg9)), gate_v % 8),
                (lambda: lib.avt_set_corr_gate(h, 1, dptr(np.array([-1.0]))), gate_v % 0),
                (lambda: lib.avt_set_corr_trim(h, 2, dptr(two), dptr(two), dptr(two), 1), trim_n),
                (lambda: lib.avt_set_corr_trim(h, npart, dptr(nan9), dptr(one), dptr(one), 1), trim_v % 3),
                (lambda: lib.avt_set_corr_trim(h, npart, dptr(one), dptr(nan9), dptr(one), 1), trim_v % 3),
                (lambda: lib.avt_set_corr_trim(h, npart, dptr(one), dptr(one), dptr(nan9), 1), trim_v % 3),
                (lambda: lib.avt_set_corr_trim(h, npart, dptr(one), dptr(neg9), dptr(one), 1), trim_v % 8),
                (lambda: lib.avt_set_corr_trim(h, npart, dptr(one), dptr(one), dptr(neg9), 1), trim_v % 8),
                (lambda: lib.avt_set_corr_trim(h, 1, dptr(np.array([0.0])), dptr(one), dptr(one), 1), trim_v % 0),
                (lambda: lib.avt_set_corr_trim(h, 1, dptr(one), dptr(np.array([1e200])), dptr(one), 1), trim_v % 0),
                (lambda: lib.avt_set_corr_trim(h, 1, dptr(one), dptr(one), dptr(np.array([np.inf])), 1), trim_v % 0),
                (lambda: lib.avt_set_corr_trim(h, npart, dptr(one), dptr(one), dptr(one), 0), "avt_set_corr_trim: min_matches = 0; >= 1 wanted (values are per part: 1 or num_parts = 9)"),
                (lambda: lib.avt_set_corr_trim(h, 1, dptr(one), None, dptr(one), 1), "avt_set_corr_trim: quantile, factor and floor_dist go together (all NULL: off)"),
                (lambda: lib.avt_set_data_term(h, 7), "avt_set_data_term: bad argument"),
                (lambda: lib.avt_set_occlusion_render(h, -1, 4, 1, 1, 1, 1), "avt_set_occlusion_render: bad image size (0 < width < 65536, height > 0, width x height < 2^31; width 0 turns the mode off)"),
                (lambda: lib.avt_set_occlusion_render(h, 65536, 4, 1, 1, 1, 1), "avt_set_occlusion_render: bad image size (0 < width < 65536, height > 0, width x height < 2^31; width 0 turns the mode off)")]
    bad_tuning = ctx.tuning()
    bad_tuning.groups = -1
    refusals.append((lambda: lib.avt_ctx_set_tuning(h, C.byref(bad_tuning)), "avt_tuning: a field is out of range (include/avt.h)"))
    for call, text in refusals:     # on the settings a context starts with
        _refused(rig, call(), text)
        assert same(settings(ctx), fresh), text
    assert not _differ(_host(rig, ctx, frs, opt), _host(rig, rig.ctx(), frs, opt))

    def configure(c):
        c.set_corr_gate(gate)
        c.set_corr_trim(rho, kap, flo, 2)
        c.set_data_term(c.DATA_TERM_ROWS)
        c.set_tuning(nspec=2)
    configure(ctx)
    held = settings(ctx)
    assert np.array_equal(held[0], gate) and same(held[1:4], (rho, kap, flo)) and held[4] == 2 and held[5] == ctx.DATA_TERM_ROWS and dict(held[6])["nspec"] == 2
    first = _host(rig, ctx, frs, opt)
    for call, text in refusals:     # on settings of the caller's
        _refused(rig, call(), text)
        assert same(settings(ctx), held), text
    again = _host(rig, ctx, frs, opt)
    other = rig.ctx()
    configure(other)
    assert not _differ(first, again) and not _differ(first, _host(rig, other, frs, opt))
    assert ctx.gated(0) > 0, "the gate of this test drops nothing"
    # the moment form where the model has none
    c5 = nomom.ctx(form=0)
    _refused(nomom, nomom.lib.avt_set_data_term(c5.h, c5.DATA_TERM_MOMENTS), f"avt_set_data_term: this model has no moment form ({fm.MOMENTS_REFUSAL})")
    assert c5.data_term() == c5.DATA_TERM_ROWS
    c5.set_data_term(c5.DATA_TERM_AUTO)
    _refused(nomom, nomom.lib.avt_set_data_term(c5.h, c5.DATA_TERM_MOMENTS), f"avt_set_data_term: this model has no moment form ({fm.MOMENTS_REFUSAL})")
    assert c5.data_term() == c5.DATA_TERM_AUTO
    o5 = nomom.opt(icp_iters=1)
    assert not _differ(_host(nomom, c5, nomom.frs[:2], o5), _host(nomom, nomom.ctx(), nomom.frs[:2], o5))


@pytest.mark.parametrize("which", ["gate", "trim", "budgets"])
def test_set_unset_set_fits_like_a_fresh_context(rigs, which):
    """b: a gate or a trim that is set, unset and set again to the same values - the device block is written, left alone, rewritten - gives
    the fits of a fresh context with that setting, and unset the fits of a fresh context; the same for a budget pattern that changes and
    comes back."""
    rig = rigs(MOM)
    opt, frs = rig.opt(), rig.frs[:3]
    gate = _gates(rig)
    if which == "budgets":
        ctx = rig.ctx()
        runs = [_staged(rig, ctx, frs, opt, b) for b in ([2, 1, 0], [2, 1, 0], [1, 2, 2], [2, 1, 0])]
        fresh = [_staged(rig, rig.ctx(), frs, opt, b) for b in ([2, 1, 0], [1, 2, 2])]
        assert not _differ(runs[0], fresh[0]) and not _differ(runs[1], fresh[0]) and not _differ(runs[2], fresh[1]) and not _differ(runs[3], fresh[0])
        assert _differ(fresh[0], fresh[1]), "the two budget patterns of this test fit alike"
        full, plain = _staged(rig, ctx, frs, opt, [2, 2, 2]), _staged(rig, rig.ctx(), frs, opt)      # every budget at icp_iters: the plain call's states
        assert not [k for k in _differ(full, plain) if not k.startswith("cloud")]
        return

    def turn(c, on):
        if which == "gate":
            c.set_corr_gate(gate if on else None)
        else:
            c.set_corr_trim(0.5, 1.0, 0.0, 2) if on else c.set_corr_trim(None)
    ctx, with_it, without = rig.ctx(), rig.ctx(), rig.ctx()
    turn(with_it, True)
    want_on, want_off = _host(rig, with_it, frs, opt), _host(rig, without, frs, opt)
    assert _differ(want_on, want_off), f"the {which} of this test changes nothing"
    dropped = [with_it.gated(f) if which == "gate" else with_it.trimmed(f) for f in range(len(frs))]
    for on in (True, False, True, True, False, False, True):
        turn(ctx, on)
        assert not _differ(_host(rig, ctx, frs, opt), want_on if on else want_off), f"{which} {'on' if on else 'off'}"
        got = [ctx.gated(f) if which == "gate" else ctx.trimmed(f) for f in range(len(frs))]
        assert got == (dropped if on else [0] * len(frs))


def test_more_launch_shapes_than_the_graph_cache_holds(rigs):
    """c: ten distinct icp_iters on one context - GRAPH_CACHE_ENTRIES is 8 - then the first again: the bits of the first run; every one of them
    the bits of a context that captured nothing else."""
    rig = rigs(MOM)
    frs = rig.frs[:2]
    ctx = rig.ctx()
    assert ctx.tuning().use_graph == 1
    runs = [_host(rig, ctx, frs, rig.opt(icp_iters=k, max_iters_per_icp=2)) for k in range(1, 11)]
    assert not _differ(_host(rig, ctx, frs, rig.opt(icp_iters=1, max_iters_per_icp=2)), runs[0])
    assert not _differ(_host(rig, ctx, frs, rig.opt(icp_iters=10, max_iters_per_icp=2)), runs[9])
    assert not _differ(_host(rig, ctx, frs, rig.opt(icp_iters=2, max_iters_per_icp=2)), runs[1])
    for k in (1, 2, 10):
        assert not _differ(_host(rig, rig.ctx(), frs, rig.opt(icp_iters=k, max_iters_per_icp=2)), runs[k - 1]), k
    assert _differ(runs[0], runs[1])
    plain = _host(rig, rig.ctx(use_graph=0), frs, rig.opt(icp_iters=2, max_iters_per_icp=2))
    assert not _differ(plain, runs[1]), "launched and replayed fits differ"


def test_a_change_of_tuning_drops_the_captured_graphs(rigs):
    """c: four frames with two frame groups, then with the default again, on one context: each the fit of a fresh context with that tuning -
    a graph kept across the change would replay the other split."""
    rig = rigs(MOM)
    frs, opt = rig.frs[:4], rig.opt()
    ctx = rig.ctx()
    default = _host(rig, ctx, frs, opt)
    assert ctx.launch_shape()[0] == 1
    ctx.set_tuning(groups=2)
    assert ctx.launch_shape()[:2] == (2, 2)
    two = _host(rig, ctx, frs, opt)
    ctx.set_tuning(groups=0)
    assert ctx.launch_shape()[0] == 1
    back = _host(rig, ctx, frs, opt)
    assert not _differ(two, _host(rig, rig.ctx(groups=2), frs, opt))
    assert not _differ(default, _host(rig, rig.ctx(), frs, opt)) and not _differ(back, default)
    # the same through the occlusion render's switch, which drops the graphs too (occlusion itself stays off in these fits)
    ctx.set_occlusion_render((16, 12), (10.0, 10.0, 8.0, 6.0))
    assert not _differ(_host(rig, ctx, frs, opt), default)
    ctx.set_occlusion_render(None)
    assert not _differ(_host(rig, ctx, frs, opt), default)


@pytest.mark.parametrize("form", ["rows", "moments"])
@pytest.mark.parametrize("nf", [1, 2, 3, 8])
def test_staged_calls_equal_the_host_pointer_call(rigs, nf, form):
    """d: bit for bit, with one empty frame in the batch (at one frame: the batch of one fitted frame, and the batch that is the empty frame
    alone, which both paths must treat alike - fit it or refuse it with the same text); then once more on the same contexts, and crosswise."""
    from avatar_amd import api
    rig = rigs(MOM)
    kind = api.Context.DATA_TERM_ROWS if form == "rows" else api.Context.DATA_TERM_MOMENTS
    opt = rig.opt()
    batches = [[rig.frs[0]], [_empty(rig.frs[0])]] if nf == 1 else [[_empty(fr) if f == 1 else fr for f, fr in enumerate(rig.frs[:nf])]]
    for frs in batches:
        cs, ch = rig.ctx(form=kind), rig.ctx(form=kind)
        try:
            host = _host(rig, ch, frs, opt)
        except api.AvtError as e:
            assert nf == 1 and not len(frs[0]["labels"])
            with pytest.raises(api.AvtError) as es:
                _staged(rig, cs, frs, opt)
            assert str(es.value) == str(e)
            continue
        staged = _staged(rig, cs, frs, opt)
        assert not _differ(staged, host), f"{nf} frames, {form}: {_differ(staged, host)}"
        assert ch.launch_shape() == cs.launch_shape()
        # the warm restart of the staged calls, and each context through the other path
        cs.state_reset()
        cs.optimize_resident(opt)
        assert not _differ(_bits(cs, frs, *cs.state_download()), host)
        assert not _differ(_host(rig, cs, frs, opt), host) and not _differ(_staged(rig, ch, frs, opt), host)
        if nf > 1:      # the fitted frames moved, the empty one did not
            p0, q0, w0 = rig.start(frs)
            assert np.array_equal(host["p"][1], p0[1]) and np.array_equal(host["q"][1].ravel(), q0[1].ravel()) and np.array_equal(host["w"][1], w0[1])
            assert not np.array_equal(host["q"][0].ravel(), q0[0].ravel())


def test_posed_outputs_of_the_host_pointer_call(rigs):
    """d: avt_optimize_posed brings back what avt_optimize and avt_get_posed bring back, and refuses posed outputs of a call without an ICP iteration."""
    from avatar_amd import api
    rig = rigs(MOM)
    fr, opt = rig.frs[0], rig.opt()
    p0, q0, w0 = fr["start"]
    ctx = rig.ctx()
    p, q, w, st, cloud, jp, jt = ctx.optimize_posed(fr["data"], fr["labels"], opt, p0, q0, w0)
    host = _host(rig, rig.ctx(), [fr], opt)
    assert np.array_equal(p, host["p"][0]) and np.array_equal(q, host["q"][0]) and np.array_equal(w, host["w"][0]) and st.final_cost == host["stats"][0][1]
    got = ctx.posed(0)
    assert np.array_equal(cloud, host["cloud0"]) and all(np.array_equal(a, b) for a, b in zip((cloud, jp, jt), got))
    with pytest.raises(api.AvtError) as e:
        ctx.optimize_posed(fr["data"], fr["labels"], rig.opt(icp_iters=0), p0, q0, w0)
    assert str(e.value) == "avt_optimize_posed: no ICP iteration, no closing update(): nothing posed to return"
