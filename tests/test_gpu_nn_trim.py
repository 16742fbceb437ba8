"""Trimmed ICP (include/avt.h avt_set_corr_trim; avatar_amd/csrc/avt_trim.hip) on the device: every case of
tests/nn_cases.py at rho = 0.5, kappa = 1 through the four device code paths of tests/test_gpu_nn_edges.py, every comparison an integer
equality - or, for the thresholds, an equality of bit patterns - against the numpy restatement (tests/nn_trim_restatement.py); the
boundaries written out by hand (tests/nn_trim_cases.py); off after on; refusals; and inside optimize(): a trimmed fit of a contaminated
frame is the fit of the kept points (CPU oracle on those points alone), trimming acts in every ICP iteration, a changed setting takes
effect on the replayed graph, and a fit whose every match is trimmed is the fit of a frame without a valid label.
tests/test_nn_trim_cpu.py shows on the CPU that none of this is vacuous."""
import numpy as np
import pytest

import nn_cases
import nn_gate_restatement as ng
import nn_restatement as nr
import nn_trim_cases as tc
import nn_trim_restatement as nt
import test_gpu_nn_edges as edges
from avatar_amd import synth
from avatar_amd.capi import Options

pytestmark = pytest.mark.gpu

SHAPES = edges.SHAPES
MAX_POINTS = edges.MAX_POINTS     # 4608, one frame: the stand-alone searches
FIT_POINTS = 5632                 # the contaminated frame has 5 501 points
_TREF = {}


@pytest.fixture(scope="module")
def contexts(gmodel):
    """One Context per (part map, shape), made on first use and kept for the module; every user sets the gate and the trim it wants first."""
    from avatar_amd import api
    made = {}

    def get(pm, npart, shape):
        key = nn_cases.map_key(pm, npart) + (shape,)
        if key not in made:
            made[key] = api.Context(gmodel, npart, pm, MAX_POINTS, 1, device=0).set_tuning(**SHAPES[shape])
        return made[key]
    return get


def _expected(corr, data, total, per_part, T, gated=0):
    return (corr, gated, total, per_part, T) + nr.nn_sums_ref(corr, data, nn_cases.V)


def _trimmed_reference(model, case):
    """What a case must give at rho = 0.5, kappa = 1, floor = 0: computed once from the untrimmed reference tests/test_gpu_nn_edges.py
    keeps, shared by the shapes, never written to."""
    name, pm, npart, cloud, vis, data, labels = case
    if name not in _TREF:
        out, total, per_part, T = nt.trim_ref(edges._reference(model, case)[0], cloud, data, labels, npart, 0.5, 1.0)
        res = _expected(out, data, total, per_part, T)
        for a in res:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _TREF[name] = res
    return _TREF[name]


def _compare(ctx, name, got, corr, gated, total, per_part, T, cnt, fsum, centre, sums=True):
    """'' when the device's indices, bookkeeping, counts of dropped matches and thresholds are the expected ones, else what differs."""
    gc, gf, gcen = ctx.nn_sums(0)
    gt, gpp = ctx.trimmed(0, per_part=True)
    gT = ctx.trim_thresholds(0)
    bad = []
    if not np.array_equal(got, corr):
        bad.append(f"{int((got != corr).sum())} of {len(corr)} indices")
    if not np.array_equal(gc, cnt):
        bad.append(f"{int((gc != cnt).sum())} counts")
    if sums and not np.array_equal(gf, fsum):
        bad.append(f"{int((gf != fsum).any(0).sum())} sums")
    if not np.array_equal(gcen, centre):
        bad.append("centre")
    if ctx.gated(0) != gated:
        bad.append(f"gated {ctx.gated(0)} for {gated}")
    if gt != total or not np.array_equal(gpp, per_part):
        bad.append(f"trimmed {gt} for {total} ({int((gpp != per_part).sum())} parts differ)")
    if gT.tobytes() != np.asarray(T, np.float64).tobytes():
        q = int(np.nonzero(gT.view(np.uint64) != np.asarray(T, np.float64).view(np.uint64))[0][0])
        bad.append(f"T of part {q}: {gT[q]!r} for {T[q]!r}")
    return f"{name}: " + ", ".join(bad) if bad else ""


# ---- 1. every case through every shape ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("group", list(nn_cases.GROUPS))
def test_every_case_through_every_shape_trimmed(smpl, contexts, group, shape):
    """rho = 0.5, kappa = 1, floor = 0, min_matches = 1: every part with two different distances drops and keeps; tests/test_nn_trim_cpu.py
    counts the parts that do, the 9 606 matches that sit exactly on their threshold and the cases with ties on it."""
    failures = []
    for case in nn_cases.cases(smpl, group):
        name, pm, npart, cloud, vis, data, labels = case
        ctx = contexts(pm, npart, shape)
        ctx.set_corr_gate(None)
        ctx.set_corr_trim(0.5, 1.0, 0.0, 1)
        msg = _compare(ctx, name, ctx.nn(cloud, vis, data, labels), *_trimmed_reference(smpl, case))
        if msg:
            failures.append(msg)
    assert not failures, f"shape {shape}: " + "; ".join(failures[:8])


# ---- 2. boundary cases written out by hand ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_boundaries_written_by_hand(smpl, contexts, shape):
    """tests/nn_trim_cases.hand_cases: n = 0, 1, 2; ramps of 255 / 256 / 257 matches (the histogram's bins), 1 023 / 1 024 / 1 025 (one
    turn of a k_trim workgroup's walk and its neighbours) and 4 095 / 4 096 / 4 097 (the LDS key capacity of k_trim and the recomputing
    path beyond it); all distances equal; keys that differ in the lowest mantissa bits; 0, a denormal and 1.79e308 in one part; k = 1
    and k = n; kappa = 0 with and without a
    floor; the floor deciding; min_matches = n and n + 1; a trimmed part beside an untrimmed one; a fixed gate and the trim together."""
    pm, npart, pov, cloud, vis, v0, v1 = tc.hand_model(smpl)
    ctx = contexts(pm, npart, shape)
    failures = []
    for case in tc.hand_cases():
        name, data, labels, gate, (rho, kappa, floor, mm), want, gated, tp, T = tc.expand(case, v0, v1, npart)
        ctx.set_corr_gate(gate)
        ctx.set_corr_trim(rho, kappa, floor, mm)
        got = ctx.nn(cloud, vis, data, labels)
        with np.errstate(invalid="ignore"):      # (tc.NO_SUMS: the reference sums of a kept point 1.3e154 m out are not defined, and not compared)
            exp = _expected(want, data, int(tp.sum()), tp, T, gated)
        msg = _compare(ctx, name, got, *exp, sums=name not in tc.NO_SUMS)
        if msg:
            failures.append(msg)
    ctx.set_corr_gate(None)
    assert not failures, f"shape {shape}: " + "; ".join(failures[:8])


def test_one_workgroup_selects_over_every_point(smpl, contexts):
    """num_parts = 1 (the 'single' part map): one k_trim workgroup walks all 4 097 queries, one more than the LDS key capacity: the recomputing path on real distances."""
    case = {c[0]: c for c in nn_cases.cases(smpl, "queries")}["queries-all-parts-4097"]
    name, _, _, cloud, vis, data, _ = case
    pm, npart = nn_cases.part_map("single")
    labels = np.zeros(len(data), np.int32)
    corr = nr.nn_ref(nn_cases.part_of_vertex(smpl, pm), npart, cloud, vis, data, labels)
    assert int((corr >= 0).sum()) > tc.LDS_KEYS
    for rho, kappa in ((0.5, 1.0), (0.9, 1.5)):
        out, total, per_part, T = nt.trim_ref(corr, cloud, data, labels, npart, rho, kappa)
        assert 0 < total < int((corr >= 0).sum())
        ctx = contexts(pm, npart, "A")
        ctx.set_corr_trim(rho, kappa)
        msg = _compare(ctx, name, ctx.nn(cloud, vis, data, labels), *_expected(out, data, total, per_part, T))
        assert not msg, msg


# ---- 3. off is off; refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_off_after_on_is_the_plain_search(smpl, contexts, shape):
    case = {c[0]: c for c in nn_cases.cases(smpl, "queries")}["queries-all-parts-513"]
    name, pm, npart, cloud, vis, data, labels = case
    corr, cnt, fsum, centre = edges._reference(smpl, case)
    ctx = contexts(pm, npart, shape)
    ctx.set_corr_gate(None)
    ctx.set_corr_trim(0.5, 1.0)
    r, k, f, mm = ctx.corr_trim()
    assert np.array_equal(r, np.full(npart, 0.5)) and np.array_equal(k, np.ones(npart)) and np.array_equal(f, np.zeros(npart)) and mm == 1
    want = _trimmed_reference(smpl, case)
    assert want[2] > 0
    msg = _compare(ctx, name, ctx.nn(cloud, vis, data, labels), *want)      # it was on
    assert not msg, msg
    ctx.set_corr_trim(None)
    msg = _compare(ctx, name, ctx.nn(cloud, vis, data, labels), corr, 0, 0, np.zeros(npart, np.int32), np.full(npart, np.inf), cnt, fsum, centre)
    assert not msg, f"shape {shape}: {msg}"
    assert np.array_equal(ctx.corr_trim()[1], np.full(npart, np.inf))
    ctx.set_corr_trim(0.5, np.inf)                                           # every part off is off
    msg = _compare(ctx, name, ctx.nn(cloud, vis, data, labels), corr, 0, 0, np.zeros(npart, np.int32), np.full(npart, np.inf), cnt, fsum, centre)
    assert not msg, f"shape {shape}: {msg}"


def test_refused_settings_leave_the_previous_one_in_force(smpl, contexts):
    from avatar_amd import api
    case = {c[0]: c for c in nn_cases.cases(smpl, "queries")}["queries-all-parts-513"]
    name, pm, npart, cloud, vis, data, labels = case
    ctx = contexts(pm, npart, "A")
    ctx.set_corr_gate(None)
    ctx.set_corr_trim(0.5, 1.0, 0.0, 1)
    nan, inf = np.nan, np.inf
    bad = [([0.5] * 5, 1.0, 0.0, 1), ([0.5] * (npart + 1), 1.0, 0.0, 1), (nan, 1.0, 0.0, 1), (0.5, nan, 0.0, 1), (0.5, 1.0, nan, 1),
           (0.0, 1.0, 0.0, 1), (-0.5, 1.0, 0.0, 1), (np.nextafter(1.0, 2.0), 1.0, 0.0, 1), (0.5, -1.0, 0.0, 1), (0.5, 1.0, -1e-300, 1),
           (0.5, 1.0, inf, 1), (0.5, 1e200, 0.0, 1), (0.5, 1.0, 0.0, 0), (0.5, 1.0, 0.0, -3),
           ([0.5] * (npart - 1) + [nan], 1.0, 0.0, 1), (0.5, [1.0] * (npart - 1) + [-1.0], 0.0, 1)]
    for args in bad:
        with pytest.raises(api.AvtError, match="num_parts"):
            ctx.set_corr_trim(*args)
    r, k, f, mm = ctx.corr_trim()
    assert np.array_equal(r, np.full(npart, 0.5)) and np.array_equal(k, np.ones(npart)) and np.array_equal(f, np.zeros(npart)) and mm == 1
    msg = _compare(ctx, name, ctx.nn(cloud, vis, data, labels), *_trimmed_reference(smpl, case))
    assert not msg, msg


def test_trimmed_is_refused_without_a_search(gmodel):
    from avatar_amd import api
    ctx = api.Context(gmodel, 24, synth.identity_part_map(), 64, 1, device=0)
    ctx.set_corr_trim(0.5, 1.0)
    with pytest.raises(api.AvtError):
        ctx.trimmed(0)
    with pytest.raises(api.AvtError):
        ctx.trim_thresholds(0)


# ---- 4. fits ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contaminated(smpl, omodel, gmodel):
    """tests/nn_trim_cases.contaminated, and per setting of the fits what the restatement drops at the start state and the CPU oracle's
    fit of the kept points alone (the same points in the same order; point 0, the frame's centre, is among them).  The thresholds are
    compared bit for bit, so they are the restatement's on the cloud the DEVICE skins from the start state (an optimize call without
    an ICP iteration leaves it; it differs from numpy's skinning in the last bits); which matches are dropped is the same on both clouds."""
    from avatar_amd import api
    c = tc.contaminated(smpl, omodel)
    p0, q0, w0 = c["start"]
    ctx = api.Context(gmodel, 24, c["pm"], FIT_POINTS, 1, device=0)
    ctx.frames_upload([c["D"]], [c["L"]])
    ctx.state_upload(p0[None], q0[None], w0[None])
    ctx.optimize_resident(Options.counted(icp_iters=0, max_iters_per_icp=2))
    cloud_dev = ctx.posed(0)[0]
    assert np.abs(cloud_dev - c["cloud0"]).max() < 1e-12
    c["fits"] = {}
    for rho, kappa, dropped in ((0.75, 3.0, 308), (0.5, 4.0, 335)):
        out, total, per_part, _ = nt.trim_ref(c["ungated_corr"], c["cloud0"], c["D"], c["L"], 24, rho, kappa)
        out_dev, _, _, T = nt.trim_ref(c["ungated_corr"], cloud_dev, c["D"], c["L"], 24, rho, kappa)
        kept = out >= 0
        assert np.array_equal(out, out_dev)
        assert total == dropped and kept[0] and (c["ungated_corr"] >= 0).all() and not kept[c["planted"]].any()
        fit = dict(corr=out, total=total, per_part=per_part, T=T, kept=kept)
        if (rho, kappa) == (0.75, 3.0):
            fit["ref"] = omodel.optimize(c["pm"], 24, c["D"][kept], c["L"][kept], c["opt"], p0, q0, w0, aggregate=1)
            assert np.array_equal(fit["ref"]["corr"], out[kept])
        c["fits"][(rho, kappa)] = fit
    return c


def _fit_ctx(gmodel, pm, shape):
    from avatar_amd import api
    return api.Context(gmodel, 24, pm, FIT_POINTS, 1, device=0).set_tuning(**({} if shape == "D" else SHAPES[shape]))


@pytest.mark.parametrize("form", ["rows", "moments"])
@pytest.mark.parametrize("shape", ["D", "B"])
def test_a_trimmed_fit_is_the_fit_of_the_kept_points(gmodel, contaminated, shape, form):
    """optimize_batch on the contaminated frame at rho = 0.75, kappa = 3 (drops the 300 planted points and 8 inliers at the start state)
    against the CPU oracle on the 5 193 kept points alone: bookkeeping equal as integers, the fit within the bounds of
    tests/test_gpu_nn_gate.test_a_gated_fit_is_the_fit_of_the_kept_points."""
    c = contaminated
    fit = c["fits"][(0.75, 3.0)]
    ref, kept = fit["ref"], fit["kept"]
    p0, q0, w0 = c["start"]
    ctx = _fit_ctx(gmodel, c["pm"], shape)
    ctx.set_data_term(ctx.DATA_TERM_ROWS if form == "rows" else ctx.DATA_TERM_MOMENTS)
    ctx.set_corr_trim(0.75, 3.0)
    p, q, w, st = ctx.optimize_batch([c["D"]], [c["L"]], c["opt"], p0[None], q0[None], w0[None])
    corr = ctx.correspondences(0, len(c["L"]))
    assert np.array_equal(corr[kept], ref["corr"]) and (corr[~kept] == -1).all()
    assert st[0].num_correspondences == 5501 - 308 == ref["stats"].num_correspondences
    assert st[0].matched_model_points == ref["stats"].matched_model_points
    total, per_part = ctx.trimmed(0, per_part=True)
    assert ctx.gated(0) == 0 and total == 308 and np.array_equal(per_part, fit["per_part"])
    assert ctx.trim_thresholds(0).tobytes() == fit["T"].tobytes()
    cnt, fsum, centre = ctx.nn_sums(0)
    rc, rf, rcen = nr.nn_sums_ref(ref["corr"], c["D"][kept], nn_cases.V)      # (the first point is kept: the same centre)
    assert np.array_equal(cnt, rc) and np.array_equal(fsum, rf) and np.array_equal(centre, rcen)
    print(f"final cost {st[0].final_cost!r} / {ref['stats'].final_cost!r}, p {np.abs(p[0] - ref['p']).max():.3e}, w {np.abs(w[0] - ref['w']).max():.3e}")
    assert st[0].gn_iterations == ref["stats"].gn_iterations and st[0].accepted_steps == ref["stats"].accepted_steps
    assert abs(st[0].final_cost - ref["stats"].final_cost) <= 1e-9 * abs(ref["stats"].final_cost)
    assert np.abs(p[0] - ref["p"]).max() < 1e-7
    dq = np.minimum(np.abs(q[0] - ref["q"]).max(1), np.abs(q[0] + ref["q"]).max(1))
    assert dq.max() < 1e-7
    assert np.abs(w[0] - ref["w"]).max() < 1e-6
    assert np.abs(ctx.cloud(0) - ref["cloud"]).max() < 1e-7


def test_a_setting_changed_between_two_fits_takes_effect_on_the_replayed_graph(gmodel, contaminated):
    """One context, the same frame and start: off, (0.75, 3), (0.5, 4), off.  The third call replays the second one's captured launch
    sequence - only on / off is part of the launch shape - and must see the new values."""
    c = contaminated
    p0, q0, w0 = c["start"]
    N = len(c["L"])
    ctx = _fit_ctx(gmodel, c["pm"], "D")

    def run():
        _, _, _, st = ctx.optimize_batch([c["D"]], [c["L"]], c["opt"], p0[None], q0[None], w0[None])
        return st[0].num_correspondences, ctx.correspondences(0, N)

    n, corr = run()
    assert n == 5501 and np.array_equal(corr, c["ungated_corr"]) and ctx.trimmed(0) == 0 and np.isinf(ctx.trim_thresholds(0)).all()
    for key in ((0.75, 3.0), (0.5, 4.0)):
        fit = c["fits"][key]
        ctx.set_corr_trim(*key)
        n, corr = run()
        assert np.array_equal(corr, fit["corr"]), key
        assert n == 5501 - fit["total"] and ctx.trimmed(0) == fit["total"] and ctx.trim_thresholds(0).tobytes() == fit["T"].tobytes(), key
    ctx.set_corr_trim(None)
    n, corr = run()
    assert n == 5501 and np.array_equal(corr, c["ungated_corr"]) and ctx.trimmed(0) == 0


@pytest.mark.parametrize("shape", ["D", "B"])
def test_trimming_acts_in_every_icp_iteration(smpl, gmodel, contaminated, shape):
    """rho = 0.75, kappa = 3 from the same start: the correspondences a call of three ICP iterations leaves are those of its third
    search, i.e. the restatement on the cloud a call of two iterations ends with (a call with icp_iters = b is reproduced bit for bit:
    the budget contract of include/avt.h) and the third iteration's visibility flags."""
    c = contaminated
    p0, q0, w0 = c["start"]
    pov = nn_cases.part_of_vertex(smpl, c["pm"])
    ctx = _fit_ctx(gmodel, c["pm"], shape)
    ctx.set_corr_trim(0.75, 3.0)
    ctx.optimize_batch([c["D"]], [c["L"]], Options.counted(icp_iters=2, max_iters_per_icp=2), p0[None], q0[None], w0[None])
    cloud_x = ctx.posed(0)[0]
    _, _, _, st = ctx.optimize_batch([c["D"]], [c["L"]], Options.counted(icp_iters=3, max_iters_per_icp=2), p0[None], q0[None], w0[None])
    vis_y = ctx.get_visibility(0)
    plain = nr.nn_ref(pov, 24, cloud_x, vis_y, c["D"], c["L"])
    out, total, per_part, T = nt.trim_ref(plain, cloud_x, c["D"], c["L"], 24, 0.75, 3.0)
    assert total > 0 and not np.array_equal(T, c["fits"][(0.75, 3.0)]["T"])      # (not the thresholds of the first search)
    assert np.array_equal(ctx.correspondences(0, len(c["L"])), out)
    gt, gpp = ctx.trimmed(0, per_part=True)
    assert gt == total and np.array_equal(gpp, per_part) and ctx.trim_thresholds(0).tobytes() == T.tobytes()
    assert st[0].num_correspondences == int((out >= 0).sum()) and int((plain >= 0).sum()) == st[0].num_correspondences + ctx.gated(0) + total


def _bits(st):
    return np.array([st.initial_cost, st.final_cost, st.lambda_, st.num_correspondences, st.matched_model_points, st.gn_iterations,
                     st.accepted_steps], np.float64).tobytes()


@pytest.mark.parametrize("shape", ["D", "B"])
def test_everything_trimmed_is_a_frame_without_a_valid_label(gmodel, contaminated, shape):
    """rho = 1, kappa = 0, floor = 0 on 600 clean points (all at nonzero distances: T = 0 drops every match), and the call ends exactly
    where an untrimmed call on the same points with every label -1 ends - both reach the solver with empty bookkeeping."""
    c = contaminated
    p0, q0, w0 = c["start"]
    data, labels = c["clean"][0][:600], c["clean"][1][:600]
    opt = Options.counted(icp_iters=2, max_iters_per_icp=2)
    ctx = _fit_ctx(gmodel, c["pm"], shape)
    ctx.set_corr_trim(1.0, 0.0, 0.0)
    p, q, w, st = ctx.optimize_batch([data], [labels], opt, p0[None], q0[None], w0[None])
    assert st[0].num_correspondences == 0 and st[0].matched_model_points == 0 and ctx.trimmed(0) == 600 and ctx.gated(0) == 0
    assert (ctx.correspondences(0, 600) == -1).all()
    cnt, fsum, _ = ctx.nn_sums(0)
    assert not cnt.any() and not fsum.any()                                   # every term taken back exactly
    ctx.set_corr_trim(None)
    p2, q2, w2, st2 = ctx.optimize_batch([data], [np.full(600, -1, np.int32)], opt, p0[None], q0[None], w0[None])
    assert ctx.trimmed(0) == 0
    assert p.tobytes() == p2.tobytes() and q.tobytes() == q2.tobytes() and w.tobytes() == w2.tobytes()
    assert _bits(st[0]) == _bits(st2[0])
