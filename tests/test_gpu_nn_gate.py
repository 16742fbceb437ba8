"""The correspondence gate (include/avt.h avt_set_corr_gate) on the device: every case of tests/nn_cases.py under
per-part gates that drop and keep (median_gates), through the four device code paths of tests/test_gpu_nn_edges.py (A k_nn<4>, B slab
k_nn_part, C full-scan k_nn_part, D k_nn_vis<4>), every comparison an integer equality against the numpy restatement
(tests/nn_gate_restatement.py on top of tests/nn_restatement.py); the boundary d2 == g2; off after on; refusals; and inside optimize():
a gated fit of a contaminated frame is the fit of the kept points (CPU oracle on those points alone), the gate acts in every ICP
iteration, and a fit whose every match is gated is the fit of a frame without a valid label."""
import numpy as np
import pytest

import nn_cases
import nn_gate_restatement as ng
import nn_restatement as nr
import test_gpu_nn_edges as edges
from avatar_amd import synth
from avatar_amd.capi import Options

pytestmark = pytest.mark.gpu

SHAPES = edges.SHAPES
MAX_POINTS = edges.MAX_POINTS     # 4608, one frame: the stand-alone searches
FIT_POINTS = 5632                 # the contaminated frame has 5 501 points
_GREF = {}


@pytest.fixture(scope="module")
def contexts(gmodel):
    """One Context per (part map, shape), made on first use and kept for the module; every user sets the gate it wants first."""
    from avatar_amd import api
    made = {}

    def get(pm, npart, shape):
        key = nn_cases.map_key(pm, npart) + (shape,)
        if key not in made:
            made[key] = api.Context(gmodel, npart, pm, MAX_POINTS, 1, device=0).set_tuning(**SHAPES[shape])
        return made[key]
    return get


def _gated_reference(model, case):
    """(gates, gated indices, gated count, counts, sums, centre) of a case under median_gates: computed once from the ungated reference
    tests/test_gpu_nn_edges.py keeps, shared by the shapes, never written to."""
    name, pm, npart, cloud, vis, data, labels = case
    if name not in _GREF:
        corr = edges._reference(model, case)[0]
        g = ng.median_gates(corr, cloud, data, labels, npart)
        cg, n = ng.gate_ref(corr, cloud, data, labels, g)
        res = (g, cg) + nr.nn_sums_ref(cg, data, nn_cases.V)
        for a in res:
            a.setflags(write=False)
        _GREF[name] = res[:2] + (n,) + res[2:]
    return _GREF[name]


def _compare(ctx, name, got, corr, n, cnt, fsum, centre):
    """'' when the device's indices, bookkeeping and gated count are the expected ones, else what differs."""
    gc, gf, gcen = ctx.nn_sums(0)
    gn = ctx.gated(0)
    bad = []
    if not np.array_equal(got, corr):
        bad.append(f"{int((got != corr).sum())} of {len(corr)} indices")
    if not np.array_equal(gc, cnt):
        bad.append(f"{int((gc != cnt).sum())} counts")
    if not np.array_equal(gf, fsum):
        bad.append(f"{int((gf != fsum).any(0).sum())} sums")
    if not np.array_equal(gcen, centre):
        bad.append("centre")
    if gn != n:
        bad.append(f"gated {gn} for {n}")
    return f"{name}: " + ", ".join(bad) if bad else ""


def _run(ctx, case, g, corr, n, cnt, fsum, centre):
    name, pm, npart, cloud, vis, data, labels = case
    ctx.set_corr_gate(g)
    return _compare(ctx, name, ctx.nn(cloud, vis, data, labels), corr, n, cnt, fsum, centre)


# ---- 1. every case through every shape ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("group", list(nn_cases.GROUPS))
def test_every_case_through_every_shape_gated(smpl, contexts, group, shape):
    """Per-part gates at the median matched distance of the part: tests/test_nn_gate_cpu.py shows that every group has cases that both
    drop and keep and that 2 778 matches sit exactly on their gate; the sweep's 511, 512 and 513 visible candidates lie on both sides of
    NN_ACC_CAP (nn_record<1> above, the LDS accumulators below)."""
    failures = []
    for case in nn_cases.cases(smpl, group):
        msg = _run(contexts(case[1], case[2], shape), case, *_gated_reference(smpl, case))
        if msg:
            failures.append(msg)
    assert not failures, f"shape {shape}: " + "; ".join(failures)


# ---- 2. boundary cases written out by hand ---------------------------------------------------------------------------------------
def _hand_model(smpl):
    """identity map; the first vertex of part 0 at the origin, the first of part 1 at (10, 0, 0), nothing else visible."""
    pm, npart = nn_cases.part_map("identity")
    pov = nn_cases.part_of_vertex(smpl, pm)
    v0, v1 = int(np.nonzero(pov == 0)[0][0]), int(np.nonzero(pov == 1)[0][0])
    cloud = np.full((nn_cases.V, 3), 100.0)
    cloud[v0] = 0.0
    cloud[v1] = (10.0, 0.0, 0.0)
    vis = np.zeros(nn_cases.V, np.uint8)
    vis[[v0, v1]] = 1
    return pm, npart, pov, cloud, vis, v0, v1


def _hand_cases(v0, v1):
    """(name, queries, labels, gates, expected indices, expected gated count), the expectations written by hand."""
    inf = np.inf
    per0 = [0.2] + [inf] * 23
    per1 = [inf, 0.2] + [inf] * 22
    two = ([(0.3, 0, 0), (0.1, 0, 0), (10.3, 0, 0), (10.1, 0, 0)], [0, 0, 1, 1])
    return [
        ("exact hit", [(0.5, 0, 0)], [0], 0.5, [v0], 0),
        ("one ulp below", [(0.5, 0, 0)], [0], np.nextafter(0.5, 0), [-1], 1),
        ("gate 0", [(0, 0, 0), (1e-9, 0, 0), (0, 0, 0)], [0, 0, 0], 0.0, [v0, -1, v0], 1),
        ("gate +inf", [(np.sqrt(1.79e308), 0, 0)], [0], inf, [v0], 0),
        ("part 0 gated", two[0], two[1], per0, [-1, v0, v1, v1], 1),
        ("part 1 gated", two[0], two[1], per1, [v0, v0, -1, v1], 1),
    ]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_boundaries_written_by_hand(smpl, contexts, shape):
    """d2 == g2 keeps, one ulp below drops, g = 0 keeps distance 0 alone, +inf keeps d2 = 1.79e308; a per-part gate on one part does
    not move the other part's matches."""
    pm, npart, pov, cloud, vis, v0, v1 = _hand_model(smpl)
    ctx = contexts(pm, npart, shape)
    failures = []
    for name, queries, labels, g, want, n in _hand_cases(v0, v1):
        data = np.array(queries, np.float64)
        labels = np.array(labels, np.int32)
        corr = nr.nn_ref(pov, npart, cloud, vis, data, labels)
        cg, cn = ng.gate_ref(corr, cloud, data, labels, g)
        assert cg.tolist() == want and cn == n, name              # the restatement agrees with the hand-written expectation
        msg = _run(ctx, (name, pm, npart, cloud, vis, data, labels), g, cg, n, *nr.nn_sums_ref(cg, data, nn_cases.V))
        if msg:
            failures.append(msg)
    assert not failures, f"shape {shape}: " + "; ".join(failures)


# ---- 3. off is off ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_off_after_on_is_the_ungated_search(smpl, contexts, shape):
    case = {c[0]: c for c in nn_cases.cases(smpl, "queries")}["queries-all-parts-513"]
    name, pm, npart, cloud, vis, data, labels = case
    corr, cnt, fsum, centre = edges._reference(smpl, case)
    ctx = contexts(pm, npart, shape)
    ctx.set_corr_gate(0.01)
    assert np.array_equal(ctx.corr_gate(), np.full(npart, 0.01))
    cg, n = ng.gate_ref(corr, cloud, data, labels, 0.01)
    assert n > 0
    assert np.array_equal(ctx.nn(cloud, vis, data, labels), cg) and ctx.gated(0) == n      # it was on
    msg = _run(ctx, case, None, corr, 0, cnt, fsum, centre)
    assert not msg, f"shape {shape}: {msg}"
    assert np.array_equal(ctx.corr_gate(), np.full(npart, np.inf))


# ---- the contaminated frame of the fits --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contaminated(smpl, omodel):
    """Every 6th pixel of synth.make_frame(smpl, 3) (5 201 points) and 300 planted points 0.6 m off a data point each, carrying that
    point's label; permuted with index 0 left first.  At the frame's start state a gate of 0.2 m drops exactly the planted points (the
    largest inlier distance is 0.189 m, the smallest planted one 0.269 m): asserted here from the restatement on the CPU."""
    from avatar_amd import api
    fr = synth.make_frame(smpl, 3)
    sel = np.arange(0, len(fr["labels"]), 6)
    data, labels = fr["data"][sel], fr["labels"][sel]
    N = len(labels)
    rng = np.random.default_rng(5)
    idx = rng.integers(1, N, 300)
    nrm = rng.normal(size=(300, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    D = np.concatenate([data, data[idx] + 0.6 * nrm])
    L = np.concatenate([labels, labels[idx]]).astype(np.int32)
    planted = np.concatenate([np.zeros(N, bool), np.ones(300, bool)])
    perm = np.concatenate([[0], 1 + rng.permutation(len(L) - 1)])
    D, L, planted = np.ascontiguousarray(D[perm]), np.ascontiguousarray(L[perm]), planted[perm]
    w0, p0, R0 = fr["start"]
    q0 = api.rot_to_quat(R0)
    pm = synth.identity_part_map()
    opt = Options.counted(icp_iters=1, max_iters_per_icp=2)
    cloud0 = synth.pose_vertices(smpl, w0, p0, R0)
    ungated = omodel.optimize(pm, 24, D, L, opt, p0, q0, w0, aggregate=1)["corr"]        # the search at the start state
    cg, n = ng.gate_ref(ungated, cloud0, D, L, 0.2)
    assert N == 5201 and n == 300 and (cg[planted] == -1).all() and int((cg[~planted] >= 0).sum()) == 5201
    kept_ref = omodel.optimize(pm, 24, D[~planted], L[~planted], opt, p0, q0, w0, aggregate=1)
    assert np.array_equal(kept_ref["corr"], cg[~planted])
    for a in (D, L, planted, cg, ungated):
        a.setflags(write=False)
    return dict(D=D, L=L, planted=planted, start=(p0, q0, w0), pm=pm, opt=opt, gated_corr=cg, ungated_corr=ungated, kept_ref=kept_ref,
                clean=(data, labels))


def _fit_ctx(gmodel, pm, shape):
    from avatar_amd import api
    return api.Context(gmodel, 24, pm, FIT_POINTS, 1, device=0).set_tuning(**({} if shape == "D" else SHAPES[shape]))


def test_a_gate_set_between_two_fits_takes_effect_on_the_second(gmodel, contaminated):
    """One context, the same frame and start twice: the second call replays the first one's captured launch sequence and must see the gate."""
    c = contaminated
    p0, q0, w0 = c["start"]
    ctx = _fit_ctx(gmodel, c["pm"], "D")
    _, _, _, st = ctx.optimize_batch([c["D"]], [c["L"]], c["opt"], p0[None], q0[None], w0[None])
    assert np.array_equal(ctx.correspondences(0, len(c["L"])), c["ungated_corr"])
    assert st[0].num_correspondences == 5501 and ctx.gated(0) == 0
    ctx.set_corr_gate(0.2)
    _, _, _, st = ctx.optimize_batch([c["D"]], [c["L"]], c["opt"], p0[None], q0[None], w0[None])
    assert np.array_equal(ctx.correspondences(0, len(c["L"])), c["gated_corr"])
    assert st[0].num_correspondences == 5201 and ctx.gated(0) == 300
    ctx.set_corr_gate(None)
    _, _, _, st = ctx.optimize_batch([c["D"]], [c["L"]], c["opt"], p0[None], q0[None], w0[None])
    assert np.array_equal(ctx.correspondences(0, len(c["L"])), c["ungated_corr"])
    assert st[0].num_correspondences == 5501 and ctx.gated(0) == 0


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refused_gates_leave_the_previous_one_in_force(smpl, contexts):
    from avatar_amd import api
    case = {c[0]: c for c in nn_cases.cases(smpl, "queries")}["queries-all-parts-513"]
    name, pm, npart, cloud, vis, data, labels = case
    ctx = contexts(pm, npart, "A")
    ctx.set_corr_gate(0.05)
    for bad in ([0.1] * 5, [0.1] * (npart + 1), [np.nan], [-1.0], [0.1] * (npart - 1) + [np.nan], [0.1] * (npart - 1) + [-1e-300]):
        with pytest.raises(api.AvtError, match="num_parts"):
            ctx.set_corr_gate(bad)
    assert np.array_equal(ctx.corr_gate(), np.full(npart, 0.05))
    cg, n = ng.gate_ref(edges._reference(smpl, case)[0], cloud, data, labels, 0.05)
    assert 0 < n < int((cg >= 0).sum()) + n
    msg = _compare(ctx, name, ctx.nn(cloud, vis, data, labels), cg, n, *nr.nn_sums_ref(cg, data, nn_cases.V))
    assert not msg, msg


def test_gated_is_refused_without_a_search(gmodel):
    from avatar_amd import api
    ctx = api.Context(gmodel, 24, synth.identity_part_map(), 64, 1, device=0)
    with pytest.raises(api.AvtError):
        ctx.gated(0)


# ---- 5. a gated fit is the fit of the kept points --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["rows", "moments"])
@pytest.mark.parametrize("shape", ["D", "B"])
def test_a_gated_fit_is_the_fit_of_the_kept_points(gmodel, contaminated, shape, form):
    """optimize_batch on the contaminated frame at g = 0.2 against the CPU oracle on the 5 201 kept points alone (the same points in the
    same order): bookkeeping equal as integers, the fit within the bounds of tests/test_gpu_parity.test_optimize_matches_oracle."""
    c = contaminated
    ref, kept = c["kept_ref"], ~c["planted"]
    p0, q0, w0 = c["start"]
    ctx = _fit_ctx(gmodel, c["pm"], shape)
    ctx.set_data_term(ctx.DATA_TERM_ROWS if form == "rows" else ctx.DATA_TERM_MOMENTS)
    ctx.set_corr_gate(0.2)
    p, q, w, st = ctx.optimize_batch([c["D"]], [c["L"]], c["opt"], p0[None], q0[None], w0[None])
    corr = ctx.correspondences(0, len(c["L"]))
    assert np.array_equal(corr[kept], ref["corr"]) and (corr[~kept] == -1).all()
    assert st[0].num_correspondences == 5201 == ref["stats"].num_correspondences
    assert st[0].matched_model_points == ref["stats"].matched_model_points
    assert ctx.gated(0) == 300
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


# ---- 6. the gate acts in every ICP iteration -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["D", "B"])
def test_the_gate_acts_in_every_icp_iteration(smpl, gmodel, contaminated, shape):
    """g = 0.1 from the same start: the correspondences a call of three ICP iterations leaves are those of its third search, i.e. the
    gated restatement on the cloud a call of two iterations ends with (a call with icp_iters = b is reproduced bit for bit: the
    budget contract of include/avt.h) and the third iteration's visibility flags."""
    c = contaminated
    p0, q0, w0 = c["start"]
    pov = nn_cases.part_of_vertex(smpl, c["pm"])
    ctx = _fit_ctx(gmodel, c["pm"], shape)
    ctx.set_corr_gate(0.1)
    ctx.optimize_batch([c["D"]], [c["L"]], Options.counted(icp_iters=2, max_iters_per_icp=2), p0[None], q0[None], w0[None])
    cloud_x = ctx.posed(0)[0]
    _, _, _, st = ctx.optimize_batch([c["D"]], [c["L"]], Options.counted(icp_iters=3, max_iters_per_icp=2), p0[None], q0[None], w0[None])
    vis_y = ctx.get_visibility(0)
    ungated = nr.nn_ref(pov, 24, cloud_x, vis_y, c["D"], c["L"])
    cg, n = ng.gate_ref(ungated, cloud_x, c["D"], c["L"], 0.1)
    assert n >= 300                                                    # (the planted points at least)
    assert np.array_equal(ctx.correspondences(0, len(c["L"])), cg)
    assert ctx.gated(0) == n and st[0].num_correspondences == int((cg >= 0).sum())
    assert int((ungated >= 0).sum()) == st[0].num_correspondences + n


# ---- 7. everything gated ---------------------------------------------------------------------------------------------------------
def _bits(st):
    return np.array([st.initial_cost, st.final_cost, st.lambda_, st.num_correspondences, st.matched_model_points, st.gn_iterations,
                     st.accepted_steps], np.float64).tobytes()


@pytest.mark.parametrize("shape", ["D", "B"])
def test_everything_gated_is_a_frame_without_a_valid_label(gmodel, contaminated, shape):
    """g = 1e-9 on 600 clean points: no correspondence survives, and the call ends exactly where an ungated call on the same points with
    every label -1 ends - both reach the solver with empty bookkeeping."""
    c = contaminated
    p0, q0, w0 = c["start"]
    data, labels = c["clean"][0][:600], c["clean"][1][:600]
    opt = Options.counted(icp_iters=2, max_iters_per_icp=2)
    ctx = _fit_ctx(gmodel, c["pm"], shape)
    ctx.set_corr_gate(1e-9)
    p, q, w, st = ctx.optimize_batch([data], [labels], opt, p0[None], q0[None], w0[None])
    assert st[0].num_correspondences == 0 and st[0].matched_model_points == 0 and ctx.gated(0) == 600
    assert (ctx.correspondences(0, 600) == -1).all()
    ctx.set_corr_gate(None)
    p2, q2, w2, st2 = ctx.optimize_batch([data], [np.full(600, -1, np.int32)], opt, p0[None], q0[None], w0[None])
    assert ctx.gated(0) == 0
    assert p.tobytes() == p2.tobytes() and q.tobytes() == q2.tobytes() and w.tobytes() == w2.tobytes()
    assert _bits(st[0]) == _bits(st2[0])
