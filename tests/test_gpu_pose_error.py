"""The pose error on the GPU (avatar_amd/csrc/avt_poseerr.hip, include/avt_poseerr.h) against its numpy restatement
(tests/pose_error_restatement.py) on the cases of tests/pose_error_cases.py: V across the workgroup's 256 lanes and the waves' 64,
J from none to SMPL's 24, the part tables, batch independence, both sources of a side, SMPL's size once, identity, the flags and
the degenerate alignments.

Tolerances.  Sums of n non-negative terms (V_SUM, V_SQ, PART_SUM, J_SUM, JR_SUM): both sides sum the same terms in different
orders with a few roundings per term: (n + 16) 2^-52 of the sum.  Maxima and per-joint raw errors: 4 ulp.  Argmax: the cases lead
their runner-up by 1e-6 relative (asserted on the restatement first), then the integer must match.  Alignment figures: per case
max(16 |svd form - quaternion form|, (n + 16) 2^-52 S), S = sum |y_k - mean y|, computed here from the restatement's two
formulations.  A status word other than 0 fails, except on the deliberate non-finite pairs."""
import numpy as np
import pytest

import pose_error_cases as pc
import pose_error_restatement as pr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
COL = {k: i for i, k in enumerate(pr.COLUMNS)}
SEEN = dict(diff=0.0, tol=0.0, ratio=0.0)         # alignment figures: the largest device difference, tolerance and ratio over the tests run so far


@pytest.fixture(scope="module")
def pe_mod():
    from avatar_amd import poseerror
    return poseerror


def _sum_ok(got, want, n):
    return abs(got - want) <= (n + 16) * EPS * want


def _ulp_ok(got, want):
    return abs(got - want) <= 4 * EPS * abs(want)


def _align_ok(got, want, tol, what, fails):
    d = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) if np.size(got) else 0.0
    SEEN["diff"], SEEN["tol"] = max(SEEN["diff"], d), max(SEEN["tol"], tol)
    if tol > 0:
        SEEN["ratio"] = max(SEEN["ratio"], d / tol)
    if not d <= tol:
        fails.append(f"{what}: off by {d:.3e}, tol {tol:.3e}")


def _check_pair(tag, dev, i, E, T, A, B, vp, P, sum_unique=True):
    """pair i of the device result `dev` against the restatement of (E, T, A, B); returns the list of failures"""
    fails = []
    V, J = len(E), 0 if A is None else len(A)
    ref = pr.pair(E, T, A, B, vp, P)
    s, r = dev["summary"][i], ref["summary"]
    if dev["status"][i] != 0:
        fails.append(f"status {dev['status'][i]}")
    for k in ("V_SUM", "V_SQ"):
        if not _sum_ok(s[COL[k]], r[COL[k]], V):
            fails.append(f"{k}: {s[COL[k]]!r} for {r[COL[k]]!r}")
    if not _ulp_ok(s[COL["V_MAX"]], r[COL["V_MAX"]]):
        fails.append(f"V_MAX: {s[COL['V_MAX']]!r} for {r[COL['V_MAX']]!r}")
    d = pr.errors(E, T)
    assert d.max() == 0 or pc.margin(d) >= pc.ARGMAX_MARGIN, f"{tag}: the case's largest vertex error does not lead"
    if dev["argmax"][i][0] != ref["argmax"][0]:
        fails.append(f"V_ARGMAX: {dev['argmax'][i][0]} for {ref['argmax'][0]}")
    sizes = np.bincount(np.zeros(V, np.int64) if vp is None else vp, minlength=P)
    for q in range(P):
        if not _sum_ok(dev["per_part"][i][0][q], ref["per_part"][0][q], sizes[q]) or not _ulp_ok(dev["per_part"][i][1][q], ref["per_part"][1][q]):
            fails.append(f"part {q} ({sizes[q]} vertices): {dev['per_part'][i][:, q]!r} for {ref['per_part'][:, q]!r}")
    tol = pr.alignment_tolerance(E, T)
    if sum_unique:
        _align_ok(s[COL["VPA_SUM"]], r[COL["VPA_SUM"]], tol["sum"], "VPA_SUM", fails)
    _align_ok(s[COL["VPA_SQ"]], r[COL["VPA_SQ"]], tol["sq"], "VPA_SQ", fails)
    _align_ok(s[COL["VPA_SCALE"]], r[COL["VPA_SCALE"]], tol["scale"], "VPA_SCALE", fails)
    if J == 0:
        if not np.isnan(s[6:]).all() or dev["argmax"][i][1] != -1:
            fails.append(f"J == 0: joint columns {s[6:]!r}, argmax {dev['argmax'][i][1]}")
    else:
        for k in ("J_SUM", "JR_SUM"):
            if not _sum_ok(s[COL[k]], r[COL[k]], J):
                fails.append(f"{k}: {s[COL[k]]!r} for {r[COL[k]]!r}")
        e = pr.errors(A, B)
        assert e.max() == 0 or pc.margin(e) >= pc.ARGMAX_MARGIN, f"{tag}: the case's largest joint error does not lead"
        if not _ulp_ok(s[COL["J_MAX"]], r[COL["J_MAX"]]) or dev["argmax"][i][1] != ref["argmax"][1]:
            fails.append(f"J_MAX / J_ARGMAX: {s[COL['J_MAX']]!r} at {dev['argmax'][i][1]} for {r[COL['J_MAX']]!r} at {ref['argmax'][1]}")
        if not (np.abs(dev["per_joint"][i][0] - ref["per_joint"][0]) <= 4 * EPS * ref["per_joint"][0]).all():
            fails.append("per-joint raw errors beyond 4 ulp")
        tj = pr.alignment_tolerance(A, B)
        if sum_unique:
            _align_ok(s[COL["JPA_SUM"]], r[COL["JPA_SUM"]], tj["sum"], "JPA_SUM", fails)
            _align_ok(dev["per_joint"][i][1], ref["per_joint"][1], tj["err"], "per-joint aligned errors", fails)
        _align_ok(s[COL["JPA_SQ"]], r[COL["JPA_SQ"]], tj["sq"], "JPA_SQ", fails)
        _align_ok(s[COL["JPA_SCALE"]], r[COL["JPA_SCALE"]], tj["scale"], "JPA_SCALE", fails)
    return [f"{tag}: {f}" for f in fails]


def _report(name):
    print(f"POSEERR {name}: alignment figures, largest device difference {SEEN['diff']:.3e}, largest tol {SEEN['tol']:.3e}, largest difference / tol {SEEN['ratio']:.3f}")


def _same_bits(a, b, i, j):
    return all(np.array_equal(a[k][i].view(np.uint8), b[k][j].view(np.uint8)) for k in ("summary", "per_joint", "per_part", "argmax")) and \
        a["status"][i] == b["status"][j]


@pytest.mark.parametrize("V", pc.V_SIZES)
def test_sizes_across_the_workgroup_and_wave_boundaries(pe_mod, V):
    fails = []
    for J in pc.J_SIZES:
        b = pc.batch(V, J)
        dev = pe_mod.PoseError(V, J, 1, None, max_pairs=len(pc.FAMILIES)).score(b["E"], b["A"], b["T"], b["B"])
        assert dev["summary"].shape == (4, 12) and dev["per_joint"].shape == (4, 2, J)
        for i, nm in enumerate(pc.FAMILIES):
            fails += _check_pair(f"V {V} J {J} {nm}", dev, i, b["E"][i], b["T"][i], None if J == 0 else b["A"][i], None if J == 0 else b["B"][i], None, 1)
    _report(f"sizes V {V}")
    assert not fails, "; ".join(fails[:10])


@pytest.mark.parametrize("table", ("one", "sparse24", "single", "all_but_one", "p254"))
def test_part_tables(pe_mod, table):
    fails = []
    for V in (65, 513):
        P, vp = pc.part_tables(V)[table]
        b = pc.batch(V, 3, seed=1)
        pe = pe_mod.PoseError(V, 3, P, vp, max_pairs=4)
        want = np.bincount(np.zeros(V, np.int64) if vp is None else vp, minlength=P)
        assert np.array_equal(pe.part_sizes, want)
        dev = pe.score(b["E"], b["A"], b["T"], b["B"])
        for i, nm in enumerate(pc.FAMILIES):
            fails += _check_pair(f"{table} V {V} {nm}", dev, i, b["E"][i], b["T"][i], b["A"][i], b["B"][i], vp, P)
            empty = want == 0
            if dev["per_part"][i][:, empty].any():
                fails.append(f"{table} V {V} {nm}: an empty part is not 0 and 0")
        m = pe.metrics(dev)
        assert np.array_equal(np.isnan(m["pve_part"]), np.tile(want == 0, (4, 1))) and np.array_equal(m["pve"], dev["summary"][:, 0] / V)
    assert not fails, "; ".join(fails[:10])


def test_batch_independence_and_repeatability(pe_mod):
    V, J = 257, 24
    P, vp = pc.part_tables(V)["sparse24"]
    b = pc.batch(V, J, seed=2)
    other = pc.batch(V, J, seed=3)
    pe = pe_mod.PoseError(V, J, P, vp, max_pairs=8)
    for k in range(4):
        one = lambda a: a[k:k + 1]
        alone = pe.score(one(b["E"]), one(b["A"]), one(b["T"]), one(b["B"]))
        again = pe.score(one(b["E"]), one(b["A"]), one(b["T"]), one(b["B"]))
        assert _same_bits(alone, again, 0, 0), f"pair {k}: two runs differ"
        first = lambda a, o: np.concatenate([a[k:k + 1], o[:1]])
        two = pe.score(first(b["E"], other["E"]), first(b["A"], other["A"]), first(b["T"], other["T"]), first(b["B"], other["B"]))
        assert len(two["status"]) == 2 and _same_bits(alone, two, 0, 0), f"pair {k}: differs as pair 0 of 2"
        last = lambda a, o: np.concatenate([np.tile(o[1:2], (7, 1, 1)), a[k:k + 1]])
        full = pe.score(last(b["E"], other["E"]), last(b["A"], other["A"]), last(b["T"], other["T"]), last(b["B"], other["B"]))
        assert len(full["status"]) == 8 and _same_bits(alone, full, 0, 7), f"pair {k}: differs as the last of max_pairs"
        assert not _check_pair(f"pair {k}", full, 7, b["E"][k], b["T"][k], b["A"][k], b["B"][k], vp, P)


def test_sources_host_and_context(pe_mod):
    import fit_models as fm
    from avatar_amd import api
    from avatar_amd.capi import Options
    J, K = 9, 4
    gm = api.AvatarModel(fm.fit_model(J, K, "star"))
    V, nf = gm.numPoints(), 5
    pm = np.arange(J, dtype=np.int32)
    rng = np.random.default_rng(11)
    wg, pg = 0.5 * rng.standard_normal((nf, K)), 0.05 * rng.standard_normal((nf, 3))
    qg = np.stack([fm._quats(rng, J, 0.15) for _ in range(nf)])
    truth = api.Context(gm, J, pm, V, nf, device=0)
    tc, tj, _ = truth.lbs_update(wg, pg, np.stack([api.quat_to_rot(q) for q in qg]))
    opt = Options.demo(enable_occlusion=0, beta_pose=0.0, beta_shape=0.12, icp_iters=1, max_iters_per_icp=2)
    q0 = np.stack([fm._quats(rng, J, 0.02) for _ in range(nf)])

    def fitted():
        c = api.Context(gm, J, pm, V, nf, device=0)
        c.frames_upload([np.ascontiguousarray(x) for x in tc], [gm.mainJoint.astype(np.int32)] * nf)
        c.state_upload(np.zeros((nf, 3)), q0, np.zeros((nf, K)))
        c.optimize_resident(opt)
        return c

    est, control = fitted(), fitted()
    posed = [est.posed(f) for f in range(nf)]
    state = est.state_download()
    assert max(np.abs(posed[f][0] - tc[f]).max() for f in range(nf)) > 1e-6          # the short fit has not reached the truth: there is something to score
    frames_e, frames_t = [3, 0, 3, 4, 1], [4, 2, 2, 0, 1]                             # not consecutive, repeated
    pe = pe_mod.PoseError.for_model(gm, J, pm, max_pairs=8)
    assert np.array_equal(pe.part_sizes, np.bincount(gm.mainJoint, minlength=J)) and (pe.V, pe.J) == (V, J)
    pe.from_context(pe_mod.ESTIMATE, est, frames_e)
    pe.from_context(pe_mod.TRUTH, truth, frames_t)
    pe.run()
    dev = pe.get()
    up = pe.score(np.stack([posed[f][0] for f in frames_e]), np.stack([posed[f][1] for f in frames_e]), tc[frames_t], tj[frames_t])
    assert all(_same_bits(dev, up, i, i) for i in range(5)), "from_context and upload give different bits"
    fails = []
    for i in range(5):
        fails += _check_pair(f"pair {i}", dev, i, posed[frames_e[i]][0], tc[frames_t[i]], posed[frames_e[i]][1], tj[frames_t[i]], gm.mainJoint, J)
    assert not fails, "; ".join(fails[:10])
    pe.from_context(pe_mod.ESTIMATE, est, None, n=5)                                  # frames 0 .. n - 1
    pe.from_context(pe_mod.TRUTH, truth, None, n=5)
    pe.run()
    seq = pe.get()
    assert not [f for i in range(5) for f in _check_pair(f"frame {i}", seq, i, posed[i][0], tc[i], posed[i][1], tj[i], gm.mainJoint, J)]
    # the contexts were only read
    for f in range(nf):
        assert all(np.array_equal(a, b) for a, b in zip(est.posed(f), posed[f]))
        assert np.array_equal(truth.posed(f)[0], tc[f]) and np.array_equal(truth.posed(f)[1], tj[f])
    after = est.state_download()
    assert all(np.array_equal(a, b) for a, b in zip(after[:3], state[:3]))
    est.optimize_resident(opt)
    control.optimize_resident(opt)
    assert all(np.array_equal(a, b) for a, b in zip(est.state_download()[:3], control.state_download()[:3])), "the scorer changed what a further optimize gives"
    assert all(np.array_equal(est.posed(f)[0], control.posed(f)[0]) for f in range(nf))
    other = api.Context(api.AvatarModel(fm.fit_model(5, 4, "star")), 5, np.arange(5, dtype=np.int32), 60, 1, device=0)
    with pytest.raises(Exception, match="V, J or device"):
        pe.from_context(pe_mod.ESTIMATE, other, [0])
    with pytest.raises(Exception, match="out of range"):
        pe.from_context(pe_mod.ESTIMATE, est, [0, nf])


def test_smpl_size_once(pe_mod):
    from avatar_amd import api, synth
    smpl = synth.load_model(0)
    gm = api.AvatarModel(smpl)
    pm = synth.identity_part_map()
    gts = [synth.sample_ground_truth(smpl, s) for s in range(3)]
    starts = [synth.perturb_start(*gt, s) for s, gt in enumerate(gts)]
    ctx = api.Context(gm, 24, pm, 1000, 3, device=0)
    tc, tj, _ = ctx.lbs_update(np.stack([g[0] for g in gts]), np.stack([g[1] for g in gts]), np.stack([g[2] for g in gts]))
    ec, ej, _ = ctx.lbs_update(np.stack([g[0] for g in starts]), np.stack([g[1] for g in starts]), np.stack([g[2] for g in starts]))
    pe = pe_mod.PoseError.for_model(gm, 24, pm, max_pairs=3)
    assert (pe.V, pe.J, pe.numParts) == (6890, 24, 24)
    dev = pe.score(ec, ej, tc, tj)
    vp = np.asarray(pm)[gm.mainJoint]
    fails = [f for i in range(3) for f in _check_pair(f"pair {i}", dev, i, ec[i], tc[i], ej[i], tj[i], vp, 24)]
    _report("SMPL size")
    m = pe.metrics(dev)
    print("POSEERR SMPL size: pve", m["pve"], "pa_pve", m["pa_pve"], "mpjpe", m["mpjpe"], "pa_mpjpe", m["pa_mpjpe"])
    assert not fails, "; ".join(fails[:10])


def test_tracker_pose_error(pe_mod):
    """MultiFrameTracker.pose_error: the estimate side from the tracker's context, streams in the caller's order"""
    from avatar_amd import api, synth
    from avatar_amd.tracker import MultiFrameTracker
    smpl = synth.load_model(0)
    gm = api.AvatarModel(smpl)
    pm = synth.identity_part_map()
    mt = MultiFrameTracker.create(gm, 2, 24, pm, max_points=4096, beta_pose=0.05, beta_shape=0.12, interval=12, frame_icp_iters=1, reinit_icp_iters=1,
                                  max_iters_per_icp=2)
    with pytest.raises(RuntimeError, match="fitted"):
        mt.pose_error([0], np.zeros((1, 6890, 3)), np.zeros((1, 24, 3)))
    frames, truth = [], []
    for s in range(2):
        w, p, R = synth.sample_ground_truth(smpl, s)
        verts = synth.pose_vertices(smpl, w, p, R)
        xyz, mask, _ = synth.render_images(smpl, verts, pm)
        frames.append((xyz, mask, None))
        truth.append(verts)
    assert all(mt.process(frames))
    streams = [1, 0, 1]
    posed = [mt.posed(s) for s in range(2)]
    tc = np.stack([truth[s] for s in streams])
    tj = np.stack([posed[s][1] + 0.01 * (i + 1) for i, s in enumerate(streams)])         # any joints will do: the plumbing is under test
    got = mt.pose_error(streams, tc, tj, pm)
    want = pe_mod.PoseError.for_model(gm, 24, pm, max_pairs=3).score(np.stack([posed[s][0] for s in streams]), np.stack([posed[s][1] for s in streams]), tc, tj)
    assert all(_same_bits(got, want, i, i) for i in range(3)) and (got["status"] == 0).all()
    assert np.array_equal(got["metrics"]["pve"], got["summary"][:, 0] / 6890) and got["metrics"]["pve_part"].shape == (3, 24)
    assert np.allclose(got["summary"][:, COL["J_SUM"]] / 24, [0.01 * np.sqrt(3) * (i + 1) for i in range(3)], rtol=1e-9)
    assert all(np.array_equal(a, b) for s in range(2) for a, b in zip(mt.posed(s), posed[s]))


def test_cpp_facade_scores_the_same_bits(pe_mod, tmp_path):
    """ark::PoseError (include/ark/PoseError.h) through tests/cpp/pose_error_demo: the bits of the Python binding"""
    import os
    import subprocess
    demo = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "pose_error_demo")
    assert os.path.exists(demo), "tests/cpp/pose_error_demo not built (make -C avatar_amd/csrc facade)"
    V, J = 65, 3
    P, vp = pc.part_tables(V)["sparse24"]
    b = pc.batch(V, J, seed=5)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        np.array([V, J, P, 4], np.int32).tofile(fh)
        vp.astype(np.int32).tofile(fh)
        for k in ("E", "A", "T", "B"):
            np.ascontiguousarray(b[k], np.float64).tofile(fh)
    r = subprocess.run([demo, "score", inp, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(outp, np.float64).reshape(4, 12 + 2 * J + 2 * P + 4)
    pe = pe_mod.PoseError(V, J, P, vp, max_pairs=4)
    want = pe.score(b["E"], b["A"], b["T"], b["B"])
    flat = np.concatenate([want["summary"], want["per_joint"].reshape(4, -1), want["per_part"].reshape(4, -1), want["argmax"].astype(np.float64),
                           want["status"].astype(np.float64)[:, None], pe.metrics(want)["pve"][:, None]], axis=1)
    assert np.array_equal(got.view(np.uint8), flat.view(np.uint8))


def test_identity_and_flags(pe_mod):
    V, J = 257, 24
    P, vp = pc.part_tables(V)["sparse24"]
    b = pc.batch(V, J, names=pc.FAMILIES[:3], seed=4)
    pe = pe_mod.PoseError(V, J, P, vp, max_pairs=3)
    same = pe.score(b["E"], b["A"], b["E"], b["A"])                                   # estimate == truth
    assert (same["status"] == 0).all() and (same["argmax"] == 0).all()                # the lowest index attains the maximum 0
    for i in range(3):
        s = same["summary"][i]
        tv, tj = pr.alignment_tolerance(b["E"][i], b["E"][i]), pr.alignment_tolerance(b["A"][i], b["A"][i])
        assert all(s[COL[k]] == 0 for k in ("V_SUM", "V_SQ", "V_MAX", "J_SUM", "J_MAX", "JR_SUM")) and not same["per_part"][i].any() and not same["per_joint"][i][0].any()
        assert abs(s[COL["VPA_SCALE"]] - 1) <= tv["scale"] and abs(s[COL["JPA_SCALE"]] - 1) <= tj["scale"]
        assert s[COL["VPA_SUM"]] <= tv["sum"] and s[COL["VPA_SQ"]] <= tv["sq"] and s[COL["JPA_SUM"]] <= tj["sum"] and s[COL["JPA_SQ"]] <= tj["sq"]
        assert (same["per_joint"][i][1] <= tj["err"]).all()
    clean = pe.score(b["E"], b["A"], b["T"], b["B"])
    assert (clean["status"] == 0).all()
    for what, side, index, value in (("NaN in a truth vertex", "T", (1, 5, 2), np.nan), ("inf in an estimate joint", "A", (1, 23, 0), np.inf),
                                     ("-inf in the last estimate vertex", "E", (1, V - 1, 1), -np.inf)):
        d = {k: v.copy() for k, v in b.items()}
        d[side][index] = value
        got = pe.score(d["E"], d["A"], d["T"], d["B"])
        assert got["status"].tolist() == [0, pe_mod.BAD_INPUT, 0], what
        assert _same_bits(got, clean, 0, 0) and _same_bits(got, clean, 2, 2), f"{what}: the other pairs changed"
        assert pr.pairs(d["E"], d["T"], d["A"], d["B"], vp, P)["status"].tolist() == [0, 1, 0]


def test_degenerate_alignments(pe_mod):
    rng = np.random.default_rng(21)
    V = 65
    E, T = pc.family("noise_shift", V, 9)
    fails = []
    # estimate joints all coincident: s = 0, the errors are the truth's distances from its centroid
    B = pc.CENTRE + 0.4 * rng.standard_normal((7, 3))
    A = np.tile(pc.CENTRE + np.array([0.1, 0.2, 0.3]), (7, 1))
    dev = pe_mod.PoseError(V, 7, 1, None, max_pairs=1).score(E[None], A[None], T[None], B[None])
    assert dev["summary"][0][COL["JPA_SCALE"]] == 0.0
    fails += _check_pair("coincident joints", dev, 0, E, T, A, B, None, 1)
    # an estimate cloud of coincident points as well
    Ec = np.tile(E[:1], (V, 1))
    devc = pe_mod.PoseError(V, 0, 1, None, max_pairs=1).score(Ec[None], None, T[None], None)
    assert devc["summary"][0][COL["VPA_SCALE"]] == 0.0
    fails += _check_pair("coincident cloud", devc, 0, Ec, T, None, None, None, 1)
    # J = 2: the rotation about the joints' axis is free, the aligned points are not
    A2, B2 = pc.CENTRE + 0.4 * rng.standard_normal((2, 3)), pc.CENTRE + 0.4 * rng.standard_normal((2, 3))
    dev2 = pe_mod.PoseError(V, 2, 1, None, max_pairs=1).score(E[None], A2[None], T[None], B2[None])
    fails += _check_pair("two joints", dev2, 0, E, T, A2, B2, None, 1)
    # truth collinear with a generic estimate: the optimum is a circle of rotations; *_SQ and *_SCALE are unique, *_SUM is not
    A3 = pc.CENTRE + 0.4 * rng.standard_normal((9, 3))
    B3 = pc.CENTRE + np.outer(rng.standard_normal(9), np.array([0.3, -0.2, 0.1]))
    Tl = pc.CENTRE + np.outer(rng.standard_normal(V), np.array([0.1, 0.4, -0.3]))
    dev3 = pe_mod.PoseError(V, 9, 1, None, max_pairs=1).score(E[None], A3[None], Tl[None], B3[None])
    fails += _check_pair("collinear truth", dev3, 0, E, Tl, A3, B3, None, 1, sum_unique=False)
    _report("degenerate")
    assert not fails, "; ".join(fails[:10])
