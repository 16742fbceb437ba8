"""Inputs of the trimmed-ICP tests (tests/test_nn_trim_cpu.py, tests/test_gpu_nn_trim.py): the boundary cases written out by hand on
the gate test's hand model, and the contaminated frame of the fits.  A helper module of the tests, not a test file; no GPU is needed
to build anything here.

The hand model: identity part map; the first vertex of part 0 at the origin, the first of part 1 at (10, 0, 0), nothing else visible.
Queries lie on an axis at multiples of 2^-10 (or at the listed values), so every squared distance is exact and the expectations
can be written down."""
from __future__ import annotations

import numpy as np

import nn_cases

LDS_KEYS = 4096            # TRIM_KEYS of avatar_amd/csrc/avt_trim.hip: matched keys of a (part, frame) kept in LDS
WALK = 1024                # TRIM_THREADS: queries a k_trim workgroup looks at per turn of a walk
INF = np.inf
STEP = 2.0 ** -10
# The fixed-point term of a point 1.3e154 m from the frame's centre is outside the range the 2^40 sums are defined for (|x| < 2^51,
# tests/nn_restatement.py).  Where that point is TRIMMED its term must have been taken back exactly - modulo 2^64, whatever it was -
# and the sums are compared; where it is kept they are not (counts and everything else are).
NO_SUMS = {"zero, denormal, huge: k = n"}


def hand_model(smpl):
    pm, npart = nn_cases.part_map("identity")
    pov = nn_cases.part_of_vertex(smpl, pm)
    v0, v1 = int(np.nonzero(pov == 0)[0][0]), int(np.nonzero(pov == 1)[0][0])
    cloud = np.full((nn_cases.V, 3), 100.0)
    cloud[v0] = 0.0
    cloud[v1] = (10.0, 0.0, 0.0)
    vis = np.zeros(nn_cases.V, np.uint8)
    vis[[v0, v1]] = 1
    return pm, npart, pov, cloud, vis, v0, v1


def _ramp(n, rho):
    """n queries of part 0 at x = i 2^-10, i = n .. 1 (descending, so that positions and ranks differ): d2 = i^2 2^-20.  At kappa 1,
    floor 0: k = ceil(rho n), T = k^2 2^-20, the queries with i <= k keep their match."""
    i = np.arange(n, 0, -1)
    k = min(max(int(np.ceil(rho * float(n))), 1), n)
    q = np.zeros((n, 3))
    q[:, 0] = i * STEP
    return q, [0] * n, ["v0" if j <= k else -1 for j in i], {0: n - k}, {0: (k * STEP) * (k * STEP)}


def hand_cases():
    """(name, queries, labels, gate, (rho, kappa, floor, min_matches), expected indices ('v0' / 'v1' / -1), expected gated count,
    expected trimmed per part {part: n}, expected finite thresholds {part: T}) - the expectations written by hand."""
    e = 2.0 ** -26
    big = float(np.sqrt(1.79e308))
    den = 2.0 ** -537                                    # d2 = 2^-1074, the smallest denormal
    one = (0.5, 1.0, 0.0, 1)
    zdh = [(0, 0, 0), (big, 0, 0), (den, 0, 0)]          # the frame's centre is its first point: the origin
    four = [(0.125, 0, 0), (0.5, 0, 0), (0.25, 0, 0), (0.375, 0, 0)]
    both = ([(0.5, 0, 0), (0.25, 0, 0), (10.5, 0, 0), (10.25, 0, 0)], [0, 0, 1, 1])
    per0 = [1.0] + [INF] * 23
    out = [
        ("n = 0 and n = 1", [(10.5, 0, 0)], [1], None, one, ["v1"], 0, {}, {1: 0.25}),
        ("n = 2", [(0.5, 0, 0), (0.25, 0, 0)], [0, 0], None, one, [-1, "v0"], 0, {0: 1}, {0: 0.0625}),
        ("all equal", [(0.5, 0, 0)] * 5, [0] * 5, None, (0.2, 1.0, 0.0, 1), ["v0"] * 5, 0, {}, {0: 0.25}),
        ("low mantissa bits k = 2", [(1, e, 0), (1, e, e), (1, 2 * e, 0)], [0] * 3, None, one, ["v0", "v0", -1], 0, {0: 1}, {0: 1.0 + 2.0 ** -51}),
        ("low mantissa bits k = 1", [(1, 2 * e, 0), (1, e, e), (1, e, 0)], [0] * 3, None, (0.3, 1.0, 0.0, 1), [-1, -1, "v0"], 0, {0: 2}, {0: 1.0 + 2.0 ** -52}),
        ("zero, denormal, huge: k = 2", zdh, [0] * 3, None, one, ["v0", -1, "v0"], 0, {0: 1}, {0: 5e-324}),
        ("zero, denormal, huge: k = n", zdh, [0] * 3, None, (1.0, 1.0, 0.0, 1), ["v0"] * 3, 0, {}, {0: big * big}),
        ("zero, denormal, huge: k = 1", zdh, [0] * 3, None, (0.1, 1.0, 0.0, 1), ["v0", -1, -1], 0, {0: 2}, {0: 0.0}),
        ("k = 1", four, [0] * 4, None, (1e-9, 1.0, 0.0, 1), ["v0", -1, -1, -1], 0, {0: 3}, {0: 0.015625}),
        ("k = n", four, [0] * 4, None, (1.0, 1.0, 0.0, 1), ["v0"] * 4, 0, {}, {0: 0.25}),
        ("kappa = 0", [(0, 0, 0), (0.125, 0, 0), (0, 0, 0)], [0] * 3, None, (1.0, 0.0, 0.0, 1), ["v0", -1, "v0"], 0, {0: 1}, {0: 0.0}),
        ("kappa = 0 with a floor", four, [0] * 4, None, (1.0, 0.0, 0.25, 1), ["v0", -1, "v0", -1], 0, {0: 2}, {0: 0.0625}),
        ("the floor decides", four, [0] * 4, None, (0.5, 1.0, 0.375, 1), ["v0", -1, "v0", "v0"], 0, {0: 1}, {0: 0.140625}),
        ("the quantile decides over the floor", four, [0] * 4, None, (0.5, 1.0, 0.125, 1), ["v0", -1, "v0", -1], 0, {0: 2}, {0: 0.0625}),
        ("kappa = 2", four, [0] * 4, None, (0.5, 2.0, 0.0, 1), ["v0", "v0", "v0", "v0"], 0, {}, {0: 0.25}),
        ("min_matches = n", four, [0] * 4, None, (0.5, 1.0, 0.0, 4), ["v0", -1, "v0", -1], 0, {0: 2}, {0: 0.0625}),
        ("min_matches = n + 1", four, [0] * 4, None, (0.5, 1.0, 0.0, 5), ["v0"] * 4, 0, {}, {}),
        ("a trimmed part beside an untrimmed one", both[0], both[1], None, (0.5, per0, 0.0, 1), [-1, "v0", "v1", "v1"], 0, {0: 1}, {0: 0.0625}),
        ("both parts trimmed", both[0], both[1], None, one, [-1, "v0", -1, "v1"], 0, {0: 1, 1: 1}, {0: 0.0625, 1: 0.0625}),
        ("a fixed gate and the trim", [(0.125, 0, 0), (0.25, 0, 0), (0.375, 0, 0), (5.0, 0, 0)], [0] * 4, 1.0, one, ["v0", "v0", -1, -1], 1, {0: 1}, {0: 0.0625}),
    ]
    for n in (255, 256, 257, WALK - 1, WALK, WALK + 1, LDS_KEYS - 1, LDS_KEYS, LDS_KEYS + 1):
        q, lab, want, trimmed, T = _ramp(n, 0.5)
        out.append((f"ramp of {n}", q, lab, None, one, want, 0, trimmed, T))
    q, lab, want, trimmed, T = _ramp(LDS_KEYS + 1, 0.999)
    out.append((f"ramp of {LDS_KEYS + 1} near the top", q, lab, None, (0.999, 1.0, 0.0, 1), want, 0, trimmed, T))
    return out


def expand(case, v0, v1, npart):
    """-> (name, data, labels, gate, settings, indices int32, gated, trimmed per part int32[npart], T float64[npart])"""
    name, queries, labels, gate, settings, want, gated, trimmed, T = case
    idx = np.array([{"v0": v0, "v1": v1}.get(w, -1) for w in want], np.int32)
    tp = np.zeros(npart, np.int32)
    for q, n in trimmed.items():
        tp[q] = n
    Tq = np.full(npart, INF)
    for q, t in T.items():
        Tq[q] = t
    return name, np.array(queries, np.float64).reshape(-1, 3), np.array(labels, np.int32), gate, settings, idx, gated, tp, Tq


def contaminated(smpl, omodel):
    """The contaminated frame of tests/test_gpu_nn_gate.py, rebuilt: every 6th pixel of synth.make_frame(smpl, 3) (5 201 points) and 300
    planted points 0.6 m off a data point each, carrying that point's label; permuted with index 0 left first.  With it the ungated
    correspondences of the start state (the CPU oracle's search) and that state's cloud."""
    from avatar_amd import api, synth
    from avatar_amd.capi import Options
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
    assert N == 5201
    for a in (D, L, planted, ungated, cloud0):
        a.setflags(write=False)
    return dict(D=D, L=L, planted=planted, start=(p0, q0, w0), pm=pm, opt=opt, ungated_corr=ungated, cloud0=cloud0, clean=(data, labels))
