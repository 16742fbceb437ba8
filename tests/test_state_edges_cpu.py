"""The conditions of tests/test_gpu_state_edges.py, on the CPU and by the oracle alone: every case of tests/state_cases.py is what its name
says, so the GPU test cannot pass vacuously - the first step has joints on the required sides of |d|^2 = 1/4, the minimising component
changes, w changes sign, the start sits on the branch of the angle-axis conversion it is there for - and every case is fit to test with:
the first step accepted, the oracle's own step well inside the bound the device is held to, lambda determined by the fit, no accepted state
with a non-root |w| so small that one ulp decides its sign, no data point with two nearest candidates nearly as far.  And api.rot_to_quat
against oracle.rot_to_quat, bit for bit, on every branch of the Eigen closed form."""
import numpy as np
import pytest

import fit_models as fm
import state_cases as sc

CASES = sc.cases()
IDS = [sc.case_id(c) for c in CASES]
NEG = [c for c in CASES if "neg" in c[1]]
EPS = float(np.finfo(np.float64).eps)
W_MIN = 1e-6        # no accepted non-root |w| below this: a condition on the inputs (the device may differ from the oracle by ulps of 1e-16), no tolerance
NN_GAP = 1e-6       # relative gap (d2 - d1) / d2 of the squared distances to the nearest and second-nearest candidate: ten orders above the rounding of a distance


def _base(case):
    return case[1].split("-")[0]


def test_the_table_lists_every_scenario_on_every_row():
    assert len(sc.ROWS) == 6 and sc.SMPL in sc.ROWS and (24, 13, "ternary", 0) in sc.ROWS
    assert any(r != sc.SMPL and r[3] == fm.MAX_COMPS for r in sc.ROWS)
    for row in sc.ROWS:
        have = {s for r, s in CASES if r == row}
        want = set(sc.SCENARIOS) - (set() if sc.has_prior(row) else {"switch"})
        assert have == want, (row, have ^ want)
    for row in sc.ROWS:
        if row != sc.SMPL:
            assert row in fm.cases()
            pr = dict(zip(fm.PROMISE_FIELDS, fm.PROMISES[row[:3]]))
            assert pr["threads"] == (1024 if row[0] == 24 else 256)
    m, om = sc.row_model(sc.SMPL)
    assert (om.J, om.K, om.P, om.arrays.ndims) == (24, 10, 85, 69) and om.arrays.ncomps > 0      # the dimensions of the literal-dims kernels
    # the two neg forms: all quaternions, and a half of them that has a joint the scenario is about; the root is in the first
    for case in NEG:
        fr = sc.frame(case)
        n = fr["negated"]
        if case[1].endswith("negall"):
            assert n.all()
        else:
            assert not n[0] and 0 < n.sum() < len(n) and n[fr["named"][0]]
        plain = sc.frame(fr["plain"])
        assert np.array_equal(fr["start"][1], np.where(n[:, None], -plain["start"][1], plain["start"][1])) and fr["data"] is plain["data"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_what_its_name_says(case):
    s = sc.study(case)
    fr, om = s["frame"], s["om"]
    J = om.J
    base, scen = _base(case), case[1]
    p0, q0, w0 = fr["start"]
    st1 = s["step1"]
    q1 = st1["q"]
    # ---- fit to test with (tests/test_fit_dims_cpu.py)
    assert len(np.unique(om.main_joint()[s["corr"][s["corr"] >= 0]])) == J                   # every joint with matched vertices
    assert (np.diag(s["H"]) > 0).all() and (s["pivots"] > 0).all()
    assert st1["stats"].accepted_steps == 1 and st1["stats"].gn_iterations == 1
    assert s["e_oracle"] <= s["bound"] / 16, (s["e_oracle"], s["bound"])
    r = sc.replay(case)
    fit = s["fit"]
    assert r["acc"] == [int(a) for a in fit["trace_acc"] if a != -2], (r["acc"], fit["trace_acc"])
    assert r["kappa"] <= fm.KAPPA_MAX, r["kappa"]
    # (the replay follows the oracle's fit: its Cholesky is numpy's, so on SMPL's steps of two radians it differs by more than kappa's share)
    assert abs(r["lam"] / fit["stats"].lambda_ - 1.0) <= 1e-9 / 16
    assert fm.state_distance(r["states"][-1], (fit["p"], fit["q"], fit["w"])) <= 1e-9
    gap = min(sc.nn_gap(case, st) for st in r["icp_states"])
    assert gap >= NN_GAP, gap
    z = sc.step_z(case)
    unit = np.abs((q0 ** 2).sum(1) - 1.0).max()
    assert unit <= 4 * EPS, unit              # (quaternions off the unit sphere are not what this is about)
    comp0 = comp1 = -1
    if sc.has_prior(case[0]):
        comp0 = om.evaluate(p0, q0, w0, s["corr"], fr["data"], *fr["betas"], aggregate=1)[3]
        comp1 = om.evaluate(st1["p"], q1, st1["w"], s["corr"], fr["data"], *fr["betas"], aggregate=1)[3]
        assert (comp0, comp1) == (om.pose_prior_residual(q0)[0], om.pose_prior_residual(q1)[0])
    # ---- what the scenario is there for
    if base == "big":
        assert (z >= 0.25).any() and (z < 0.25).any() and (z > 0).all()
        assert ((z > 0.2) & (z < 0.25)).any() and ((z >= 0.25) & (z < 0.35)).any(), np.sort(z)      # (every row's seed gives these)
    if base == "switch":
        assert comp0 != comp1 and comp0 >= 0 and comp1 >= 0
    if base == "cross":
        crossed = [j for j in fr["named"] if (q0[j, 3] < 0) != (q1[j, 3] < 0)]
        assert crossed and all(j > 0 for j in crossed), (q0[fr["named"], 3], q1[fr["named"], 3])
    if base in ("cross", "pi"):
        states = r["states"][1:] if base == "pi" else r["states"]
        wmin = min(float(np.abs(st[1][1:, 3]).min()) for st in states)
        assert wmin > W_MIN, wmin
    if base == "pi":
        a, b = fr["named"]
        assert a > 0 and b > 0 and a != b
        assert q0[a, 3] == 0.0 and not np.signbit(q0[a, 3]) and q0[b, 3] == 0.0 and np.signbit(q0[b, 3])
        x = om.pose_prior_residual(q0)[1] if sc.has_prior(case[0]) else None
        if x is not None:        # the angle is pi, along +axis for both signs of the zero
            for j in (a, b):
                assert np.abs(x[3 * (j - 1):3 * j] - np.pi * q0[j, :3]).max() <= 4 * EPS
    if base == "ident" and "neg" not in scen:
        others = [j for j in range(J) if not (scen != "ident" and j == 1)]
        assert (q0[others] == np.array([0.0, 0.0, 0.0, 1.0])).all()
        n1 = float(np.sqrt(q0[1, 0] * q0[1, 0] + q0[1, 1] * q0[1, 1] + q0[1, 2] * q0[1, 2]))
        if scen == "ident":
            assert n1 == 0.0
        elif scen == "ident-eps":
            assert 0.0 < n1 < EPS
        else:
            assert n1 == 0.0 and q0[1, 0] == 1e-200           # the plain norm underflows, the stable one does not
        if sc.has_prior(case[0]):
            x = om.pose_prior_residual(q0)[1]
            want = {"ident": (0.0, 0.0), "ident-eps": (2 * 3e-17, 2 * -4e-17), "ident-tiny": (2e-200, 0.0)}[scen]
            assert np.allclose(x[:2], want, rtol=1e-12, atol=0.0) and (x[2:] == 0.0).all(), x[:3]
    if "neg" in scen:
        assert (q0[fr["negated"], 3] < 0).sum() >= 1
    print(f"STATEEDGES cpu {sc.case_id(case)} z>=1/4 {int((z >= 0.25).sum())}/{J} max|d| {np.sqrt(z.max()):.2f} comp {comp0}->{comp1} w<0 at start {int((q0[1:, 3] < 0).sum())} "
          f"after the step {int((q1[1:, 3] < 0).sum())} acc {r['acc']} cond {s['cond']:.2e} bound {s['bound']:.2e} E_oracle {s['e_oracle']:.2e} kappa {r['kappa']:.1e} nn gap {gap:.1e}")


def test_some_fit_rejects_a_step_and_every_branch_is_driven():
    rejected = [c for c in CASES if 0 in sc.replay(c)["acc"]]
    assert rejected
    # a REJECTED trial point whose minimising component is not the current point's: the solve goes back to the current slot and loads the
    # prior of its component again - on a 256-thread solve (SMPL's) and on a 1024-thread one
    back = set()
    for c in CASES:
        r = sc.replay(c)
        if any(a == 0 and cur != tri for (cur, tri), a in zip(r["comps"], [a for a in r["acc"] if a != -1])):
            back.add(c[0])
    assert sc.SMPL in back and any(r != sc.SMPL and r[0] == 24 for r in back), back
    for row in sc.ROWS:
        lib = poly = False
        for sn in ("big", "switch", "cross", "pi", "ident"):
            if (row, sn) in CASES:
                z = sc.step_z((row, sn))
                lib, poly = lib or bool((z >= 0.25).any()), poly or bool((z < 0.25).any())
        assert lib and poly, row
        if sc.has_prior(row):      # the component reload of k_solve's per-slot choice, in a fit that goes on behind it
            s = sc.study((row, "switch"))
            assert s["fit"]["stats"].accepted_steps >= 2


@pytest.mark.parametrize("case", NEG, ids=[sc.case_id(c) for c in NEG])
def test_oracle_fit_from_the_negated_start_is_the_plain_fit(case):
    """q and -q are one rotation, and every operation of the fit is odd or even in each joint's quaternion: the oracle's fit from the negated
    start equals the fit from the plain start bit for bit, the negated joints' quaternions with the other sign."""
    fr = sc.frame(case)
    a, b = sc.study(case)["fit"], sc.study(fr["plain"])["fit"]
    sign = np.where(fr["negated"], -1.0, 1.0)[:, None]
    assert np.array_equal(a["p"], b["p"]) and np.array_equal(a["w"], b["w"]) and np.array_equal(a["q"], sign * b["q"])
    assert np.array_equal(a["trace_cost"], b["trace_cost"]) and np.array_equal(a["trace_acc"], b["trace_acc"]) and np.array_equal(a["corr"], b["corr"])
    assert (a["stats"].lambda_, a["stats"].final_cost, a["stats"].gn_iterations, a["stats"].accepted_steps) == \
        (b["stats"].lambda_, b["stats"].final_cost, b["stats"].gn_iterations, b["stats"].accepted_steps)


def _rot(axis, angle):
    from avatar_amd import api
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return api.quat_to_rot(np.concatenate([np.sin(0.5 * angle) * a, [np.cos(0.5 * angle)]]))[0]


def test_rot_to_quat_equals_the_oracles_on_every_branch():
    """api.rot_to_quat claims the oracle's roundings; the fits only ever gave it the trace > 0 branch."""
    from avatar_amd import api
    from oracle import oracle as orc
    skew = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    named = {
        "identity": np.eye(3),
        "pi about x": np.diag([1.0, -1.0, -1.0]), "pi about y": np.diag([-1.0, 1.0, -1.0]), "pi about z": np.diag([-1.0, -1.0, 1.0]),
        "pi about a skew axis": 2.0 * np.outer(skew, skew) - np.eye(3),
        "trace > 0": _rot([0.3, -0.5, 0.8], 0.9),
        "largest diagonal 0": _rot([0.9, 0.2, -0.1], 2.7), "largest diagonal 1": _rot([0.1, -0.9, 0.2], 2.7), "largest diagonal 2": _rot([-0.2, 0.1, 0.9], 2.7),
        "trace 0 exactly": np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]),
    }
    rng = np.random.default_rng(20261019)
    for i in range(8):          # 1 + 2 cos(2 pi / 3) = 0: the trace is what rounding leaves of it, of either sign
        named[f"trace about 0 ({i})"] = _rot(rng.standard_normal(3), 2.0 * np.pi / 3.0)
    R = np.stack(list(named.values()))
    tr = np.trace(R, axis1=1, axis2=2)
    diag = np.diagonal(R, axis1=1, axis2=2)
    by = dict(zip(named, range(len(named))))
    assert tr[by["trace > 0"]] > 0.5 and tr[by["identity"]] == 3.0
    for k, ax in enumerate("xyz"):
        assert tr[by[f"pi about {ax}"]] == -1.0 and tr[by[f"largest diagonal {k}"]] < 0 and diag[by[f"largest diagonal {k}"]].argmax() == k
    near = [i for n, i in by.items() if n.startswith("trace about 0")]
    assert (np.abs(tr[near]) <= 1e-15).all() and (tr[near] > 0).any() and (tr[near] <= 0).any(), tr[near]
    got, want = api.rot_to_quat(R), orc.rot_to_quat(R)
    for n, i in by.items():
        assert got[i].tobytes() == want[i].tobytes(), (n, got[i], want[i])
    assert (want[:, 3] >= 0).all()        # (why no fit ever started in the other hemisphere)
