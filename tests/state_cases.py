"""Frames that put the fit at the edges of its STATE space, on rows of tests/fit_models.py and on the synthetic SMPL model: steps on both
sides of the retraction's |d|^2 = 1/4 (avt_lm.hip k_solve), a minimising mixture component that changes with the step, w crossing zero, w
exactly +-0, the identity and the two small-norm branches of the quaternion -> angle-axis conversion (avt_prior.h), and the other
hemisphere (q and -q are one rotation).  A helper module of the tests, not a test file; building a frame needs neither a GPU nor more of
the oracle than its forward model.  tests/test_state_edges_cpu.py proves with the oracle alone that every case is what its name says.

  ROWS        the models: five fit_models cases and "smpl" (literal-dims kernels)
  cases()     [(row, scenario)]; case_id(case)
  frame(case) dict like fit_models.fit_frame's, plus `named` (the joints the scenario is about) and, for a "-neg" scenario,
              `negated` (bool per joint) and `plain` (the case it negates)
  study(case) fit_models.study_frame of the case, cached"""
from __future__ import annotations

import numpy as np

import fit_models as fm

SMPL = "smpl"
ROWS = [(3, 3, "star", 3), (9, 6, "star", 16), (23, 15, "ternary", 3), (24, 13, "ternary", 3), (24, 13, "ternary", 0), SMPL]
SMPL_STRIDE = 24            # every 24th pixel of the synthetic frame: about 1.5 k data points
# "switch" needs a prior; the "-neg" scenarios negate the start of the scenario in front of the dash (all joints, or an arbitrary half).
# "pi" has no negated form: at w = +-0 Eigen's conversion takes the axis as +xyz for both zeros (-0 < 0 is false), so negating such a joint
# turns its angle-axis vector round - the one point where q and -q are not the same state to the prior, in the oracle as on the device
SCENARIOS = ("big", "switch", "cross", "pi", "ident", "ident-eps", "ident-tiny", "big-negall", "cross-neghalf", "ident-eps-negall")
ONE_STEP = ("big", "switch", "cross", "pi", "ident", "ident-eps", "ident-tiny")        # held to the long-double step
# per (row, scenario): what the scenario turns and by how much, and the seed of its draws; found by search so that the conditions of
# tests/test_state_edges_cpu.py hold (as SEEDS of fit_models)
#   big / switch: root (turn the root) or joints (turn these) by `angle` from the ground truth
#   cross:        w0, the start's w of the named joints (the ground truth has -0.1)
DEFAULTS = dict(big=dict(joints=(1, -1), angle=1.5, seed=0), switch=dict(joints=(1, -1), angle=2.5, seed=0), cross=dict(w0=0.1, seed=0),
                pi=dict(seed=0), ident=dict(seed=0))
PARAMS = {
    ((3, 3, "star", 3), "big"): dict(root=True, angle=2.0, seed=3), ((3, 3, "star", 3), "switch"): dict(root=True, angle=1.2),
    ((9, 6, "star", 16), "big"): dict(root=True, angle=2.5), ((9, 6, "star", 16), "switch"): dict(root=True, angle=1.2),
    ((23, 15, "ternary", 3), "big"): dict(angle=1.2), ((23, 15, "ternary", 3), "switch"): dict(root=True, angle=1.5),
    ((23, 15, "ternary", 3), "cross"): dict(w0=0.05),
    ((24, 13, "ternary", 3), "big"): dict(root=True, angle=1.2), ((24, 13, "ternary", 3), "switch"): dict(root=True, angle=1.2),
    ((24, 13, "ternary", 3), "cross"): dict(w0=0.05),
    ((24, 13, "ternary", 0), "big"): dict(root=True, angle=1.2), ((24, 13, "ternary", 0), "cross"): dict(w0=0.05, seed=2),
    ((24, 13, "ternary", 0), "pi"): dict(seed=2),
    (SMPL, "big"): dict(root=True, angle=1.2), (SMPL, "switch"): dict(root=True, angle=2.0),
}
_FRAMES, _STUDY, _OM = {}, {}, {}


def has_prior(row):
    return row == SMPL or row[3] > 0


def cases():
    return [(row, sc) for row in ROWS for sc in SCENARIOS if has_prior(row) or not sc.startswith("switch")]


def row_id(row):
    return SMPL if row == SMPL else fm.case_id(row)


def case_id(case):
    return f"{row_id(case[0])}-{case[1]}"


def params(case):
    row, sc = case
    base = sc.split("-")[0]
    return {**DEFAULTS[base], **PARAMS.get((row, base), {})}


def row_model(row):
    """(model dict, OracleModel) of the row, one per process"""
    if row not in _OM:
        from oracle import oracle as orc
        if row == SMPL:
            from avatar_amd import synth
            m = synth.load_model(0)
        else:
            m = fm.case_model(row)
        _OM[row] = (m, orc.OracleModel(m))
    return _OM[row]


def quat_mul(a, b):
    """a b, (x, y, z, w)"""
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def _axis(rng):
    a = rng.standard_normal(3)
    return a / np.linalg.norm(a)


def _about(axis, w):
    """the unit quaternion about `axis` whose scalar part is w"""
    return np.concatenate([np.sqrt(1.0 - w * w) * axis, [w]])


def _grid(data):
    return np.ascontiguousarray(np.rint(np.asarray(data, np.float64) * 2.0 ** 40) / 2.0 ** 40)      # (fit_models.fit_frame)


def _base(row):
    """the row's benign frame: fit_models' own, or the synthetic SMPL frame 0 with its start quaternions"""
    m, om = row_model(row)
    if row != SMPL:
        return fm.case_frame(row, om)
    if "base" not in _OM:
        _OM["base"] = _smpl_base(m, om)
    return _OM["base"]


def _smpl_base(m, om):
    from avatar_amd import api, synth
    f = synth.make_frame(m, 0)
    w, p, R = f["gt"]
    w0, p0, R0 = f["start"]
    sel = np.arange(0, len(f["labels"]), SMPL_STRIDE)
    return dict(data=_grid(f["data"][sel]), labels=np.ascontiguousarray(f["labels"][sel]), part_map=synth.identity_part_map(), num_parts=om.J,
                start=(p0, api.rot_to_quat(R0), w0), gt=(p, api.rot_to_quat(R), w), betas=(0.05, 0.12))


def _data_of(row, gt, rng):
    """a data cloud of the ground truth gt = (p, q, w): the model's points with 2 mm of noise, or for SMPL the rendered depth cloud"""
    m, om = row_model(row)
    if row != SMPL:
        return _grid(om.points(*gt) + 0.002 * rng.standard_normal((om.V, 3))), om.main_joint().astype(np.int32)
    from avatar_amd import api, synth
    p, q, w = gt
    data, labels = synth.render_cloud(m, synth.pose_vertices(m, w, p, api.quat_to_rot(q)), synth.identity_part_map())
    sel = np.arange(0, len(labels), SMPL_STRIDE)
    return _grid(data[sel]), np.ascontiguousarray(labels[sel])


def _joints(J, js):
    return [j % J for j in js]


def _plain_frame(row, base, prm):
    """the frame of a scenario without a "-neg" suffix"""
    m, om = row_model(row)
    J = om.J
    b = _base(row)
    fr = dict(b)
    rng = np.random.default_rng([20261019, 7, J, om.K, prm["seed"], ("big", "switch", "cross", "pi", "ident").index(base)])
    pg, qg, wg = (np.array(x, np.float64) for x in b["gt"])
    p0, q0, w0 = (np.array(x, np.float64) for x in b["start"])
    if base in ("big", "switch"):
        named = [0] if prm.get("root") else _joints(J, prm["joints"])
        for j in named:
            h = 0.5 * prm["angle"]
            q0[j] = quat_mul(qg[j], np.concatenate([np.sin(h) * _axis(rng), [np.cos(h)]]))
        fr.update(start=(p0, q0, w0), named=named)
    elif base in ("cross", "pi"):
        named = _joints(J, (1, -1))
        axes = [_axis(rng) for _ in named]
        if base == "cross":      # the ground truth just behind w = 0, the start just in front of it, about one axis
            for j, a in zip(named, axes):
                qg[j], q0[j] = _about(a, -0.1), _about(a, prm["w0"])
        else:                    # the start a rotation by pi exactly, w = +0 and w = -0; the ground truth on either side
            for j, a, z, wgt in zip(named, axes, (0.0, -0.0), (0.1, -0.1)):
                qg[j], q0[j] = _about(a, wgt), np.concatenate([a, [z]])
        data, labels = _data_of(row, (pg, qg, wg), rng)
        fr.update(start=(p0, q0, w0), gt=(pg, qg, wg), data=data, labels=labels, named=named)
    else:
        q0 = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (J, 1))
        fr.update(start=(p0, q0, w0), named=[1])
    return fr


def frame(case):
    if case in _FRAMES:
        return _FRAMES[case]
    row, sc = case
    parts = sc.split("-")
    neg = parts[-1] if parts[-1].startswith("neg") else None
    plain_sc = "-".join(parts[:-1]) if neg else sc
    base = parts[0]
    m, om = row_model(row)
    if neg:
        fr = dict(frame((row, plain_sc)))
        p0, q0, w0 = fr["start"]
        if neg == "negall":
            negated = np.ones(om.J, bool)
        else:       # an arbitrary half, without the root (negall has it)
            negated = np.zeros(om.J, bool)
            pick = np.random.default_rng([20261019, 8, om.J]).permutation(np.arange(1, om.J))[:max(1, om.J // 2)]
            negated[pick] = True
            negated[fr["named"][0]] = True        # (and one of the joints the scenario is about: its sign is the one that matters)
        fr.update(start=(p0, np.where(negated[:, None], -q0, q0), w0), negated=negated, plain=(row, plain_sc))
    else:
        fr = _plain_frame(row, base, params(case))
        if sc == "ident-eps":         # |xyz| = 5e-17 < eps: the stableNorm branch
            fr["start"][1][1] = (3e-17, -4e-17, 0.0, 1.0)
        elif sc == "ident-tiny":      # x^2 underflows: the plain norm is 0, the stable one 1e-200
            fr["start"][1][1] = (1e-200, 0.0, 0.0, 1.0)
    _FRAMES[case] = fr
    return fr


def study(case):
    """fit_models.study_frame of the case (cached), plus fit (the oracle's 2 ICP x 4 GN fit) and replay (fit_models.replay_fit)"""
    if case not in _STUDY:
        m, om = row_model(case[0])
        fr = frame(case)
        s = fm.study_frame(m, om, fr)
        s["case"] = case
        s["fit"] = om.optimize(fr["part_map"], fr["num_parts"], fr["data"], fr["labels"], fm.options(fr, icp_iters=2, max_iters_per_icp=4), *fr["start"], aggregate=1)
        _STUDY[case] = s
    return _STUDY[case]


def replay(case):
    s = study(case)
    if "replay" not in s:
        s["replay"] = fm.replay_fit(s["om"], s["frame"])
    return s["replay"]


def step_z(case):
    """|d|^2 per joint of the long-double first step"""
    d = study(case)["delta_ld"]
    J = study(case)["om"].J
    return (d[3:3 + 3 * J].reshape(J, 3) ** 2).sum(1)


def nn_gap(case, state):
    """smallest relative gap (d2 - d1) / d2 between the squared distances of a data point to its nearest and second-nearest candidate
    (the model points of the point's part) at `state`"""
    s = study(case)
    fr, om = s["frame"], s["om"]
    cloud = om.points(*state)
    part = np.asarray(fr["part_map"])[om.main_joint()]
    worst = np.inf
    for l in np.unique(fr["labels"]):
        cand = cloud[part == l]
        pts = fr["data"][fr["labels"] == l]
        if l < 0 or len(cand) < 2 or not len(pts):
            continue
        d2 = np.sort(((pts[:, None, :] - cand[None, :, :]) ** 2).sum(-1), axis=1)
        worst = min(worst, float(((d2[:, 1] - d2[:, 0]) / d2[:, 1]).min()))
    return worst
