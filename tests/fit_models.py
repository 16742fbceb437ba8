"""Small models that can be FITTED, at the system sizes and kernel variants avt_model_create accepts (J <= 64, K <= 16, P = 3 + 3 J + K
<= 179) and the fitting kernels branch on (avt_eval.hip launch_eval, avt_lm.hip k_solve, avt_moments.hip, avt_prep.h).  A helper module of
the tests, not a test file; building a model needs neither a GPU nor the oracle.

  fit_model(J, K, tree, ncomps, seed)   an SMPL-npz-style dict that capi.ModelArrays takes: 12 vertices per joint, every joint with
                                        vertices of its own (the data term has no zero rows), optionally a pose prior
  fit_frame(model, om, seed)            ground truth, data cloud, labels, part map, start state and betas of one frame (om: an OracleModel)

ROWS is the table of (J, K, tree); PROMISES what every row promises about itself, written out by hand; promises(J, K, tree) the same from the
formulas of the kernels.  tests/test_fit_dims_cpu.py compares the two and checks that the rows hit every boundary."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

PER_JOINT = 12
MAX_COMPS = 16              # AVT_MAX_COMPS
LEVELS_REG, TITEM_THREADS = 10, 256      # AVT_PREP_LEVELS_REG, AVT_PREP_TITEM_THREADS (avt_internal.h)
MOMENTS_REFUSAL = "K + 1 <= 16 and 3 + 3J + K <= 87 required"     # avt_set_data_term(MOMENTS) on a model without the moment form

# (J, K, tree): why the row is there
ROWS = [
    ((1, 1, "chain"), "root only, no prior possible; NT 1, HS 8, NR 2"),
    ((3, 3, "star"), "P + 1 = 16, one tile filled exactly; HS 16"),
    ((4, 1, "star"), "first column of a second tile; P % 4 == 0; HS 20"),
    ((4, 0, "chain"), "K = 0: empty shape tables"),
    ((5, 16, "star"), "K = AVT_MAX_SHAPE on a 256-thread solve; moment form refused because K + 1 > 16"),
    ((9, 4, "star"), "3 K + 4 = 16, k_moments<1> at its top; level 1 has 8 x 24 = 192 items, fk_reg 1"),
    ((9, 6, "star"), "mom_ntp 2; 8 x 30 = 240 items, the last fk_reg 1 by width; P % 4 == 0"),
    ((9, 7, "star"), "8 x 33 = 264 items, the first fk_reg 0 by width on the 256-thread solve"),
    ((10, 2, "chain"), "10 levels, the last fk_reg 1 by depth"),
    ((11, 2, "chain"), "11 levels, the first fk_reg 0 by depth"),
    ((16, 2, "chain"), "16 ancestors = AVT_ANC_MAX; NT 4; the worst-conditioned row"),
    ((23, 15, "ternary"), "largest 256-thread system; mom_ntp 4, so k_moments<4>; S1 = 16; HS 88"),
    ((24, 13, "ternary"), "smallest 1024-thread system (HS 92, 23 blocks); moment form refused because P > 87; P % 4 == 0"),
    ((40, 4, "ternary"), "NT 8, the top of k_eval<0,0,8>"),
    ((40, 5, "ternary"), "NT 9, the first row-dealt k_eval"),
    ((45, 5, "ternary"), "NT 9 filled exactly"),
    ((45, 6, "ternary"), "NT 10"),
    ((50, 7, "ternary"), "NT 11 at its first column"),
    ((54, 11, "ternary"), "NT 12 at its first column"),
    ((54, 14, "ternary"), "the ABI's largest P with a wide shape block; HS 180, NR 45"),
    ((58, 2, "ternary"), "the ABI's largest P with the most joints"),
]
# by hand: (P, NT, HS, NR, k_solve threads, mom_ok, mom_ntp, fk_reg, MT of the k_eval<0, 0, MT, *> launch_eval takes, tree levels, most ancestors)
PROMISES = {
    (1, 1, "chain"): (7, 1, 8, 2, 256, True, 1, 1, 8, 1, 1),
    (3, 3, "star"): (15, 1, 16, 4, 256, True, 1, 1, 8, 2, 2),
    (4, 1, "star"): (16, 2, 20, 4, 256, True, 1, 1, 8, 2, 2),
    (4, 0, "chain"): (15, 1, 16, 4, 256, True, 1, 1, 8, 4, 4),
    (5, 16, "star"): (34, 3, 36, 9, 256, False, 4, 1, 8, 2, 2),
    (9, 4, "star"): (34, 3, 36, 9, 256, True, 1, 1, 8, 2, 2),
    (9, 6, "star"): (36, 3, 40, 9, 256, True, 2, 1, 8, 2, 2),
    (9, 7, "star"): (37, 3, 40, 10, 256, True, 2, 0, 8, 2, 2),
    (10, 2, "chain"): (35, 3, 36, 9, 256, True, 1, 1, 8, 10, 10),
    (11, 2, "chain"): (38, 3, 40, 10, 256, True, 1, 0, 8, 11, 11),
    (16, 2, "chain"): (53, 4, 56, 14, 256, True, 1, 0, 8, 16, 16),
    (23, 15, "ternary"): (87, 6, 88, 22, 256, True, 4, 0, 8, 4, 4),
    (24, 13, "ternary"): (88, 6, 92, 22, 1024, False, 3, 0, 8, 4, 4),
    (40, 4, "ternary"): (127, 8, 128, 32, 1024, False, 1, 0, 8, 4, 4),
    (40, 5, "ternary"): (128, 9, 132, 32, 1024, False, 2, 0, 9, 4, 4),
    (45, 5, "ternary"): (143, 9, 144, 36, 1024, False, 2, 0, 9, 5, 5),
    (45, 6, "ternary"): (144, 10, 148, 36, 1024, False, 2, 0, 10, 5, 5),
    (50, 7, "ternary"): (160, 11, 164, 40, 1024, False, 2, 0, 11, 5, 5),
    (54, 11, "ternary"): (176, 12, 180, 44, 1024, False, 3, 0, 12, 5, 5),
    (54, 14, "ternary"): (179, 12, 180, 45, 1024, False, 3, 0, 12, 5, 5),
    (58, 2, "ternary"): (179, 12, 180, 45, 1024, False, 1, 0, 12, 5, 5),
}
PROMISE_FIELDS = ("P", "NT", "HS", "NR", "threads", "mom_ok", "mom_ntp", "fk_reg", "eval_mt", "levels", "anc_max")
NCOMPS16 = [(9, 6, "star"), (24, 13, "ternary")]         # one 256-thread and one 1024-thread row also run with AVT_MAX_COMPS components
# a row whose frame misses a condition of tests/test_fit_dims_cpu.py gets another seed here: (J, K, tree, ncomps) -> seed
SEEDS = {(3, 3, "star", 3): 1, (4, 0, "chain", 3): 2, (5, 16, "star", 3): 1, (9, 4, "star", 0): 1, (9, 4, "star", 3): 2, (9, 6, "star", 16): 1,
         (24, 13, "ternary", 0): 1, (24, 13, "ternary", 3): 1, (24, 13, "ternary", 16): 3, (45, 5, "ternary", 0): 1, (45, 6, "ternary", 0): 2,
         (45, 6, "ternary", 3): 1, (50, 7, "ternary", 3): 1, (54, 11, "ternary", 0): 3, (54, 14, "ternary", 0): 2}      # (all: lambda_conditioning above KAPPA_MAX at seed 0)
# lambda is held to 1e-9 relative (tests/test_gpu_fit_dims.py).  The moment form makes the cost from expanded sums; allowed the 64 x 2^-53 of
# relative error the one-step bound allows the solve, lambda moves by kappa times that (lambda_conditioning): a factor 4 stays in hand
KAPPA_MAX = 1e-9 / 4 / (64 * 2.0 ** -53)
_CACHE = {}


def tree_parent(J, tree):
    p = np.full(J, -1, np.int64)
    for j in range(1, J):
        p[j] = j - 1 if tree == "chain" else 0 if tree == "star" else (j - 1) // 3
    return p


def tree_levels(parent):
    lv = np.zeros(len(parent), np.int64)
    for j in range(1, len(parent)):
        lv[j] = lv[parent[j]] + 1
    return lv


def promises(J, K, tree):
    """The same tuple as PROMISES holds, from the formulas: avt_model.cpp (NT, HS, mom_ntp, mom_ok, fk_reg), avt_lm.hip (solve_big, the round
    count of the LDL^T), avt_eval.hip (launch_eval)."""
    P = 3 + 3 * J + K
    NT = (P + 1 + 15) // 16
    HS = 4 * ((P + 4) // 4)
    NR = (P + 3) // 4
    big = HS // 4 > 22
    lv = tree_levels(tree_parent(J, tree))
    widest = int(np.bincount(lv).max()) * (12 + 3 * K)
    fk_reg = int(lv.max() + 1 <= LEVELS_REG and widest <= TITEM_THREADS)
    return (P, NT, HS, NR, 1024 if big else 256, K + 1 <= 16 and not big, (3 * (K + 1) + 1 + 15) // 16, fk_reg, 8 if NT <= 8 else NT,
            int(lv.max()) + 1, int(lv.max()) + 1)       # (every joint has vertices of its own: the deepest joint's chain is the longest ancestor list)


def cases():
    """[(J, K, tree, ncomps)] of the table: ncomps 0 and 3 (0 only where J = 1), 16 on the two rows of NCOMPS16."""
    out = []
    for (J, K, tree), _ in ROWS:
        out += [(J, K, tree, nc) for nc in ((0,) if J == 1 else (0, 3))]
        if (J, K, tree) in NCOMPS16:
            out.append((J, K, tree, MAX_COMPS))
    return out


def case_id(case):
    J, K, tree, nc = case
    return f"J{J}-K{K}-{tree}-nc{nc}"


def _quats(rng, J, s):
    """J quaternions (x, y, z, w): angle s N(0, 1) about a random axis"""
    q = np.zeros((J, 4))
    for j in range(J):
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        a = s * rng.standard_normal()
        q[j] = np.concatenate([np.sin(a / 2) * ax, [np.cos(a / 2)]])
    return q


def fit_model(J, K, tree, ncomps=0, seed=0, per_joint=PER_JOINT):
    """per_joint: vertices per joint (the table's rows keep PER_JOINT; tests/data_term_cases.py asks for more)"""
    key = (J, K, tree, ncomps, seed) if per_joint == PER_JOINT else (J, K, tree, ncomps, seed, per_joint)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng([20261019, J, K, seed])
    parent = tree_parent(J, tree)
    jpos = np.zeros((J, 3))
    for j in range(1, J):
        d = rng.standard_normal(3)
        jpos[j] = jpos[parent[j]] + 0.25 * d / np.linalg.norm(d)
    V = per_joint * J
    vt = np.zeros((V, 3))
    rows, cols, vals = [], [], []
    for j in range(J):
        for i in range(per_joint):
            v = j * per_joint + i
            vt[v] = jpos[j] + 0.12 * rng.standard_normal(3)
            if parent[j] >= 0 and i % 3 == 0:           # shared with the parent
                a = rng.uniform(0.6, 0.9)
                rows += [v, v]; cols += [int(parent[j]), j]; vals += [1 - a, a]
            else:
                rows.append(v); cols.append(j); vals.append(1.0)
    W = sp.csr_matrix((np.array(vals), (np.array(rows), np.array(cols))), shape=(V, J))
    Jr = np.zeros((J, V))
    for j in range(J):
        Jr[j, j * per_joint:(j + 1) * per_joint] = 1.0 / per_joint
    faces = rng.integers(0, V, (max(1, V // 2), 3))      # unused: the fits run with enable_occlusion = 0
    m = dict(v_template=vt, f=faces, kintree_table=np.stack([parent, np.arange(J)]), J_regressor=Jr, weights=W,
             shapedirs=rng.normal(0.0, 0.02, (V, 3, K)))
    if ncomps and J > 1:
        nd = 3 * (J - 1)
        prng = np.random.default_rng([20261019, J, K, seed, ncomps])
        cov = np.zeros((ncomps, nd, nd))
        weight, mean = prng.dirichlet(np.ones(ncomps)), 0.1 * prng.standard_normal((ncomps, nd))
        for c in range(ncomps):
            A = prng.standard_normal((nd, nd)) / np.sqrt(nd)
            cov[c] = 0.05 * (np.eye(nd) + 0.3 * A @ A.T)
        m.update(prior_weight=weight, prior_mean=mean, prior_cov=cov)
    _CACHE[key] = m
    return m


def case_model(case):
    J, K, tree, nc = case
    return fit_model(J, K, tree, nc, SEEDS.get(case, 0))


def fit_frame(model, om, seed=0):
    """One frame for `model` (om: its OracleModel, for the forward model and the main joints): dict(data (V, 3), labels, part_map, num_parts,
    start (p, q, w), gt (p, q, w), betas (beta_pose, beta_shape))."""
    J, K, V = om.J, om.K, om.V
    rng = np.random.default_rng([20261019, 3, J, K, seed])
    pg, qg, wg = 0.05 * rng.standard_normal(3), _quats(rng, J, 0.15), 0.5 * rng.standard_normal(K)
    data = om.points(pg, qg, wg) + 0.002 * rng.standard_normal((V, 3))
    # the device sums the matched data points in 2^-40 fixed point about the frame's first point (avt_nn.hip, AVT_FIX_SCALE): data on that grid
    # reach its data term exactly, and the one-step test measures the solve, not 1e-12 of input rounding
    data = np.rint(data * 2.0 ** 40) / 2.0 ** 40
    start = (np.zeros(3), _quats(rng, J, 0.02), np.zeros(K))
    betas = (0.05, 0.12) if model.get("prior_weight") is not None else (0.0, 0.12)
    return dict(data=np.ascontiguousarray(data), labels=om.main_joint().astype(np.int32), part_map=np.arange(J, dtype=np.int32), num_parts=J,
                start=start, gt=(pg, qg, wg), betas=betas)


def case_frame(case, om):
    return fit_frame(case_model(case), om, SEEDS.get(case, 0))


# ---- what both test files need of a case, computed once with the CPU oracle ---------------------------------------------------------------
_STUDY = {}


def options(fr, **kw):
    """Options.demo with the frame's betas, occlusion off"""
    from avatar_amd.capi import Options
    return Options.demo(enable_occlusion=0, beta_pose=fr["betas"][0], beta_shape=fr["betas"][1], **kw)


def state_distance(a, b):
    """largest absolute difference of two states (p, q, w)"""
    return max(float(np.abs(np.asarray(x, np.float64).ravel() - np.asarray(y, np.float64).ravel()).max()) if np.size(x) else 0.0 for x, y in zip(a, b))


def study_frame(m, om, fr):
    """What study() holds of a case, for any model m (om: its OracleModel) and frame fr of it."""
    import fit_restatement as fr_
    p0, q0, w0 = fr["start"]
    opt1 = options(fr, icp_iters=1, max_iters_per_icp=1)
    step1 = om.optimize(fr["part_map"], fr["num_parts"], fr["data"], fr["labels"], opt1, p0, q0, w0, aggregate=1)
    cost, g, H, _ = om.evaluate(p0, q0, w0, step1["corr"], fr["data"], fr["betas"][0], fr["betas"][1], aggregate=1)
    lam = opt1.lm_lambda0
    A = H + lam * np.diag(np.diag(H))
    s = dict(model=m, om=om, frame=fr, corr=step1["corr"], H=H, g=g, cost=cost, lam=lam, A=A, step1=step1)
    if (np.diag(H) > 0).all():
        s["cond"] = float(np.linalg.cond(A))
        delta, piv, pred = fr_.lm_step_ld(H, g, lam)
        s.update(delta_ld=delta, pivots=piv, pred=pred, target=om.retract(p0, q0, w0, delta))
        s["bound"] = 64.0 * s["cond"] * 2.0 ** -53 * float(np.abs(delta).max())
        s["e_oracle"] = state_distance((step1["p"], step1["q"], step1["w"]), s["target"])
    return s


def study(case):
    """dict of the case: model, om (OracleModel), frame, and at the start state with the oracle's correspondences of the first ICP iteration:
    corr, H, g (with the betas, aggregate = 1), A = H + lambda0 D, cond, delta_ld / pivots / pred (fit_restatement.lm_step_ld), target =
    retract(start, delta_ld), bound = 64 cond(A) 2^-53 max|delta_ld|, step1 (the oracle's one-iteration run), e_oracle (its distance from target)."""
    if case in _STUDY:
        return _STUDY[case]
    from oracle import oracle as orc
    m = case_model(case)
    om = orc.OracleModel(m)
    s = study_frame(m, om, case_frame(case, om))
    s["case"] = case
    _STUDY[case] = s
    return s


REFUSED = [(9, 7, "star", 0), (24, 13, "ternary", 0)]


def refused_frame(case, om):
    """The case's frame with the data points of the last (a leaf) joint labelled -1 and no shape prior: the leaf's rotation has no rows,
    H + lambda diag(H) is singular at every lambda and every factorisation is refused."""
    fr = dict(case_frame(case, om))
    labels = fr["labels"].copy()
    labels[labels == om.J - 1] = -1
    fr.update(labels=labels, betas=(0.0, 0.0))
    return fr


def lambda_conditioning(case):
    """(lambda, kappa) of the oracle's fit (2 ICP x 4 GN iterations) replayed step by step with OracleModel.evaluate / retract: lambda as the
    gain-ratio schedule leaves it, and kappa = sum over the accepted steps whose factor 1 - (2 rho - 1)^3 is not clamped of
    |d ln lambda / d eps| for a relative error eps in each of the step's two costs: rho = (c0 - c1) / pred moves by eps rho (c0 + c1) / (c0 - c1),
    the factor by 6 u^2 times that.  A fit whose last steps shave 1e-6 off the cost has kappa ~ 1e6: its lambda says more about the last bits
    of the cost than about the kernels."""
    s = study(case)
    r = replay_fit(s["om"], s["frame"])
    return r["lam"], r["kappa"]


def replay_fit(om, fr, max_iters_per_icp=4):
    """lambda_conditioning's replay for any frame fr of om's model (2 ICP x max_iters_per_icp GN iterations): dict(lam, kappa, acc (1 accepted / 0 rejected / -1 not factorable, per GN
    iteration), states (the start and the state behind every accepted step), icp_states (the state each ICP iteration's correspondences are
    searched at), comps ((minimising mixture component at the current point, at the trial point) per factorable GN iteration; -1 without a prior))."""
    bp, bs = fr["betas"]
    opt = options(fr, icp_iters=2, max_iters_per_icp=max_iters_per_icp)
    p, q, w = (np.array(x, np.float64) for x in fr["start"])
    lam, nu, kappa = opt.lm_lambda0, opt.lm_up, 0.0
    acc, states, icp_states, comps = [], [(p, q, w)], [], []
    for icp in range(opt.icp_iters):
        icp_states.append((p, q, w))
        corr = om.optimize(fr["part_map"], fr["num_parts"], fr["data"], fr["labels"], options(fr, icp_iters=1, max_iters_per_icp=0), p, q, w, aggregate=1)["corr"]
        c, g, H, comp = om.evaluate(p, q, w, corr, fr["data"], bp, bs, aggregate=1)
        for it in range(opt.max_iters_per_icp):
            D = np.diag(H)
            try:
                L = np.linalg.cholesky(H + lam * np.diag(D))
            except np.linalg.LinAlgError:
                lam = min(lam * nu, opt.lm_lambda_max); nu *= 2.0
                acc.append(-1)
                continue
            d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            p2, q2, w2 = om.retract(p, q, w, d)
            c2, g2, H2, comp2 = om.evaluate(p2, q2, w2, corr, fr["data"], bp, bs, aggregate=1)
            comps.append((comp, comp2))
            if c2 < c:
                pred = 0.5 * float((d * (lam * D * d - g)).sum())
                rho = (c - c2) / pred
                u = 2.0 * rho - 1.0
                f = 1.0 - u ** 3
                if f > opt.lm_down:
                    kappa += 6.0 * u * u * rho * (c + c2) / (c - c2) / f
                lam = min(max(lam * max(opt.lm_down, f), opt.lm_lambda_min), opt.lm_lambda_max)
                nu = opt.lm_up
                done = opt.function_tolerance > 0.0 and (c - c2) <= opt.function_tolerance * c
                p, q, w, c, g, H, comp = p2, q2, w2, c2, g2, H2, comp2
                acc.append(1)
                states.append((p, q, w))
                if done:
                    break
            else:
                lam = min(lam * nu, opt.lm_lambda_max); nu *= 2.0
                acc.append(0)
    return dict(lam=lam, kappa=kappa, acc=acc, states=states, icp_states=icp_states, comps=comps)
