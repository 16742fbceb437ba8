"""The fitting kernels at the edges of their STATE space (tests/state_cases.py; tests/test_state_edges_cpu.py proves with the oracle alone
that every case is what its name says): the retraction of k_solve on both sides of |d|^2 = 1/4 (Horner chains / library sin and cos), the
quaternion -> angle-axis conversion of avt_prior.h on its small-norm, zero-norm, w < 0 and w = +-0 branches in k_eval's extra workgroups,
k_pairpass and k_prior, the reload of the prior when the minimising component changes with the step, and w crossing zero.  Through the
existing ABI only, enable_occlusion = 0, max_points = the frame's points; launch shapes as tests/test_gpu_fit_dims.py (1, 3 and 7 frames,
the row form, the moment form where the model has one).

  a  one step against the long-double restatement: state_distance <= min(64 cond(A) 2^-53 max|delta|, 1e-9), accepted 1 of 1, the oracle's
     correspondences; quaternions compared as given, not up to sign
  b  the 2 ICP x 4 GN fit against the oracle at the bars of test_fit_matches_oracle (cost 1e-8, lambda 1e-9, p and q 1e-6, w 1e-5, equal
     step counts), the objective trace of the last ICP iteration at 1e-8, the launch shapes among themselves to 1e-9, the replayed graph
     and the two assemblies of the moment form bit for bit
  c  hemisphere symmetry: from a start with negated quaternions p, w, the statistics and the objective trace are bit for bit those of the
     plain start, q is the plain start's with the sign flipped on exactly the negated joints
  d  seven frames carrying different scenarios in one launch: each equals its single-frame run to 1e-9 with equal step counts
  e  nothing not finite anywhere: states, costs, lambda, the normal equations"""
import numpy as np
import pytest

import fit_models as fm
import state_cases as sc

pytestmark = pytest.mark.gpu

CASES = sc.cases()
IDS = [sc.case_id(c) for c in CASES]
STEP_CASES = [c for c in CASES if c[1] in sc.ONE_STEP]
NEG = [c for c in CASES if "neg" in c[1]]
FRAMES = (1, 3, 7)
SHAPE_BAR = 1e-9
MIXED = ("big", "ident", "cross", "big-negall", "pi", "ident-eps", "cross-neghalf")        # one launch, seven frames
_FITS = {}


@pytest.fixture(scope="module")
def gmodels(gmodel):
    from avatar_amd import api
    made = {sc.SMPL: gmodel}

    def get(row):
        if row not in made:
            made[row] = api.AvatarModel(fm.case_model(row))
        return made[row]
    return get


def _mom_ok(row):
    return row == sc.SMPL or dict(zip(fm.PROMISE_FIELDS, fm.PROMISES[row[:3]]))["mom_ok"]


def _threads(row):
    return 256 if row == sc.SMPL else dict(zip(fm.PROMISE_FIELDS, fm.PROMISES[row[:3]]))["threads"]


def _forms(row):
    """[(name, data term, tuning)] as tests/test_gpu_fit_dims.py: rows and moments where the model has the moment form; else rows, and AUTO
    told to prefer moments"""
    from avatar_amd import api
    C = api.Context
    if _mom_ok(row):
        return [("rows", C.DATA_TERM_ROWS, {}), ("moments", C.DATA_TERM_MOMENTS, {})]
    return [("rows", C.DATA_TERM_ROWS, {}), ("auto", C.DATA_TERM_AUTO, dict(mom_min_frames=1))]


def _context(gm, frs, form, tuning):
    from avatar_amd import api
    ctx = api.Context(gm, frs[0]["num_parts"], frs[0]["part_map"], max(len(f["labels"]) for f in frs), len(frs), device=0)
    if tuning:
        ctx.set_tuning(**tuning)
    ctx.set_data_term(form)
    return ctx


def _run(ctx, frs, opt, trace=0):
    """one optimize over the frames frs (one dict each): p, q, w, stats, correspondences, objective traces"""
    ctx.frames_upload([f["data"] for f in frs], [f["labels"] for f in frs])
    ctx.state_upload(np.stack([f["start"][0] for f in frs]), np.stack([f["start"][1] for f in frs]), np.stack([f["start"][2] for f in frs]))
    ctx.optimize_resident(opt)
    p, q, w, st = ctx.state_download()
    return p, q, w, st, [ctx.correspondences(i, len(f["labels"])) for i, f in enumerate(frs)], [ctx.cost_trace(i, n=trace)[:st[i].gn_iterations + 1] for i in range(len(frs))]


def _stats(s):
    return (s.gn_iterations, s.accepted_steps, s.initial_cost, s.final_cost, s.lambda_)


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and all(np.array_equal(x, y) for x, y in zip(a[4], b[4])) and \
        all(np.array_equal(x, y) for x, y in zip(a[5], b[5])) and all(_stats(s) == _stats(t) for s, t in zip(a[3], b[3]))


def _finite(out, f, ctx=None):
    p, q, w, st = out[:4]
    if ctx is not None:
        H, g, cost = ctx.normal_equations(f)
        if not (np.isfinite(H).all() and np.isfinite(g).all() and np.isfinite(cost)):
            return False
    return bool(np.isfinite(p[f]).all() and np.isfinite(q[f]).all() and np.isfinite(w[f]).all() and np.isfinite(_stats(st[f])).all() and np.isfinite(out[5][f]).all())


def _fit_opt(fr):
    return fm.options(fr, icp_iters=2, max_iters_per_icp=4)


def _fit(gmodels, case, nf, fname):
    """the 2 x 4 fit of nf copies of the case's frame in the form `fname`, once per process: dict(out (of _run), finite (per frame, the normal
    equations included), replay / asm (the second run on the cached graph / the other assembly of the moment form repeats the bits), shape
    (Context.launch_shape))"""
    key = (case, nf, fname)
    if key not in _FITS:
        fr = sc.frame(case)
        _, form, tun = next(x for x in _forms(case[0]) if x[0] == fname)
        ctx = _context(gmodels(case[0]), [fr] * nf, form, tun)
        out = _run(ctx, [fr] * nf, _fit_opt(fr), trace=9)
        res = dict(out=out, finite=[_finite(out, f, ctx) for f in range(nf)], asm=True, shape=ctx.launch_shape())
        res["replay"] = _same_bits(_run(ctx, [fr] * nf, _fit_opt(fr), trace=9), out)
        if fname == "moments":
            assert ctx.tuning().asm_parts == 1
            ctx.set_tuning(asm_parts=0)       # (k_assemble where its LDS fits; the role workgroups again where it does not)
            res["asm"] = _same_bits(_run(ctx, [fr] * nf, _fit_opt(fr), trace=9), out)
        _FITS[key] = res
    return _FITS[key]


@pytest.mark.parametrize("case", STEP_CASES, ids=[sc.case_id(c) for c in STEP_CASES])
def test_one_step_against_long_double(gmodels, case):
    """a and e of the module's docstring."""
    s = sc.study(case)
    fr = s["frame"]
    bound = min(s["bound"], 1e-9)
    opt = fm.options(fr, icp_iters=1, max_iters_per_icp=1)
    failures, worst = [], 0.0
    for nf in FRAMES:
        for fname, form, tun in _forms(case[0]):
            ctx = _context(gmodels(case[0]), [fr] * nf, form, tun)
            out = _run(ctx, [fr] * nf, opt, trace=2)
            p, q, w, st, corr, _ = out
            for f in range(nf):
                tag = f"{nf} frames/{fname} frame {f}"
                if not _finite(out, f, ctx):
                    failures.append(f"{tag}: something is not finite")
                    continue
                if not np.array_equal(corr[f], s["corr"]):
                    failures.append(f"{tag}: {int((corr[f] != s['corr']).sum())} correspondences differ from the oracle's")
                    continue
                if (st[f].accepted_steps, st[f].gn_iterations) != (1, 1):
                    failures.append(f"{tag}: accepted {st[f].accepted_steps} of {st[f].gn_iterations}")
                e = fm.state_distance((p[f], q[f], w[f]), s["target"])           # (quaternions as given: a wrong sign is a distance of 2 |q|)
                worst = max(worst, e)
                if not e <= bound:
                    failures.append(f"{tag}: {e:.2e} from the long-double step, bound {bound:.2e}")
    z = sc.step_z(case)
    print(f"STATEEDGES step {sc.case_id(case)} z>=1/4 {int((z >= 0.25).sum())}/{len(z)} E_oracle {s['e_oracle']:.2e} bound {bound:.2e} gpu {worst:.2e}")
    assert not failures, f"{sc.case_id(case)}: " + "; ".join(failures[:12])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fit_matches_oracle(gmodels, case):
    """b and e of the module's docstring."""
    s = sc.study(case)
    fr, ref = s["frame"], s["fit"]
    rs = ref["stats"]
    K = s["om"].K
    acc = [int(a) for a in ref["trace_acc"]]
    n1, n2 = sum(a != -2 for a in acc[:4]), sum(a != -2 for a in acc[4:])
    ref_trace = ref["trace_cost"][5:5 + n2 + 1]
    failures, worst, worst_tr = [], 0.0, 0.0
    for nf in FRAMES:
        for fname, form, tun in _forms(case[0]):
            res = _fit(gmodels, case, nf, fname)
            out = res["out"]
            p, q, w, st, corr, tr = out
            one = _fit(gmodels, case, 1, fname)["out"]
            # the component and slot handling differs between the riding and the batch shapes: one frame rides, seven are a batch, three ride
            # in one group each where the solve has 256 threads (tests/test_gpu_fit_dims.py)
            if fname == "rows" and nf == 3:
                assert (res["shape"][0] == 3) == (_threads(case[0]) == 256), (res["shape"], nf)
            if nf != 3:
                assert (res["shape"][2] >= 64) == (nf == 1), (res["shape"], nf)
            for f in range(nf):
                tag = f"{nf} frames/{fname} frame {f}"
                if not res["finite"][f]:
                    failures.append(f"{tag}: something is not finite")
                    continue
                if not np.array_equal(corr[f], ref["corr"]):
                    failures.append(f"{tag}: {int((corr[f] != ref['corr']).sum())} correspondences differ from the oracle's")
                if (st[f].gn_iterations, st[f].accepted_steps) != (rs.gn_iterations, rs.accepted_steps):
                    failures.append(f"{tag}: accepted {st[f].accepted_steps} of {st[f].gn_iterations}, the oracle {rs.accepted_steps} of {rs.gn_iterations}")
                    continue
                ec = abs(st[f].final_cost - rs.final_cost) / abs(rs.final_cost)
                el = abs(st[f].lambda_ - rs.lambda_) / abs(rs.lambda_)
                ep, eq = float(np.abs(p[f] - ref["p"]).max()), float(np.abs(q[f] - ref["q"]).max())
                ew = float(np.abs(w[f] - ref["w"]).max()) if K else 0.0
                et = float(np.abs(tr[f][n1:n1 + n2 + 1] / ref_trace - 1.0).max())
                worst, worst_tr = max(worst, ep, eq, ew), max(worst_tr, et)
                if not (ec < 1e-8 and el < 1e-9 and ep < 1e-6 and eq < 1e-6 and ew < 1e-5 and et < 1e-8):
                    failures.append(f"{tag}: cost {ec:.2e} lambda {el:.2e} p {ep:.2e} q {eq:.2e} w {ew:.2e} trace {et:.2e} from the oracle")
                es = fm.state_distance((p[f], q[f], w[f]), (one[0][0], one[1][0], one[2][0]))
                if not (es <= SHAPE_BAR and (st[f].gn_iterations, st[f].accepted_steps) == (one[3][0].gn_iterations, one[3][0].accepted_steps)):
                    failures.append(f"{tag}: {es:.2e} from the single-frame run")
            if not res["replay"]:        # the cached graph replayed
                failures.append(f"{nf} frames/{fname}: the second run differs from the first")
            if not res["asm"]:
                failures.append(f"{nf} frames/moments: asm_parts 0 differs from asm_parts 1")
    print(f"STATEEDGES fit {sc.case_id(case)} accepted {rs.accepted_steps}/{rs.gn_iterations} acc {[a for a in acc if a != -2]} gpu-oracle {worst:.2e} trace {worst_tr:.2e}")
    assert not failures, f"{sc.case_id(case)}: " + "; ".join(failures[:12])


@pytest.mark.parametrize("case", NEG, ids=[sc.case_id(c) for c in NEG])
def test_negated_start_is_the_same_fit(gmodels, case):
    """c of the module's docstring.  q -> -q of one joint leaves its rotation matrix (even in q), the angle-axis vector of the prior
    (|xyz|, |w| and the axis xyz / (+-|xyz|) with the sign of w: even) and the Jacobians alone, and negates the retracted quaternion
    (delta q x q: odd), operation by operation - IEEE negation commutes with every rounding - so nothing but the sign may differ."""
    fr = sc.frame(case)
    sign = np.where(fr["negated"], -1.0, 1.0)[None, :, None]
    failures = []
    for nf in FRAMES:
        for fname, _, _ in _forms(case[0]):
            a, b = _fit(gmodels, case, nf, fname)["out"], _fit(gmodels, fr["plain"], nf, fname)["out"]
            flipped = (b[0], sign * b[1]) + tuple(b[2:])
            if not _same_bits(a, flipped):
                dq = float(np.abs(a[1] - flipped[1]).max())
                failures.append(f"{nf} frames/{fname}: p {float(np.abs(a[0] - b[0]).max()):.2e} q {dq:.2e} lambda {a[3][0].lambda_} / {b[3][0].lambda_} "
                                f"steps {a[3][0].accepted_steps}/{a[3][0].gn_iterations} / {b[3][0].accepted_steps}/{b[3][0].gn_iterations}")
    print(f"STATEEDGES neg {sc.case_id(case)} negated {int(fr['negated'].sum())}/{len(fr['negated'])} joints: {'bit for bit' if not failures else 'DIFFERS'}")
    assert not failures, f"{sc.case_id(case)}: " + "; ".join(failures[:12])


@pytest.mark.parametrize("row", sc.ROWS, ids=[sc.row_id(r) for r in sc.ROWS])
def test_mixed_batch_equals_the_single_frames(gmodels, row):
    """d of the module's docstring: the per-lane and per-workgroup branches diverge inside one launch."""
    cases = [(row, sn) for sn in MIXED]
    frs = [sc.frame(c) for c in cases]
    failures, worst = [], 0.0
    for fname, form, tun in _forms(row):
        ctx = _context(gmodels(row), frs, form, tun)
        out = _run(ctx, frs, _fit_opt(frs[0]), trace=9)
        p, q, w, st = out[:4]
        for f, case in enumerate(cases):
            one = _fit(gmodels, case, 1, fname)["out"]
            tag = f"{fname} frame {f} ({case[1]})"
            if not _finite(out, f):
                failures.append(f"{tag}: something is not finite")
                continue
            es = fm.state_distance((p[f], q[f], w[f]), (one[0][0], one[1][0], one[2][0]))
            worst = max(worst, es)
            if not np.array_equal(out[4][f], one[4][0]):
                failures.append(f"{tag}: correspondences differ from the single-frame run's")
            if not (es <= SHAPE_BAR and (st[f].gn_iterations, st[f].accepted_steps) == (one[3][0].gn_iterations, one[3][0].accepted_steps)):
                failures.append(f"{tag}: {es:.2e} from the single-frame run, accepted {st[f].accepted_steps}/{st[f].gn_iterations} for {one[3][0].accepted_steps}/{one[3][0].gn_iterations}")
    print(f"STATEEDGES mixed {sc.row_id(row)} {len(cases)} scenarios in one launch, from the single frames {worst:.2e}")
    assert not failures, f"{sc.row_id(row)}: " + "; ".join(failures[:12])
