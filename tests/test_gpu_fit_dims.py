"""The fitting kernels (avt_eval.hip k_eval / k_reduce*, avt_lm.hip k_solve, avt_moments.hip k_moments / k_pairpass / k_assemble* / k_prior,
avt_prep.h) at every system size and kernel variant the ABI accepts: the table of tests/fit_models.py, whose conditions
tests/test_fit_dims_cpu.py checks with the oracle alone.  Every fit runs with enable_occlusion = 0 on a context with max_points = V.

  a  one step against the long-double restatement (tests/fit_restatement.py): isolates k_solve, the retraction and the skeleton pass from
     the oracle's Cholesky; bound = 64 cond(A) 2^-53 max|delta| with A = H + lambda0 D (the forward error of a backward-stable LDL^T; the
     64 stands in for the dimension factor and the kernel's Newton reciprocals), never above 1e-9
  b  the normal equations at the returned state against the oracle's, 1e-9 relative, H exactly symmetric
  c  the fit (2 ICP x 4 GN iterations) against the oracle at the bars of test_52_joint_model_matches_oracle; 1, 3 and 7 frames agree to 1e-9;
     the cached graph repeats the first run bit for bit; the two assemblies of the moment form agree bit for bit
  d  avt_set_data_term(MOMENTS) is refused where the model has no moment form, AUTO keeps the row form
  e  a refused factorisation away from SMPL returns the state bit for bit"""
import numpy as np
import pytest

import fit_models as fm

pytestmark = pytest.mark.gpu

CASES = fm.cases()
IDS = [fm.case_id(c) for c in CASES]
FRAMES = (1, 3, 7)            # the few-frames shape (riding, for the 256-thread solve), three frame groups / strips, the batch shape
SHAPE_BAR = 1e-9              # the same frame through different launch shapes (tests/test_gpu_parity_more.py)


@pytest.fixture(scope="module")
def gmodels():
    from avatar_amd import api
    made = {}

    def get(case):
        if case not in made:
            made[case] = api.AvatarModel(fm.case_model(case))
        return made[case]
    return get


def _promise(case):
    return dict(zip(fm.PROMISE_FIELDS, fm.PROMISES[case[:3]]))


def _forms(case):
    """[(name, data term, tuning)]: rows and moments where the model has the moment form; else rows, and AUTO told to prefer moments"""
    from avatar_amd import api
    C = api.Context
    if _promise(case)["mom_ok"]:
        return [("rows", C.DATA_TERM_ROWS, {}), ("moments", C.DATA_TERM_MOMENTS, {})]
    return [("rows", C.DATA_TERM_ROWS, {}), ("auto", C.DATA_TERM_AUTO, dict(mom_min_frames=1))]


def _context(gm, fr, nf, form, tuning):
    from avatar_amd import api
    ctx = api.Context(gm, fr["num_parts"], fr["part_map"], len(fr["labels"]), nf, device=0)
    if tuning:
        ctx.set_tuning(**tuning)
    ctx.set_data_term(form)
    return ctx


def _run(ctx, fr, nf, opt):
    p0, q0, w0 = fr["start"]
    ctx.frames_upload([fr["data"]] * nf, [fr["labels"]] * nf)
    ctx.state_upload(np.repeat(p0[None], nf, 0), np.repeat(q0[None], nf, 0), np.repeat(w0[None], nf, 0))
    ctx.optimize_resident(opt)
    p, q, w, st = ctx.state_download()
    return p, q, w, st, [ctx.correspondences(f, len(fr["labels"])) for f in range(nf)]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and all(np.array_equal(x, y) for x, y in zip(a[4], b[4])) and \
        all((s.gn_iterations, s.accepted_steps, s.final_cost, s.lambda_) == (t.gn_iterations, t.accepted_steps, t.final_cost, t.lambda_) for s, t in zip(a[3], b[3]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_step_against_long_double(gmodels, case):
    """a and b of the module's docstring."""
    s = fm.study(case)
    fr, om = s["frame"], s["om"]
    bound = min(s["bound"], 1e-9)
    opt = fm.options(fr, icp_iters=1, max_iters_per_icp=1)
    failures, worst, worst_ne = [], 0.0, 0.0
    for nf in FRAMES:
        for fname, form, tun in _forms(case):
            ctx = _context(gmodels(case), fr, nf, form, tun)
            p, q, w, st, corr = _run(ctx, fr, nf, opt)
            for f in range(nf):
                tag = f"{nf} frames/{fname} frame {f}"
                if not np.array_equal(corr[f], s["corr"]):
                    failures.append(f"{tag}: {int((corr[f] != s['corr']).sum())} correspondences differ from the oracle's")
                    continue
                if (st[f].accepted_steps, st[f].gn_iterations) != (1, 1):
                    failures.append(f"{tag}: accepted {st[f].accepted_steps} of {st[f].gn_iterations}")
                e = fm.state_distance((p[f], q[f], w[f]), s["target"])
                worst = max(worst, e)
                if not e <= bound:
                    failures.append(f"{tag}: {e:.2e} from the long-double step, bound {bound:.2e}")
                H, g, cost = ctx.normal_equations(f)
                oc, og, oH, _ = om.evaluate(p[f], q[f], w[f], corr[f], fr["data"], 0.0, 0.0, aggregate=0)
                eh, eg = float(np.abs(H - oH).max() / np.abs(oH).max()), float(np.abs(g - og).max() / max(1.0, np.abs(og).max()))
                worst_ne = max(worst_ne, eh, eg)
                if not (eh < 1e-9 and eg < 1e-9):
                    failures.append(f"{tag}: normal equations off by {eh:.2e} (H), {eg:.2e} (g)")
                if not np.array_equal(H, H.T):
                    failures.append(f"{tag}: H is not symmetric ({int((H != H.T).sum())} entries)")
    print(f"FITDIMS step {fm.case_id(case)} E_oracle {s['e_oracle']:.2e} bound {s['bound']:.2e} gpu {worst:.2e} normal_equations {worst_ne:.2e}")
    assert not failures, f"{fm.case_id(case)}: " + "; ".join(failures[:12])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fit_matches_oracle(gmodels, case):
    """c and d of the module's docstring; the launch shape and the refusal cross-check the row's promises (solve shape, mom_ok).

    What this test found (MI355X, before the fix of backsub_chain in avt_lm.hip): 33 of the 43 cases agreed with the oracle's fit to 4.7e-15,
    the 10 cases of 256-thread solves with HS <= 56 whose gain ratio matters did not - the same figures on 1, 3 and 7 frames and both forms
    (state / relative lambda from the oracle): J3-K3-star-nc3 5.1e-07 / 0.69, J4-K0-chain-nc3 1.2e-06 / 0.94, J5-K16-star-nc3 4.4e-16 / 0.57,
    J9-K4-star-nc0 6.0e-08 / 0.63, J9-K4-star-nc3 7.0e-07 / 0.71, J9-K6-star-nc16 1.6e-07 / 0.08, J11-K2-chain-nc3 2.6e-06 / 0.013,
    J16-K2-chain-nc3 9.5e-04 / 0.59; J10-K2-chain-nc0 accepted 6 of 6 for the oracle's 7 of 7, J11-K2-chain-nc0 6 of 6 for 8 of 8.  Cause: all
    64 lanes of the back substitution stored an unknown; below 62 rows the lanes past the last block wrote behind s_delta, into the gradient
    and diagonal the predicted decrease is formed from.  Rows (40, 5) and (50, 7) then failed now and then, every step refused or rejected: with
    P a multiple of four the 1024-thread back substitution began at the block that holds row P alone, which no round factors (backsub_tri)."""
    from avatar_amd import api
    s = fm.study(case)
    fr, om = s["frame"], s["om"]
    pr = _promise(case)
    opt = fm.options(fr, icp_iters=2, max_iters_per_icp=4)
    ref = om.optimize(fr["part_map"], fr["num_parts"], fr["data"], fr["labels"], opt, *fr["start"], aggregate=1)
    rs = ref["stats"]
    failures, worst = [], 0.0
    results = {}
    for nf in FRAMES:
        for fname, form, tun in _forms(case):
            ctx = _context(gmodels(case), fr, nf, form, tun)
            if not pr["mom_ok"]:        # d
                with pytest.raises(api.AvtError) as err:
                    ctx.set_data_term(api.Context.DATA_TERM_MOMENTS)
                assert "no moment form" in str(err.value) and ("K + 1 <= 16" if case[1] + 1 > 16 else "3 + 3J + K <= 87") in str(err.value), str(err.value)
                assert ctx.data_term() == form
            out = _run(ctx, fr, nf, opt)
            p, q, w, st, corr = out
            if fname == "rows" and nf == 3:      # two and three frames run one group each where the solve rides: the 256-thread solves do
                assert (ctx.launch_shape()[0] == 3) == (pr["threads"] == 256), (ctx.launch_shape(), pr["threads"])
            if nf != 3:
                assert (ctx.launch_shape()[2] >= 64) == (nf == 1), ctx.launch_shape()
            results[(nf, fname)] = out
            for f in range(nf):
                tag = f"{nf} frames/{fname} frame {f}"
                if not np.array_equal(corr[f], ref["corr"]):
                    failures.append(f"{tag}: {int((corr[f] != ref['corr']).sum())} correspondences differ from the oracle's")
                if (st[f].gn_iterations, st[f].accepted_steps) != (rs.gn_iterations, rs.accepted_steps):
                    failures.append(f"{tag}: accepted {st[f].accepted_steps} of {st[f].gn_iterations}, the oracle {rs.accepted_steps} of {rs.gn_iterations}")
                ec = abs(st[f].final_cost - rs.final_cost) / abs(rs.final_cost)
                el = abs(st[f].lambda_ - rs.lambda_) / abs(rs.lambda_)
                ep, eq = float(np.abs(p[f] - ref["p"]).max()), float(np.abs(q[f] - ref["q"]).max())
                ew = float(np.abs(w[f] - ref["w"]).max()) if case[1] else 0.0
                worst = max(worst, ep, eq, ew)
                if not (ec < 1e-8 and el < 1e-9 and ep < 1e-6 and eq < 1e-6 and ew < 1e-5):
                    failures.append(f"{tag}: cost {ec:.2e} lambda {el:.2e} p {ep:.2e} q {eq:.2e} w {ew:.2e} from the oracle")
                one = results[(1, fname)]
                es = fm.state_distance((p[f], q[f], w[f]), (one[0][0], one[1][0], one[2][0]))
                if not (es <= SHAPE_BAR and (st[f].gn_iterations, st[f].accepted_steps) == (one[3][0].gn_iterations, one[3][0].accepted_steps)):
                    failures.append(f"{tag}: {es:.2e} from the single-frame run")
            if not _same_bits(_run(ctx, fr, nf, opt), out):        # the cached graph replayed
                failures.append(f"{nf} frames/{fname}: the second run differs from the first")
            if fname == "moments":
                assert ctx.tuning().asm_parts == 1
                ctx.set_tuning(asm_parts=0)       # (k_assemble where its LDS fits; the role workgroups again where it does not)
                if not _same_bits(_run(ctx, fr, nf, opt), out):
                    failures.append(f"{nf} frames/moments: asm_parts 0 differs from asm_parts 1")
            if fname == "auto" and not _same_bits(out, results[(nf, "rows")]):
                failures.append(f"{nf} frames: AUTO on a model without the moment form differs from the row form")
    print(f"FITDIMS fit {fm.case_id(case)} accepted {rs.accepted_steps}/{rs.gn_iterations} gpu-oracle {worst:.2e}")
    assert not failures, f"{fm.case_id(case)}: " + "; ".join(failures[:12])


@pytest.mark.parametrize("case", fm.REFUSED, ids=[fm.case_id(c) for c in fm.REFUSED])
def test_refused_factorisation_away_from_smpl(gmodels, case):
    """e: a leaf joint without data points and no priors - every factorisation refused, by the 256-thread solve without the (level, thread)
    table and by the smallest 1024-thread solve: the state comes back bit for bit, lambda and the step counts are the oracle's."""
    from avatar_amd import api
    s = fm.study(case)
    om = s["om"]
    fr = fm.refused_frame(case, om)
    opt = fm.options(fr, icp_iters=2, max_iters_per_icp=4)
    ref = om.optimize(fr["part_map"], fr["num_parts"], fr["data"], fr["labels"], opt, *fr["start"], aggregate=1)
    assert ref["stats"].accepted_steps == 0 and (ref["trace_acc"] == -1).all()
    for nf in (1, 3):
        ctx = _context(gmodels(case), fr, nf, api.Context.DATA_TERM_ROWS, {})
        p, q, w, st, corr = _run(ctx, fr, nf, opt)
        for f in range(nf):
            assert np.array_equal(corr[f], ref["corr"]), (nf, f)
            assert np.array_equal(p[f], fr["start"][0]) and np.array_equal(q[f], fr["start"][1]) and np.array_equal(w[f], fr["start"][2]), (nf, f)
            assert (st[f].gn_iterations, st[f].accepted_steps) == (ref["stats"].gn_iterations, 0), (nf, f, st[f].gn_iterations, st[f].accepted_steps)
            assert st[f].lambda_ == ref["stats"].lambda_, (nf, f, st[f].lambda_, ref["stats"].lambda_)
