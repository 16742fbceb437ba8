"""The ICP data term along its POINT axis: matched vertices M, data points N and evaluation workgroups G at the values where its kernels
take another path - the cases of tests/data_term_cases.py, whose promises tests/test_data_term_cases_cpu.py checks with the oracle alone.
Everything goes through the public path (api.Context: set_tuning, set_data_term, frames_upload, state_upload, optimize_resident,
normal_equations, correspondences, launch_shape, state_download), and every run asserts launch_shape()[2] == G for the grid it means.

Which boundary of which kernel a case stands on:
  k_records (avt_eval.hip)      the last batch with 15, 16 and 1 records: M = 16 G - 1, 16 G, 16 G + 1; M = 1, 15, 16, 17; a vertex with 1, 2 and
                                1000 matches, one vertex with all 2049 (the weight c_m of a record)
  k_eval                        strided deal (G = 64, 65, 127, 128) and contiguous deal (G = 1, 2, 63); zero-batch workgroups (M <= 17 at every
                                strided G; SMPL's full frame, 126 batches, at G = 127 and 128); exactly one batch each (M = 16 G - 1, 16 G), a second
                                batch for workgroup 0 alone (16 G + 1), a THIRD batch (32 G + 1; j9k4's full frame: 131 batches at G = 64);
                                k_eval<24,10,6> (SMPL) and its run-time copy (literal_dims = 0), k_eval<0,0,8> (j9k4, j2k2, j1k1), the row-dealt
                                k_eval<0,0,9> (j45k5)
  the three reductions          k_reduce<1> (G < 64; j45k5: pairs >= 64 past the written-mask's 64 bits), k_reduce_strip<8> / <4> (one / three
                                frames, normal_equations and ride = 0) and the riding reduction of k_solve with 4 and 8 strips, at G = 65, 71 and
                                127: no multiple of their 4, 8, 16 or 32 slices (test c); the written-mask over stale partial tiles (test b)
  eval_ranges (avt_lm.hip)      the cost-balanced ranges (G = 1, 2, 63) and the equal-count fallback: j1k1's full frame, 1026 batches >
                                AVT_ERANGE_CAP and > the HS = 8 solve's room
  cost constant                 N = 255, 256, 257 (blocks of 256, row form) and 2047, 2048, 2049 (blocks of 2048, moment form), the last block without a
                                matched point, max_points = N + 7
  k_moments (avt_moments.hip)   segments of MOM_SEG = 512 entries: j2k2's pair (0, 0) (1374 entries) with (0, 8, 0), (1, 0, 7), (9, 512, 6), (511, 0, 1)
                                and (512, 512, 6) matched entries per segment - empty segments, full ones, and 0 to 7 weight-zero padding entries; j1k1's
                                33 segments

  a  one LM step, then the normal equations at the returned state against the oracle's at the device's correspondences (which are the
     oracle's, bit for bit): H 1e-9 (rows) / 1e-10 (moments) of max|oH|, g 1e-9 of max(1, max|og|), H == H.T, rows against moments 1e-11 / 1e-9,
     the cost 1e-9 relative (data_term_cases.KAPPA_C_MAX makes that reachable).  Per G of GRIDS for the row form, once for the moment form
     (it has no G); on one frame and as the last of three different frames.  M = 0: no correspondences, the state untouched bit for bit
     (normal_equations is not asked: the frame has no system), the other frames of the batch at the bars.
  b  stale memory: one context through six cases of shrinking and growing M and G, in both forms: every result equals the fresh context's bit for bit
  c  SMPL at G = 64, 65, 71, 127 with the riding reduction (4 and 8 strips) and without: H and g as at G = 128 within the bars of a, the
     same step counts; ride = 0 against ride = 1 to 1e-12 relative after one LM step (tests/test_gpu_parity_more.py
     test_in_launch_hand_over_is_reproducible promises agreement to summation order, not bit for bit: the two reductions cut G into different slices)
  d  short fits (2 ICP x 3 GN iterations) at the bars of tests/test_gpu_fit_dims.py test_fit_matches_oracle
  e  the segment cases with both assemblies of the moment form: bit-identical

Largest errors printed on an MI355X (the bars in brackets), over all cases, grids and frame counts:
  rows                 H 8.3e-14 (1e-9)   g 1.6e-13 (1e-9)   cost 1.1e-14 (1e-9)
  moments              H 7.1e-14 (1e-10)  g 3.1e-12 (1e-9)   cost 8.5e-13 (1e-9)
  rows against moments H 1.2e-15 (1e-11)  g 1.4e-10 (1e-9; j1k1's full frame, relative to a gradient the step has nearly cancelled)
  c                    against G = 128: H 3.0e-14, g 1.2e-13; ride = 1 against ride = 0: H 4.1e-14, g 1.7e-13 (1e-12)
  d                    cost 9.7e-13 (1e-8), lambda 2.6e-10 (1e-9; j9k4-mult-1000, whose lambda_conditioning is 3.4e4 of the 3.5e4 allowed), p and q 3.9e-13 (1e-6), w 1.1e-13 (1e-5)
No case failed.  What the file notices, tried on deliberately wrong builds: a k_eval whose strided workgroups stop after their second batch
fails j9k4's M = 2049 and full-frame cases at G = 64 and 65 (H off by 2e-2) and j1k1's full frame; a k_reduce_strip that ignores the written-masks
fails b on SMPL (H off by a factor 4 behind a larger frame) and c at every G.
"""
import numpy as np
import pytest

import data_term_cases as dc

pytestmark = pytest.mark.gpu

H_BAR = {"rows": 1e-9, "moments": 1e-10}
G_BAR, COST_BAR, RM_BAR = 1e-9, dc.COST_BAR, (1e-11, 1e-9)
# (variant, model, tuning): SMPL's literal-dimension kernels and their run-time copies
VARIANTS = [("smpl", "smpl", {}), ("smpl-lit0", "smpl", dict(literal_dims=0))] + [(n, n, {}) for n in dc.MODELS[1:]]
A_CASES = [(v, n, tun, k) for v, n, tun in VARIANTS for k in dc.case_keys(n)]
_ORACLE = {}


@pytest.fixture(scope="module")
def gmodels():
    from avatar_amd import api
    made = {}

    def get(name):
        if name not in made:
            made[name] = api.AvatarModel(dc.base(name)["model"])
        return made[name]
    return get


def _context(gm, name, cases, form, **tun):
    """a context for the frames `cases` (max_points = the longest + 7) with the data term `form` ("rows" / "moments")"""
    from avatar_amd import api
    fr = dc.base(name)["frame"]
    ctx = api.Context(gm, fr["num_parts"], fr["part_map"], max(c["N"] for c in cases) + 7, len(cases), device=0)
    if tun:
        ctx.set_tuning(**tun)
    _form(ctx, name, form)
    return ctx


def _form(ctx, name, form):
    from avatar_amd import api
    if form == "moments" and not dc.MOM_OK[name]:
        with pytest.raises(api.AvtError):
            ctx.set_data_term(ctx.DATA_TERM_MOMENTS)
        pytest.fail(f"{name}: asked for a moment form the model does not have")
    ctx.set_data_term(ctx.DATA_TERM_MOMENTS if form == "moments" else ctx.DATA_TERM_ROWS)


def _forms(name):
    return ("rows", "moments") if dc.MOM_OK[name] else ("rows",)


def _grid(ctx, G):
    """sets the evaluation grid and asserts that the next optimize() runs it"""
    ctx.set_tuning(g=G)
    assert ctx.launch_shape()[2] == G, (ctx.launch_shape(), G)


def _upload(ctx, cases):
    ctx.frames_upload([c["data"] for c in cases], [c["labels"] for c in cases])


def _run(ctx, name, cases, opt):
    """the frames are resident: start state, optimize; (p, q, w, stats, [correspondences])"""
    p0, q0, w0 = dc.base(name)["frame"]["start"]
    nf = len(cases)
    ctx.state_upload(np.repeat(p0[None], nf, 0), np.repeat(q0[None], nf, 0), np.repeat(w0[None], nf, 0))
    ctx.optimize_resident(opt)
    p, q, w, st = ctx.state_download()
    return p, q, w, st, [ctx.correspondences(f, c["N"]) for f, c in enumerate(cases)]


def _oracle(name, c, p, q, w):
    """the oracle's data term (H, g; no priors, rows summed one by one) and full cost at a state, with the case's correspondences; cached per
    (case, state): it does not depend on G"""
    key = (name, c["key"], p.tobytes(), q.tobytes(), w.tobytes())
    if key not in _ORACLE:
        b = dc.base(name)
        fr = b["frame"]
        _, og, oH, _ = b["om"].evaluate(p, q, w, c["corr"], c["data"], 0.0, 0.0, aggregate=0)
        oc = b["om"].evaluate(p, q, w, c["corr"], c["data"], fr["betas"][0], fr["betas"][1], aggregate=1)[0]
        _ORACLE[key] = (oH, og, oc)
    return _ORACLE[key]


class Worst:
    def __init__(self):
        self.e = {}

    def add(self, form, eh, eg, ec):
        w = self.e.setdefault(form, [0.0, 0.0, 0.0])
        self.e[form] = [max(a, b) for a, b in zip(w, (eh, eg, ec))]

    def line(self):
        return " | ".join(f"{k} H {v[0]:.2e} g {v[1]:.2e} cost {v[2]:.2e}" for k, v in self.e.items()) or "nothing compared"


def _check_frame(ctx, name, c, f, out, form, tag, failures, worst):
    """frame f of a run (out: _run's) against the oracle at the bars of a; returns (H, g, cost) or None"""
    p, q, w, st, corr = out
    start = dc.base(name)["frame"]["start"]
    if not np.array_equal(corr[f], c["corr"]):
        failures.append(f"{tag}: {int((corr[f] != c['corr']).sum())} correspondences differ from the oracle's")
        return None
    if c["M"] == 0:
        if not (st[f].num_correspondences == 0 and np.array_equal(p[f], start[0]) and np.array_equal(q[f], start[1]) and np.array_equal(w[f], start[2])):
            failures.append(f"{tag}: a frame without correspondences did not keep its state bit for bit")
        return None
    H, g, cost = ctx.normal_equations(f)
    oH, og, oc = _oracle(name, c, p[f], q[f], w[f])
    eh, eg, ec = float(np.abs(H - oH).max() / np.abs(oH).max()), float(np.abs(g - og).max() / max(1.0, np.abs(og).max())), abs(cost - oc) / oc
    worst.add(form, eh, eg, ec)
    if not (eh < H_BAR[form] and eg < G_BAR and ec <= COST_BAR):
        failures.append(f"{tag}: H {eh:.2e} g {eg:.2e} cost {ec:.2e} from the oracle")
    if not np.array_equal(H, H.T):
        failures.append(f"{tag}: H is not symmetric ({int((H != H.T).sum())} entries)")
    return H, g, cost


@pytest.mark.parametrize("variant,name,tun,key", A_CASES, ids=[f"{v}-{dc.key_id(k)}" for v, _, _, k in A_CASES])
def test_normal_equations_across_grids(gmodels, variant, name, tun, key):
    """a of the module's docstring."""
    c = dc.case(name, key)
    fr = dc.base(name)["frame"]
    opt = dc.options(fr, icp_iters=1, max_iters_per_icp=1)
    others = [dc.case(name, ("all",)), dc.case(name, ("M", 17, "rand", None))]
    failures, worst = [], Worst()
    for cases in ([c], others + [c]):
        nf, f = len(cases), len(cases) - 1
        ctx = _context(gmodels(name), name, cases, "rows", **tun)
        _upload(ctx, cases)
        for G in dc.GRIDS:
            _grid(ctx, G)
            out = _run(ctx, name, cases, opt)
            tag = f"{nf} frames/rows G {G}"
            rows = _check_frame(ctx, name, c, f, out, "rows", tag, failures, worst)
            if c["M"] == 0 and nf > 1 and G in (63, 128):          # the other frames of the batch are what they are without the empty one
                for f2 in range(nf - 1):
                    _check_frame(ctx, name, cases[f2], f2, out, "rows", f"{tag} frame {f2} beside the empty frame", failures, worst)
            if rows is not None and dc.MOM_OK[name] and G == 128:       # the moment form at the same state and correspondences
                ctx.set_data_term(ctx.DATA_TERM_MOMENTS)
                Hm, gm, _ = ctx.normal_equations(f)
                ctx.set_data_term(ctx.DATA_TERM_ROWS)
                eh, eg = float(np.abs(Hm - rows[0]).max() / np.abs(rows[0]).max()), float(np.abs(gm - rows[1]).max() / max(1e-300, np.abs(rows[1]).max()))
                worst.add("rows-moments", eh, eg, 0.0)
                if not (eh < RM_BAR[0] and eg < RM_BAR[1]):
                    failures.append(f"{tag}: moments against rows H {eh:.2e} g {eg:.2e}")
        if dc.MOM_OK[name]:
            _form(ctx, name, "moments")
            ctx.set_tuning(g=0)
            out = _run(ctx, name, cases, opt)
            _check_frame(ctx, name, c, f, out, "moments", f"{nf} frames/moments", failures, worst)
            if c["M"] == 0 and nf > 1:
                for f2 in range(nf - 1):
                    _check_frame(ctx, name, cases[f2], f2, out, "moments", f"{nf} frames/moments frame {f2} beside the empty frame", failures, worst)
        del ctx
    print(f"DATATERM a {variant}-{dc.key_id(key)} M {c['M']} N {c['N']} {worst.line()}")
    assert not failures, f"{variant}-{dc.key_id(key)}: " + "; ".join(failures[:12])


def _stale_sequence(name):
    """[(key, G)]: the all-matched case at G = 128, M = 17, M = 0, M = 16 G + 1 at G = 64, all at G = 63, M = 1 at G = 2.  j45k5 has no 1025
    matched vertices (N = 257 stands in), j1k1 no M = 1 case (data_term_cases.EXCLUDED: M = 15 stands in)."""
    keys = dc.case_keys(name)
    mid = ("M", 1025, "first", 64) if ("M", 1025, "first", 64) in keys else ("N", 257)
    last = ("M", 1, "first", None) if ("M", 1, "first", None) in keys else ("M", 15, "first", None)
    return [(("all",), 128), (("M", 17, "first", None), 128), (("M", 0, "first", None), 128), (mid, 64), (("all",), 63), (last, 2)]


def _bits(ctx, name, c, opt):
    """one LM step on the resident frame c; everything the stale-memory test compares, as one tuple of arrays"""
    out = _run(ctx, name, [c], opt)
    p, q, w, st, corr = out
    res = [p[0], q[0], w[0], corr[0], np.array([st[0].final_cost, st[0].lambda_, st[0].accepted_steps, st[0].gn_iterations], np.float64)]
    if c["M"] > 0:
        H, g, cost = ctx.normal_equations(0)
        res += [H, g, np.array([cost])]
    return res, out


@pytest.mark.parametrize("name", dc.MODELS)
def test_stale_memory_of_larger_frames_changes_no_bit(gmodels, name):
    """b of the module's docstring: partial tiles, written-masks, records, evaluation ranges and moment blocks of a former, larger frame lie in
    memory at every step but the first."""
    fr = dc.base(name)["frame"]
    opt = dc.options(fr, icp_iters=1, max_iters_per_icp=1)
    seq = [(dc.case(name, k), G) for k, G in _stale_sequence(name)]
    biggest = max((c for c, _ in seq), key=lambda c: c["N"])
    used = _context(gmodels(name), name, [biggest], "rows")
    failures, worst = [], Worst()
    for form in _forms(name):
        _form(used, name, form)
        for step, (c, G) in enumerate(seq):
            got = []
            for ctx in (used, _context(gmodels(name), name, [biggest], form)):
                _upload(ctx, [c])
                _grid(ctx, G)
                res, out = _bits(ctx, name, c, opt)
                got.append(res)
                if ctx is used:
                    _check_frame(ctx, name, c, 0, out, form, f"{form} step {step} G {G}", failures, worst)
            diff = [i for i, (a, b) in enumerate(zip(*got)) if not np.array_equal(a, b)]
            if diff or len(got[0]) != len(got[1]):
                failures.append(f"{form} step {step} ({dc.key_id(c['key'])} at G {G}): results {diff} of (p, q, w, corr, stats, H, g, cost) differ from the fresh context's")
    print(f"DATATERM b {name} {worst.line()}")
    assert not failures, f"{name}: " + "; ".join(failures[:12])


@pytest.mark.parametrize("nf", (1, 3))
def test_slices_that_do_not_divide_the_grid(gmodels, nf):
    """c of the module's docstring.  One LM step for the comparisons of H and g (what differs is then one reduction's summation order); three
    GN iterations for the step counts and the state (1e-9, the bar of one frame through different launch shapes in tests/test_gpu_fit_dims.py)."""
    name = "smpl"
    fr = dc.base(name)["frame"]
    cases = [dc.case(name, k) for k in ((("all",),) if nf == 1 else (("N", 2049), ("M", 1025, "rand", 64), ("all",)))]
    opt1, opt3 = dc.options(fr, icp_iters=1, max_iters_per_icp=1), dc.options(fr, icp_iters=1, max_iters_per_icp=3)
    variants = {"ride4": dict(ride=1, ride_strips=4), "ride8": dict(ride=1, ride_strips=8), "noride": dict(ride=0)}
    failures, worst, res = [], Worst(), {}
    for vname, tun in variants.items():
        ctx = _context(gmodels(name), name, cases, "rows", **tun)
        _upload(ctx, cases)
        for G in (128, 64, 65, 71, 127):
            _grid(ctx, G)
            out1 = _run(ctx, name, cases, opt1)
            ne = [_check_frame(ctx, name, c, f, out1, "rows", f"{vname} G {G} frame {f}", failures, worst) for f, c in enumerate(cases)]
            out3 = _run(ctx, name, cases, opt3)
            res[(vname, G)] = (ne, out3)
    for (vname, G), (ne, out3) in res.items():
        ne0, ref3 = res[(vname, 128)]
        for f in range(nf):
            if ne[f] is None or ne0[f] is None:
                continue
            tag = f"{vname} G {G} frame {f}"
            eh, eg = float(np.abs(ne[f][0] - ne0[f][0]).max() / np.abs(ne0[f][0]).max()), float(np.abs(ne[f][1] - ne0[f][1]).max() / max(1.0, np.abs(ne0[f][1]).max()))
            worst.add("against G 128", eh, eg, 0.0)
            if not (eh < H_BAR["rows"] and eg < G_BAR):
                failures.append(f"{tag}: H {eh:.2e} g {eg:.2e} from G = 128")
            s, s0 = out3[3][f], ref3[3][f]
            es = max(float(np.abs(out3[i][f] - ref3[i][f]).max()) for i in range(3))
            if (s.gn_iterations, s.accepted_steps) != (s0.gn_iterations, s0.accepted_steps) or not es <= 1e-9:
                failures.append(f"{tag}: accepted {s.accepted_steps} of {s.gn_iterations} (G = 128: {s0.accepted_steps} of {s0.gn_iterations}), state {es:.2e} away")
            if vname != "noride":
                a = res[("noride", G)][0][f]
                eh, eg = float(np.abs(ne[f][0] - a[0]).max() / np.abs(a[0]).max()), float(np.abs(ne[f][1] - a[1]).max() / max(1e-300, np.abs(a[1]).max()))
                worst.add("ride 1 against 0", eh, eg, 0.0)
                if not (eh <= 1e-12 and eg <= 1e-12):
                    failures.append(f"{tag}: H {eh:.2e} g {eg:.2e} from ride = 0")
    print(f"DATATERM c {nf} frames {worst.line()}")
    assert not failures, "; ".join(failures[:12])


SHORT = dc.short_fit_cases()


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and all(np.array_equal(x, y) for x, y in zip(a[4], b[4])) and \
        all((s.gn_iterations, s.accepted_steps, s.final_cost, s.lambda_) == (t.gn_iterations, t.accepted_steps, t.final_cost, t.lambda_) for s, t in zip(a[3], b[3]))


@pytest.mark.parametrize("name,key,G", SHORT, ids=[f"{n}-{dc.key_id(k)}" for n, k, _ in SHORT])
def test_short_fit_matches_oracle(gmodels, name, key, G):
    """d of the module's docstring, in the manner of tests/test_gpu_fit_dims.py test_fit_matches_oracle."""
    b, c = dc.base(name), dc.case(name, key)
    om, fr = b["om"], c["frame"]
    opt = dc.options(fr, **dc.SHORT_FIT)
    ref = om.optimize(fr["part_map"], fr["num_parts"], fr["data"], fr["labels"], opt, *fr["start"], aggregate=1)
    rs = ref["stats"]
    failures, worst = [], [0.0] * 5
    for form in _forms(name):
        ctx = _context(gmodels(name), name, [c], form)
        _upload(ctx, [c])
        if G and form == "rows":
            _grid(ctx, G)
        out = _run(ctx, name, [c], opt)
        p, q, w, st, corr = out
        if not np.array_equal(corr[0], ref["corr"]):
            failures.append(f"{form}: {int((corr[0] != ref['corr']).sum())} correspondences differ from the oracle's")
        if (st[0].gn_iterations, st[0].accepted_steps) != (rs.gn_iterations, rs.accepted_steps):
            failures.append(f"{form}: accepted {st[0].accepted_steps} of {st[0].gn_iterations}, the oracle {rs.accepted_steps} of {rs.gn_iterations}")
        e = [abs(st[0].final_cost - rs.final_cost) / abs(rs.final_cost), abs(st[0].lambda_ - rs.lambda_) / abs(rs.lambda_), float(np.abs(p[0] - ref["p"]).max()),
             float(np.abs(q[0] - ref["q"].reshape(-1, 4)).max()), float(np.abs(w[0] - ref["w"]).max())]
        worst = [max(x, y) for x, y in zip(worst, e)]
        if not (e[0] < 1e-8 and e[1] < 1e-9 and e[2] < 1e-6 and e[3] < 1e-6 and e[4] < 1e-5):
            failures.append(f"{form}: cost {e[0]:.2e} lambda {e[1]:.2e} p {e[2]:.2e} q {e[3]:.2e} w {e[4]:.2e} from the oracle")
        if not _same_bits(_run(ctx, name, [c], opt), out):        # the cached graph replayed
            failures.append(f"{form}: the second run differs from the first")
    print(f"DATATERM d {name}-{dc.key_id(key)} accepted {rs.accepted_steps}/{rs.gn_iterations} cost {worst[0]:.2e} lambda {worst[1]:.2e} p {worst[2]:.2e} q {worst[3]:.2e} w {worst[4]:.2e}")
    assert not failures, f"{name}-{dc.key_id(key)}: " + "; ".join(failures[:12])


@pytest.mark.parametrize("seg", dc.SEGMENTS, ids=["x".join(str(x) for x in s) for s in dc.SEGMENTS])
def test_moment_segments_with_both_assemblies(gmodels, seg):
    """e of the module's docstring: k_assemble_parts (asm_parts = 1) and k_assemble (0) on the segment cases, at the bars of a and bit-identical."""
    name = "j2k2"
    c = dc.case(name, ("seg", seg))
    opt = dc.options(dc.base(name)["frame"], icp_iters=1, max_iters_per_icp=1)
    failures, worst, got = [], Worst(), []
    for asm in (1, 0):
        ctx = _context(gmodels(name), name, [c], "moments", asm_parts=asm)
        assert ctx.tuning().asm_parts == asm
        _upload(ctx, [c])
        res, out = _bits(ctx, name, c, opt)
        _check_frame(ctx, name, c, 0, out, "moments", f"asm_parts {asm}", failures, worst)
        got.append(res)
    if not all(np.array_equal(a, b) for a, b in zip(*got)):
        failures.append("asm_parts 0 differs from asm_parts 1")
    print(f"DATATERM e {dc.key_id(c['key'])} {worst.line()}")
    assert not failures, "; ".join(failures)
