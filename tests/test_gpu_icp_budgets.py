"""Per-frame ICP budgets (avt_optimize_resident_budgets) and per-frame state installs (avt_state_upload_frames): a frame with budget b
ends bit for bit where a call with icp_iters = b over the same resident frames leaves it."""
import numpy as np
import pytest

from avatar_amd import synth
from avatar_amd.capi import Options

ICP = 3
STAT_FIELDS = ("initial_cost", "final_cost", "lambda_", "num_correspondences", "matched_model_points", "gn_iterations", "accepted_steps")


@pytest.fixture(scope="module")
def frames(smpl):
    from avatar_amd import api
    out = []
    for seed in (30, 31, 32, 33, 34):
        fr = synth.make_frame(smpl, seed)
        w0, p0, R0 = fr["start"]
        sel = np.arange(0, len(fr["labels"]), 3)
        out.append((fr["data"][sel], fr["labels"][sel], p0, api.rot_to_quat(R0), w0))
    return out


def _batch(frames, n):
    fs = [frames[f % len(frames)] for f in range(n)]
    return [f[0] for f in fs], [f[1] for f in fs], np.array([f[2] for f in fs]), np.array([f[3] for f in fs]), np.array([f[4] for f in fs])


def _ctx(gmodel, n, data_term=None):
    from avatar_amd import api
    ctx = api.Context(gmodel, 24, synth.identity_part_map(), 20000, n)
    if data_term is not None:
        ctx.set_data_term(data_term)
    return ctx


def _stats(st):
    return tuple(getattr(st, k) for k in STAT_FIELDS)


def _same(a, b):
    """bit for bit: p, q, w and every statistic of one frame"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and _stats(a[3]) == _stats(b[3]))


def _run(ctx, datas, labs, p0, q0, w0, opt, budgets=None):
    ctx.frames_upload(datas, labs)
    ctx.state_upload(p0, q0, w0)
    if budgets is None:
        ctx.optimize_resident(opt)
    else:
        ctx.optimize_resident_budgets(opt, budgets)
    p, q, w, st = ctx.state_download()
    return [(p[f], q[f], w[f], st[f]) for f in range(len(datas))]


def _check_budgets(gmodel, frames, n, opt_kw, data_term=None):
    ctx = _ctx(gmodel, n, data_term)
    datas, labs, p0, q0, w0 = _batch(frames, n)
    budgets = np.array([f % (ICP + 1) for f in range(n)], np.int32)
    uniform, posed = {}, {}
    for b in range(ICP + 1):
        uniform[b] = _run(ctx, datas, labs, p0, q0, w0, Options.demo(icp_iters=b, **opt_kw))
        posed[b] = {f: ctx.posed(f)[0] for f in range(n) if budgets[f] == b}
    opt = Options.demo(icp_iters=ICP, **opt_kw)
    got = _run(ctx, datas, labs, p0, q0, w0, opt, budgets)
    for f in range(n):
        assert _same(got[f], uniform[int(budgets[f])][f]), f"frame {f} (budget {budgets[f]}) differs from the uniform icp_iters run"
        if budgets[f] == 0:
            assert np.array_equal(got[f][0], p0[f]) and np.array_equal(got[f][1], q0[f]) and np.array_equal(got[f][2], w0[f])
        assert np.abs(ctx.posed(f)[0] - posed[int(budgets[f])][f]).max() <= 1e-12     # (budget 0: the skinning of the start state)
    again = _run(ctx, datas, labs, p0, q0, w0, opt, budgets)           # run to run (the cached graph replayed)
    assert all(_same(got[f], again[f]) for f in range(n))
    full = _run(ctx, datas, labs, p0, q0, w0, opt, np.full(n, ICP, np.int32))     # every budget at icp_iters: the plain call
    assert all(_same(full[f], uniform[ICP][f]) for f in range(n))
    # a different pattern replays the same graph and still holds every frame where its budget ends
    rev = (ICP - budgets).astype(np.int32)
    got2 = _run(ctx, datas, labs, p0, q0, w0, opt, rev)
    assert all(_same(got2[f], uniform[int(rev[f])][f]) for f in range(n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 12, 45])
def test_budgets_match_uniform_runs(gmodel, frames, n):
    _check_budgets(gmodel, frames, n, dict(max_iters_per_icp=5))


@pytest.mark.gpu
@pytest.mark.parametrize("lm_policy,ftol", [(0, 0.0), (0, 1e-4), (1, 0.0)])
def test_budgets_both_damping_policies_and_tolerances(gmodel, frames, lm_policy, ftol):
    _check_budgets(gmodel, frames, 12, dict(max_iters_per_icp=5, lm_policy=lm_policy, function_tolerance=ftol))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 12])
@pytest.mark.parametrize("form", ["rows", "moments"])
def test_budgets_on_both_data_term_forms(gmodel, frames, n, form):
    from avatar_amd import api
    term = api.Context.DATA_TERM_ROWS if form == "rows" else api.Context.DATA_TERM_MOMENTS
    _check_budgets(gmodel, frames, n, dict(max_iters_per_icp=4), term)


@pytest.mark.gpu
def test_bad_budgets_and_installs_are_rejected_with_the_state_unchanged(gmodel, frames):
    from avatar_amd import api
    n = 4
    ctx = _ctx(gmodel, n)
    datas, labs, p0, q0, w0 = _batch(frames, n)
    opt = Options.demo(icp_iters=2, max_iters_per_icp=3)
    with pytest.raises(api.AvtError):          # nothing resident yet
        ctx._F = n
        ctx.optimize_resident_budgets(opt, [1] * n)
    before = _run(ctx, datas, labs, p0, q0, w0, opt, [2, 1, 0, 2])
    for bad in ([0, 1, 3, 2], [0, -1, 0, 0]):
        with pytest.raises(api.AvtError):
            ctx.optimize_resident_budgets(opt, bad)
    with pytest.raises(api.AvtError):
        ctx.optimize_resident_budgets(opt, [1] * (n - 1))
    for frames_ids in ([4], [-1], [1, 1], [0, 1, 2, 3, 0]):
        k = len(frames_ids)
        with pytest.raises(api.AvtError):
            ctx.state_upload_frames(frames_ids, np.zeros((k, 3)), np.zeros((k, 24, 4)), np.zeros((k, 10)))
    p, q, w, st = ctx.state_download()
    for f in range(n):
        assert _same((p[f], q[f], w[f], st[f]), before[f])


@pytest.mark.gpu
def test_state_upload_frames_installs_only_the_listed_frames(gmodel, frames):
    n = 5
    ctx = _ctx(gmodel, n)
    datas, labs, p0, q0, w0 = _batch(frames, n)
    opt = Options.demo(icp_iters=2, max_iters_per_icp=4)
    first = _run(ctx, datas, labs, p0, q0, w0, opt)          # the warm states
    sel = [3, 1]
    ctx.frames_upload(datas, labs)                           # same number of frames: the warm states stay resident
    ctx.state_upload_frames(sel, p0[sel], q0[sel], w0[sel])
    ctx.optimize_resident_budgets(opt, [2, 2, 0, 2, 1])
    p, q, w, st = ctx.state_download()
    # the reference: every state installed from the host
    pr, qr, wr = (np.array([x[i] for x in first]) for i in range(3))
    pr[sel], qr[sel], wr[sel] = p0[sel], q0[sel], w0[sel]
    ref = _run(ctx, datas, labs, pr, qr, wr, opt, [2, 2, 0, 2, 1])
    for f in sel:            # re-installed: exactly what a host install of the same state gives
        assert _same((p[f], q[f], w[f], st[f]), ref[f])
    for f in (0, 4):         # kept their warm state (and control block): the same fit to rounding
        assert np.abs(p[f] - ref[f][0]).max() < 1e-9 and np.abs(q[f] - ref[f][1]).max() < 1e-9 and np.abs(w[f] - ref[f][2]).max() < 1e-9
    assert np.array_equal(p[2], first[2][0]) and np.array_equal(q[2], first[2][1]) and np.array_equal(w[2], first[2][2])     # budget 0: the warm state as it was
    assert _stats(st[2]) == _stats(first[2][3])
