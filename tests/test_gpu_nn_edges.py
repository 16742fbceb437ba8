"""The nearest-neighbour kernels (avatar_amd/csrc/avt_nn.hip, avt_bucket.h) at their internal boundaries, through all four device
code paths, every comparison an integer equality against the numpy restatement (tests/nn_restatement.py; tests/test_nn_edges_cpu.py
ties it to the CPU oracle on the same cases, tests/nn_cases.py builds them):

  A  latency shape   k_compact + k_nn<4>                                     (the defaults, stand-alone avt_nn)
  B  slab scan       k_compact sorting by (y, vertex id) + k_nn_part         (avt_tuning.nn_force_part = 1)
  C  full scan       k_compact unsorted + k_nn_part over every candidate     (nn_force_part = 1, nn_slab = 0)
  D  fused shape     k_nn_vis<4>, what every single-frame optimize() runs    (nn_force_vis = 1)

Beside the indices, the per-vertex match counts and 2^40 fixed-point sums the kernels accumulate (nn_record<4>, nn_record<1> above
NN_ACC_CAP visible candidates, the LDS accumulators below) are compared exactly (Context.nn_sums)."""
import numpy as np
import pytest

import nn_cases
import nn_restatement as nr
from avatar_amd import synth
from avatar_amd.capi import Options

pytestmark = pytest.mark.gpu

SHAPES = {"A": {}, "B": dict(nn_force_part=1), "C": dict(nn_force_part=1, nn_slab=0), "D": dict(nn_force_vis=1)}
MAX_POINTS = 4608                 # the largest case has 4097 queries
_REF = {}


@pytest.fixture(scope="module")
def contexts(gmodel):
    """One Context per (part map, shape), made on first use and kept for the module."""
    from avatar_amd import api
    made = {}

    def get(pm, npart, shape):
        key = nn_cases.map_key(pm, npart) + (shape,)
        if key not in made:
            made[key] = api.Context(gmodel, npart, pm, MAX_POINTS, 1, device=0).set_tuning(**SHAPES[shape])
            t = made[key].tuning()
            assert all(getattr(t, k) == v for k, v in SHAPES[shape].items())
        return made[key]
    return get


def _reference(model, case):
    """(indices, counts, sums, centre) of a case from the restatement: computed once, shared by the shapes, never written to."""
    name, pm, npart, cloud, vis, data, labels = case
    if name not in _REF:
        corr = nr.nn_ref(nn_cases.part_of_vertex(model, pm), npart, cloud, vis, data, labels)
        res = (corr,) + nr.nn_sums_ref(corr, data, nn_cases.V)
        for a in res:
            a.setflags(write=False)
        _REF[name] = res
    return _REF[name]


def _run(ctx, model, case):
    """'' when the device's indices and bookkeeping equal the restatement's, else what differs."""
    name, pm, npart, cloud, vis, data, labels = case
    corr, cnt, fsum, centre = _reference(model, case)
    got = ctx.nn(cloud, vis, data, labels)
    gc, gf, gcen = ctx.nn_sums(0)
    bad = []
    if not np.array_equal(got, corr):
        bad.append(f"{int((got != corr).sum())} of {len(corr)} indices")
    if not np.array_equal(gc, cnt):
        bad.append(f"{int((gc != cnt).sum())} counts")
    if not np.array_equal(gf, fsum):
        bad.append(f"{int((gf != fsum).any(0).sum())} sums")
    if not np.array_equal(gcen, centre):
        bad.append("centre")
    return f"{name}: " + ", ".join(bad) if bad else ""


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("group", list(nn_cases.GROUPS))
def test_every_case_through_every_shape(smpl, contexts, group, shape):
    """sweep: visible counts of a part at 4, 32, 16, 64, NN_ACC_CAP 512, NN_SORT_CAP = NN_TILE 1024, each +-1; tiles: a part across a
    tile of the part-sorted arrays; ties: exact ties across sub-lanes, groups and tiles, and the slab's stop rule at equality; slabs:
    one y, queries outside the y range, distance 0, a wide slab; magnitudes: 1e3 +- 1e-9, subnormal and underflowing distances
    (float64 subnormals are kept by the CPU and must be by the device); queries: N at 1, 64, 256, 512, 2048 +- 1, invalid labels,
    parts without queries or without vertices, 64 parts; runs: runs of equal matches for the in-wave merge."""
    failures = []
    for case in nn_cases.cases(smpl, group):
        msg = _run(contexts(case[1], case[2], shape), smpl, case)
        if msg:
            failures.append(msg)
    assert not failures, f"shape {shape}: " + "; ".join(failures)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_repeats_on_one_context_leave_nothing_behind(smpl, contexts, shape):
    """A large frame followed by one query, twenty times on one context: equal indices and equal sums every time (stale counts,
    sums or bucket counters of the call before would show)."""
    by_name = {c[0]: c for c in nn_cases.cases(smpl, "queries") + nn_cases.cases(smpl, "runs")}
    pair = [by_name["queries-all-parts-4097"], by_name["queries-one-part-1"], by_name["runs-identity-400-first-1"]]
    ctx = contexts(pair[0][1], pair[0][2], shape)
    failures = []
    for rep in range(20):
        for case in pair:
            msg = _run(ctx, smpl, case)
            if msg:
                failures.append(f"repeat {rep} {msg}")
    assert not failures, f"shape {shape}: " + "; ".join(failures[:8])


# ---- the query side inside optimize(): one ICP iteration leaves the correspondences of the start state behind ------------------------
def _frames(smpl):
    """Pixels of a rendered frame, truncated to the boundary counts (every part stays present) or relabelled."""
    fr = synth.make_frame(smpl, 3)
    sel = np.arange(0, len(fr["labels"]), 6)
    data, labels = fr["data"][sel], fr["labels"][sel]
    assert len(labels) >= 4097
    rng = np.random.default_rng(11)
    out = []
    for n in nn_cases.QUERY_N:
        idx = np.arange(n) * len(labels) // n
        out.append((f"N={n}", data[idx], labels[idx].copy()))
    d, l = data[:600], labels[:600]
    invalid = np.array([-1, 24, 2 ** 31 - 1, -2 ** 31], np.int64)
    out.append(("all invalid", d, invalid[rng.integers(0, 4, 600)].astype(np.int32)))
    some = l.copy()
    some[::5] = invalid[rng.integers(0, 4, len(some[::5]))]
    out.append(("some invalid", d, some))
    out.append(("first part only", d, np.zeros(600, np.int32)))
    out.append(("last part only", d, np.full(600, 23, np.int32)))
    out.append(("parts 3 and 20", d, np.array([3, 20], np.int32)[rng.integers(0, 2, 600)]))
    return fr, out


@pytest.fixture(scope="module")
def optimize_reference(smpl, omodel):
    from avatar_amd import api
    fr, frames = _frames(smpl)
    w0, p0, R0 = fr["start"]
    q0 = api.rot_to_quat(R0)
    opt = Options.counted(icp_iters=1, max_iters_per_icp=2)
    pm = synth.identity_part_map()
    refs = [omodel.optimize(pm, 24, d, l, opt, p0, q0, w0, aggregate=1) for _, d, l in frames]
    return frames, refs, opt, (p0, q0, w0), pm


@pytest.mark.parametrize("shape", ["D", "B"])
def test_query_boundaries_inside_optimize(smpl, gmodel, optimize_reference, shape):
    """optimize_batch on one frame (shape D: k_nn_vis<4>, and the throughput shape with nn_force_part = 1): the correspondences of
    the one ICP iteration equal the oracle's, the statistics count that array, and the bookkeeping left behind (the closing launch of
    optimize() resets none of it) is that array's."""
    from avatar_amd import api
    frames, refs, opt, (p0, q0, w0), pm = optimize_reference
    ctx = api.Context(gmodel, 24, pm, MAX_POINTS, 1, device=0).set_tuning(**({} if shape == "D" else SHAPES["B"]))
    failures = []
    for (name, data, labels), ref in zip(frames, refs):
        p, q, w, st = ctx.optimize_batch([data], [labels], opt, p0[None], q0[None], w0[None])
        corr = ctx.correspondences(0, len(labels))
        cnt, fsum, centre = ctx.nn_sums(0)
        rc, rf, rcen = nr.nn_sums_ref(ref["corr"], data, nn_cases.V)
        m = corr[corr >= 0]
        ok = (np.array_equal(corr, ref["corr"]) and st[0].num_correspondences == len(m) == ref["stats"].num_correspondences
              and st[0].matched_model_points == len(np.unique(m)) == ref["stats"].matched_model_points
              and np.array_equal(cnt, rc) and np.array_equal(fsum, rf) and np.array_equal(centre, rcen))
        if not ok:
            failures.append(f"{name}: {int((corr != ref['corr']).sum())} indices, stats {st[0].num_correspondences}/{st[0].matched_model_points} "
                            f"for {len(m)}/{len(np.unique(m))}, {int((cnt != rc).sum())} counts, {int((fsum != rf).any(0).sum())} sums")
    assert not failures, f"shape {shape}: " + "; ".join(failures)


def test_nn_sums_is_refused_without_a_search(gmodel):
    from avatar_amd import api
    ctx = api.Context(gmodel, 24, synth.identity_part_map(), 64, 1, device=0)
    with pytest.raises(api.AvtError):
        ctx.nn_sums(0)
