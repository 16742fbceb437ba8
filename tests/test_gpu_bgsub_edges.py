"""GPU background subtraction (avatar_amd/csrc/avt_bgsub.hip) at its edges: the known answers of test_bgsub_cpu.py, the
300 random scenes, odd sizes, component shapes that stress the tile-border union, squared distances within 2 ulp of
both thresholds, the 254-component cap and the kept-list bound, and the state a handle keeps between runs.  Every
comparison is exact against tests/bgsub_restatement.py (literal for small images, fast otherwise): mask bytes, box,
capped, comps_by_size, fg_count and the masked depth as uint32 bits.  The scenes are built in tests/bgsub_scenes.py."""
import warnings
from collections import defaultdict

import numpy as np
import pytest

import bgsub_restatement as R
import bgsub_scenes as S
from avatar_amd import bgsub

pytestmark = pytest.mark.gpu
ZERO = ((0, 0), (0, 0))


def ref(bg, im, nn, nb, prev=ZERO):
    """the restatement: literal up to 10k pixels, fast above"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # inf - inf, NaN arithmetic: the reference's float semantics
        f = R.literal if im.shape[0] * im.shape[1] <= 10000 else R.fast
        return f(bg, im, nn, nb, prev)


def check(got, want, what=""):
    assert np.array_equal(got["mask"], want["mask"]), f"{what}: mask, {int((got['mask'] != want['mask']).sum())} pixels differ"
    assert (got["top_left"], got["bot_right"]) == (want["top_left"], want["bot_right"]), f"{what}: box"
    assert got["capped"] == want["capped"], f"{what}: capped"
    assert got["comps"] == want["comps"], f"{what}: comps_by_size"
    assert got["fg_count"] == want["fg_count"], f"{what}: fg_count"
    assert np.array_equal(got["masked_depth"].view(np.uint32), want["masked_depth"].view(np.uint32)), f"{what}: masked depth"


def single(b, im, nn, nb, prev=ZERO, bgi=0):
    b.nnDistThreshRel, b.neighbThreshRel = nn, nb
    b.topLeft, b.botRight = prev
    mask, comps = b.run(im, comps_by_size=True, background_index=bgi)
    return dict(mask=mask, top_left=b.topLeft, bot_right=b.botRight, capped=b.capped, comps=comps, masked_depth=b.maskedDepth,
                fg_count=b.fgCount)


def _d(r):
    return dict(mask=r.mask, top_left=r.topLeft, bot_right=r.botRight, capped=r.capped, comps=r.comps_by_size, masked_depth=r.masked_depth,
                fg_count=r.fg_count)


def batch(b, ims, bgi, nn, nb, prev=None):
    """run_batch; prev: a list of ((x, y), (x, y)) boxes, or None (every slot keeps its box)"""
    b.nnDistThreshRel, b.neighbThreshRel = nn, nb
    pb = None if prev is None else np.array([[*tl, *br] for tl, br in prev], np.int32)
    return [_d(r) for r in b.run_batch(np.stack(ims), np.asarray(bgi, np.int32), pb)]


def boxes(n, seed):
    rng = np.random.default_rng(seed)
    return [((int(a), int(c)), (int(d), int(e))) for a, c, d, e in rng.integers(0, 40, (n, 4))]


def run_group(scenes, what, batch_too=True):
    """scenes: (name, (bg, im, nn, nb, prev)) of one shape.  Every scene alone through one handle holding all their
    backgrounds (image i against background i), then, per threshold pair, as one resident batch with the backgrounds
    in reverse order and random previous boxes."""
    bgs = np.stack([s[0] for _, s in scenes])
    b = bgsub.BGSubtractor(bgs)
    refs = []
    for i, (name, (bg, im, nn, nb, prev)) in enumerate(scenes):
        want = ref(bg, im, nn, nb, prev)
        check(single(b, im, nn, nb, prev, bgi=i), want, f"{what} {name}")
        refs.append(want)
    if not batch_too:
        return refs
    by_rel = defaultdict(list)
    for i, (_, s) in enumerate(scenes):
        by_rel[(s[2], s[3])].append(i)
    for (nn, nb), idx in by_rel.items():
        order = idx[::-1] + idx                   # every image twice, against two backgrounds where the group has them
        bgi = [idx[(k + 1) % len(idx)] if k < len(idx) else i for k, i in enumerate(order)]
        prev = boxes(len(order), len(order))
        got = batch(b, [scenes[i][1][1] for i in order], bgi, nn, nb, prev)
        for k, i in enumerate(order):
            want = refs[i] if bgi[k] == i and prev[k] == scenes[i][1][4] else ref(bgs[bgi[k]], scenes[i][1][1], nn, nb, prev[k])
            check(got[k], want, f"{what} batch slot {k} ({scenes[i][0]} against background {bgi[k]})")
    return refs


# ---- the known answers of the CPU tests

def test_known_answers_on_the_gpu():
    groups = defaultdict(list)
    for name, s in S.known_answer_scenes():
        groups[s[1].shape].append((name, s))
    refs = {}
    for shape, scenes in groups.items():
        for (name, _), r in zip(scenes, run_group(scenes, f"known answer {shape}")):
            refs[name] = r
    # the answers the CPU tests derive by hand hold here too (a check that the scenes are the known ones)
    assert refs["tie"]["comps"] == [(130, 0)] and refs["zero_bg_-0.0"]["comps"] == [(144, 0)] and refs["zero_bg_1e-30"]["comps"] == []
    assert refs["nan_inf_nan"]["comps"] == [(144, 0)] and refs["nan_inf_inf"]["comps"] == []
    assert refs["min_pts"]["comps"] == [(100, 0)] and refs["min_pts_minus_1"]["comps"] == []
    assert refs["cap"]["capped"] and refs["cap_exact"]["capped"] and len(refs["cap_exact"]["comps"]) == 254
    assert refs["ids_equal"]["comps"] == [(200, 1), (200, 0)]
    assert refs["denormal"]["comps"] == [(128, 0)]          # f32 denormal depths are kept, not flushed


# ---- the 300 random scenes of the CPU tests

def test_random_scenes_on_the_gpu():
    by_shape = defaultdict(list)
    for seed in range(300):
        bg, im, nn, nb = S._random_scene(seed)
        by_shape[im.shape].append((seed, (bg, im, nn, nb, S.PREV)))
    assert len(by_shape) > 200
    for shape, scenes in by_shape.items():
        run_group([(f"seed {s}", sc) for s, sc in scenes], f"random {shape}", batch_too=False)
    # a resident batch of random scenes at one size with mixed backgrounds: partial tiles both ways, 2 x 2 tiles
    scenes = [(f"seed {s}", S._random_scene(s, shape=(37, 45))[:2] + (0.0015, 0.003, S.PREV)) for s in range(12)]
    run_group(scenes, "random batch (37, 45)")


# ---- odd sizes

ODD = [(1, 1), (1, 200), (200, 1), (31, 33), (32, 32), (33, 31), (64, 64), (65, 97), (97, 1025), (721, 1279), (2, 65535)]


@pytest.mark.parametrize("shape", ODD, ids=[f"{r}x{c}" for r, c in ODD])
def test_odd_sizes(shape):
    rows, cols = shape
    k = 100 if min(shape) < 8 else None           # long runs of one level in the thin images, so something is kept
    scenes = [(f"blocky {s}", S.blocky_scene(rows, cols, seed=s, k=k)) for s in range(3)]
    refs = run_group(scenes, f"odd size {shape}", batch_too=rows * cols <= 200000)
    if rows * cols >= 1000:
        assert any(r["comps"] for r in refs), "the scenes keep no component at this size"


# ---- hard component shapes across tiles

def test_hard_shapes_across_tiles():
    scenes = S.hard_shape_scenes()                # 100 x 130: 4 x 5 tiles, partial in both directions
    wall = np.zeros_like(scenes[0][1][0])
    wall[:, :, 2] = 2.0                           # a second background: the shapes at (0, 0, 2) vanish into it
    for name, s in scenes:
        bg, im, nn, nb, prev = s
        b = bgsub.BGSubtractor(np.stack([bg, wall]))
        want = ref(bg, im, nn, nb, prev)
        check(single(b, im, nn, nb, prev), want, name)
        if name in ("serpentine", "spiral", "comb"):
            assert len(want["comps"]) == 1
        check(single(b, im, nn, nb, prev, bgi=1), ref(wall, im, nn, nb, prev), f"{name} against the wall")
    b = bgsub.BGSubtractor(np.stack([scenes[0][1][0], wall]))
    ims = [s[1] for _, s in scenes]
    bgi = [i % 2 for i in range(len(ims))]
    prev = boxes(len(ims), 5)
    for k, got in enumerate(batch(b, ims, bgi, 0.005, 0.005, prev)):
        check(got, ref((scenes[0][1][0], wall)[bgi[k]], ims[k], 0.005, 0.005, prev[k]), f"hard shapes batch slot {k}")


def test_one_full_frame_component():
    bg, im, nn, nb, prev = S.full_frame_scene()
    b = bgsub.BGSubtractor(bg)
    want = ref(bg, im, nn, nb, prev)
    assert want["comps"] == [(720 * 1280, 0)]
    check(single(b, im, nn, nb, prev), want, "full frame")


# ---- squared distances within 2 ulp of both thresholds

@pytest.mark.parametrize("shape", [(720, 1280), (301, 467)])
def test_near_threshold_fields(shape):
    (bga, ima, nn, nb, prev), ks = S.near_background_field(*shape)
    (bgb, imb, nn2, nb2, _), (coff, roff, _, _) = S.near_neighbour_field(*shape)
    assert (nn, nb) == (nn2, nb2)
    placed = ks[ks != 99]
    assert (placed < 0).mean() > 0.3 and (placed >= 0).mean() > 0.5 and (placed == 0).mean() > 0.15
    both = np.concatenate([coff, roff])
    assert (both <= 0).mean() > 0.3 and (both > 0).mean() > 0.2
    b = bgsub.BGSubtractor(np.stack([bga, bgb]))
    wa, wb = ref(bga, ima, nn, nb, prev), ref(bgb, imb, nn, nb, prev)
    assert wa["comps"] and len(wb["comps"]) > 5
    check(single(b, ima, nn, nb, prev, bgi=0), wa, "near the background threshold")
    check(single(b, imb, nn, nb, prev, bgi=1), wb, "near the join threshold")
    got = batch(b, [imb, ima], [1, 0], nn, nb, [prev, prev])
    check(got[0], wb, "batch: near the join threshold")
    check(got[1], wa, "batch: near the background threshold")


# ---- the cap and the kept-list bound across tiles

def test_cap_boundaries_across_tiles():
    scenes = [(f"{n} kept", S.cap_blocks_scene(n)) for n in (253, 254, 255)]
    scenes.append(("254 kept, no small before", S.cap_blocks_scene(254, small_before=False)))
    refs = run_group(scenes, "cap blocks")
    assert [r["capped"] for r in refs] == [False, True, True, True]
    assert [len(r["comps"]) for r in refs] == [253, 254, 254, 254]
    assert refs[0]["mask"][100, 10] == 255 and refs[1]["mask"][100, 20] == 254 and refs[2]["mask"][100, 30] == 254


@pytest.mark.parametrize("cols", [1009, 1000])
def test_kept_list_at_its_bound(cols):
    bg, im, nn, nb, prev = S.columns_scene(cols)
    far = np.zeros_like(bg)
    far[:, :, 2] = 50.0
    b = bgsub.BGSubtractor(np.stack([bg, far]))
    want = ref(bg, im, nn, nb, prev)
    assert want["capped"] and want["comps"] == [(100, i) for i in range(254)]
    check(single(b, im, nn, nb, prev), want, f"100 x {cols} columns")
    prev2 = boxes(2, cols)
    got = batch(b, [im, im[:, ::-1]], [1, 0], nn, nb, prev2)
    check(got[0], ref(far, im, nn, nb, prev2[0]), "columns batch slot 0")
    check(got[1], ref(bg, np.ascontiguousarray(im[:, ::-1]), nn, nb, prev2[1]), "columns batch slot 1")


# ---- the state a handle keeps between runs

def _state_scenes():
    """130 x 260 scenes: uncapped ones with different boxes, capped ones"""
    hard = dict(S.hard_shape_scenes(130, 260))
    unc = [S.cap_blocks_scene(253)[:2], hard["u"][:2], hard["serpentine"][:2], S.blocky_scene(130, 260, 4)[:2], hard["comb"][:2]]
    cap = [S.cap_blocks_scene(254)[:2], S.cap_blocks_scene(255)[:2], S.cap_blocks_scene(254, small_before=False)[:2]]
    return unc, cap


def test_handle_state_across_runs_and_batch_sizes():
    """one handle: single run, batch of 2, batch of 5, single run, batch of 3 without previous boxes, different scenes
    each time; every slot must hold the box of its last run"""
    unc, cap = _state_scenes()
    nn, nb = 0.005, 0.0005
    bgs = (unc[0][0], unc[3][0])                  # a zero background and the blocky scene's, near parts of its image
    b = bgsub.BGSubtractor(np.stack(bgs))
    held = {}

    def expect(i, bg, im, prev=None):
        w = ref(bg, im, nn, nb, held.get(i, ZERO) if prev is None else prev)
        held[i] = (w["top_left"], w["bot_right"])
        return w

    w = expect(0, *unc[1], prev=((3, 4), (50, 60)))
    check(single(b, unc[1][1], nn, nb, ((3, 4), (50, 60))), w, "run 1")
    steps = [[cap[0], unc[2]], [unc[3], cap[1], cap[2], unc[0], cap[0]], None, [cap[1], cap[2], cap[0]]]
    for n, step in enumerate(steps):
        if step is None:                          # a single run with an explicit previous box on slot 0
            w = expect(0, *cap[2], prev=((7, 8), (9, 10)))
            check(single(b, cap[2][1], nn, nb, ((7, 8), (9, 10))), w, "single run between batches")
            continue
        bgi = [i % 2 for i in range(len(step))]
        wants = [expect(i, bgs[bgi[i]], im) for i, (_, im) in enumerate(step)]
        for i, got in enumerate(batch(b, [im for _, im in step], bgi, nn, nb)):
            check(got, wants[i], f"step {n}, batch of {len(step)}, slot {i}")


def test_growing_a_handle_keeps_the_boxes_of_its_slots():
    """avt_bgsub.h: without prev_boxes every slot keeps the box of its previous run, (0,0),(0,0) for a slot new to the
    handle.  The box shows when a run is capped: it is reported and it masks the depth and bounds fg_count."""
    unc, cap = _state_scenes()
    nn, nb = 0.005, 0.0005
    bg = unc[0][0]
    b = bgsub.BGSubtractor(bg)
    first = batch(b, [unc[1][1], unc[2][1]], [0, 0], nn, nb)
    earlier = []
    for i, im in enumerate((unc[1][1], unc[2][1])):
        w = ref(bg, im, nn, nb)
        check(first[i], w, f"first batch slot {i}")
        earlier.append((w["top_left"], w["bot_right"]))
    assert earlier[0] != earlier[1] and ZERO not in earlier
    ims = [cap[0][1], cap[1][1], unc[3][1], cap[2][1]]
    got = batch(b, ims, [0] * 4, nn, nb)             # the handle grows from 2 slots to 4
    held = [earlier[0], earlier[1], None, ZERO]
    for i in (0, 1, 3):
        w = ref(bg, ims[i], nn, nb, held[i])
        assert w["capped"] and (w["top_left"], w["bot_right"]) == held[i]
        assert (got[i]["top_left"], got[i]["bot_right"]) == held[i], f"slot {i} lost its box when the handle grew"
        check(got[i], w, f"grown batch slot {i}")
    w = ref(bg, ims[2], nn, nb)
    check(got[2], w, "grown batch slot 2")
    held[2] = (w["top_left"], w["bot_right"])
    ims = [cap[2][1], cap[0][1], cap[1][1]]
    got = batch(b, ims, [0] * 3, nn, nb)             # no growth: each slot keeps the box it reported last
    for i in range(3):
        w = ref(bg, ims[i], nn, nb, held[i])
        assert w["capped"]
        check(got[i], w, f"third batch slot {i}")
