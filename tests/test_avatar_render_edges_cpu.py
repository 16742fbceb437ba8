"""The cases of tests/avatar_render_cases.py on the CPU: every case really has the property it was built for, and the restatement of the
reference's renderer (tests/cpp/avatar_renderer_restatement.cpp) is checked on them before tests/test_gpu_avatar_render_edges.py trusts
it: its painter order against plain numpy, the face a stack shows, its vertex normals against a long-double sum, a handful of answers
worked out by hand.  The non-finite group is never given to the restatement (std::sort and stable_sort are undefined on NaN keys); a
numpy transcription of k_paint_rank, as it was and as it is, shows what the device does with them.  No GPU."""
import numpy as np
import pytest

import avatar_render_cases as ac

F32 = np.float32
LD = np.longdouble
RESTATEMENT_CAP_SECONDS = 2.0       # per case and image, the largest (F = 16385) included; 0.05 s measured for it
# Vertex normals, restatement (doubles, summed in painter order) against the long-double sum of this file, over every vertex of every
# restated case whose summed normal is at least 0.5 long: the largest difference measured is 9.2e-15 (shade-fan-700: the hub's 700-term
# sum in doubles); ten times that for the order-dependence of a 700-term sum (docs/MEASURED_HISTORY.md).
VNORMAL_MEASURED, VNORMAL_BOUND = 9.2e-15, 9.2e-14


def _restated():
    return [c for g in ac.RESTATED for c in ac.cases(g)]


def test_the_table_has_every_group_and_unique_names():
    names = [c["name"] for g in ac.GROUPS for c in ac.cases(g)]
    assert len(names) == len(set(names)) == 81, len(names)
    assert {g: len(ac.cases(g)) for g in ac.GROUPS} == {"order": 37, "non-finite": 2, "shading": 10, "fill": 20, "parts": 1, "tails": 11}
    stacks = sorted(c["promise"]["F"] for c in ac.cases("order") if c["name"].startswith("stack-shuffle-"))
    assert stacks == [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 16383, 16384, 16385]
    for pattern in ("increasing", "decreasing", "shuffle", "equal", "two-runs", "ulp", "negative", "zeros", "subnormal", "inf"):
        sizes = sorted(len(c["mesh"]) for c in ac.cases("order") if c["name"].startswith(f"stack-{pattern}-"))
        assert 1025 in sizes and any(s != 1025 and min(abs(s - p) for p in (256, 512, 1024, 2048, 4096)) == 1 for s in sizes), (pattern, sizes)
    for c in _restated() + ac.cases("non-finite"):
        W, H = c["size"]
        assert (W <= 64 and H <= 48) or (W, H) in ac.SIZES, c["name"]
        assert 3 + 3 * c["n_joints"] + 1 <= 179, c["name"]


def test_a_model_of_300_joints_cannot_be_created():
    """J = 300 with V = 3 would give k_rend_project a second workgroup of joints only; avt_model_create refuses it (J <= 64, and 3 + 3 J + K <= 179), so
    the tails group stops at the 58 joints a model can have"""
    from avatar_amd import capi
    tri = ac.by_name("tails-J58-V3")["clouds"][0]
    with pytest.raises(capi.AvtError, match="J<=64"):
        ac.tiny_model(tri, [[0, 1, 2]], joint=[299, 0, 150], n_joints=300)
    assert ac.tiny_model(tri, [[0, 1, 2]], joint=[57, 0, 31], n_joints=58).numJoints() == 58


@pytest.mark.parametrize("group", list(ac.GROUPS))
def test_every_promise_holds(group):
    for case in ac.cases(group):
        got = ac.measure(case)
        assert case["promise"], case["name"]
        for k, want in case["promise"].items():
            assert k in got and got[k] == want, (case["name"], k, got.get(k), want)


@pytest.mark.parametrize("group", ac.RESTATED)
def test_the_restatement_runs_on_every_case_within_its_time_cap(group):
    for case in ac.cases(group):
        for i in range(len(case["clouds"])):
            o = ac.reference(case, i)
            assert ac.RESTATEMENT_SECONDS[(case["name"], i)] < RESTATEMENT_CAP_SECONDS, (case["name"], ac.RESTATEMENT_SECONDS[(case["name"], i)])
            assert not np.isnan(o["points"]).any() and not np.isnan(o["keys"]).any(), case["name"]      # array_equal can compare them


# ---- order --------------------------------------------------------------------------------------------------------------------------
def test_restated_order_is_numpys():
    """decreasing float32 key, equal keys (-0 and +0 among them) by ascending face id"""
    for case in _restated():
        for i in range(len(case["clouds"])):
            keys = ac.keys_of(case, i)
            order = ac.numpy_order(keys)
            o = ac.reference(case, i)
            assert np.array_equal(o["ordered"], case["mesh"][order]), case["name"]
            assert np.array_equal(o["keys"].view(np.uint32), keys[order].view(np.uint32)), case["name"]         # the sign of a zero too


def test_a_stack_shows_the_face_painted_last():
    """at every covered pixel of a stack, `faces` holds the position of the smallest key among the faces that paint, the largest face id
    among ties; and what the position says about the faces that paint nothing"""
    seen = 0
    for case in ac.cases("order"):
        for i in range(len(case["clouds"])):
            keys, vis = ac.keys_of(case, i), ac.stack_visible(case, i)
            pos = np.empty(len(keys), np.int64)
            pos[ac.numpy_order(keys)] = np.arange(len(keys))
            img = ac.reference(case, i)["faces"]
            if not vis.any():
                assert (img == -1).all(), case["name"]
                continue
            ids = np.flatnonzero(vis)
            winner = ids[keys[ids] == keys[ids].min()].max()
            assert (img >= 0).sum() >= 40 and (img[img >= 0] == pos[winner]).all(), (case["name"], pos[winner], np.unique(img))
            assert (img[:2] == -1).all() and (img[:, 15:] == -1).all(), case["name"]
            seen += 1
    assert seen == 39


def _rank(keys, bits):
    """k_paint_rank in numpy: position = number of faces with a key painted earlier, or the same key and a smaller face id.  bits=False
    compares the floats (the kernel before), bits=True the mapped 32-bit patterns (painter_key_bits, the kernel now and k_rend_sort)."""
    g = np.arange(len(keys))
    if bits:
        k = ac.key_bits(keys)
        first, same = k[None, :] < k[:, None], k[None, :] == k[:, None]
    else:
        with np.errstate(invalid="ignore"):
            first, same = keys[None, :] > keys[:, None], keys[None, :] == keys[:, None]
    return (first | (same & (g[None, :] < g[:, None]))).sum(1)


def test_rank_count_on_float_compares_is_no_permutation_on_nan_keys():
    """The finding: comparing floats, every NaN-key face counts nothing before it (position 0), positions collide and entries of `order`
    stay unwritten; no position exceeds the number of keys that are not NaN, so nothing was read out of bounds.  Comparing the mapped
    patterns gives a permutation: positive NaN first, negative NaN last, every other key where numpy puts it."""
    for case in ac.cases("non-finite"):
        keys = ac.keys_of(case)
        F, nan = len(keys), np.isnan(keys)
        old = _rank(keys, bits=False)
        assert (old[nan] == 0).all() and len(set(old.tolist())) < F and old.max() < (~nan).sum(), case["name"]
        new = _rank(keys, bits=True)
        assert np.array_equal(np.sort(new), np.arange(F)), case["name"]
        words = (ac.key_bits(keys).astype(np.uint64) << np.uint64(32)) | np.arange(F, dtype=np.uint64)      # what k_rend_sort sorts
        assert np.array_equal(np.argsort(words), np.argsort(new)), case["name"]
        npos, nneg = case["promise"]["nan_keys"]
        assert set(new[nan & ~np.signbit(keys)].tolist()) == set(range(npos)) and set(new[nan & np.signbit(keys)].tolist()) == set(range(F - nneg, F))
        rest = np.flatnonzero(~nan)
        assert np.array_equal(rest[np.argsort(new[rest])], rest[ac.numpy_order(keys[rest])]), case["name"]


def test_rank_count_on_patterns_is_the_float_order_on_every_other_key():
    for case in ac.cases("order"):
        if len(case["mesh"]) > 4097:
            continue
        for i in range(len(case["clouds"])):
            keys = ac.keys_of(case, i)
            pos = np.empty(len(keys), np.int64)
            pos[ac.numpy_order(keys)] = np.arange(len(keys))
            assert np.array_equal(_rank(keys, bits=True), pos) and np.array_equal(_rank(keys, bits=False), pos), case["name"]


# ---- vertex normals -----------------------------------------------------------------------------------------------------------------
def _long_double_normals(cloud, mesh):
    """face normals, summed over incident slots (a face that names a vertex twice adds twice), normalised, turned to face the camera"""
    cl = cloud.astype(LD)
    a, b, c = (cl[mesh[:, i]] for i in range(3))
    ab, ac_ = b - a, c - a
    n = np.stack([ab[:, 1] * ac_[:, 2] - ab[:, 2] * ac_[:, 1], ab[:, 2] * ac_[:, 0] - ab[:, 0] * ac_[:, 2], ab[:, 0] * ac_[:, 1] - ab[:, 1] * ac_[:, 0]], 1)
    z = (n * n).sum(1)
    n = np.where((z > 0)[:, None], n / np.sqrt(np.where(z > 0, z, LD(1)))[:, None], n)
    vs = np.zeros((len(cl), 3), LD)
    np.add.at(vs, mesh.reshape(-1), np.repeat(n, 3, 0))
    norm = np.sqrt((vs * vs).sum(1))
    unit = vs / np.where(norm > 0, norm, LD(1))[:, None]
    return np.where((unit[:, 2] > 0)[:, None], -unit, unit), norm


def test_restated_vertex_normals_against_a_long_double_sum():
    worst, where, checked = 0.0, None, 0
    for case in _restated():
        for i in range(len(case["clouds"])):
            with np.errstate(all="ignore"):
                want, norm = _long_double_normals(case["clouds"][i], case["mesh"])
            got = ac.reference(case, i)["vnormal"]
            ok = np.isfinite(norm.astype(np.float64)) & (norm >= 0.5)
            if not ok.any():
                continue
            d = float(np.abs(got[ok].astype(LD) - want[ok]).max())
            checked += int(ok.sum())
            if d > worst:
                worst, where = d, case["name"]
    print(f"vertex normals: largest difference {worst:.3e} ({where}), {checked} vertices, bound {VNORMAL_BOUND:.1e}")
    assert checked > 100000 and worst <= VNORMAL_BOUND, (worst, where)
    hub = ac.reference(ac.by_name("shade-fan-700"))["vnormal"][0]
    assert abs(np.linalg.norm(hub) - 1.0) < 1e-15 and hub[2] < -0.9
    iso = ac.reference(ac.by_name("shade-vertex-in-no-face"))
    assert np.isnan(iso["vnormal"][3]).all() and np.isnan(iso["lambert_v"][3]) and np.isfinite(iso["vnormal"][:3]).all()
    assert np.isnan(ac.reference(ac.by_name("shade-normals-cancel-exactly"))["vnormal"][:3]).all()
    assert np.isfinite(ac.reference(ac.by_name("shade-normals-cancel-almost"))["vnormal"]).all()
    sign = ac.reference(ac.by_name("shade-nz-positive-negative-zero"))["vnormal"]
    assert np.array_equal(sign[:6], np.tile([0.0, 0.0, -1.0], (6, 1))) and np.array_equal(sign[6:], np.tile([0.0, -1.0, 0.0], (3, 1)))
    lights = ac.reference(ac.by_name("shade-vertices-on-the-lights"))
    assert np.isfinite(lights["lambert_v"]).all() and np.isfinite(lights["vnormal"]).all()


def test_the_faces_around_the_lambert_rule_are_lit_or_not():
    """|n_z| exactly 1e-2 is not `> 1e-2`: painted by renderFaces, dark in renderLambert although its vertices are lit; the face a little
    above the rule shows them"""
    at_rule, above = ac.reference(ac.by_name("shade-nz-alone-=1e-2")), ac.reference(ac.by_name("shade-nz-alone-<0.1"))
    assert (at_rule["faces"] >= 0).sum() > 20 and (at_rule["lambert"] == 0).all() and (at_rule["lambert_v"] > 10).all()
    assert (above["lambert"] > 10).sum() > 20
    both = ac.reference(ac.by_name("shade-nz-around-0.1-and-1e-2"))
    assert (both["depth"] > 0).any() and (both["lambert"] > 0).any()


# ---- answers by hand ----------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_fill_group():
    o = ac.reference(ac.by_name("fill-whole-image"))
    assert (np.abs(o["depth"] - 2.0) < 1e-4).all() and (o["mask"] == 0).all() and (o["lambert"] > 0).all()
    # the single-colour fill leaves the last column out, and with a flat top (ay == by) it starts one row below the middle vertex's, clamped to 0
    assert (o["faces"][1:, :-1] == 0).all() and (o["faces"][:, -1] == -1).all() and (o["faces"][0] == -1).all()
    o = ac.reference(ac.by_name("fill-outside-on-four-sides"))
    assert (o["depth"] == 0).all() and (o["mask"] == 255).all() and (o["lambert"] == 0).all() and (o["faces"] == -1).all()
    o = ac.reference(ac.by_name("fill-size-1x1"))
    assert o["depth"].shape == (1, 1) and o["depth"][0, 0] > 0 and o["mask"][0, 0] == 0 and o["faces"][0, 0] == -1
    o = ac.reference(ac.by_name("fill-depth-above-255"))
    assert o["depth"].max() == 255.0 and (o["depth"][:, :15][o["depth"][:, :15] > 0] == 255.0).all() and (o["depth"][:, :15] > 0).sum() > 50
    right = o["depth"][:, 16:]
    assert ((right > 250) & (right < 255)).sum() > 10 and (right == 255.0).sum() > 10
    o = ac.reference(ac.by_name("fill-integer-vertices"))
    assert o["ordered"][0].tolist() == [3, 4, 5] and (o["faces"] != 0).all() and (o["faces"] == 1).sum() > 100       # row 21's triangle paints nothing
    assert o["depth"][3, 4] == 2.0 and o["depth"][19, 4] == 2.0 and o["depth"][3, 20] == 2.0 and o["depth"][21].max() == 0
    for name in ("x-max", "x-min", "y-min", "y-max"):
        assert (ac.reference(ac.by_name("fill-beyond-int-" + name))["faces"] >= 0).sum() >= 0       # it returns; the device must paint the same


def test_known_answers_of_the_parts_group():
    """(unsigned char) of the part: 256 -> 0, 511 -> 255, -1 -> 255 (the background's value); 0, 23, 254 and 255 as they are"""
    o = ac.reference(ac.by_name("parts-beyond-a-byte"))
    want = {0: 0, 1: 23, 2: 254, 3: 255, 4: 0, 5: 255, 6: 255}
    for t, value in want.items():
        x0, y0 = 2 + 15 * (t % 4), 3 + 22 * (t // 4)
        assert o["faces"][y0 + 6, x0 + 5] >= 0 and o["mask"][y0 + 6, x0 + 5] == value, (t, o["mask"][y0 + 6, x0 + 5])
    last = o["mask"][26:45, 47:63]
    assert {0, 23} <= set(np.unique(last).tolist()) <= {0, 23, 255}
