"""ark::AvatarRenderer on the GPU (avatar_amd/csrc/avt_render.hip: k_rend_project, k_rend_faces, k_rend_sort, k_rend_scatter, k_rend_vnormal,
k_rend_cover, k_rend_resolve, k_paint_rank) on the cases of tests/avatar_render_cases.py, every comparison an array equality against the
CPU restatement of the reference's renderer (tests/test_avatar_render_edges_cpu.py checks the restatement and what each case promises):
the four images, the projections, the painter order, the per-vertex shading; under both orderings, which must agree with each other as
well.  The non-finite group (NaN sort keys, where the reference is undefined) is held to the project's own order instead: a permutation,
the same from the sort and from the rank count."""
import numpy as np
import pytest

import avatar_render_cases as ac

pytestmark = pytest.mark.gpu

IMAGES = ("depth", "mask", "lambert", "faces")
_MODELS = {}


def _model(case):
    if case["name"] not in _MODELS:
        _MODELS[case["name"]] = ac.model_of(case)
    return _MODELS[case["name"]]


def _renderer(case, max_images=None):
    from avatar_amd import render
    rend = render.Renderer(_model(case), case["size"][0], case["size"][1], case["intr"], len(case["clouds"]) if max_images is None else max_images)
    if case["part_map"] is not None:
        rend.set_part_map(case["part_map"])
    return rend


def _outputs(rend, i, joints=True):
    """everything the handle returns for image i after run(ALL), as one dict"""
    out = dict(rend.download(i))
    out.update(rend.projection(i, joints=joints))
    out["vnormal"], out["lambert_v"] = rend.vertex_shading(i)
    return out


def _run(case, ordering, images=None):
    from avatar_amd import render
    idx = list(range(len(case["clouds"]))) if images is None else images
    rend = _renderer(case, len(idx))
    rend.set_ordering(ordering)
    rend.upload(case["clouds"][idx], None if case["joints"] is None else case["joints"][idx])
    rend.run(render.ALL)
    return [_outputs(rend, i, case["joints"] is not None) for i in range(len(idx))]


def _against_reference(case, got, image, what):
    ref, bad = ac.reference(case, image), []
    for k in IMAGES + ("points", "keys", "ordered") + (("joints",) if case["joints"] is not None else ()):
        if not np.array_equal(got[k], ref[k]):
            bad.append(f"{k} ({int((got[k] != ref[k]).sum())} entries)")
    for k in ("vnormal", "lambert_v"):
        if not np.array_equal(got[k], ref[k], equal_nan=True):
            bad.append(k)
    pos = np.empty(len(case["mesh"]), np.int64)
    pos[ac.numpy_order(ac.keys_of(case, image))] = np.arange(len(case["mesh"]))
    if not np.array_equal(got["pos"], pos):
        bad.append("pos")
    return [f"{case['name']} image {image} {what}: " + ", ".join(bad)] if bad else []


def _check_case(case):
    from avatar_amd import render
    failures = []
    by_sort, by_rank = _run(case, render.ORDER_SORT), _run(case, render.ORDER_RANK)
    for i, (a, b) in enumerate(zip(by_sort, by_rank)):
        failures += _against_reference(case, a, i, "sorted") + _against_reference(case, b, i, "ranked")
        differ = [k for k in a if not np.array_equal(a[k], b[k], equal_nan=k in ("vnormal", "lambert_v"))]
        if differ:
            failures.append(f"{case['name']} image {i}: the two orderings differ in {differ}")
    return failures


def _names(group):
    return [c["name"] for c in ac.cases(group)]


@pytest.mark.parametrize("name", _names("order"))
def test_order_cases(name):
    """stacks of 1 .. 16385 coincident faces: every width of the bitonic sort, with and without padding, a thread owning a real and a padding
    entry, the hand-over to the rank count at 16385 (where both settings take it); keys increasing, decreasing, shuffled, all equal, in two
    long tied runs, one ulp apart, negative, +0 and -0, subnormal, infinite; three images that order their faces differently"""
    case = ac.by_name(name)
    assert ac.measure(case)["rank_path"] == (len(case["mesh"]) > 16384)
    assert _check_case(case) == []


@pytest.mark.parametrize("group", ["shading", "fill", "parts", "tails"])
def test_cases_of_the_other_groups(group):
    """shading: valence 700, a vertex named twice and three times by one face, a vertex in no face, sums that cancel, vertices on the lights,
    n_z > 0 and exactly 0, |n_z| around 0.1 and 1e-2 and exactly on them; fill: integer vertices, flat tops and bottoms, the middle vertex
    outside, a covered image, faces outside, projections beyond int, z = 0 and z < 0, depths above 255, images of 1x1 .. 257x1, both
    windings; parts: values beyond a byte; tails: V and F at 255 / 256 / 257, more joints than vertices, one joint"""
    failures = []
    for case in ac.cases(group):
        failures += _check_case(case)
    assert not failures, "; ".join(failures)


def test_batch_of_three_equals_three_single_runs():
    from avatar_amd import render
    case = ac.by_name("batch-1025x3")
    for ordering in (render.ORDER_SORT, render.ORDER_RANK):
        batch = _run(case, ordering)
        assert len({b["pos"].tobytes() for b in batch}) == 3
        for i in range(3):
            alone = _run(case, ordering, images=[i])[0]
            for k in batch[i]:
                assert np.array_equal(batch[i][k], alone[k], equal_nan=True), f"image {i}: batched {k} differs from the single run"


@pytest.mark.parametrize("name", _names("non-finite"))
def test_nan_keys_take_their_place_in_one_total_order(name):
    """NaN sort keys of both signs among finite and infinite ones: under both orderings the positions are a permutation of 0 .. F - 1, the
    same permutation, the keys that are not NaN keep the order numpy gives them, and the projection is served (it refuses an order that is
    no permutation).  Before k_paint_rank compared the mapped bit patterns it gave every NaN-key face position 0."""
    from avatar_amd import render
    case = ac.by_name(name)
    F = len(case["mesh"])
    keys = ac.keys_of(case)
    rest = np.flatnonzero(~np.isnan(keys))
    got = {}
    for ordering in (render.ORDER_SORT, render.ORDER_RANK):
        rend = _renderer(case)
        rend.set_ordering(ordering)
        rend.upload(case["clouds"], case["joints"])
        rend.run(render.ALL)
        p = rend.projection(0)
        pos = p["pos"]
        assert np.array_equal(np.sort(pos), np.arange(F)), f"{name} ordering {ordering}: positions are no permutation"
        assert np.array_equal(rest[np.argsort(pos[rest])], rest[ac.numpy_order(keys[rest])]), f"{name} ordering {ordering}: finite keys out of order"
        assert np.array_equal(p["ordered"], case["mesh"][np.argsort(pos)])
        got[ordering] = pos
    assert np.array_equal(got[render.ORDER_SORT], got[render.ORDER_RANK])


def _shifted(case, n=3):
    """n images of a one-image case: the cloud moved sideways a little more in each"""
    cl = np.stack([case["clouds"][0] + [0.05 * i, -0.03 * i, 0.01 * i] for i in range(n)])
    jt = np.stack([case["joints"][0] + [0.02 * i, 0.0, 0.0] for i in range(n)])
    return dict(case, name=f"{case['name']} in {n} places", clouds=cl, joints=jt)


def test_handle_bookkeeping_across_runs_and_uploads():
    """one renderer of three images: what the last run rendered is what download serves, nothing is stale after a run of other outputs, a
    smaller upload and an upload without joints take effect, and the lazily grown key images end where a fresh handle's do"""
    from avatar_amd import render
    from avatar_amd.capi import AvtError
    case = _shifted(ac.by_name("tails-V257-F255"))
    ref = [ac.reference(case, i) for i in range(3)]
    rend = _renderer(case, 3)
    rend.upload(case["clouds"], case["joints"])
    with pytest.raises(AvtError, match="no run since"):
        rend.download(0, render.DEPTH)
    rend.run(render.DEPTH)
    assert np.array_equal(rend.download(2, render.DEPTH)["depth"], ref[2]["depth"])
    with pytest.raises(AvtError, match="did not render"):
        rend.download(0, render.LAMBERT)
    with pytest.raises(AvtError, match="Lambert"):
        rend.vertex_shading(0)
    rend.run(render.LAMBERT)
    for i in range(3):
        assert np.array_equal(rend.download(i, render.LAMBERT)["lambert"], ref[i]["lambert"])
        assert np.array_equal(rend.vertex_shading(i)[1], ref[i]["lambert_v"], equal_nan=True)
    with pytest.raises(AvtError, match="did not render"):
        rend.download(0, render.DEPTH)
    rend.run(0)
    p = rend.projection(1)
    assert all(np.array_equal(p[k], ref[1][k]) for k in ("points", "joints", "keys", "ordered"))
    for what in (render.DEPTH, render.PART_MASK, render.LAMBERT, render.FACES):
        with pytest.raises(AvtError, match="did not render"):
            rend.download(1, what)
    # one image after three: images 1 and 2 are gone, and image 0 is the new one
    rend.upload(case["clouds"][2], case["joints"][2])
    with pytest.raises(AvtError, match="no run since"):
        rend.projection(0)
    rend.run(render.FACES | render.PART_MASK)
    got = rend.download(0, render.FACES | render.PART_MASK)
    assert np.array_equal(got["faces"], ref[2]["faces"]) and np.array_equal(got["mask"], ref[2]["mask"])
    for i in (1, 2):
        with pytest.raises(AvtError, match="bad image"):
            rend.download(i, render.FACES)
        with pytest.raises(AvtError, match="bad image"):
            rend.projection(i)
    # no joints after joints
    rend.upload(case["clouds"][:2])
    rend.run(render.DEPTH)
    for i in (0, 1):
        with pytest.raises(AvtError, match="no joints"):
            rend.projection(i, joints=True)
        assert np.array_equal(rend.projection(i, joints=False)["points"], ref[i]["points"])
    # every output after runs with fewer: what a fresh handle gives, and the restatement
    rend.upload(case["clouds"], case["joints"])
    rend.run(render.ALL)
    fresh = _run(case, render.ORDER_SORT)
    for i in range(3):
        got = _outputs(rend, i)
        for k in got:
            assert np.array_equal(got[k], fresh[i][k], equal_nan=True), f"image {i}: {k} differs from a fresh handle's"
        assert _against_reference(case, got, i, "after smaller runs") == []
