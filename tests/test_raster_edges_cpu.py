"""The cases of tests/raster_cases.py on the CPU: the numpy restatement of the z-buffer generator (tests/raster_restatement.py) equals
the host twin (avatar_amd/csrc/synth_render.cpp, independent code) bit for bit on every z-buffer case, every case really has the
property it was built for (the tie is a tie, the block count is 1025, the equidistant pixel is equidistant in float32, the 0.1 pair
straddles 0.1), the painter cases have theirs in the oracle's output, and a handful of answers are computed by hand.  No GPU;
tests/test_gpu_raster_edges.py demands the same arrays from the device."""
import numpy as np
import pytest

import raster_cases as rc
import raster_restatement as rr
from avatar_amd import synth

F32 = np.float32
ZGROUPS = ("edges", "rejection", "labels", "clipping", "scan", "chunks", "sequence")
_REF = {}


def _ref(case, frame=0):
    """the restatement's (depth, face, label, data, labels) of a frame: computed once, shared, never written to"""
    key = (case["name"], frame)
    if key not in _REF:
        k = case["cam"]
        res = rr.render(rc.intended_cloud(case, frame), case["mesh"], rc.vertex_part(case), k, k["width"], k["height"])
        for a in res:
            a.setflags(write=False)
        _REF[key] = res
    return _REF[key]


def _solo(case, face):
    """the restatement of the case with one face only"""
    k = case["cam"]
    return rr.render(rc.intended_cloud(case, 0), case["mesh"][face:face + 1], rc.vertex_part(case), k, k["width"], k["height"])


def _nz_ratio(case, face):
    a, b, c = (case["verts"][i] for i in case["mesh"][face])
    n = np.cross(b - a, c - a)
    return abs(n[2]) / np.linalg.norm(n)


def test_the_table_has_every_group_and_unique_names():
    names = [c["name"] for g in rc.GROUPS for c in rc.cases(g)]
    assert len(names) == len(set(names)) == 69, len(names)
    assert len(rc.zbuffer_cases()) == 55 and len(rc.cases("painter")) == 10
    for g in rc.GROUPS:
        for c in rc.cases(g):
            m = rc.model_dict(c)
            J, K = m["weights"].shape[1], m["shapedirs"].shape[2]
            assert 3 + 3 * J + K <= 179 and c["part_map"].max() < c["num_parts"] <= 64
            assert np.array_equal(synth.main_joint(m)[:-1], c["joint"]) and not (c["mesh"] == len(c["verts"])).any()


@pytest.mark.parametrize("group", ZGROUPS)
def test_restatement_equals_the_host_twin(group):
    """every z-buffer case, every frame: back-projected points, labels, and the two images"""
    failures = []
    for case in rc.cases(group):
        if case["painter"]:
            continue
        m, k = rc.model_dict(case), case["cam"]
        for f in range(len(case["trans"])):
            cloud = rc.intended_cloud(case, f)
            depth, face, label, data, labels = _ref(case, f)
            data_h, lab_h = synth.render_cloud(m, cloud, case["part_map"], intrin=k)
            xyz, mask, n = synth.render_images(m, cloud, case["part_map"], intrin=k)
            fg = label >= 0
            ok = (np.array_equal(data_h, data) and np.array_equal(lab_h, labels) and n == len(labels) and np.array_equal(mask != 255, fg)
                  and np.array_equal(mask[fg], label[fg]) and np.array_equal(xyz[:, :, 2][fg], depth[fg]) and not xyz[~fg].any())
            if not ok:
                failures.append(f"{case['name']} frame {f}: host {len(lab_h)} points, restatement {len(labels)}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("group", ZGROUPS)
def test_every_case_has_the_property_it_was_built_for(group):
    for case in rc.cases(group):
        if case["painter"]:
            continue
        name, pr, k = case["name"], case["promise"], case["cam"]
        W, H = k["width"], k["height"]
        depth, face, label, data, labels = _ref(case)
        fg = label >= 0
        if "T" in pr:
            assert [len(_ref(case, f)[4]) for f in range(len(pr["T"]))] == pr["T"], name
        for (r, c), want in pr.get("face_at", {}).items():
            assert face[r, c] == want, (name, r, c, face[r, c])
        for (r, c), want in pr.get("label_at", {}).items():
            assert label[r, c] == want, (name, r, c, label[r, c])
        solo = {}
        for (r, c), faces in pr.get("tie", []) + pr.get("both_cover", []):
            for f in faces:
                if f not in solo:
                    solo[f] = _solo(case, f)
                assert solo[f][2][r, c] >= 0, (name, "face", f, "does not cover", r, c)
        for (r, c), faces in pr.get("tie", []):
            bits = {solo[f][0][r, c].view(np.uint32) for f in faces}
            assert len(bits) == 1 and face[r, c] == min(faces), (name, r, c, bits)
        if "both_cover" in pr:                                       # depth first, then face id
            for (r, c), faces in pr["both_cover"]:
                keys = [(int(solo[f][0][r, c].view(np.uint32)), f) for f in faces]
                assert face[r, c] == min(keys)[1], (name, r, c)
        if pr.get("empty"):
            assert not fg.any(), name
        if pr.get("nonempty"):
            assert fg.sum() > 100, name
        if "faces_seen" in pr:
            assert sorted(set(face[fg].tolist())) == pr["faces_seen"], (name, sorted(set(face[fg].tolist())))
        for f in pr.get("faces_never", []):
            assert not (face == f).any(), (name, f)
        if "nz_ratio" in pr:
            f, ratio = pr["nz_ratio"]
            got = _nz_ratio(case, f)
            assert abs(got / ratio - 1.0) < 1e-9 and abs(ratio / 0.1 - 1.0) <= 0.0101 and (got < 0.1) == (ratio < 0.1), (name, got)
        for f in pr.get("nz_above", []):
            assert _nz_ratio(case, f) > 0.2, name
        px, py = rr.project(rc.intended_cloud(case, 0), k)
        for f in pr.get("denom_zero", []):
            ia, ib, ic = case["mesh"][f]
            assert (py[ib] - py[ic]) * (px[ia] - px[ic]) + (px[ic] - px[ib]) * (py[ia] - py[ic]) == F32(0.0), name
            assert len({(px[i], py[i]) for i in (ia, ib, ic)}) == 3, name
        if pr.get("depth_subnormal"):
            assert fg.any() and (depth[fg] > 0).all() and (depth[fg] < np.finfo(F32).tiny).all(), name
        for (r, c), f, which in pr.get("equidistant", []):
            assert face[r, c] == f, (name, r, c)
            d = {s: (px[v] - F32(c)) * (px[v] - F32(c)) + (py[v] - F32(r)) * (py[v] - F32(r)) for s, v in zip("abc", case["mesh"][f])}
            assert len({d[s] for s in which}) == 1, (name, r, c, d)
            assert all(d[s] > d[which[0]] for s in "abc" if s not in which), (name, r, c, d)
        if "npix" in pr:
            assert W * H == pr["npix"], name
        if "nblocks" in pr:
            assert (W * H + 255) // 256 == pr["nblocks"], name
        if "runs_straddle" in pr:
            flat = fg.reshape(-1)
            starts = np.flatnonzero(flat[1:] & ~flat[:-1]) + 1
            assert (starts % 64 != 0).any() and not flat.all(), name
            for m in pr["runs_straddle"]:
                i = np.arange(m, len(flat), m)
                assert (flat[i] & flat[i - 1]).any(), (name, m)                 # a run goes on across a multiple of m
        if "beyond_int" in pr:
            for v in pr["beyond_int"]:
                assert max(abs(float(px[v])), abs(float(py[v]))) > 2.0 ** 31, (name, v)
        if "crosses_chunk" in pr:
            assert (len(case["trans"]) > rc.chunk_frames(W, H, False)) == pr["crosses_chunk"], name
        if pr.get("frames_differ"):
            n = len(case["trans"])
            assert len({_ref(case, f)[3].tobytes() for f in range(n)}) == n and all(len(_ref(case, f)[4]) > 1000 for f in range(n)), name
        if case["exact"]:                                            # every vertex in a face lands on the coordinate it was given
            used = np.unique(case["mesh"])
            assert np.array_equal(px[used], np.round(px[used] * 2) / 2) and np.array_equal(py[used], np.round(py[used] * 2) / 2), name


def test_chunk_formula_and_frame_counts():
    """avt_synth_render_frames_mode (avt_capi.cpp) renders chunks of (256 MiB) / (npix * 9 + 64) frames, npix * 21 in painter's mode:
    8 bytes of key and 1 of label per pixel, and another key, a float and the per-face arrays for the painter.  The chunk cases cross it."""
    W, H = rc.K4A_SIZE
    assert rc.chunk_frames(W, H, False) == 32 and rc.chunk_frames(W, H, True) == 13
    n = {c["name"]: (len(c["trans"]), c["painter"]) for c in rc.cases("chunks")}
    assert n == {"chunk-zbuffer-33": (33, False), "chunk-painter-14": (14, True), "chunk-painter-13": (13, True)}
    for c in rc.cases("chunks"):
        assert (c["cam"]["width"], c["cam"]["height"]) == (W, H)
        assert (len(c["trans"]) > rc.chunk_frames(W, H, c["painter"])) == c["promise"]["crosses_chunk"]
    seq = [(c["cam"]["width"], c["cam"]["height"], c["painter"]) for c in rc.cases("sequence")]
    assert seq == [(1280, 720, False), (17, 31, False), (64, 48, True), (640, 410, False), (1280, 720, True)]


def test_known_answers():
    # the right triangle with legs of 16 pixels: 17 * 18 / 2 lattice points, all at depth 2, first point from pixel (4, 3)
    case = rc.by_name("edge-right-triangle")
    depth, face, label, data, labels = _ref(case)
    assert len(labels) == 153 and (depth[label >= 0] == 2.0).all()
    assert [int(x) for x in (label >= 0).sum(1)[3:20]] == list(range(17, 0, -1))
    assert np.array_equal(data[0], [(4 - 16) * 2 / 128, -(3 - 12) * 2 / 128, 2.0]) and np.array_equal(data[-1], [(4 - 16) * 2 / 128, -(19 - 12) * 2 / 128, 2.0])
    assert label[3, 4] == 1 and label[3, 20] == 2 and label[19, 4] == 3 and label[3, 12] == 2     # (12, 3) is 8 from a and from b: b
    # the split square: 17 x 17 pixels, the 17 diagonal ones from face 0 whichever way the mesh lists the two
    for name in ("edge-shared-diagonal", "edge-shared-diagonal-swapped"):
        depth, face, label, data, labels = _ref(rc.by_name(name))
        assert (face >= 0).sum() == 289 and all(face[3 + i, 20 - i] == 0 for i in range(17))
        assert all(depth[3 + i, 20 - i] == F32(2.0625) for i in range(17)) and depth[3, 4] == 2.0 and depth[19, 20] == 2.0
    # near in front of far, whatever the order
    for name in ("depth-near-after-far", "depth-near-before-far"):
        depth = _ref(rc.by_name(name))[0]
        assert depth[8, 8] == 1.0 and depth[2, 3] == 4.0 and np.isinf(depth[23, 31])
    # a covered image has a point for every pixel, in row-major order
    for W, H in rc.SIZES:
        depth, face, label, data, labels = _ref(rc.by_name(f"clip-covered-{W}x{H}"))
        assert len(labels) == W * H
        k = rc.cam(W, H)
        cols = np.rint(data[:, 0] * k["fx"] / data[:, 2] + k["cx"]).astype(int)
        rows = np.rint(-data[:, 1] * k["fy"] / data[:, 2] + k["cy"]).astype(int)
        assert np.array_equal(rows * W + cols, np.arange(W * H))
    # the vertex at float depth 0 on the optical axis: its own pixel is the only hole of the quadrant
    face = _ref(rc.by_name("vertex-z-1e-300-on-axis"))[1]
    assert (face[12:, 16:] == 0).sum() == 12 * 16 - 1 and face[12, 16] == -1 and (face[:12] == -1).all() and (face[:, :16] == -1).all()


def test_out_of_range_projection_is_drawn_by_the_host_twin():
    """Before the bounds were clamped in float, the host converted ceil(2.5e9) to INT_MIN and dropped this face whole (0 points), while
    the device's conversion saturates.  Now both paint up to the image border: 540 points."""
    case = rc.by_name("overflow-x-max")
    k = case["cam"]
    assert np.array_equal(case["verts"], [[0, 0, 2], [0, 0.2, 2], [1, 0, 4e-8]]) and (k["fx"], k["cx"], k["cy"], k["width"]) == (100.0, 10.0, 40.0, 64)
    data_h, lab_h = synth.render_cloud(rc.model_dict(case), rc.intended_cloud(case, 0), case["part_map"], intrin=k)
    assert len(lab_h) == 540 == len(_ref(case)[4]) and np.array_equal(data_h, _ref(case)[3])
    counts = {n: len(_ref(rc.by_name(n))[4]) for n in ("overflow-x-min", "overflow-y-min", "overflow-y-max")}
    assert counts == {"overflow-x-min": 110, "overflow-y-min": 410, "overflow-y-max": 240}, counts
    assert rr.clamped_box(F32(-3e9), F32(2.5e9), 64) == (0, 63) and rr.clamped_box(F32(2.5e9), F32(3e9), 64) == (64, 63)
    assert rr.clamped_box(F32(-3e9), F32(-2.5e9), 64) == (0, -1) and rr.clamped_box(F32(np.inf), F32(np.inf), 64) == (64, 63)
    assert rr.clamped_box(F32(2.25), F32(7.5), 64) == (2, 8) and rr.clamped_box(F32(-0.5), F32(63.5), 64) == (0, 63)


def test_default_camera_of_the_host_helpers_is_unchanged(smpl):
    w, p, R = synth.sample_ground_truth(smpl, 0)
    verts = synth.pose_vertices(smpl, w, p, R)
    pm = synth.identity_part_map()
    d0, l0 = synth.render_cloud(smpl, verts, pm)
    d1, l1 = synth.render_cloud(smpl, verts, pm, intrin=synth.K4A_INTRIN)
    assert np.array_equal(d0, d1) and np.array_equal(l0, l1) and 15000 < len(l0) < 60000


# ---- painter cases: what each was built for, in the oracle's output ---------------------------------------------------------------
def _oracle(case):
    from oracle import render_oracle as ro
    k = case["cam"]
    depth, mask = ro.render(rc.intended_cloud(case, 0), case["mesh"], rc.vertex_part(case), k, k["width"], k["height"], stable=True)
    return depth, mask, ro.backproject(depth, mask, k)


def test_painter_cases_have_the_property_they_were_built_for():
    for case in rc.cases("painter"):
        name, pr = case["name"], case["promise"]
        depth, mask, (data, labels) = _oracle(case)
        assert (depth > 0).sum() == len(labels) > 20, name
        for (r, c), want in pr.get("depth_at", {}).items():
            assert abs(depth[r, c] - want) < 1e-6, (name, r, c, depth[r, c])
        for (r, c), want in pr.get("mask_at", {}).items():
            assert mask[r, c] == want, (name, r, c, mask[r, c])
        for f in pr.get("edge_on", []):
            assert _nz_ratio(case, f) < 0.1, name
        if "holes_in_row" in pr:
            row = depth[pr["holes_in_row"]]
            holes = np.flatnonzero(row[18:30] == 0) + 18
            assert len(holes) >= 3 and (mask[pr["holes_in_row"], holes] == 255).all() and abs(row[holes.max() + 1] - 5.0) < 1e-6, name
            assert len(labels) == (depth > 0).sum() < (_oracle(dict(case, mesh=case["mesh"][:1]))[0] > 0).sum(), name
        if pr.get("equal_keys"):
            z = rc.intended_cloud(case, 0)[:, 2]
            keys = [F32((z[a] + z[b] + z[c]) / F32(3.0)) for a, b, c in case["mesh"]]
            assert keys[0] == keys[1], name
            d0, d1 = (_oracle(dict(case, mesh=case["mesh"][f:f + 1]))[0] for f in (0, 1))
            both = (d0 > 0) & (d1 > 0)
            assert both.sum() > 50 and (d0[both] != d1[both]).sum() > 50 and np.array_equal(depth[both], d1[both]), name      # the later face id is painted last
        if "depth_all" in pr:
            assert (depth[depth > 0] == pr["depth_all"]).all() and (data[:, 2] == pr["depth_all"]).all(), name
        if pr.get("label_255"):
            assert ((depth > 0) & (mask == 255)).any() and (labels == 255).any() and (labels != 255).any(), name
        if "beyond_int" in pr:
            px, py = rr.project(rc.intended_cloud(case, 0), case["cam"])
            assert all(max(abs(float(px[v])), abs(float(py[v]))) > 2.0 ** 31 for v in pr["beyond_int"]), name
    for c in rc.cases("chunks") + rc.cases("sequence"):
        if c["painter"]:
            assert (_oracle(c)[0] > 0).sum() > (1000 if c["cam"]["width"] > 64 else 100), c["name"]
