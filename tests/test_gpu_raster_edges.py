"""The synthetic depth-frame generator (avt_synth_render_frames[_mode]; k_raster, k_raster_label, k_raster_scan, k_raster_emit and the
k_paint_* hand-over of avatar_amd/csrc/avt_render.hip) at its edges, every comparison an array equality: point counts, back-projected
points and labels against the numpy restatement (tests/raster_restatement.py; tests/test_raster_edges_cpu.py ties it to the host twin
and checks what each case promises, tests/raster_cases.py builds the cases), and in painter's mode the two images as well, against
oracle/render_oracle.  The expectation of a frame is always computed from the cloud that lbs_update returns for it."""
import numpy as np
import pytest

import raster_cases as rc
import raster_restatement as rr

pytestmark = pytest.mark.gpu

_MODELS = {}
_EXPECTED = {}


def _model(case):
    """one AvatarModel per mesh, kept for the module (cases that share vertices, joints and faces share it)"""
    from avatar_amd import api
    key = (case["verts"].tobytes(), case["joint"].tobytes(), case["mesh"].tobytes())
    if key not in _MODELS:
        _MODELS[key] = api.AvatarModel(rc.model_dict(case))
    return _MODELS[key]


def _context(case, max_points=None, frames=None):
    from avatar_amd import api
    k = case["cam"]
    if max_points is None:                       # small images: every pixel; large ones: the intended cloud's count and a margin
        npix = k["width"] * k["height"]
        max_points = npix if npix <= 4096 else min(npix, _expect(case, rc.intended_cloud(case, 0))["N"] * 2 + 4096)
    return api.Context(_model(case), case["num_parts"], case["part_map"], max_points, len(case["trans"]) if frames is None else frames, device=0)


def _expect(case, cloud):
    """what a frame of the case must be, from its posed cloud: the restatement in z-buffer mode, the reference's renderer in painter's"""
    k = case["cam"]
    key = (case["name"], case["painter"], cloud.tobytes())          # computed once per posed cloud, shared, never written to
    if key not in _EXPECTED:
        vp = rc.vertex_part(case)
        if case["painter"]:
            from oracle import render_oracle as ro
            depth, mask = ro.render(cloud, case["mesh"], vp, k, k["width"], k["height"], stable=True)
            data, labels = ro.backproject(depth, mask, k)
            want = dict(N=len(labels), data=data, labels=labels, depth=depth, mask=mask)
        else:
            depth, face, label, data, labels = rr.render(cloud, case["mesh"], vp, k, k["width"], k["height"])
            want = dict(N=len(labels), data=data, labels=labels)
        for a in want.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _EXPECTED[key] = want
    return _EXPECTED[key]


def _posed(ctx, case):
    w, p, R = rc.pose_arguments(case)
    cloud, _, _ = ctx.lbs_update(w, p, R)
    if case["exact"]:
        for f in range(len(cloud)):
            assert np.array_equal(cloud[f], rc.intended_cloud(case, f)), f"{case['name']}: the posed cloud is not the intended one"
    return (w, p, R), cloud


def _compare(ctx, case, n, f, want, images):
    """'' when frame f on the device equals `want`, else what differs"""
    bad = []
    if n[f] != want["N"]:
        bad.append(f"N {n[f]} for {want['N']}")
    else:
        data, labels = ctx.frame_download(f)
        if not np.array_equal(data, want["data"]):
            bad.append(f"{int((data != want['data']).any(1).sum())} of {want['N']} points")
        if not np.array_equal(labels, want["labels"]):
            bad.append(f"{int((labels != want['labels']).sum())} of {want['N']} labels")
    if images:
        depth, mask = ctx.render_images(f)
        if not np.array_equal(depth, want["depth"]):
            bad.append(f"{int((depth != want['depth']).sum())} depth pixels")
        if not np.array_equal(mask, want["mask"]):
            bad.append(f"{int((mask != want['mask']).sum())} mask pixels")
    return f"{case['name']} frame {f}: " + ", ".join(bad) if bad else ""


def _run(case, ctx=None, images=None):
    """every frame of the case through render_frames on a context sized to it; the list of what differs"""
    ctx = _context(case) if ctx is None else ctx
    (w, p, R), cloud = _posed(ctx, case)
    n = ctx.render_frames(w, p, R, intrin=case["cam"], painter=case["painter"])
    images = case["painter"] if images is None else images
    return [m for m in (_compare(ctx, case, n, f, _expect(case, cloud[f]), images) for f in range(len(cloud))) if m]


@pytest.mark.parametrize("group", ["edges", "rejection", "labels", "clipping", "scan"])
def test_zbuffer_cases(group):
    """edges: pixel centres on edges and vertices, ties of depth going to the lower face id in both mesh orders and windings, near and far
    in both orders; rejection: |n_z| / |n| on both sides of 0.1, zero area, collinear projections, vertices at z = 0, z < 0 and z = 1e-300,
    subnormal depths; labels: equal distances to two and to three projected vertices, a part map that is not the identity; clipping: every
    border and corner, faces wholly outside, images of 1x1, 1x300, 300x1, 15x17, 16x16, 17x31 pixels, projections beyond the range of int;
    scan: full and checkerboard grids over 1, 1024 and 1025 blocks of 256 pixels."""
    failures = []
    for case in rc.cases(group):
        failures += _run(case)
    assert not failures, "; ".join(failures)


def test_painter_cases():
    """the known-answer scenes of tests/test_render_oracle_cpu.py, an edge-on face in front of a plane (depth 0 and no point under it), equal
    sort keys in both mesh orders, depth clamped at 255, points with label 255 where only the row fill covers, projections beyond int"""
    failures = []
    for case in rc.cases("painter"):
        failures += _run(case)
    assert not failures, "; ".join(failures)


def test_max_points_at_the_point_count_and_one_below():
    """T == max_points is accepted.  T == max_points + 1 is an error that names max_points_per_frame and leaves no frame to download; the
    next call on the same context is exact again."""
    from avatar_amd import api
    case = rc.by_name("grid-checker-16x16")
    aside = dict(case, name="grid-checker-16x16 moved aside", trans=np.array([[0.125, 0.0, 0.0]]), exact=False)   # 8 pixels to the right: fewer points
    k = case["cam"]
    T = _expect(case, rc.intended_cloud(case, 0))["N"]
    assert 1 < _expect(aside, rc.intended_cloud(aside, 0))["N"] < T - 1 and T < k["width"] * k["height"]
    assert _run(case, _context(case, max_points=T)) == []
    ctx = _context(case, max_points=T - 1)
    assert _run(aside, ctx) == []
    w, p, R = rc.pose_arguments(case)
    with pytest.raises(api.AvtError, match="max_points_per_frame"):
        ctx.render_frames(w, p, R, intrin=k)
    with pytest.raises(api.AvtError):
        ctx.frame_download(0)
    assert _run(aside, ctx) == []
    assert _run(case, _context(case, max_points=T + 1)) == []


def test_frames_across_a_scratch_chunk_in_zbuffer_mode():
    """33 frames at 1280x720 are rendered in chunks of 32 and 1 (avt_synth_render_frames_mode: (256 MiB) / (npix * 9 + 64) frames per chunk):
    every frame, the last of the first chunk and the first of the second among them, is its own expectation."""
    case = rc.by_name("chunk-zbuffer-33")
    k = case["cam"]
    chunk = (256 << 20) // (k["width"] * k["height"] * 9 + 64)
    assert chunk == 32 == rc.chunk_frames(k["width"], k["height"], False) and len(case["trans"]) == chunk + 1
    assert _run(case) == []


def test_frames_across_a_scratch_chunk_in_painters_mode():
    """14 painter frames at 1280x720 are rendered in chunks of 13 and 1 ((256 MiB) / (npix * 21 + 64)): every frame is the oracle's, and the
    images, which only the last chunk's scratch still holds, are refused; after 13 frames they are served and are the oracle's."""
    from avatar_amd import api
    over, fits = rc.by_name("chunk-painter-14"), rc.by_name("chunk-painter-13")
    k = over["cam"]
    chunk = (256 << 20) // (k["width"] * k["height"] * 21 + 64)
    assert chunk == 13 == rc.chunk_frames(k["width"], k["height"], True) and len(over["trans"]) == chunk + 1 and len(fits["trans"]) == chunk
    ctx = _context(over)
    assert _run(over, ctx, images=False) == []
    with pytest.raises(api.AvtError, match="one scratch chunk"):
        ctx.render_images(0)
    assert _run(fits, ctx) == []


def test_one_context_through_sizes_and_modes_leaves_nothing_behind():
    """1280x720 z-buffer, 17x31 z-buffer, 64x48 painter, 640x410 z-buffer, 1280x720 painter on one context, whose scratch only grows and is
    shared by the two modes: every run is the expectation computed fresh, and the second pass gives the arrays of the first."""
    seq = rc.cases("sequence")
    ctx = _context(seq[0], max_points=max(_expect(c, rc.intended_cloud(c, 0))["N"] for c in seq) + 4096)
    passes = []
    for rep in range(2):
        got = []
        for case in seq:
            assert _run(case, ctx) == [], f"pass {rep}"
            got.append(ctx.frame_download(0) + (ctx.render_images(0) if case["painter"] else ()))
        passes.append(got)
    for a, b in zip(*passes):
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
