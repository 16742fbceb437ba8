"""Seeded, named inputs that put the synthetic depth-frame generator (avt_synth_render_frames[_mode]: k_raster, k_raster_label,
k_raster_scan, k_raster_emit and the k_paint_* hand-over of avatar_amd/csrc/avt_render.hip) at its edges: pixel centres exactly on
edges, depth ties, the rejection rules on both sides, equal label distances, clipping at every border, odd image sizes, block counts
of the scan at 1, 1024 and 1025, frame counts across a scratch chunk.  A helper module of the tests, not a test file; no GPU is
needed to build a case.

A case is a dict: name, group, verts (V,3) and joint (V,) of a hand-built mesh, mesh (F,3), part_map (one part per joint), num_parts,
cam (fx, fy, cx, cy, width, height), trans (frames,3) root translations, painter (bool), exact (the posed cloud must equal
verts + trans bit for bit) and promise (what the case says about itself; tests/test_raster_edges_cpu.py checks it on the CPU).

model_dict(case) is the SMPL-layout model of a case: NJ joints, every vertex bound with weight 1 to its joint, one more vertex at the
origin that no face uses and that every joint regresses to, one all-zero shape key.  With w = 0, R = I the posed cloud is
v_template + p.  Exact cases use a dyadic camera (fx = fy = 128, dyadic principal point) and depths of few bits (powers of two, 2.0625, 2.03125): then
(x - cx) z / fx is exact, and p.x fx / p.z + cx - an exact product divided by z again - lands exactly on the intended pixel coordinate.
Depth differences stay small: a face that rises by its own width in depth is edge-on at these focal lengths."""
from __future__ import annotations

import numpy as np

NJ = 4
PARENT = np.array([-1, 0, 0, 0])
IDENTITY = np.arange(NJ, dtype=np.int32)
SHUFFLED = np.array([5, 2, 7, 0], np.int32)            # a part map that is not the identity, 8 parts
K4A_SIZE = (1280, 720)
CHUNK_BYTES = 256 << 20                                 # avt_capi.cpp, avt_synth_render_frames_mode: frames per scratch chunk =
CHUNK_PER_PIXEL = {False: 9, True: 21}                  # (256 MiB) / (npix * 9 + 64), * 21 in painter's mode


def chunk_frames(width, height, painter):
    return max(1, CHUNK_BYTES // (width * height * CHUNK_PER_PIXEL[bool(painter)] + 64))


def cam(width, height, cx=None, cy=None, f=128.0):
    return dict(fx=float(f), fy=float(f), cx=float(width // 2 if cx is None else cx), cy=float(height // 2 if cy is None else cy),
                width=int(width), height=int(height))


def at(k, x, y, z):
    """the camera-space point that projects to pixel coordinate (x, y) at depth z (y up in camera space)"""
    return [(x - k["cx"]) * z / k["fx"], -(y - k["cy"]) * z / k["fy"], z]


def _case(name, group, verts, joint, mesh, k, part_map=IDENTITY, num_parts=None, trans=None, painter=False, exact=False, **promise):
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    joint = np.broadcast_to(np.asarray(joint, np.int64), (len(verts),)).copy()
    mesh = np.asarray(mesh, np.int32).reshape(-1, 3)
    assert mesh.min() >= 0 and mesh.max() < len(verts) and joint.min() >= 0 and joint.max() < NJ
    trans = np.zeros((1, 3)) if trans is None else np.asarray(trans, np.float64).reshape(-1, 3)
    pm = np.asarray(part_map, np.int32)
    return dict(name=name, group=group, verts=verts, joint=joint, mesh=mesh, cam=k, part_map=pm,
                num_parts=int(pm.max()) + 1 if num_parts is None else num_parts, trans=trans, painter=painter, exact=exact, promise=promise)


def model_dict(case):
    v = np.concatenate([case["verts"], np.zeros((1, 3))])          # the anchor: at the origin, in no face
    V = len(v)
    weights = np.zeros((V, NJ))
    weights[np.arange(V - 1), case["joint"]] = 1.0
    weights[V - 1, 0] = 1.0
    jreg = np.zeros((NJ, V))
    jreg[:, V - 1] = 1.0
    return dict(v_template=v, f=case["mesh"], kintree_table=np.stack([PARENT, np.arange(NJ)]), J_regressor=jreg, weights=weights,
                shapedirs=np.zeros((V, 3, 1)))


def vertex_part(case):
    """part of every vertex of model_dict(case), the anchor included"""
    return case["part_map"][np.concatenate([case["joint"], [0]])].astype(np.int32)


def intended_cloud(case, frame):
    return np.concatenate([case["verts"], np.zeros((1, 3))]) + case["trans"][frame]


def pose_arguments(case):
    """(w, p, R) of Context.render_frames / lbs_update"""
    n = len(case["trans"])
    return np.zeros((n, 1)), case["trans"].copy(), np.tile(np.eye(3), (n, NJ, 1, 1))


# ---- edges and ties -------------------------------------------------------------------------------------------------------
K32 = cam(32, 24)


def _tri(k, pts, z=2.0):
    zs = [z] * 3 if np.isscalar(z) else z
    return [at(k, x, y, zz) for (x, y), zz in zip(pts, zs)]


def edges():
    out = []
    # legs of 16 pixels: the weights' denominator is 256, every weight is exact, centres on the three edges have a weight of exactly 0
    right = [(4, 3), (20, 3), (4, 19)]
    out.append(_case("edge-right-triangle", "edges", _tri(K32, right), [1, 2, 3], [[0, 1, 2]], K32, exact=True, T=[153],
                     face_at={(3, 4): 0, (3, 20): 0, (19, 4): 0, (3, 12): 0, (10, 4): 0, (11, 12): 0, (12, 12): -1, (2, 4): -1, (3, 3): -1, (3, 21): -1}))
    # a square split along the diagonal B-C, which has the constant depth 2.0625 on both faces: the shared pixels tie and go to face 0
    # (k z / 128 is exact for a depth of few bits, and the projection divides that exact product by z again)
    sq = _tri(K32, [(4, 3), (20, 3), (4, 19), (20, 19)], [2.0, 2.0625, 2.0625, 2.0])
    diag = [((3 + i, 20 - i), [0, 1]) for i in range(17)]
    for name, mesh, win in (("edge-shared-diagonal", [[0, 1, 2], [3, 2, 1]], 0), ("edge-shared-diagonal-swapped", [[3, 2, 1], [0, 1, 2]], 0)):
        out.append(_case(name, "edges", sq, [0, 1, 2, 3], mesh, K32, exact=True, T=[17 * 17], tie=diag, face_at={p: win for p, _ in diag}))
    # the same split with the diagonal sloping in depth (2 at B, 2.0625 at C): whatever the two interpolations give, depth first, then face id
    sq2 = _tri(K32, [(4, 3), (20, 3), (4, 19), (20, 19)], [2.0, 2.0, 2.0625, 2.0625])
    out.append(_case("edge-shared-diagonal-sloped", "edges", sq2, [0, 1, 2, 3], [[0, 1, 2], [3, 2, 1]], K32, exact=True, T=[17 * 17], both_cover=diag))
    # coincident faces on separate vertices with different parts: equal depth bits everywhere, the lower face id shows its labels
    two = _tri(K32, right) + _tri(K32, right)
    every = [((r, c), [0, 1]) for r in range(3, 20) for c in range(4, 24 - r)]
    out.append(_case("tie-coincident", "edges", two, [1, 1, 1, 2, 2, 2], [[0, 1, 2], [3, 4, 5]], K32, exact=True, T=[153], tie=every,
                     label_at={(8, 8): 1, (3, 4): 1}))
    out.append(_case("tie-coincident-swapped", "edges", two, [1, 1, 1, 2, 2, 2], [[3, 4, 5], [0, 1, 2]], K32, exact=True, T=[153], tie=every,
                     label_at={(8, 8): 2, (3, 4): 2}))
    out.append(_case("tie-opposite-winding", "edges", two, [1, 1, 1, 2, 2, 2], [[0, 1, 2], [3, 5, 4]], K32, exact=True, T=[153], tie=every,
                     label_at={(8, 8): 1}))
    out.append(_case("tie-opposite-winding-swapped", "edges", two, [1, 1, 1, 2, 2, 2], [[3, 5, 4], [0, 1, 2]], K32, exact=True, T=[153], tie=every,
                     label_at={(8, 8): 2}))
    near, far = _tri(K32, right, 1.0), _tri(K32, [(2, 1), (30, 1), (2, 23)], 4.0)
    out.append(_case("depth-near-after-far", "edges", far + near, [1, 1, 1, 2, 2, 2], [[0, 1, 2], [3, 4, 5]], K32, exact=True,
                     face_at={(8, 8): 1, (2, 3): 0}, label_at={(8, 8): 2, (2, 3): 1}))
    out.append(_case("depth-near-before-far", "edges", near + far, [2, 2, 2, 1, 1, 1], [[0, 1, 2], [3, 4, 5]], K32, exact=True,
                     face_at={(8, 8): 0, (2, 3): 1}, label_at={(8, 8): 2, (2, 3): 1}))
    return out


# ---- rejection rules ------------------------------------------------------------------------------------------------------
def _witness(k):
    """a small face in the bottom right corner that every rejection case keeps, so that the frame is not empty"""
    W, H = k["width"], k["height"]
    return _tri(k, [(W - 5, H - 5), (W - 1, H - 5), (W - 5, H - 1)], 8.0)


def rejection():
    out = []
    wit = _witness(K32)
    for name, ratio, drawn in (("edge-on-below-0.1", 0.099, False), ("edge-on-above-0.1", 0.1009, True)):
        # a = (.., 2), b = a + (u, 0, 0), c = a + (0, -v, s): the normal is (0, -u s, -u v), |n_z| / |n| = v / sqrt(s^2 + v^2)
        a = np.array(at(K32, 8, 6, 2.0))
        v = 0.1
        s = v * np.sqrt(1.0 / ratio ** 2 - 1.0)
        verts = [a, a + [0.25, 0.0, 0.0], a + [0.0, -v, s]]
        out.append(_case(name, "rejection", verts, [1, 2, 3], [[0, 1, 2]], K32, nz_ratio=(0, ratio), empty=not drawn))
        out.append(_case(name + "-with-witness", "rejection", verts + wit, [1, 2, 3, 0, 0, 0], [[0, 1, 2], [3, 4, 5]], K32, nz_ratio=(0, ratio),
                         faces_seen=[0, 1] if drawn else [1]))
    right = _tri(K32, [(4, 3), (20, 3), (4, 19)])
    out.append(_case("zero-area-repeated-vertex", "rejection", right + wit, 1, [[0, 0, 1], [3, 4, 5]], K32, exact=True, faces_seen=[1], T=[15]))
    out.append(_case("zero-area-coincident-vertices", "rejection", [right[0], right[1], right[1]] + wit, 1, [[0, 1, 2], [3, 4, 5]], K32, exact=True,
                     faces_seen=[1], T=[15]))
    # three projections on one image row from a face that is far from edge-on: the plane y = z / 2 passes through the camera
    col = [[0.0, 1.0, 2.0], [0.25, 1.0, 2.0], [1.0, 2.0, 4.0]]
    out.append(_case("collinear-projections", "rejection", col + wit, 1, [[0, 1, 2], [3, 4, 5]], K32, exact=True, faces_seen=[1], T=[15],
                     denom_zero=[0], nz_above=[0]))
    for name, z in (("vertex-z-zero", 0.0), ("vertex-z-negative", -1.0)):
        verts = [right[0], right[1], [right[2][0], right[2][1], z]]
        out.append(_case(name, "rejection", verts + wit, 1, [[0, 1, 2], [3, 4, 5]], K32, faces_seen=[1], T=[15]))
    # z = 1e-300 passes `z <= 0`; as a float it is 0.  On the optical axis it projects to the principal point (16, 12), and the face - wide
    # enough not to be edge-on: its other vertices are two focal lengths off the axis - is drawn except where its interpolated depth is
    # not > 0: at that vertex itself
    wide = [at(K32, 272, 12, 2.0), at(K32, 16, 268, 2.0)]
    out.append(_case("vertex-z-1e-300-on-axis", "rejection", [[0.0, 0.0, 1e-300]] + wide, 1, [[0, 1, 2]], K32, nz_above=[0],
                     face_at={(12, 16): -1, (13, 17): 0, (12, 17): 0, (13, 16): 0, (11, 16): -1}))
    # off the axis it projects to +inf: the box is clamped to the image, every weight is NaN or -inf, nothing is drawn
    verts = [[1.0, 0.0, 1e-300]] + wide
    out.append(_case("vertex-z-1e-300-infinite-projection", "rejection", verts + wit, 1, [[0, 1, 2], [3, 4, 5]], K32, nz_above=[0], faces_seen=[1], T=[15]))
    # a face at z = 2^-130: every vertex depth and every interpolated depth is a float subnormal, and positive
    z = 2.0 ** -130
    out.append(_case("subnormal-depth", "rejection", _tri(K32, [(4, 3), (20, 3), (4, 19)], z), [1, 2, 3], [[0, 1, 2]], K32, exact=True, T=[153],
                     depth_subnormal=True))
    return out


# ---- label rule -----------------------------------------------------------------------------------------------------------
def labels():
    # face 0: a (4,4) b (12,4) c (4,12), parts of joints 1, 2, 3; face 1: a (22,18) b (18,2) c (26,2), joints 3, 1, 2.  Denominators 64 and 128.
    verts = _tri(K32, [(4, 4), (12, 4), (4, 12)]) + _tri(K32, [(22, 18), (18, 2), (26, 2)])
    joint = [1, 2, 3, 3, 1, 2]
    out = []
    for name, pm in (("label-ties-identity", IDENTITY), ("label-ties-shuffled-parts", SHUFFLED)):
        out.append(_case(name, "labels", verts, joint, [[0, 1, 2], [3, 4, 5]], K32, part_map=pm, exact=True,
                         equidistant=[((4, 8), 0, "ab"), ((5, 8), 0, "ab"), ((8, 4), 0, "ac"), ((8, 5), 0, "ac"), ((8, 8), 0, "abc"),
                                      ((2, 22), 1, "bc"), ((4, 22), 1, "bc")],
                         label_at={(4, 8): pm[2], (5, 8): pm[2], (8, 4): pm[3], (8, 5): pm[3], (8, 8): pm[3], (2, 22): pm[2], (4, 22): pm[2],
                                   (4, 4): pm[1], (4, 12): pm[2], (12, 4): pm[3], (18, 22): pm[3], (2, 18): pm[1], (2, 26): pm[2]}))
    return out


# ---- clipping -------------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (1, 300), (300, 1), (15, 17), (16, 16), (17, 31), (32, 24))


def _clip_mesh(k):
    """a triangle across the middle of each border, across each corner and wholly outside on each side, each at a depth of its own"""
    W, H = k["width"], k["height"]
    s = max(2.0, min(W, H) / 4.0)
    s = float(int(s))
    mx, my = float(W // 2), float(H // 2)
    centres = [(mx, 0.0), (mx, H - 1.0), (0.0, my), (W - 1.0, my), (0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0),
               (mx, -3 * s), (mx, H - 1 + 3 * s), (-3 * s, my), (W - 1 + 3 * s, my)]
    verts = []
    for i, (x, y) in enumerate(centres):
        verts += _tri(k, [(x - s, y - s), (x + s, y - s), (x, y + s)], 2.0 ** (i - 4))
    return verts, np.arange(36).reshape(12, 3)


def clipping():
    out = []
    for W, H in SIZES:
        k = cam(W, H)
        verts, mesh = _clip_mesh(k)
        out.append(_case(f"clip-borders-{W}x{H}", "clipping", verts, np.arange(36) % NJ, mesh, k, part_map=SHUFFLED, exact=True, npix=W * H,
                         faces_never=[8, 9, 10, 11]))
        big = _tri(k, [(-4.0 * W - 8, -8.0), (4.0 * W + 8, -8.0), (W // 2, 8.0 * H + 8)])
        out.append(_case(f"clip-covered-{W}x{H}", "clipping", big, [1, 2, 3], [[0, 1, 2]], k, T=[W * H], npix=W * H))
    # seeded triangles with vertices anywhere in a window three images wide: no coordinate is exact, most faces are clipped
    rng = np.random.default_rng([20261017, 3])
    k = cam(17, 31, cx=7.75, cy=16.5, f=100.0)
    xy = rng.uniform([-17, -31], [34, 62], (120, 2))
    z = rng.uniform(1.0, 3.0, 120)
    out.append(_case("clip-seeded-soup-17x31", "clipping", [at(k, x, y, zz) for (x, y), zz in zip(xy, z)], rng.integers(0, NJ, 120),
                     np.arange(120).reshape(40, 3), k, part_map=SHUFFLED))
    # a projected coordinate beyond the range of int: a vertex 40 nm in front of the camera plane
    k = dict(fx=100.0, fy=100.0, cx=10.0, cy=40.0, width=64, height=64)
    zc = 4e-8
    for name, verts in (("overflow-x-max", [[0, 0, 2], [0, 0.2, 2], [1, 0, zc]]), ("overflow-x-min", [[0, 0, 2], [0, 0.2, 2], [-1, 0, zc]]),
                        ("overflow-y-min", [[0, 0, 2], [0.2, 0, 2], [0, 1, zc]]), ("overflow-y-max", [[0, 0, 2], [0.2, 0, 2], [0, -1, zc]])):
        out.append(_case(name, "clipping", verts, [1, 2, 3], [[0, 1, 2]], k, beyond_int=[2], nonempty=True))
    wit = _witness(k)
    out.append(_case("overflow-whole-face-x-max", "clipping", [[1, 0, zc], [1, 1e-9, zc], [1.5, 0, zc]] + wit, 1, [[0, 1, 2], [3, 4, 5]], k,
                     beyond_int=[0, 1, 2], faces_seen=[1]))
    out.append(_case("overflow-whole-face-x-min", "clipping", [[-1, 0, zc], [-1, 1e-9, zc], [-1.5, 0, zc]] + wit, 1, [[0, 1, 2], [3, 4, 5]], k,
                     beyond_int=[0, 1, 2], faces_seen=[1]))
    return out


# ---- scan and emit --------------------------------------------------------------------------------------------------------
def _grid(k, q, x0, y0, checker):
    """quads of q x q pixels from (x0, y0) to beyond the image, two faces each; with `checker` every other quad is left out.  q is a power
    of two, so the weights' denominator is one too and a centre on a shared edge has a weight of exactly 0 on both sides."""
    W, H = k["width"], k["height"]
    nx, ny = -(-(W - 1 - x0) // q), -(-(H - 1 - y0) // q)
    ii, jj = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    z = np.where((ii + jj) % 3 == 0, 2.03125, 2.0)
    verts = np.stack([(x0 + q * ii - k["cx"]) * z / k["fx"], -(y0 + q * jj - k["cy"]) * z / k["fy"], z], -1).reshape(-1, 3)
    joint = ((ii + 2 * jj) % NJ).reshape(-1)
    vid = lambda i, j: j * (nx + 1) + i
    mesh = []
    for j in range(ny):
        for i in range(nx):
            if checker and (i + j) % 2:
                continue
            mesh += [[vid(i, j), vid(i + 1, j), vid(i, j + 1)], [vid(i + 1, j + 1), vid(i, j + 1), vid(i + 1, j)]]
    return verts, joint, mesh


def scan():
    out = []
    for (W, H), q, nblocks in (((16, 16), 4, 1), ((512, 512), 16, 1024), ((640, 410), 16, 1025)):
        k = cam(W, H)
        verts, joint, mesh = _grid(k, q, 0, 0, False)
        out.append(_case(f"grid-full-{W}x{H}", "scan", verts, joint, mesh, k, exact=True, T=[W * H], nblocks=nblocks, npix=W * H))
        verts, joint, mesh = _grid(k, q, -3, -5 if H > 16 else -1, True)
        out.append(_case(f"grid-checker-{W}x{H}", "scan", verts, joint, mesh, k, part_map=SHUFFLED, exact=True, nblocks=nblocks,
                         runs_straddle=(64, 256) if W > 16 else (64,)))
    return out


# ---- chunks ---------------------------------------------------------------------------------------------------------------
def _patch(k, n=4, q=24, x0=600.0, y0=320.0):
    W, H = k["width"], k["height"]
    ii, jj = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="xy")
    z = 2.0 + 0.25 * ((ii * jj) % 3)
    verts = np.stack([(x0 + q * ii - k["cx"]) * z / k["fx"], -(y0 + q * jj - k["cy"]) * z / k["fy"], z], -1).reshape(-1, 3)
    vid = lambda i, j: j * (n + 1) + i
    mesh = [t for j in range(n) for i in range(n) for t in ([vid(i, j), vid(i + 1, j), vid(i, j + 1)], [vid(i + 1, j + 1), vid(i, j + 1), vid(i + 1, j)])]
    return verts, ((ii + jj) % NJ).reshape(-1), mesh


def chunks():
    W, H = K4A_SIZE
    k = cam(W, H, f=512.0)
    verts, joint, mesh = _patch(k)
    out = []
    for name, n, painter in (("chunk-zbuffer-33", 33, False), ("chunk-painter-14", 14, True), ("chunk-painter-13", 13, True)):
        rng = np.random.default_rng([20261017, 5, n])
        trans = np.concatenate([rng.uniform(-1.0, 1.0, (n, 2)), rng.uniform(-0.5, 0.5, (n, 1))], 1)     # a different place in every frame
        out.append(_case(name, "chunks", verts, joint, mesh, k, part_map=SHUFFLED, trans=trans, painter=painter,
                         crosses_chunk=n > chunk_frames(W, H, painter), frames_differ=True))
    return out


# ---- state left behind ----------------------------------------------------------------------------------------------------
def sequence():
    """one mesh under five cameras, in the order the test renders them on one context"""
    rng = np.random.default_rng([20261017, 7])
    uv = rng.uniform(-0.6, 0.6, (180, 2))                # normalised image coordinates, so that every camera sees the same picture
    z = rng.uniform(1.5, 3.0, 180)
    verts = np.stack([uv[:, 0] * z, uv[:, 1] * z * 0.6, z], 1)
    joint = rng.integers(0, NJ, 180)
    out = []
    for i, ((W, H), painter) in enumerate((((1280, 720), False), ((17, 31), False), ((64, 48), True), ((640, 410), False), ((1280, 720), True))):
        k = cam(W, H, f=float(W) / 2)
        out.append(_case(f"sequence-{i}-{W}x{H}-{'painter' if painter else 'zbuffer'}", "sequence", verts, joint, np.arange(180).reshape(60, 3), k,
                         part_map=SHUFFLED, painter=painter))
    return out


# ---- painter's hand-over (expectations from oracle/render_oracle) ------------------------------------------------------------
KP = dict(fx=100.0, fy=100.0, cx=32.0, cy=24.0, width=64, height=48)


def painter():
    out = []
    P = lambda name, verts, joint, mesh, k=KP, **pr: _case(name, "painter", verts, joint, mesh, k, part_map=SHUFFLED, painter=True, **pr)
    # the three known-answer scenes of tests/test_render_oracle_cpu.py
    right = [(10, 5), (30, 5), (10, 25)]
    out.append(P("painter-single-triangle", _tri(KP, right), [1, 2, 3], [[0, 1, 2]]))
    near, far = _tri(KP, right, 1.5), _tri(KP, [(8, 4), (40, 4), (8, 40)], 3.0)
    out.append(P("painter-near-listed-first", near + far, [1, 1, 1, 2, 2, 2], [[0, 1, 2], [3, 4, 5]], depth_at={(10, 12): 1.5, (30, 10): 3.0}))
    out.append(P("painter-far-listed-first", far + near, [2, 2, 2, 1, 1, 1], [[0, 1, 2], [3, 4, 5]], depth_at={(10, 12): 1.5, (30, 10): 3.0}))
    # an edge-on face in front of a plane: it paints 0 with an end-exclusive row fill, so there are holes without points and the last pixel
    # of each of its rows keeps the plane
    back = _tri(KP, [(5, 5), (50, 5), (5, 40)], 5.0)
    steep = [at(KP, 20, 10, 2.0), at(KP, 26, 10, 2.0), at(KP, 23, 20, 6.0)]
    out.append(P("painter-edge-on-in-front", back + steep, [1, 1, 1, 2, 2, 2], [[0, 1, 2], [3, 4, 5]], edge_on=[1], holes_in_row=12))
    # equal sort keys (both mean depths are exactly 2), overlapping, different depths: the painter position goes by face id
    flat, tilt = _tri(KP, right, 2.0), _tri(KP, [(12, 6), (28, 8), (12, 22)], [1.96875, 2.0, 2.03125])
    out.append(P("painter-equal-keys", flat + tilt, [1, 1, 1, 2, 2, 2], [[0, 1, 2], [3, 4, 5]], equal_keys=True))
    out.append(P("painter-equal-keys-swapped", tilt + flat, [2, 2, 2, 1, 1, 1], [[0, 1, 2], [3, 4, 5]], equal_keys=True))
    # deeper than 255: the depth image is clamped, and the points are emitted at 255
    out.append(P("painter-depth-300-clamped", _tri(KP, right, 300.0), [1, 2, 3], [[0, 1, 2]], depth_all=255.0))
    # the row fill (depth) of this face covers pixels that its column fill (labels) does not; they become points with label 255
    out.append(P("painter-row-fill-without-column-fill", _tri(KP, [(31.75, 42.0), (10.25, 41.75), (20.0, 19.75)]), [1, 2, 3], [[0, 1, 2]], label_255=True))
    # a vertex projecting beyond the range of int: the reference's x86 conversions give INT_MIN
    ko = dict(fx=100.0, fy=100.0, cx=10.0, cy=40.0, width=64, height=64)
    out.append(P("painter-overflow-x", [[0, 0, 2], [0, 0.2, 2], [1, 0, 4e-8]], [1, 2, 3], [[0, 1, 2]], k=ko, beyond_int=[2]))
    out.append(P("painter-overflow-y", [[0, 0, 2], [0.2, 0, 2], [0, 1, 4e-8]], [1, 2, 3], [[0, 1, 2]], k=ko, beyond_int=[2]))
    return out


GROUPS = {"edges": edges, "rejection": rejection, "labels": labels, "clipping": clipping, "scan": scan, "chunks": chunks, "sequence": sequence,
          "painter": painter}
_BUILT = {}


def cases(group):
    if group not in _BUILT:
        _BUILT[group] = GROUPS[group]()
        names = [c["name"] for g in _BUILT.values() for c in g]
        assert len(names) == len(set(names)), "case names are unique"
    return _BUILT[group]


def by_name(name):
    for g in GROUPS:
        for c in cases(g):
            if c["name"] == name:
                return c
    raise KeyError(name)


def zbuffer_cases():
    return [c for g in GROUPS for c in cases(g) if not c["painter"]]
