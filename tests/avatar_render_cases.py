"""Seeded, named inputs that take ark::AvatarRenderer on the GPU (avatar_amd/csrc/avt_render.hip: k_rend_project, k_rend_faces, k_rend_sort,
k_rend_scatter, k_rend_vnormal, k_rend_cover, k_rend_resolve, and k_paint_rank as the renderer uses it) away from SMPL's mesh and poses:
the bitonic sort at every width, every kind of sort key, the rank count beside it, valences of hundreds, the fills at their branches,
part values beyond a byte, grid tails.  A helper module of the tests, not a test file; no GPU is needed to build a case.

A case is a dict: name, group, clouds (n, V, 3), mesh (F, 3), joint (V,) the joint of every vertex, n_joints, joints (n, J, 3) or None,
part_map (one part per joint) or None, intr (fx, fy, cx, cy), size (width, height) and promise: what the case says about itself, written
by hand.  measure(case) computes the same quantities from the arrays; tests/test_avatar_render_edges_cpu.py compares the two.

Order group.  A *stack* is F disjoint triangles whose projections coincide: face f has its own three vertices S_k * z_f, with S_k the
direction of pixel FOOT[k] through a dyadic camera (fx = fy = 128).  All three vertices share z_f, a float32 value, so the face's sort key
float((z + z + z) / 3.f) is z_f exactly, and S_k z fx / z + cx is exact too: every face with a finite, non-zero z covers the same pixels,
and the face seen at them is the one painted last.  A face with z = +-0 keeps S_k unscaled (its projection is +-inf), one with an
infinite or NaN z too (it projects to the principal point, or to NaN): they paint nothing, but they take their places in the order and
move everybody else's position, which is what the `faces` image shows."""
from __future__ import annotations

import numpy as np

F32 = np.float32
SORT_CAP = 16384                                        # REND_SORT_CAP (avt_render.hip): larger meshes take the rank count
MAX_JOINTS = 58                                         # avt_model_create: 3 + 3 J + K <= 179, and the recipe has one shape key
MAIN_LIGHT, BACK_LIGHT = np.array([0.8, 1.5, -1.2]), np.array([-0.2, -1.5, 0.4])
NEG_NAN = float(np.copysign(np.nan, -1.0))


def model_dict(cloud, mesh, joint=None, n_joints=1):
    """a one-shape-key model whose rest pose is `cloud`: n_joints joints in a star, every vertex bound with weight 1 to joint[v] (joint 0
    without one).  The renderer only needs the mesh and the vertex -> joint map."""
    V, J = len(cloud), int(n_joints)
    weights = np.zeros((V, J))
    weights[np.arange(V), np.zeros(V, np.int64) if joint is None else np.asarray(joint, np.int64)] = 1.0
    parent = np.array([-1] + [0] * (J - 1))
    return dict(v_template=np.asarray(cloud, np.float64), f=np.asarray(mesh, np.int32), kintree_table=np.stack([parent, np.arange(J)]),
                J_regressor=np.full((J, V), 1.0 / V), weights=weights, shapedirs=np.zeros((V, 3, 1)))


def tiny_model(cloud, mesh, joint=None, n_joints=1):
    from avatar_amd import api
    return api.AvatarModel(model_dict(cloud, mesh, joint, n_joints))


def model_of(case):
    return tiny_model(case["clouds"][0], case["mesh"], case["joint"], case["n_joints"])


def vertex_part(case):
    """what set_part_map makes of the case: the part of every vertex, as the ints the restatement is given"""
    j = case["joint"]
    return (j if case["part_map"] is None else np.asarray(case["part_map"])[j]).astype(np.int32)


def cam(width, height, cx=None, cy=None, f=128.0):
    return dict(fx=float(f), fy=float(f), cx=float(width // 2 if cx is None else cx), cy=float(height // 2 if cy is None else cy)), (int(width), int(height))


def at(k, x, y, z):
    """the camera-space point that projects to pixel coordinate (x, y) at depth z (y up in camera space)"""
    return [(x - k["cx"]) * z / k["fx"], -(y - k["cy"]) * z / k["fy"], z]


def _tri(k, pts, z=2.0):
    zs = [z] * 3 if np.isscalar(z) else z
    return [at(k, x, y, zz) for (x, y), zz in zip(pts, zs)]


def _case(name, group, clouds, mesh, k, size, joint=None, n_joints=1, joints="seeded", part_map=None, **promise):
    clouds = np.asarray(clouds, np.float64)
    clouds = clouds[None] if clouds.ndim == 2 else clouds
    n, V = clouds.shape[:2]
    mesh = np.asarray(mesh, np.int32).reshape(-1, 3)
    joint = np.zeros(V, np.int64) if joint is None else np.asarray(joint, np.int64)
    assert mesh.min() >= 0 and mesh.max() < V and joint.min() >= 0 and joint.max() < n_joints <= MAX_JOINTS
    if isinstance(joints, str):
        rng = np.random.default_rng([20261018, 37, V, len(mesh), n_joints])
        joints = np.concatenate([rng.uniform(-0.5, 0.5, (n, n_joints, 2)), rng.uniform(1.0, 3.0, (n, n_joints, 1))], 2)
    return dict(name=name, group=group, clouds=clouds, mesh=mesh, joint=joint, n_joints=int(n_joints), joints=joints,
                part_map=None if part_map is None else np.asarray(part_map, np.int32), intr=k, size=size, promise=promise)


# ---- what a case is, computed ---------------------------------------------------------------------------------------------------------
def keys_of(case, image=0):
    """the float32 sort keys (AvatarRenderer.cpp:62-66): the three depths summed as doubles, divided by 3.f, stored as float"""
    z = case["clouds"][image][:, 2][case["mesh"]]
    with np.errstate(invalid="ignore", over="ignore"):
        return (((z[:, 0] + z[:, 1]) + z[:, 2]) / np.float64(F32(3.0))).astype(F32)


def numpy_order(keys):
    """the painter order in plain numpy: decreasing key, ties (-0 and +0 among them) by ascending face id; keys must not be NaN"""
    return np.lexsort((np.arange(len(keys)), -keys.astype(np.float64)))


def key_bits(keys):
    """painter_key_bits of avt_render.hip in numpy: uint32 whose ascending order is the painter's order, on every bit pattern"""
    k = np.asarray(keys, F32).copy()
    k[k == 0] = 0.0                                      # -0 folded onto +0
    u = k.view(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return ~u


def unit_normals(cloud, mesh):
    """face normals as face_key_normal computes them (doubles, a zero vector unchanged)"""
    a, b, c = (cloud[mesh[:, i]] for i in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        ab, ac = b - a, c - a
        n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
        z = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        s = np.sqrt(np.where(z > 0, z, 1.0))
    return np.where((z > 0)[:, None], n / s[:, None], n)


def project(case, image=0):
    k, cl = case["intr"], case["clouds"][image]
    with np.errstate(all="ignore"):
        return (cl[:, 0] * k["fx"] / cl[:, 2] + k["cx"]).astype(F32), (-cl[:, 1] * k["fy"] / cl[:, 2] + k["cy"]).astype(F32)


def _nz_class(nz):
    a = abs(nz)
    if np.isnan(a):
        return "nan"
    for lim, name in ((1e-2, "1e-2"), (0.1, "0.1")):
        if a < lim:
            return "<" + name
        if a == lim:
            return "=" + name
    return ">0.1"


def measure(case):
    """every quantity a promise may name, from the arrays of the case (image 0 where a quantity belongs to one image)"""
    cl, mesh = case["clouds"][0], case["mesh"]
    n, V = case["clouds"].shape[:2]
    F, (W, H) = len(mesh), case["size"]
    keys = keys_of(case)
    P = 1
    while P < F:
        P <<= 1
    out = dict(F=F, V=V, J=case["n_joints"], images=n, pow2_pad=P - F, rank_path=F > SORT_CAP, entries_per_thread=-(-P // 1024), npix=W * H,
               v256=V % 256, f256=F % 256, j_above_v=case["n_joints"] > V)
    fin = keys[~np.isnan(keys)]
    _, counts = np.unique(fin.astype(np.float64) + 0.0, return_counts=True)
    out["tied_run"] = int(counts.max()) if len(counts) else 0
    out["distinct_keys"] = int(len(counts))
    d = np.diff(keys.astype(np.float64))
    out["monotone"] = 0 if F < 2 or np.isnan(d).any() else 1 if (d > 0).all() else -1 if (d < 0).all() else 0
    out["negative_keys"] = int((keys < 0).sum())
    out["zero_keys"] = (int(((keys == 0) & ~np.signbit(keys)).sum()), int(((keys == 0) & np.signbit(keys)).sum()))
    tiny = np.finfo(F32).tiny
    out["subnormal_keys"] = (int(((keys > 0) & (keys < tiny)).sum()), int(((keys < 0) & (keys > -tiny)).sum()))
    out["inf_keys"] = (int((keys == np.inf).sum()), int((keys == -np.inf).sum()))
    out["nan_keys"] = (int((np.isnan(keys) & ~np.signbit(keys)).sum()), int((np.isnan(keys) & np.signbit(keys)).sum()))
    bits = np.sort(np.unique(keys[np.isfinite(keys)].view(np.uint32).astype(np.int64)))
    out["one_ulp_apart"] = bool(len(bits) > 1 and (np.diff(bits) == 1).all())
    slots = np.bincount(mesh.reshape(-1), minlength=V)
    out["max_valence"] = int(slots.max())
    same = (mesh[:, 0] == mesh[:, 1]).astype(int) + (mesh[:, 1] == mesh[:, 2]) + (mesh[:, 0] == mesh[:, 2])     # 0, 1 or 3 equal pairs
    out["named_twice"], out["named_thrice"] = int((same == 1).sum()), int((same == 3).sum())
    out["isolated"] = int((slots == 0).sum())
    out["on_light"] = [int(v) for v in np.flatnonzero((cl == MAIN_LIGHT).all(1) | (cl == BACK_LIGHT).all(1))]
    out["part_values"] = sorted({int(p) for p in vertex_part(case)[mesh.reshape(-1)]})
    if F <= 64:
        fn = unit_normals(cl, mesh)
        out["nz_class"] = [_nz_class(z) for z in fn[:, 2]]
        vs = np.zeros((V, 3))
        np.add.at(vs, mesh.reshape(-1), np.repeat(fn, 3, 0))
        with np.errstate(invalid="ignore"):
            norm = np.sqrt((vs ** 2).sum(1))
        used = slots > 0
        out["zero_sums"] = int((used & (norm == 0)).sum())
        out["cancelling_sums"] = int((used & (norm > 0) & (norm < 0.5)).sum())
        out["nz_sum_positive"] = int((used & (vs[:, 2] > 0)).sum())
        out["nz_sum_zero"] = int((used & (vs[:, 2] == 0) & (norm > 0)).sum())
        px, py = project(case)
        with np.errstate(invalid="ignore"):
            out["beyond_int"] = [int(v) for v in range(V) if max(abs(float(px[v])), abs(float(py[v]))) > 2.0 ** 31 and np.isfinite(px[v]) and np.isfinite(py[v])]
        out["integer_projections"] = bool(np.array_equal(px, np.round(px)) and np.array_equal(py, np.round(py)))
        out["z_zero"] = int((cl[np.unique(mesh), 2] == 0).sum())
        out["z_negative"] = int((cl[np.unique(mesh), 2] < 0).sum())
    if n > 1:
        out["orders_differ"] = len({numpy_order(keys_of(case, i)).tobytes() for i in range(n)}) == n
    return out


# ---- order group ----------------------------------------------------------------------------------------------------------------------
K32, S32 = cam(32, 24)
FOOT = ((4.0, 3.0), (14.0, 3.0), (4.0, 13.0))          # about 10 x 10 pixels
STACK_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 16383, 16384, 16385)


def stack_cloud(z, k=K32):
    z = np.asarray(z, np.float64)
    S = np.array([[(x - k["cx"]) / k["fx"], -(y - k["cy"]) / k["fy"]] for x, y in FOOT])
    scale = np.where(np.isfinite(z) & (z != 0), z, 1.0)
    cl = np.empty((len(z), 3, 3))
    cl[:, :, :2] = S[None] * scale[:, None, None]
    cl[:, :, 2] = z[:, None]
    return cl.reshape(-1, 3)


def stack_visible(case, image=0):
    """the faces of a stack that paint: finite, non-zero z"""
    z = case["clouds"][image][::3, 2]
    return np.isfinite(z) & (z != 0)


def key_pattern(pattern, F):
    rng = np.random.default_rng([20261018, 31, F, sum(map(ord, pattern))])
    f = np.arange(F)
    inc = 2.0 + f * 2.0 ** -12                          # float32 values: 2 .. 6.0003
    sign = np.where(rng.random(F) < 0.5, -1.0, 1.0)
    mixed = rng.permutation(inc) * sign
    if pattern == "increasing":
        z = inc
    elif pattern == "decreasing":
        z = inc[::-1].copy()
    elif pattern == "shuffle":
        z = rng.permutation(inc)
    elif pattern == "equal":
        z = np.full(F, 2.5)
    elif pattern == "two-runs":                          # two long tied runs interleaved by face id
        z = np.where(f % 2 == 0, 2.0, 3.0)
    elif pattern == "ulp":                               # neighbouring floats, in a seeded order
        z = (np.uint32(0x40000000) + rng.permutation(F).astype(np.uint32)).view(F32).astype(np.float64)
    elif pattern == "negative":                          # faces behind the camera among faces in front
        z = mixed
    elif pattern == "zeros":                             # +0 and -0 interleaved: they tie and go by face id
        z = mixed
        z[f % 4 == 0] = 0.0
        z[f % 4 == 2] = -0.0
    elif pattern == "subnormal":                         # float32 subnormals of both signs around +-0, and the smallest normals
        z = rng.integers(1, 1 << 22, F) * 2.0 ** -149 * sign
        z[f % 5 == 0] = 0.0
        z[f % 5 == 1] = -0.0
        z[f % 5 == 2] = 2.0 ** -126 * sign[f % 5 == 2]
        z[:4] = np.array([1.0, -1.0, 2.0, -2.0])[:min(F, 4)] * 2.0 ** -149
    elif pattern == "inf":
        z = mixed
        z[f % 5 == 0] = np.inf
        z[f % 5 == 3] = -np.inf
    elif pattern == "nan":                               # NaN of both signs among finite and infinite keys
        z = mixed
        z[f % 5 == 0] = np.nan
        z[f % 5 == 2] = NEG_NAN
        z[f % 10 == 1] = np.inf
        z[f % 10 == 6] = -np.inf
    else:
        raise KeyError(pattern)
    return z


def _stack(name, group, zs, **promise):
    zs = np.atleast_2d(np.asarray(zs, np.float64))
    F = zs.shape[1]
    return _case(name, group, np.stack([stack_cloud(z) for z in zs]), np.arange(3 * F).reshape(F, 3), K32, S32, **promise)


def order():
    pad = lambda F: (1 << max(F - 1, 0).bit_length()) - F
    out = [_stack(f"stack-shuffle-{F}", "order", key_pattern("shuffle", F), F=F, pow2_pad=pad(F), rank_path=F > SORT_CAP, distinct_keys=F,
                  **({"entries_per_thread": 2} if F == 1025 else {})) for F in STACK_SIZES]
    P = lambda pattern, F, **pr: out.append(_stack(f"stack-{pattern}-{F}", "order", key_pattern(pattern, F), F=F, pow2_pad=pad(F), **pr))
    P("increasing", 1025, monotone=1); P("increasing", 255, monotone=1)
    P("decreasing", 1025, monotone=-1); P("decreasing", 257, monotone=-1)
    P("equal", 1025, tied_run=1025); P("equal", 1023, tied_run=1023)
    P("two-runs", 1025, tied_run=513, distinct_keys=2); P("two-runs", 4097, tied_run=2049, distinct_keys=2)
    P("ulp", 1025, one_ulp_apart=True, distinct_keys=1025); P("ulp", 2047, one_ulp_apart=True, distinct_keys=2047)
    P("negative", 1025, negative_keys=505); P("negative", 2049, negative_keys=1037)
    P("zeros", 1025, zero_keys=(257, 256), tied_run=513); P("zeros", 257, zero_keys=(65, 64), tied_run=129)
    P("subnormal", 1025, subnormal_keys=(206, 207), zero_keys=(204, 204), tied_run=408); P("subnormal", 1023, subnormal_keys=(191, 220), zero_keys=(204, 204), tied_run=408)
    P("inf", 1025, inf_keys=(205, 205)); P("inf", 255, inf_keys=(51, 51))
    out.append(_stack("batch-1025x3", "order", [key_pattern(p, 1025) for p in ("increasing", "shuffle", "negative")], F=1025, images=3,
                      orders_differ=True))
    return out


def non_finite():
    return [_stack("stack-nan-5", "non-finite", key_pattern("nan", 5), F=5, nan_keys=(1, 1), inf_keys=(1, 0)),
            _stack("stack-nan-1025", "non-finite", key_pattern("nan", 1025), F=1025, nan_keys=(205, 205), inf_keys=(103, 102))]


# ---- shading group --------------------------------------------------------------------------------------------------------------------
K64, S64 = cam(64, 48)


def _nz(a, b, c):
    return unit_normals(np.array([a, b, c]), np.array([[0, 1, 2]]))[0, 2]


def edge_face(a, ratio, exact=False):
    """a, a + (0.25, 0, 0), a + (0, 0.1, s): the normal is (0, -s / 4, 0.025), turned to (0, +, -) to face the camera, so the main light
    (above) lights it; |n_z| of the unit normal is 0.1 / sqrt(s^2 + 0.01) = ratio.  exact: s is moved by ulps until the double that
    face_key_normal computes IS the double `ratio`."""
    a = np.asarray(a, np.float64)
    s = 0.1 * np.sqrt(1.0 / ratio ** 2 - 1.0)
    face = lambda s, v=0.1: [a, a + [0.25, 0.0, 0.0], a + [0.0, v, s]]
    if exact:                                             # c.z = a.z + s is coarser than s: the rise v is moved by ulps as well
        for j in range(256):
            v = np.int64(np.float64(0.1).view(np.int64) + j).view(np.float64)
            lo, hi = int(np.float64(s * (1 - 1e-9)).view(np.int64)), int(np.float64(s * (1 + 1e-9)).view(np.int64))  # |n_z| falls as s grows
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if abs(_nz(*face(np.int64(mid).view(np.float64), v))) > ratio else (lo, mid)
            hit = [i for i in range(lo - 16, lo + 16) if abs(_nz(*face(np.int64(i).view(np.float64), v))) == ratio]
            if hit:
                return face(np.int64(hit[0]).view(np.float64), v)
        raise AssertionError(f"no face puts |n_z| exactly on {ratio}")
    return face(s)


def shading():
    out = []
    # a fan whose hub has 700 faces: the selection loop of k_rend_vnormal runs 700 x 700 steps for it, and sums 700 normals in painter order
    t = 2 * np.pi * np.arange(700) / 700
    rim = np.stack([0.55 * np.cos(t), 0.4 * np.sin(t), 2.5 + 0.3 * np.sin(3 * t) + 1e-4 * np.arange(700)], 1)
    fan = [[0, 1 + i, 1 + (i + 1) % 700] for i in range(700)]
    out.append(_case("shade-fan-700", "shading", np.concatenate([[[0.0, 0.0, 2.5]], rim]), fan, K64, S64, F=700, V=701, max_valence=700))
    # an open fan of 59 faces, one face that names the hub twice and one that names it three times: 64 slots, two positions met 2 and 3 times
    t = 2 * np.pi * np.arange(60) / 64
    rim = np.stack([0.5 * np.cos(t), 0.38 * np.sin(t), 2.2 + 0.25 * np.cos(2 * t)], 1)
    mesh = [[0, 1 + i, 2 + i] for i in range(59)]
    mesh[20:20] = [[0, 0, 31]]
    mesh[45:45] = [[0, 0, 0]]
    out.append(_case("shade-hub-64-repeats", "shading", np.concatenate([[[0.0, 0.0, 2.3]], rim]), mesh, K64, S64, F=61, max_valence=64,
                     named_twice=1, named_thrice=1))
    tri = _tri(K64, [(10, 8), (30, 10), (14, 30)], [2.0, 2.2, 2.1])
    out.append(_case("shade-vertex-in-no-face", "shading", tri + [[0.1, 0.1, 2.0]], [[0, 1, 2]], K64, S64, isolated=1, joints=None))
    lit = _tri(K64, [(40, 8), (60, 10), (44, 30)], [2.0, 2.2, 2.1])
    out.append(_case("shade-normals-cancel-exactly", "shading", tri + lit, [[0, 1, 2], [3, 4, 5], [0, 2, 1]], K64, S64, zero_sums=3))
    near = [list(np.add(tri[2], [0.0, 1e-9, 0.0])), list(np.add(tri[1], [0.0, 0.0, 1e-9]))]
    out.append(_case("shade-normals-cancel-almost", "shading", tri + near + lit, [[0, 1, 2], [0, 3, 4], [5, 6, 7]], K64, S64, zero_sums=0,
                     cancelling_sums=1))
    p = _tri(K64, [(20, 10), (30, 30), (40, 12), (50, 36)], [2.0, 2.5, 2.0, 2.5])
    out.append(_case("shade-vertices-on-the-lights", "shading", [list(MAIN_LIGHT), p[0], p[1], list(BACK_LIGHT), p[2], p[3]], [[0, 1, 2], [3, 4, 5], [1, 2, 4]],
                     K64, S64, on_light=[0, 3], z_negative=1))
    up = [[0.0, 0.0, 2.0], [0.2, 0.0, 2.0], [0.0, 0.2, 2.0]]                     # (b - a) x (c - a) = (0, 0, +0.04): turned round
    down = [[-0.3, 0.0, 2.0], [-0.3, 0.2, 2.0], [-0.1, 0.0, 2.0]]                # the other winding: (0, 0, -0.04), kept
    side = [[0.3, 0.0, 2.0], [0.4, 0.0, 2.0], [0.3, 0.0, 2.5]]                   # (0, -0.05, +0): n_z is exactly 0, kept
    out.append(_case("shade-nz-positive-negative-zero", "shading", up + down + side, np.arange(9).reshape(3, 3), K64, S64,
                     nz_class=[">0.1", ">0.1", "<1e-2"], nz_sum_positive=3, nz_sum_zero=3))
    faces, classes = [], []
    for i, (ratio, exact, cls) in enumerate(((0.099, False, "<0.1"), (0.1, True, "=0.1"), (0.1009, False, ">0.1"), (0.0099, False, "<1e-2"),
                                             (1e-2, True, "=1e-2"), (0.0101, False, "<0.1"))):
        faces += edge_face(at(K64, 4 + 10 * i, 44 - 4 * (i % 3), 2.0), ratio, exact)
        classes.append(cls)
    out.append(_case("shade-nz-around-0.1-and-1e-2", "shading", faces, np.arange(18).reshape(6, 3), K64, S64, nz_class=classes))
    for i, cls in ((4, "=1e-2"), (5, "<0.1")):            # the two faces around renderLambert's rule alone: lit or not, nothing painted over them
        out.append(_case(f"shade-nz-alone-{cls}", "shading", faces[3 * i:3 * i + 3], [[0, 1, 2]], K64, S64, nz_class=[cls]))
    return out


# ---- fill group -----------------------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (1, 40), (40, 1), (17, 15), (16, 16), (257, 1))


def _soup(k, size, n_tri, seed, spread=0.5, zlo=1.5, zhi=3.0):
    W, H = size
    rng = np.random.default_rng([20261018, 41, W, H, n_tri, seed])
    xy = rng.uniform([-spread * W, -spread * H], [(1 + spread) * W, (1 + spread) * H], (3 * n_tri, 2))
    z = rng.uniform(zlo, zhi, 3 * n_tri)
    return [at(k, x, y, zz) for (x, y), zz in zip(xy, z)]


def fill():
    out = []
    C = lambda name, verts, mesh=None, k=K32, size=S32, **pr: out.append(
        _case(name, "fill", verts, np.arange(len(verts)).reshape(-1, 3) if mesh is None else mesh, k, size, **pr))
    # every vertex on an integer row and column: floor and ceil change nothing; the second triangle lies on row 21 alone and returns at ay == cy
    C("fill-integer-vertices", _tri(K32, [(4, 3), (20, 3), (4, 19)]) + _tri(K32, [(4, 21), (10, 21), (16, 21)], [2.0, 3.0, 2.0]), integer_projections=True)
    C("fill-flat-top-and-bottom", _tri(K32, [(5, 4), (13, 4), (9, 11.5)]) + _tri(K32, [(22, 3.5), (18, 11), (29, 11)], 2.25)
      + _tri(K32, [(5, 13.25), (13, 13.25), (9, 21.5)], 2.5) + _tri(K32, [(22, 13.5), (18, 20.75), (29, 20.75)], 2.75), F=4)
    # the middle vertex (by row, then by column) above / left of the image, inside it, below / right of it
    C("fill-middle-vertex-rows", _tri(K32, [(5, -20), (25, -6), (12, 18)], 3.0) + _tri(K32, [(3, -10), (28, 10), (12, 20)], 2.5)
      + _tri(K32, [(6, 4), (25, 30), (12, 40)], 2.0), F=3)
    C("fill-middle-vertex-columns", _tri(K32, [(-20, 5), (-6, 20), (18, 12)], 3.0) + _tri(K32, [(-10, 3), (10, 22), (20, 12)], 2.5)
      + _tri(K32, [(4, 6), (40, 20), (50, 3)], 2.0), F=3)
    C("fill-whole-image", _tri(K32, [(-4.0 * 32 - 8, -8.0), (4.0 * 32 + 8, -8.0), (16, 8.0 * 24 + 8)]), F=1)
    C("fill-outside-on-four-sides", _tri(K32, [(4, -30), (20, -28), (10, -9)]) + _tri(K32, [(4, 33), (20, 31), (10, 60)]) + _tri(K32, [(-30, 4), (-28, 20), (-7, 10)])
      + _tri(K32, [(40, 4), (42, 20), (70, 10)]), F=4)
    ko, so = dict(fx=100.0, fy=100.0, cx=12.0, cy=30.0), (64, 48)
    zc = 3e-8                                             # 30 nm in front of the camera plane: the projection leaves the range of int
    for name, verts in (("x-max", [[0, 0, 2], [0, 0.15, 2], [1, 0, zc]]), ("x-min", [[0.5, 0, 2], [0.5, 0.15, 2], [-1, 0, zc]]),
                        ("y-min", [[0, 0, 2], [0.15, 0, 2], [0, 1, zc]]), ("y-max", [[0, 0.4, 2], [0.15, 0.4, 2], [0, -1, zc]])):
        C("fill-beyond-int-" + name, verts, k=ko, size=so, beyond_int=[2])
    C("fill-vertex-at-z-zero", _tri(K32, [(4, 3), (20, 3)]) + [[0.25, -0.25, 0.0]] + _tri(K32, [(20, 20), (30, 20), (24, 10)]), z_zero=1)
    C("fill-vertex-at-z-negative", _tri(K32, [(4, 3), (20, 3)]) + [[0.25, -0.25, -1.0]] + _tri(K32, [(20, 20), (30, 20), (24, 10)]), z_negative=1)
    C("fill-depth-above-255", _tri(K32, [(2, 2), (14, 3), (4, 20)], 300.0) + _tri(K32, [(16, 2), (30, 3), (18, 20)], [250.0, 258.0, 262.0]), F=2)
    for W, H in SIZES:
        k, size = cam(W, H, f=64.0)
        big = _tri(k, [(-4.0 * W - 8, -8.0), (4.0 * W + 8, -8.0), (W // 2, 8.0 * H + 8)], 4.0)     # behind the soup: every pixel is painted
        C(f"fill-size-{W}x{H}", big + _soup(k, size, 12, 0), k=k, size=size, F=13, npix=W * H)
    soup = _soup(K32, S32, 6, 1, spread=0.1)
    C("fill-both-windings", soup + soup, np.concatenate([np.arange(18).reshape(6, 3), 18 + np.arange(18).reshape(6, 3)[:, ::-1]]), F=12)
    return out


# ---- parts group ----------------------------------------------------------------------------------------------------------------------
PART_VALUES = (0, 23, 254, 255, 256, 511, -1)


def parts():
    """seven triangles side by side, triangle t on joint t with part PART_VALUES[t], and an eighth whose vertices carry 256, 23 and -1"""
    verts, joint = [], []
    for t in range(7):
        x0, y0 = 2 + 15 * (t % 4), 3 + 22 * (t // 4)
        verts += _tri(K64, [(x0, y0), (x0 + 12, y0 + 2), (x0 + 3, y0 + 17)], 2.0 + 0.125 * t)
        joint += [t, t, t]
    verts += _tri(K64, [(47, 25), (62, 28), (50, 45)], 3.0)
    joint += [4, 1, 6]
    return [_case("parts-beyond-a-byte", "parts", verts, np.arange(24).reshape(8, 3), K64, S64, joint=joint, n_joints=7, part_map=PART_VALUES,
                  part_values=sorted(PART_VALUES), J=7)]


# ---- tails group ----------------------------------------------------------------------------------------------------------------------
def tails():
    out = []
    for V in (255, 256, 257):
        for F in (255, 256, 257):
            rng = np.random.default_rng([20261018, 43, V, F])
            xy = rng.uniform([2, 2], [62, 46], (V, 2))
            z = rng.uniform(2.0, 3.0, V)
            mesh = np.stack([rng.permutation(V)[:3] for _ in range(F)])       # three different vertices per face
            out.append(_case(f"tails-V{V}-F{F}", "tails", [at(K64, x, y, zz) for (x, y), zz in zip(xy, z)], mesh, K64, S64,
                             joint=rng.integers(0, 3, V), n_joints=3, part_map=(5, 0, 9), v256=V % 256, f256=F % 256, V=V, F=F))
    tri = _tri(K64, [(10, 8), (50, 12), (24, 40)], [2.0, 2.5, 2.25])
    # more joints than vertices: k_rend_project's grid is sized by max(V, J) and its joint branch runs beyond V.  58 joints is the most a
    # model can have (3 + 3 J + K <= 179); the 300 joints that would take a second workgroup cannot be created.
    out.append(_case("tails-J58-V3", "tails", tri, [[0, 1, 2]], K64, S64, joint=[57, 0, 31], n_joints=58, part_map=np.arange(58) * 3 % 61,
                     J=58, V=3, j_above_v=True))
    out.append(_case("tails-J1-V3", "tails", tri, [[0, 1, 2]], K64, S64, J=1, V=3, j_above_v=False))
    return out


GROUPS = {"order": order, "non-finite": non_finite, "shading": shading, "fill": fill, "parts": parts, "tails": tails}
RESTATED = ("order", "shading", "fill", "parts", "tails")      # the groups the restatement is defined on
_BUILT = {}


def cases(group):
    if group not in _BUILT:
        _BUILT[group] = GROUPS[group]()
        names = [c["name"] for g in _BUILT.values() for c in g]
        assert len(names) == len(set(names)), "case names are unique"
    return _BUILT[group]


_REF = {}
RESTATEMENT_SECONDS = {}                                # case name, image -> what the restatement took


def reference(case, image=0):
    """the restatement's outputs for one image of a case (tests/avatar_render_restatement.py): computed once, shared, never written to"""
    import time
    import avatar_render_restatement as rst
    assert case["group"] in RESTATED, "the reference's sort is undefined on NaN keys"
    key = (case["name"], image)
    if key not in _REF:
        rst.lib()
        (W, H), t0 = case["size"], time.perf_counter()
        jt = None if case["joints"] is None else case["joints"][image]
        o = rst.render(case["clouds"][image], case["mesh"], case["intr"], W, H, vertex_part=vertex_part(case), joints=jt)
        RESTATEMENT_SECONDS[key] = time.perf_counter() - t0
        for a in o.values():
            a.setflags(write=False)
        _REF[key] = o
    return _REF[key]


def by_name(name):
    for g in GROUPS:
        for c in cases(g):
            if c["name"] == name:
                return c
    raise KeyError(name)
