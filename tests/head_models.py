"""Models away from SMPL's mesh size (V = 6890, F = 13776) for the kernels at the head of every ICP iteration (avatar_amd/csrc/
avt_kernels.hip: k_lbs, k_lbs_multi, k_visibility, k_visibility_frame, k_finalize, k_budget_hold).  A helper module of the tests, not a
test file; no GPU and no oracle are needed to build a model.

  procedural(V, F, J, K, tree, seed)   a made-up skeleton and mesh, for skinning and stand-alone visibility only (never fitted)
  resized(smpl, V, F, seed)            the synthetic SMPL model - skeleton, ten shape keys and prior unchanged - on another mesh

Both return SMPL-npz-style dicts that capi.ModelArrays takes (procedural: "weights" is a scipy.sparse V x J matrix, so that a stored 0.0
stays a stored entry).  PROMISES: case name -> what the case promises about itself; tests/test_head_edges_cpu.py checks every one."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from avatar_amd import synth

PROMISES = {}
MAX_LEVEL = 10              # joints with weights lie no deeper: <= 11 ancestors per vertex, avt_model_create allows 16
VIS_FRAME_LDS = 150 * 1024  # k_visibility_frame runs while 16 V + roundup4(V) fits (avt_capi.cpp)

# (V, F, J, K, tree): why
PROCEDURAL = [
    ((1, 1, 1, 1, "chain"), "one vertex, root only"),
    ((3, 1, 2, 1, "chain"), "smallest non-degenerate face"),
    ((255, 257, 3, 1, "star"), "last partial workgroup on V, first extra workgroup on F"),
    ((256, 256, 3, 9, "star"), "exact multiples; K just below the unrolled path"),
    ((257, 255, 3, 11, "star"), "one vertex into a second workgroup; K just above the unrolled path"),
    ((257, 255, 3, 16, "star"), "K at AVT_MAX_SHAPE"),
] + [((257, 255, J, 3, "random"), "the 12 J and 9 J loops on both sides of 256 and 512") for J in (21, 22, 28, 29, 42, 43, 56, 57)] + [
    ((513, 511, 58, 2, "chain"), "P = 179, the ABI's largest; 58 tree levels"),
]
# what the rows promise, written out by hand: (V % 256, F % 256, passes of the 9 J loop, passes of the 12 J loop, most ancestors on a vertex)
_PROCEDURAL_PROMISES = {
    (1, 1, 1, 1): (1, 1, 1, 1, 1), (3, 1, 2, 1): (3, 1, 1, 1, 2), (255, 257, 3, 1): (255, 1, 1, 1, 2), (256, 256, 3, 9): (0, 0, 1, 1, 2),
    (257, 255, 3, 11): (1, 255, 1, 1, 2), (257, 255, 3, 16): (1, 255, 1, 1, 2),
    (257, 255, 21, 3): (1, 255, 1, 1, None), (257, 255, 22, 3): (1, 255, 1, 2, None), (257, 255, 28, 3): (1, 255, 1, 2, None),
    (257, 255, 29, 3): (1, 255, 2, 2, None), (257, 255, 42, 3): (1, 255, 2, 2, None), (257, 255, 43, 3): (1, 255, 2, 3, None),
    (257, 255, 56, 3): (1, 255, 2, 3, None), (257, 255, 57, 3): (1, 255, 3, 3, None), (513, 511, 58, 2): (1, 255, 3, 3, 11),
}
RESIZED = [(255, 257), (256, 256), (257, 255), (1023, 1025), (1024, 1024), (1025, 1023), (8192, 13776), (8193, 13777), (9035, 2048), (9036, 2049)]
# (V % 256, F % 256, ceil(V / 1024), k_finalize's path, 16 V + roundup4(V), k_visibility_frame allowed)
_RESIZED_PROMISES = {
    (255, 257): (255, 1, 1, "registers", 4336, True), (256, 256): (0, 0, 1, "registers", 4352, True), (257, 255): (1, 255, 1, "registers", 4372, True),
    (1023, 1025): (255, 1, 1, "registers", 17392, True), (1024, 1024): (0, 0, 1, "registers", 17408, True), (1025, 1023): (1, 255, 2, "registers", 17428, True),
    (8192, 13776): (0, 208, 8, "registers", 139264, True), (8193, 13777): (1, 209, 9, "loop", 139284, True),
    (9035, 2048): (75, 0, 9, "loop", 153596, True), (9036, 2049): (76, 1, 9, "loop", 153612, False),
}
SKINNED_RESIZED = [(255, 257), (1025, 1023), (9036, 2049)]       # the resized models that also go through the skinning tests
_CACHE = {}


def dense_weights(model):
    W = model["weights"]
    return np.asarray(W.toarray() if sp.issparse(W) else W, np.float64)


def parents(model):
    p = np.asarray(model["kintree_table"])[0].astype(np.int64).copy()
    p[0] = -1
    return p


def levels(parent):
    lv = np.zeros(len(parent), np.int64)
    for j in range(1, len(parent)):
        lv[j] = lv[parent[j]] + 1
    return lv


def ancestor_counts(model):
    """Per vertex: joints on the union of the root chains of its joints with a weight above 1e-12 (AvatarOptimizer.cpp:187-213)."""
    W, parent = dense_weights(model), parents(model)
    J = len(parent)
    under = np.zeros((J, J), bool)                 # under[a, j]: a lies on the root chain of j
    for j in range(J):
        a = j
        while a != -1:
            under[a, j] = True
            a = parent[a]
    return ((W > 1e-12).astype(np.int64) @ under.T.astype(np.int64) > 0).sum(1)


def shape_promises(V, F, J):
    """What the kernels' constants make of (V, F, J), computed: the CPU test compares them with the hand-written tables above."""
    lds = 16 * V + ((V + 3) & ~3)
    chunk = (V + 1023) // 1024
    return dict(v256=V % 256, f256=F % 256, passes9=(9 * J + 255) // 256, passes12=(12 * J + 255) // 256, chunk=chunk,
                finalize="registers" if chunk <= 8 else "loop", vis_lds=lds, vis_frame=lds <= VIS_FRAME_LDS)


# ---- procedural models ------------------------------------------------------------------------------------------------------------------
def threshold_faces(F):
    """Face indices that carry the threshold triangles: 0, 255, 256 and F - 1 where F allows, filled up to four from 1, 2, 3."""
    if F < 4:
        return []
    at = sorted({i for i in (0, 255, 256, F - 1) if i < F})
    at += [i for i in (1, 2, 3) if i not in at][:4 - len(at)]
    return sorted(at)


def procedural(V, F, J, K, tree, seed=0):
    key = ("procedural", V, F, J, K, tree, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng([20261018, V, F, J, K, seed])
    parent = np.full(J, -1, np.int64)
    for j in range(1, J):
        parent[j] = j - 1 if tree == "chain" else 0 if tree == "star" else int(rng.integers(max(0, j - 3), j))      # random: one of the three in front
    lv = levels(parent)
    shallow = np.nonzero(lv <= MAX_LEVEL)[0]
    deepest = int(shallow[np.argmax(lv[shallow])])
    # special vertices: a stored 0.0 weight (the first of them in the first slot), weights that sum to 0.7
    special = rng.permutation(V)[:6] if (V >= 8 and J >= 2) else np.zeros(0, np.int64)
    zero_at, low_sum = list(special[:3]), list(special[3:])
    rows, cols, vals = [], [], []
    for v in range(V):
        want_zero = v in zero_at
        pool = shallow[lv[shallow] >= 1] if want_zero else shallow
        leaf = deepest if v == 0 else int(pool[rng.integers(len(pool))])
        chain = []
        a = leaf
        while a != -1:
            chain.append(a)
            a = int(parent[a])
        chain = chain[::-1]                                         # root first = ascending joint id
        n = int(rng.integers(2 if want_zero else 1, min(4, len(chain)) + 1))
        js = sorted([int(j) for j in rng.choice(chain[:-1], n - 1, replace=False)] + [leaf])
        w = rng.dirichlet(np.ones(n)) * 0.9 + 0.1 / n               # every weight at least 0.1 / n
        if want_zero:
            slot = 0 if v == zero_at[0] else int(rng.integers(n))
            w[slot] = 0.0
            w /= w.sum()
        if v in low_sum:
            w *= 0.7
        rows += [v] * n; cols += js; vals += list(w)
    W = sp.csr_matrix((np.array(vals), (np.array(rows), np.array(cols))), shape=(V, J))
    assert W.nnz == len(vals)                                       # the stored zeros are still stored
    # faces: random triples; the threshold triangles (threshold_cloud) on vertices no other face uses; one degenerate face
    at = threshold_faces(F)
    pool = V - 3 * len(at)
    assert pool >= 1
    if V >= 3 and F == 1:
        faces = np.array([[0, 1, 2]], np.int64)
    else:
        faces = rng.integers(0, pool, (F, 3))
    for i, fidx in enumerate(at):
        faces[fidx] = pool + 3 * i + np.arange(3)
    if F >= 8:
        d = next(i for i in range(F // 2, F) if i not in at)
        faces[d, 1] = faces[d, 0]
    Jr = np.zeros((J, V))
    for j in range(J):
        np.add.at(Jr[j], rng.integers(0, V, 5), rng.dirichlet(np.ones(5)))
    kin = np.stack([parent, np.arange(J)])
    m = dict(v_template=rng.uniform(-1.0, 1.0, (V, 3)), f=faces, kintree_table=kin, J_regressor=Jr, weights=W,
             shapedirs=rng.normal(0.0, 0.02, (V, 3, K)))
    m["_special"] = dict(stored_zero=[int(v) for v in zero_at], first_slot_zero=int(zero_at[0]) if zero_at else None, low_sum=[int(v) for v in low_sum])
    _CACHE[key] = m
    return m


def procedural_name(row):
    V, F, J, K, tree = row
    return f"procedural-{V}-{F}-{J}-{K}-{tree}"


def procedural_cases():
    """[(name, model)] of the table; PROMISES filled."""
    out = []
    for row, why in PROCEDURAL:
        V, F, J, K, tree = row
        name = procedural_name(row)
        v256, f256, p9, p12, anc = _PROCEDURAL_PROMISES[(V, F, J, K)]
        PROMISES[name] = dict(why=why, v256=v256, f256=f256, passes9=p9, passes12=p12, chunk=1, finalize="registers", vis_frame=True,
                              anc_max=anc, anc_le=MAX_LEVEL + 1, levels={"chain": J, "star": min(J, 2)}.get(tree))
        out.append((name, procedural(*row)))
    return out


# ---- the synthetic SMPL model on another mesh -------------------------------------------------------------------------------------------
def resized(smpl, V, F, seed=0):
    key = ("resized", id(smpl), V, F, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng([20261018, 7, V, F, seed])
    vt = np.asarray(smpl["v_template"], np.float64)
    sd = np.asarray(smpl["shapedirs"], np.float64)
    W = np.asarray(smpl["weights"], np.float64)
    faces = np.asarray(smpl["f"]).astype(np.int64)
    V0, J = W.shape
    jpos = np.asarray(smpl["J_regressor"], np.float64) @ vt
    if V < V0:
        mj = synth.main_joint(smpl)
        counts = np.bincount(mj, minlength=J)
        quota = np.maximum(4, counts * V // V0)
        while quota.sum() > V:
            quota[np.argmax(quota)] -= 1
        while quota.sum() < V:
            quota[np.argmax(counts - quota)] += 1
        assert (quota >= 4).all() and (quota <= counts).all()
        keep = np.sort(np.concatenate([rng.choice(np.nonzero(mj == j)[0], quota[j], replace=False) for j in range(J)]))
        new = np.full(V0, -1, np.int64)
        new[keep] = np.arange(V)
        nf = new[faces]
        nf = nf[(nf >= 0).all(1)]
        vt2, sd2, W2 = vt[keep], sd[keep], W[keep]
    else:
        e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
        e = np.unique(e, axis=0)
        e = e[np.sort(rng.choice(len(e), V - V0, replace=False))]
        vt2 = np.concatenate([vt, 0.5 * (vt[e[:, 0]] + vt[e[:, 1]])])
        sd2 = np.concatenate([sd, 0.5 * (sd[e[:, 0]] + sd[e[:, 1]])])
        W2 = np.concatenate([W, W[e[:, 0]]])
        nf = faces
    assert len(np.unique(vt2, axis=0)) == V                        # no two vertices coincide
    nf = nf[:F]
    if len(nf) < F:
        nf = np.concatenate([nf, rng.integers(0, V, (F - len(nf), 3))])
    Jr = np.zeros((J, V))
    for j in range(J):
        near = np.argsort(((vt2 - jpos[j]) ** 2).sum(1), kind="stable")[:8]
        Jr[j, near] = 0.125
    m = dict(smpl)
    m.update(v_template=vt2, shapedirs=sd2, weights=W2, f=nf, J_regressor=Jr)
    _CACHE[key] = m
    return m


def resized_name(V, F):
    return f"resized-{V}-{F}"


def resized_cases(smpl, sizes=None):
    out = []
    for V, F in (RESIZED if sizes is None else sizes):
        name = resized_name(V, F)
        v256, f256, chunk, path, lds, frame = _RESIZED_PROMISES[(V, F)]
        PROMISES[name] = dict(v256=v256, f256=f256, passes9=1, passes12=2, chunk=chunk, finalize=path, vis_lds=lds, vis_frame=frame, anc_max=None, anc_le=16)
        out.append((name, resized(smpl, V, F)))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def poses(model, n, seed=0):
    """n seeded poses (w (n, K), p (n, 3), R (n, J, 3, 3)): |w| up to 3, joint rotations up to 1.5 rad about random axes."""
    J = np.asarray(model["kintree_table"]).shape[1]
    K = np.asarray(model["shapedirs"]).shape[2]
    rng = np.random.default_rng([20261018, 11, J, K, seed])
    w = rng.uniform(-3.0, 3.0, (n, K))
    p = rng.uniform(-1.0, 1.0, (n, 3)) + np.array([0.0, 0.0, 2.5])
    R = np.empty((n, J, 3, 3))
    for f in range(n):
        for j in range(J):
            ax = rng.normal(size=3)
            R[f, j] = synth.rodrigues(ax / np.linalg.norm(ax) * rng.uniform(0.0, 1.5))
    return w, p, R


def probe(model, cloud, seed):
    """A frame that probes the head of an ICP iteration: the cloud's own vertices as data (every one at distance zero from its vertex),
    labelled with the vertex's part under the identity part map, about 1 % of the labels (three at least) set to -1."""
    rng = np.random.default_rng([20261018, 17, len(cloud), seed])
    labels = synth.main_joint(model).astype(np.int32)
    labels[rng.choice(len(labels), max(3, len(labels) // 100), replace=False)] = -1
    return np.ascontiguousarray(cloud, np.float64), labels


def starts(smpl, n, first=40):
    """n start states (p (n, 3), q (n, 24, 4), w (n, 10)) of the SMPL skeleton: different poses in front of the camera."""
    from avatar_amd import api
    st = [synth.sample_ground_truth(smpl, first + s) for s in range(n)]
    return np.array([s[1] for s in st]), np.array([api.rot_to_quat(s[2]) for s in st]), np.array([s[0] for s in st])


THRESHOLD_C = (1e-4, float(np.nextafter(1e-4, 1.0)), -1e-4)


def threshold_clouds(model, seed=0):
    """Clouds that put faces exactly at the visibility threshold: a face gets p1 = (0, 0), p2 = (1, 0), p3 = (0, -c), hence
    z = (p2 - p1) x (p1 - p3) = c exactly, with c = 1e-4 (kind 0, not visible: the test is strict), the next double above (kind 1, visible),
    -1e-4 (kind 2), and the next double above 1e-4 with the winding reversed (kind 3, z = -c).  Every other vertex lies at (0, 0): a face
    that shares vertices with one threshold face only has z in {0, +-c} and is visible only where the threshold face itself is.
    The faces are threshold_faces(F).  Where their vertices are theirs alone (the procedural models) there are four clouds, every face
    going through every kind; where the mesh shares vertices between them (a real mesh) every cloud holds one face of one kind.
    Returns [(cloud, {face index: (kind, vertices)})]."""
    faces = np.asarray(model["f"]).astype(np.int64)
    V = np.asarray(model["v_template"]).shape[0]
    at = threshold_faces(len(faces))
    rng = np.random.default_rng([20261018, 13, V, len(faces), seed])
    used = np.bincount(faces.reshape(-1), minlength=V)
    if (used[faces[at].reshape(-1)] == 1).all():                    # twelve vertices, each in its threshold face alone
        plans = [[(f, (i + r) % 4) for i, f in enumerate(at)] for r in range(4)]
    else:
        plans = [[(f, k)] for f in at for k in range(4)]
    out = []
    for plan in plans:
        cloud = np.zeros((V, 3))
        cloud[:, 2] = rng.uniform(1.0, 3.0, V)
        placed = {}
        for fidx, kind in plan:
            i1, i2, i3 = faces[fidx]
            assert len({int(i1), int(i2), int(i3)}) == 3
            c = THRESHOLD_C[kind] if kind < 3 else THRESHOLD_C[1]
            a, b = ((1.0, 0.0), (0.0, -c)) if kind < 3 else ((0.0, -c), (1.0, 0.0))
            cloud[i1, :2] = (0.0, 0.0); cloud[i2, :2] = a; cloud[i3, :2] = b
            placed[int(fidx)] = (kind, (int(i1), int(i2), int(i3)))
        out.append((cloud, placed))
    return out
