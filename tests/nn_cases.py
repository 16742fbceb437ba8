"""Seeded inputs that put the nearest-neighbour kernels (avatar_amd/csrc/avt_nn.hip, avt_bucket.h) at their internal
boundaries: visible-candidate counts of a part at the kernels' constants, exact ties, the slab scan's stop rule, query
counts at the workgroup and tile sizes, and runs of equal matches for the bookkeeping.  A helper module of the tests, not a
test file; no GPU and no oracle are needed to build a case.

Every builder returns a list of cases (name, part_map, num_parts, cloud, vis, data, labels) for the SMPL-sized synthetic
model (synth.load_model(0), V = 6890; the vertices per main joint are 592, 700, 691, 450, ..., 69).  The expected values
come from tests/nn_restatement.py alone.  Some builders also return what they promise about their case (PROMISES: name ->
dict), which tests/test_nn_edges_cpu.py checks on the CPU."""
from __future__ import annotations

import numpy as np

from avatar_amd import synth

V = synth.NUM_VERTS
J = synth.NUM_JOINTS
SWEEP_N = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1983)
QUERY_N = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 2047, 2048, 2049, 4097)
TWIN_GAPS = (1, 2, 3, 4, 8, 31, 32, 33)
RUNS = (1, 2, 15, 16, 17, 63, 64, 65, 129, 600)
INVALID = (-1, None, 2 ** 31 - 1, -2 ** 31)           # None: num_parts
PROMISES = {}                                          # case name -> what the case promises about itself

_MJ = {}


def main_joint(model):
    if id(model) not in _MJ:
        _MJ[id(model)] = synth.main_joint(model)
    return _MJ[id(model)]


# ---- part maps ------------------------------------------------------------------------------------------------------
def part_map(name):
    """(part_map int32[24], num_parts)."""
    if name == "identity":
        return np.arange(J, dtype=np.int32), J
    if name == "merged":                                # joints 0, 1, 2 -> part 0 (1983 vertices), the rest -> 1..21
        return np.array([0, 0, 0] + list(range(1, J - 2)), np.int32), J - 2
    if name == "single":                                # 6890 candidates in one part: seven tiles, unsorted, above both caps
        return np.zeros(J, np.int32), 1
    if name == "sparse64":                              # the ABI's maximum; parts without a vertex in between and at both ends
        return np.array([2 + 2 * j + j // 6 for j in range(J)], np.int32), 64
    raise KeyError(name)


def part_of_vertex(model, pm):
    return np.asarray(pm)[main_joint(model)]


def _rng(*key):
    return np.random.default_rng([20261017, *key])


def _box(rng, n):
    return rng.uniform(-1.0, 1.0, (n, 3))              # a 2 m box


def _grid(rng, n, den=256, half=1):
    """n x 3 coordinates k / den in [-half, half]: squares and sums of differences are exact in float64."""
    return rng.integers(-half * den, half * den + 1, (n, 3)) / float(den)


def _half_vis(rng):
    return (rng.random(V) < 0.5).astype(np.uint8)


def _case(name, mapname, cloud, vis, data, labels, **promise):
    pm, npart = part_map(mapname)
    if promise:
        PROMISES[name] = promise
    return (name, pm, npart, np.ascontiguousarray(cloud, np.float64), np.ascontiguousarray(vis, np.uint8),
            np.ascontiguousarray(np.asarray(data, np.float64).reshape(-1, 3)), np.ascontiguousarray(labels, np.int32))


# ---- visible-candidate counts of a part at the kernels' constants ----------------------------------------------------
def sweep(model):
    out = []
    for mapname, part, ns in (("merged", 0, SWEEP_N), ("identity", 1, (511, 512, 513))):
        pm, npart = part_map(mapname)
        pov = part_of_vertex(model, pm)
        ids = np.nonzero(pov == part)[0]
        for n in ns:
            rng = _rng(1, part, n)
            vis = _half_vis(rng)
            vis[ids] = 0
            vis[rng.choice(ids, n, replace=False)] = 1
            data = _box(rng, 700)
            labels = np.concatenate([np.full(300, part), rng.integers(-1, npart + 1, 400)])      # -1 and num_parts included
            out.append(_case(f"sweep-{mapname}-{n}", mapname, _box(rng, V), vis, data, labels, part=part, visible=n))
    return out


# ---- a part that straddles a 1024-position tile of the part-sorted arrays ---------------------------------------------
def tiles(model):
    """identity: part 0 owns positions 0..591 and part 1 positions 592..1291, so for a workgroup whose queries begin in part 0
    the first tile ends at part 1's 432nd vertex.  A few queries of part 0 come first, then the queries of part 1, each a hair
    beside a vertex of part 1: half of them beside vertices in front of the boundary, half behind it."""
    pm, npart = part_map("identity")
    pov = part_of_vertex(model, pm)
    ids1 = np.nonzero(pov == 1)[0]
    split = 1024 - int((pov == 0).sum())
    out = []
    for k, kind in enumerate(("all-visible", "half-visible", "first-tile-empty")):
        rng = _rng(2, k)
        cloud = _box(rng, V)
        vis = np.ones(V, np.uint8) if kind == "all-visible" else _half_vis(rng)
        if kind == "first-tile-empty":
            vis[ids1[:split]] = 0
            vis[ids1[split:]] = 1
        lo = ids1[:split][vis[ids1[:split]] != 0]
        hi = ids1[split:][vis[ids1[split:]] != 0]
        tgt = np.concatenate([rng.choice(lo, 60) if len(lo) else rng.choice(hi, 60), rng.choice(hi, 60)])
        tgt = rng.permutation(tgt)
        data = np.concatenate([_box(rng, 8), cloud[tgt] + rng.uniform(-1e-4, 1e-4, (120, 3))])
        labels = np.concatenate([np.zeros(8), np.ones(120)])
        out.append(_case(f"tile-{kind}", "identity", cloud, vis, data, labels, split=split, targets=tgt, first=8))
    return out


# ---- exact ties -----------------------------------------------------------------------------------------------------
def _twin_case(model, name, mapname, part, gap, rng, front=0):
    """Vertices i and i + gap of the part's visible order share one position; one query beside every pair."""
    pm, npart = part_map(mapname)
    pov = part_of_vertex(model, pm)
    cloud = _grid(rng, V, den=64)
    vis = _half_vis(rng)
    vl = np.nonzero((pov == part) & (vis != 0))[0]
    first = np.array([i for i in range(len(vl) - gap) if (i // gap) % 2 == 0])
    cloud[vl[first + gap]] = cloud[vl[first]]
    off = np.array([1.0, -2.0, 1.0]) / 1024.0
    data = np.concatenate([_grid(rng, front, den=64), cloud[vl[first]] + off])
    labels = np.concatenate([np.zeros(front), np.full(len(first), part)])
    return _case(name, mapname, cloud, vis, data, labels, tie_queries=np.arange(front, len(labels)))


def ties(model):
    out = []
    # twins at one position with any other id of the part, under identity and single
    for k, mapname in enumerate(("identity", "single")):
        pm, npart = part_map(mapname)
        pov = part_of_vertex(model, pm)
        rng = _rng(3, 0, k)
        cloud = _box(rng, V)
        vis = _half_vis(rng)
        for q in range(npart):
            ids = rng.permutation(np.nonzero((pov == q) & (vis != 0))[0])
            half = len(ids) // 2
            cloud[ids[half:2 * half]] = cloud[ids[:half]]
        labels = rng.integers(0, npart, 900)
        out.append(_case(f"tie-twins-{mapname}", mapname, cloud, vis, _box(rng, 900), labels, tie_queries=np.arange(900)))
    # twins a fixed number of places apart in the part's visible order: same and different sub-lanes, same and different groups,
    # both sides of a tile boundary (identity: a few queries of part 0 in front, so that the workgroup's tiles begin at part 0)
    for gap in TWIN_GAPS:
        out.append(_twin_case(model, f"tie-gap{gap}-identity", "identity", 1, gap, _rng(3, 1, gap), front=8))
        out.append(_twin_case(model, f"tie-gap{gap}-merged", "merged", 0, gap, _rng(3, 2, gap)))
    # every visible vertex of a part at one point: the smallest visible id
    for k, (mapname, part) in enumerate((("identity", 1), ("merged", 0), ("single", 0))):
        pm, npart = part_map(mapname)
        pov = part_of_vertex(model, pm)
        rng = _rng(3, 3, k)
        cloud = _grid(rng, V)
        vis = _half_vis(rng)
        if mapname == "identity":
            vis[pov == part] = 1                        # 700 candidates, sorted; the others cross both caps
        cloud[pov == part] = np.array([0.25, -0.5, 0.125])
        data = _grid(rng, 300)
        labels = np.concatenate([np.full(200, part), rng.integers(0, npart, 100)])
        out.append(_case(f"tie-one-point-{mapname}", mapname, cloud, vis, data, labels, tie_queries=np.arange(200)))
    # tied pairs that differ in y - the sort separates them - with the smaller id at the larger y
    pm, npart = part_map("identity")
    pov = part_of_vertex(model, pm)
    rng = _rng(3, 4)
    cloud = _grid(rng, V, den=64)
    vis = _half_vis(rng)
    data, labels = [], []
    for q in (1, 3, 9, 23):
        vl = np.nonzero((pov == q) & (vis != 0))[0]
        pick = np.sort(rng.choice(len(vl), 2 * (len(vl) // 4), replace=False)).reshape(-1, 2)       # disjoint pairs, a < b
        Q = _grid(rng, len(pick), den=64)
        cloud[vl[pick[:, 0]]] = Q + np.array([1.0, 2.0, 0.0]) / 1024.0
        cloud[vl[pick[:, 1]]] = Q + np.array([1.0, -2.0, 0.0]) / 1024.0
        data.append(Q); labels.append(np.full(len(Q), q))
    data, labels = np.concatenate(data), np.concatenate(labels)
    out.append(_case("tie-y-split", "identity", cloud, vis, data, labels, tie_queries=np.arange(len(labels))))
    # tied pairs on ONE y at different x: nothing but the vertex id orders them in the sorted candidates
    rng = _rng(3, 6)
    cloud = _grid(rng, V, den=64)
    vis = _half_vis(rng)
    data, labels = [], []
    for q in (1, 3, 9, 23):
        vl = np.nonzero((pov == q) & (vis != 0))[0]
        pick = np.sort(rng.choice(len(vl), 2 * (len(vl) // 4), replace=False)).reshape(-1, 2)
        Q = _grid(rng, len(pick), den=64)
        flip = np.where(rng.random(len(pick)) < 0.5, 1.0, -1.0)[:, None]                 # the smaller id at the larger or the smaller x
        cloud[vl[pick[:, 0]]] = Q + flip * np.array([2.0, 0.0, 0.0]) / 1024.0 + np.array([0.0, 1.0, 1.0]) / 1024.0
        cloud[vl[pick[:, 1]]] = Q - flip * np.array([2.0, 0.0, 0.0]) / 1024.0 + np.array([0.0, 1.0, 1.0]) / 1024.0
        data.append(Q); labels.append(np.full(len(Q), q))
    data, labels = np.concatenate(data), np.concatenate(labels)
    out.append(_case("tie-x-split", "identity", cloud, vis, data, labels, tie_queries=np.arange(len(labels))))
    out += gap_ties(model)
    return out


def gap_ties(model):
    """The slab scan's stop rule at equality.  In every part: query q = (0, 0, 0) + t, candidate B = (0.75, 1.0, 0) + t with the
    larger id, candidate A = (0, 1.25, 0) + t with the smaller id, t = (0.25, -0.5, 2.5): both squared distances are exactly
    1.5625, and A's y gap squared is exactly the best distance once B has been seen - a scan that stops at 'gap * gap >= best'
    never looks at A.  Every query of the part is that one point, so the wave's worst best distance is 1.5625 too.  The answer
    is A.  Eight candidates lie on the other side (|y - y_q| >= 3); the rest lies behind A (|y - y_q| >= 3).
    'between': m further candidates between B and A in y, 6 m away in x (they cannot win), m = another number in every part,
    so that in some part A is the candidate just outside a round's chunk, wherever the walk started.  'mirror': y -> -y."""
    pm, npart = part_map("identity")
    pov = part_of_vertex(model, pm)
    t = np.array([0.25, -0.5, 2.5])
    out = []
    for kind, rot, sign in (("literal", None, 1.0), ("between", 0, 1.0), ("between", 12, 1.0), ("literal", None, -1.0), ("between", 0, -1.0), ("between", 12, -1.0)):
        rng = _rng(3, 5, 0 if rot is None else rot + 1, int(sign > 0))
        cloud = np.zeros((V, 3))
        vis = np.ones(V, np.uint8)
        answers = {}
        for q in range(npart):
            ids = np.nonzero(pov == q)[0]
            m = 0 if rot is None else (q + rot) % 24
            nfront = 8 if rot is not None else q % 17
            rel = _grid(rng, len(ids), den=64, half=2)
            rel[:, 1] = 3.0 + rng.integers(0, 129, len(ids)) / 64.0                    # behind A
            rel[0] = (0.0, 1.25, 0.0)                                                   # A: the smallest id of the part
            rel[1] = (0.75, 1.0, 0.0)                                                   # B
            rel[2:2 + nfront, 1] *= -1.0                                                # the other side of the query
            btw = slice(2 + nfront, 2 + nfront + m)
            rel[btw, 0] = 6.0
            rel[btw, 1] = 1.0 + rng.integers(1, 16, m) / 64.0
            rel[:, 1] *= sign
            cloud[ids] = rel + t
            answers[q] = int(ids[0])
        labels = np.repeat(np.arange(npart), 6)
        data = np.tile(t, (len(labels), 1))
        name = f"tie-stop-rule-{kind}{'' if rot is None else rot}{'-mirror' if sign < 0 else ''}"
        out.append(_case(name, "identity", cloud, vis, data, labels, tie_queries=np.arange(len(labels)), gap_tie=True, answers=answers))
    return out


# ---- geometry of the slab scan ----------------------------------------------------------------------------------------
def slabs(model):
    pm, npart = part_map("identity")
    pov = part_of_vertex(model, pm)
    out = []
    # all candidates of a part on one y
    rng = _rng(4, 0)
    cloud = _box(rng, V)
    vis = _half_vis(rng)
    for q in range(npart):
        cloud[pov == q, 1] = 0.03125 * q - 0.25
    labels = rng.integers(0, npart, 800)
    data = _box(rng, 800)
    data[::3, 1] = 0.03125 * labels[::3] - 0.25                                       # a third of the queries on that y as well
    out.append(_case("slab-one-y", "identity", cloud, vis, data, labels))
    # queries 10 m above and 10 m below every candidate: whole waves of either kind
    rng = _rng(4, 1)
    data = _box(rng, 1800)
    labels = np.repeat([1, 9, 22], 600)
    data[:, 1] += np.tile(np.repeat([10.0, -10.0], 300), 3)
    out.append(_case("slab-outside", "identity", _box(rng, V), _half_vis(rng), data, labels))
    # queries equal to a candidate (the best distance of a whole wave is 0), other candidates on the same y at smaller and
    # larger ids, some of them at the very same point
    rng = _rng(4, 2)
    cloud = _grid(rng, V, den=64)
    vis = _half_vis(rng)
    data, labels = [], []
    for q in (1, 4, 15):
        vl = np.nonzero((pov == q) & (vis != 0))[0]
        cloud[vl, 1] = rng.integers(0, 6, len(vl)) / 8.0                               # six levels of y
        tw = rng.permutation(len(vl))[:60].reshape(2, 30)
        cloud[vl[tw[1]]] = cloud[vl[tw[0]]]
        pick = rng.choice(vl, 256)
        pick = pick[np.argsort(cloud[pick, 1], kind="stable")]                        # thin slabs: a wave sees one or two levels
        data.append(cloud[pick]); labels.append(np.full(256, q))
    out.append(_case("slab-zero-distance", "identity", cloud, vis, np.concatenate(data), np.concatenate(labels), zero=True))
    # the pixels of a rendered frame against the posed model, in pixel order and in a random permutation (a wide slab)
    fr = synth.make_frame(model, 2)
    w0, p0, R0 = fr["start"]
    cloud = synth.pose_vertices(model, w0, p0, R0)
    rng = _rng(4, 3)
    vis = _half_vis(rng)
    sel = np.arange(0, len(fr["labels"]), 12)
    out.append(_case("slab-pixel-order", "identity", cloud, vis, fr["data"][sel], fr["labels"][sel]))
    sel = rng.permutation(sel)
    out.append(_case("slab-permuted", "identity", cloud, vis, fr["data"][sel], fr["labels"][sel]))
    # one wave (128 queries) that spans the whole y range of its part
    rng = _rng(4, 4)
    cloud = _box(rng, V)
    vis = _half_vis(rng)
    data = _box(rng, 128)
    y1 = cloud[(pov == 1) & (vis != 0), 1]
    data[:, 1] = rng.permutation(np.linspace(y1.min(), y1.max(), 128))
    out.append(_case("slab-whole-range", "identity", cloud, vis, data, np.ones(128)))
    return out


# ---- magnitudes -------------------------------------------------------------------------------------------------------
def magnitudes(model):
    pm, npart = part_map("identity")
    pov = part_of_vertex(model, pm)
    out = []
    rng = _rng(5, 0)
    cloud = 1e3 + rng.integers(-200, 201, (V, 3)) * 1e-9
    data = 1e3 + rng.integers(-200, 201, (600, 3)) * 1e-9
    out.append(_case("mag-1e3-1e-9", "identity", cloud, _half_vis(rng), data, rng.integers(0, npart, 600)))
    # differences of 1e-155 and 2e-155 along one axis: r = 1e-310 against 4e-310, both subnormal; the nearer candidates have
    # the larger ids, so a device that flushed subnormals would see all-zero distances and answer the part's first vertex
    for name, near, far in (("mag-subnormal", 1e-155, 2e-155), ("mag-underflow", 1e-170, 1e-170)):
        rng = _rng(5, 1 if near != far else 2)
        cloud = np.zeros((V, 3))
        vis = _half_vis(rng)
        for q in range(npart):
            ids = np.nonzero(pov == q)[0]
            cloud[ids, q % 3] = far
            cloud[ids[len(ids) // 2:], q % 3] = near
            cloud[ids[::2], q % 3] *= -1.0
        labels = rng.integers(0, npart, 400)
        out.append(_case(name, "identity", cloud, vis, np.zeros((400, 3)), labels, subnormal=(near != far), tie_queries=np.arange(400)))
    return out


# ---- query-side counts ------------------------------------------------------------------------------------------------
def _invalid_labels(rng, n, npart):
    vals = np.array([npart if v is None else v for v in INVALID], np.int64)
    return vals[rng.integers(0, len(vals), n)].astype(np.int32)


def queries(model):
    out = []
    pm, npart = part_map("identity")
    rng = _rng(6, 0)
    cloud, vis = _box(rng, V), _half_vis(rng)
    for n in QUERY_N:
        rng = _rng(6, 1, n)
        out.append(_case(f"queries-one-part-{n}", "identity", cloud, vis, _box(rng, n), np.full(n, 5)))
        out.append(_case(f"queries-all-parts-{n}", "identity", cloud, vis, _box(rng, n), rng.integers(0, npart, n)))
    rng = _rng(6, 2)
    out.append(_case("queries-all-invalid", "identity", cloud, vis, _box(rng, 300), _invalid_labels(rng, 300, npart)))
    out.append(_case("queries-first-part", "identity", cloud, vis, _box(rng, 300), np.zeros(300)))
    out.append(_case("queries-last-part", "identity", cloud, vis, _box(rng, 300), np.full(300, npart - 1)))
    out.append(_case("queries-parts-3-20", "identity", cloud, vis, _box(rng, 300), np.array([3, 20])[rng.integers(0, 2, 300)]))
    lab = rng.integers(0, npart, 600).astype(np.int32)
    lab[::5] = _invalid_labels(rng, len(lab[::5]), npart)
    out.append(_case("queries-some-invalid", "identity", cloud, vis, _box(rng, 600), lab))
    # 64 parts, most of them without a vertex: queries for those too, and invalid labels
    lab = rng.integers(0, 64, 900).astype(np.int32)
    lab[::7] = _invalid_labels(rng, len(lab[::7]), 64)
    out.append(_case("queries-sparse64", "sparse64", cloud, vis, _box(rng, 900), lab))
    out.append(_case("queries-sparse64-empty-parts-only", "sparse64", cloud, vis, _box(rng, 200), np.array([0, 1, 3, 52, 63])[rng.integers(0, 5, 200)]))
    for n in (1, 513, 4097):
        rng = _rng(6, 3, n)
        out.append(_case(f"queries-single-{n}", "single", cloud, vis, _box(rng, n), np.zeros(n)))
    return out


# ---- runs of equal matches for the bookkeeping ------------------------------------------------------------------------
def runs(model):
    """Consecutive queries of the frame that all match one vertex, in runs of RUNS, then an a, b, a, b alternation; the frame's
    first point lies 1.5 m from the rest (it is the centre of the fixed-point sums, whatever its label)."""
    out = []
    for k, (mapname, part, nvis, first_label) in enumerate((("identity", 1, 400, -1), ("identity", 1, 400, 1), ("merged", 0, 1200, 0), ("single", 0, 3000, 0))):
        pm, npart = part_map(mapname)
        pov = part_of_vertex(model, pm)
        rng = _rng(7, k)
        cloud = _box(rng, V)
        vis = _half_vis(rng)
        ids = np.nonzero(pov == part)[0]
        vis[ids] = 0
        vl = np.sort(rng.choice(ids, nvis, replace=False))
        vis[vl] = 1
        tg = rng.choice(vl, len(RUNS) + 2, replace=False)
        seq = np.concatenate([np.full(r, tg[i]) for i, r in enumerate(RUNS)] + [np.tile(tg[-2:], 100)])
        data = np.concatenate([[[2.5, 0.3, -0.2]], cloud[seq] + rng.uniform(-1e-5, 1e-5, (len(seq), 3))])
        labels = np.concatenate([[first_label], np.full(len(seq), part)])
        out.append(_case(f"runs-{mapname}-{nvis}-first{first_label}", mapname, cloud, vis, data, labels, sequence=seq))
    return out


GROUPS = {"sweep": sweep, "tiles": tiles, "ties": ties, "slabs": slabs, "magnitudes": magnitudes, "queries": queries, "runs": runs}
_CACHE = {}


def cases(model, group):
    if group not in _CACHE:
        _CACHE[group] = GROUPS[group](model)
    return _CACHE[group]


def all_cases(model):
    return [c for g in GROUPS for c in cases(model, g)]


def map_key(pm, npart):
    return (bytes(np.asarray(pm, np.int32).tobytes()), int(npart))
