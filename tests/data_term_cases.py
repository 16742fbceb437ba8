"""Frames that walk the ICP data term along its POINT axis: the number of matched vertices M, of data points N and of evaluation workgroups
G, at the values where the kernels of the row form (avt_eval.hip k_records / k_eval / k_reduce*, avt_lm.hip eval_ranges and the riding
reduction) and of the moment form (avt_moments.hip k_moments) take another path.  A helper module of the tests (host only: numpy and the
oracle); tests/test_data_term_cases_cpu.py checks what every case promises, tests/test_gpu_data_term_grid.py runs them.

The data term works on matched VERTICES: the matches of a vertex are aggregated into one weighted record (weight c_m = its number of matched
data points), 16 records are a batch, and workgroup g of G takes the batches g, g + G, .. (G >= 64) or a contiguous range (G < 64).

  base(name)          a model with a FULL frame: fit_models.fit_frame (SMPL: synth.make_frame, data rounded to the 2^-40 grid), occlusion off.
                      The small models' frames get one more data point for every vertex the frame leaves unmatched, 0.45 of the way to the
                      vertex's nearest neighbour of its part: every vertex is matched, so M reaches V (131 batches at V = 2088, 1026 at 16416)
  case_keys(name)     the cases of the model, case(name, key) one of them: the data points whose match (the oracle's, at the start state) is
                      in a chosen set of M matched vertices - a query's match does not depend on the other queries, so M is exact.  The first
                      data point of the full frame stays in every case (labelled -1 where its match is not chosen): the same frame centre.
"""
from __future__ import annotations

import zlib

import numpy as np

import fit_models as fm

EVAL_PTS = 16               # AVT_EVAL_PTS (avt_internal.h): matched vertices per batch
G_MAX = 128                 # AVT_G_MAX (avt_internal.h)
ERANGE_CAP = 1024           # AVT_ERANGE_CAP (avt_lm.hip): more batches than this and eval_ranges deals equal counts
ERANGE_ROOM_HS8 = 982       # the ints the HS = 8 solve has for eval_ranges' prefix sums (avt_lm.hip k_solve: room - 2)
MOM_SEG = 512               # MOM_SEG (avt_moments.hip): list entries compacted per pass
MOM_UN = 2                  # MOM_UN (avt_moments.hip); a segment's matched entries are padded to a multiple of 4 MOM_UN
MOM_PAD = 4 * MOM_UN
CONST_ROWS, CONST_MOMENTS = 256, 2048       # data points per cost-constant block (fb.const_used: avt_kernels.hip, avt_capi.cpp)
STRIDED_MIN = 64            # G >= 64: strided batches, k_reduce_strip (avt_eval.hip, avt_capi.cpp choose_G)
GRIDS = (1, 2, 63, 64, 65, 127, 128)
FIX = 2.0 ** 40             # AVT_FIX_SCALE (avt_nn.hip)
COST_BAR = 1e-9             # the GPU file's bar on the cost ...
KAPPA_C_MAX = COST_BAR / 4 / (64 * 2.0 ** -53)      # ... and what it allows the cost's cancellation factor, a factor 4 in hand like fm.KAPPA_MAX
SHORT_FIT = dict(icp_iters=2, max_iters_per_icp=3)

# name -> (J, K, tree, ncomps, per_joint) of fit_models.fit_model; "smpl" is the suite's synthetic SMPL
SMALL = {
    "j9k4": (9, 4, "star", 3, 232),         # V = 2088, 131 batches: the smallest that gives a G = 64 workgroup a third batch
    "j2k2": (2, 2, "chain", 0, 1030),       # pair lists of 1374 / 344 / 1030 entries: MOM_SEG crossed twice, the shared pair (0, 1)
    "j45k5": (45, 5, "ternary", 0, 12),     # NT = 9: the row-dealt k_eval<0,0,9>, the 1024-thread solve, k_reduce with pair >= 64
    "j1k1": (1, 1, "chain", 0, 16416),      # 1026 batches: above ERANGE_CAP and the HS = 8 solve's room - eval_ranges' equal counts
}
MODELS = ("smpl",) + tuple(SMALL)
MOM_OK = {"smpl": True, "j9k4": True, "j2k2": True, "j45k5": False, "j1k1": True}      # K + 1 <= 16 and 3 + 3J + K <= 87 (avt_model.cpp); V does not enter
# the frame's seed: a model whose cases miss a condition of tests/test_data_term_cases_cpu.py gets another one here
FRAME_SEED = {"smpl": 0, "j9k4": 0, "j2k2": 0, "j45k5": 0, "j1k1": 0}
# (model, key) -> seed of a random selection, where seed 0 misses the cap on kappa_c or the conditions on the short fits
SEL_SEED = {("j2k2", ("M", 17, "rand", None)): 1}       # (seed 0: its short fit ends 1e-7 of the start cost away from zero, lambda_conditioning 5e6)
SEGMENTS = ((0, 8, 0), (1, 0, 7), (9, 512, 6), (511, 0, 1), (512, 512, 6))      # matched entries per segment of j2k2's pair (0, 0)
# j1k1 fits ONE matched vertex exactly (a translation does): the cost behind the step is 1e-9 of its terms at every seed (kappa_c 7e8), and
# no double-precision evaluation has nine digits of it.  M = 1 stays with the four other models.
EXCLUDED = {("j1k1", 1)}
POINT_COUNTS = (255, 256, 257, 2047, 2048, 2049)
_BASE, _CASE = {}, {}


def tail_of(N):
    """how many of a point-count case's N data points, the last ones, carry label -1: 300, or 100 where the frame is too short for that -
    the last cost-constant block of either form (N = 257: one point; N = 2049) then holds no matched point"""
    return 300 if N > 600 else 100


def _on_grid(x):
    return np.rint(np.asarray(x, np.float64) * FIX) / FIX


def _nn(b, data, labels):
    fr = b["frame"]
    return b["om"].nn(fr["part_map"], fr["num_parts"], b["cloud0"], np.ones(b["om"].V, np.uint8), data, labels)


def base(name):
    """dict(name, model, om, frame (as fit_models.fit_frame: data, labels, part_map, num_parts, start (p, q, w), betas), cloud0 (the model's
    points at the start state), corr (the oracle's correspondences of the full frame there), matched (its distinct matched vertices, sorted),
    count (matches per vertex), centre (the first data point))"""
    if name in _BASE:
        return _BASE[name]
    from oracle import oracle as orc
    seed = FRAME_SEED[name]
    if name == "smpl":
        from avatar_amd import api, synth
        from avatar_amd.capi import Options
        m = synth.load_model(0)
        om = orc.OracleModel(m)
        sf = synth.make_frame(m, 70 + seed)
        w0, p0, R0 = sf["start"]
        o = Options.demo()
        fr = dict(data=np.ascontiguousarray(_on_grid(sf["data"])), labels=np.ascontiguousarray(sf["labels"], np.int32), part_map=synth.identity_part_map(),
                  num_parts=om.J, start=(np.asarray(p0, np.float64), api.rot_to_quat(R0), np.asarray(w0, np.float64)), betas=(o.beta_pose, o.beta_shape))
    else:
        J, K, tree, nc, per = SMALL[name]
        m = fm.fit_model(J, K, tree, nc, seed, per_joint=per)
        om = orc.OracleModel(m)
        fr = dict(fm.fit_frame(m, om, seed))
    b = dict(name=name, model=m, om=om, frame=fr, cloud0=om.points(*fr["start"]))
    if name != "smpl":
        _fill(b, seed)
    b["corr"] = _nn(b, fr["data"], fr["labels"])
    b["matched"] = np.unique(b["corr"][b["corr"] >= 0])
    b["count"] = np.bincount(b["corr"][b["corr"] >= 0], minlength=om.V)
    b["centre"] = fr["data"][0].copy()
    _BASE[name] = b
    return b


def _fill(b, seed):
    """one more data point for every vertex the frame leaves unmatched: 0.45 of the distance to the vertex's nearest neighbour of its part
    away from it in a random direction, on the grid, labelled with the part"""
    from scipy.spatial import cKDTree
    fr, om = b["frame"], b["om"]
    corr = _nn(b, fr["data"], fr["labels"])
    mj = om.main_joint()
    missing = np.setdiff1d(np.arange(om.V), corr[corr >= 0])
    if not len(missing):
        return
    rng = np.random.default_rng([20261019, 7, om.J, om.K, seed])
    gap = np.full(om.V, 0.05)
    for j in range(om.J):
        vs = np.nonzero(mj == j)[0]
        if len(vs) > 1:
            gap[vs] = cKDTree(b["cloud0"][vs]).query(b["cloud0"][vs], k=2)[0][:, 1]
    d = rng.standard_normal((len(missing), 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    extra = _on_grid(b["cloud0"][missing] + 0.45 * gap[missing, None] * d)
    fr["data"] = np.ascontiguousarray(np.concatenate([fr["data"], extra]))
    fr["labels"] = np.ascontiguousarray(np.concatenate([fr["labels"], fr["part_map"][mj[missing]]]).astype(np.int32))


def grid_counts(V):
    """the values of M the grids G = 64 and 128 ask for, below V: (M, G)"""
    out = [(0, None), (1, None), (15, None), (16, None), (17, None)]
    for G in (64, 128):
        out += [(16 * G - 1, G), (16 * G, G), (16 * G + 1, G), (32 * G + 1, G)]
    return [(M, G) for M, G in out if M < V]


def case_keys(name):
    """[key]: ("M", M, "first" | "rand", G or None), ("all",), ("mult", copies), ("one", 2049), ("N", N), ("seg", (a, b, c))"""
    b = base(name)
    nm, nfull = len(b["matched"]), len(b["frame"]["labels"])
    keys = []
    for M, G in grid_counts(nm):
        if (name, M) in EXCLUDED:
            continue
        keys += [("M", M, "first", G)] + ([("M", M, "rand", G)] if M else [])
    keys.append(("all",))
    if name in ("smpl", "j9k4"):
        keys += [("mult", 1), ("mult", 2), ("mult", 1000), ("one", 2049)]
    keys += [("N", N) for N in POINT_COUNTS if N <= nfull]
    if name == "j2k2":
        keys += [("seg", s) for s in SEGMENTS]
    return keys


def key_id(key):
    return "-".join("x".join(str(y) for y in x) if isinstance(x, tuple) else str(x) for x in key if x is not None)


def pair_lists(model):
    """{(a, b): vertices}, a <= b: the static lists of k_moments as avt_model.cpp build_moment_tables makes them - per pair of joints the
    vertices assigned to both (weight > 1e-12, avt_model_create), in vertex order.  (No avt_model_* accessor gives them: derived from the weights.)"""
    W = np.asarray(model["weights"].todense()) if hasattr(model["weights"], "todense") else np.asarray(model["weights"])
    on = W > 1e-12
    out = {}
    for v in range(W.shape[0]):
        js = np.nonzero(on[v])[0]
        for a in js:
            for c in js:
                if a <= c:
                    out.setdefault((int(a), int(c)), []).append(v)
    return {k: np.array(v) for k, v in out.items()}


def segment_counts(lst, count):
    """matched entries per MOM_SEG segment of a pair list (count: matches per vertex)"""
    return tuple(int((count[lst[s:s + MOM_SEG]] > 0).sum()) for s in range(0, len(lst), MOM_SEG))


def deal(nb, G):
    """batches per workgroup under the strided deal of k_eval: workgroup g takes g, g + G, .. below nb"""
    return np.array([len(range(g, nb, G)) for g in range(G)])


def _select(b, chosen):
    """the full frame's data points whose match is in `chosen`, the first data point kept in any case"""
    fr = b["frame"]
    keep = np.isin(b["corr"], chosen) & (b["corr"] >= 0)
    idx = np.nonzero(keep)[0]
    labels = fr["labels"].copy()
    corr = b["corr"].copy()
    if not keep[0]:
        idx = np.concatenate([[0], idx])
        labels[0], corr[0] = -1, -1
    return fr["data"][idx], labels[idx], corr[idx]


def _copies(b, i0, n, rng):
    """n copies of data point i0, all but the first moved by at most 1e-4 per coordinate, on the grid"""
    d = np.repeat(b["frame"]["data"][i0][None], n, 0)
    d[1:] += _on_grid(rng.uniform(-1e-4, 1e-4, (n - 1, 3)))
    return _on_grid(d)


def case(name, key):
    """dict(name, key, data, labels, corr (the oracle's, what the case expects of the device), M, N, nb (batches), grid (the G the case is named
    for, or None), frame (data and labels in fit_models' frame format), seg (matched entries per segment of pair (0, 0): the segment cases))"""
    if (name, key) in _CASE:
        return _CASE[(name, key)]
    b = base(name)
    fr = b["frame"]
    matched = b["matched"]
    rng = np.random.default_rng([20261019, 11, zlib.crc32(repr((name, key)).encode()), SEL_SEED.get((name, key), 0)])
    grid = None
    if key[0] == "M":
        _, M, how, grid = key
        chosen = matched[:M] if how == "first" else np.sort(rng.choice(matched, M, replace=False))
        data, labels, corr = _select(b, chosen)
    elif key[0] == "all":
        data, labels, corr = fr["data"], fr["labels"], b["corr"]
    elif key[0] == "mult":
        # a data point other than the first whose jittered copies keep its match, and the only match of its vertex's own that stays
        for i0 in range(1, len(corr := b["corr"])):
            v = corr[i0]
            if v < 0 or v == corr[0]:
                continue
            cp = _copies(b, i0, key[1], rng)
            if (_nn(b, cp, np.full(len(cp), fr["labels"][i0], np.int32)) == v).all():
                break
        rest = corr != v
        data = np.concatenate([fr["data"][rest], cp])
        labels = np.concatenate([fr["labels"][rest], np.full(len(cp), fr["labels"][i0], np.int32)])
        corr = np.concatenate([corr[rest], np.full(len(cp), v, np.int32)])
    elif key[0] == "one":
        data = _copies(b, 0, key[1], rng)
        labels = np.full(key[1], fr["labels"][0], np.int32)
        corr = np.full(key[1], b["corr"][0], np.int32)
    elif key[0] == "N":
        N = key[1]
        idx = np.rint(np.linspace(0, len(fr["labels"]) - 1, N)).astype(np.int64)       # spread over the frame, the first point first
        data = fr["data"][idx]
        labels = fr["labels"][idx].copy()
        corr = b["corr"][idx].copy()
        labels[N - tail_of(N):] = -1
        corr[N - tail_of(N):] = -1
    elif key[0] == "seg":
        lst = pair_lists(b["model"])[(0, 0)]
        chosen = []
        for s, want in enumerate(key[1]):
            seg = lst[s * MOM_SEG:(s + 1) * MOM_SEG]
            seg = seg[b["count"][seg] > 0]
            chosen += list(seg[:want] if s % 2 == 0 else seg[len(seg) - want:])       # from the front and from the back of a segment
        data, labels, corr = _select(b, np.array(chosen, np.int64))
    else:
        raise KeyError(key)
    data = np.ascontiguousarray(data, np.float64)
    labels = np.ascontiguousarray(labels, np.int32)
    corr = np.ascontiguousarray(corr, np.int32)
    M = len(np.unique(corr[corr >= 0]))
    c = dict(name=name, key=key, data=data, labels=labels, corr=corr, M=M, N=len(labels), nb=(M + EVAL_PTS - 1) // EVAL_PTS, grid=grid,
             frame=dict(fr, data=data, labels=labels))
    _CASE[(name, key)] = c
    return c


def options(fr, **kw):
    return fm.options(fr, **kw)


def one_step(name, key):
    """The oracle's LM step from the start state (one ICP, one GN iteration) and, at the state it returns with the case's correspondences:
    the data term (cost, g, H; no priors) with aggregate = 0 and 1, the full cost (with the priors), and the cost's cancellation factor
    kappa_c = (sum_i |d_i - centre|^2 + sum_m c_m |x_m - centre|^2) / cost - the cost is what is left of sums of that size."""
    c = case(name, key)
    if "step" in c:
        return c["step"]
    b = base(name)
    om, fr = b["om"], c["frame"]
    r = om.optimize(fr["part_map"], fr["num_parts"], fr["data"], fr["labels"], options(fr, icp_iters=1, max_iters_per_icp=1), *fr["start"], aggregate=1)
    st = (r["p"], r["q"].reshape(-1, 4), r["w"])
    ev = [om.evaluate(*st, r["corr"], fr["data"], 0.0, 0.0, aggregate=a) for a in (0, 1)]
    full = om.evaluate(*st, r["corr"], fr["data"], fr["betas"][0], fr["betas"][1], aggregate=1)[0]
    ok = r["corr"] >= 0
    x = om.points(*st)
    cnt = np.bincount(r["corr"][ok], minlength=om.V)
    big = float(((fr["data"][ok] - b["centre"]) ** 2).sum() + (cnt[:, None] * (x - b["centre"]) ** 2).sum())
    c["step"] = dict(run=r, state=st, rows=ev[0], agg=ev[1], cost_full=full, kappa_c=big / ev[1][0] if ev[1][0] > 0 else 0.0)
    return c["step"]


# ---- the short fits of tests/test_gpu_data_term_grid.py d: (model, key, G) -----------------------------------------------------------------
def short_fit_cases():
    out = []
    for name in MODELS:
        keys = case_keys(name)
        want = [("M", 17, "rand", None), ("M", 16 * 64 + 1, "rand", 64), ("N", 2049), ("mult", 1000)]
        out += [(name, k, k[3] if k[0] == "M" and k[3] else None) for k in want if k in keys]
    out.append(("j1k1", ("all",), 63))
    return out
