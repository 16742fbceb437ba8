"""Scene builders of the background subtraction tests (include/avt_bgsub.h): shared by tests/test_bgsub_cpu.py, which
checks the two restatements of tests/bgsub_restatement.py against each other on them, and tests/test_gpu_bgsub_edges.py,
which feeds them to the kernel.  A helper module of the tests, not a test file.

Every builder returns (bg, im, nn_rel, neighb_rel, prev_box); the near-threshold fields also return how their
controlled pairs sit against the threshold, so a test can check that they have teeth."""
from __future__ import annotations

import numpy as np

import bgsub_restatement as R

F = np.float32
PREV = ((1, 2), (3, 4))


def _flat(rows, cols, v, bgv=(0, 0, 0)):
    im = np.empty((rows, cols, 3), F)
    im[:] = v
    bg = np.empty((rows, cols, 3), F)
    bg[:] = bgv
    return bg, im


def _random_scene(seed, shape=None):
    """blocky XYZ maps (components of a few levels), noise, sensor holes, NaN / inf coordinates, a background that
    lies near the image on part of the frame and has holes of its own; thresholds scaled to the image size.
    shape (rows, cols) replaces the drawn size; the rest of the scene is drawn as for the drawn size's stream."""
    rng = np.random.default_rng(seed)
    rows, cols = (int(v) for v in rng.integers(8, 41, 2))
    if shape is not None:
        rows, cols = shape
    k = int(rng.integers(2, 12))
    levels = rng.choice([1.0, 1.2, 2.0, 3.0], size=((rows + k - 1) // k + 1, (cols + k - 1) // k + 1, 3)).astype(F)
    im = np.repeat(np.repeat(levels, k, 0), k, 1)[:rows, :cols].copy()
    im += rng.normal(0, rng.choice([0, 0.01, 0.05]), im.shape).astype(F)
    bg = np.full_like(im, 10.0)
    near = rng.random((rows, cols)) < rng.choice([0, 0.1, 0.4])
    bg[near] = im[near] + rng.normal(0, 0.05, (int(near.sum()), 3)).astype(F)
    bg[rng.random((rows, cols)) < 0.1, 2] = 0
    im[rng.random((rows, cols)) < rng.choice([0, 0.03, 0.15]), 2] = 0
    sp = rng.random((rows, cols))
    im[sp < 0.01] = np.nan
    im[(sp > 0.01) & (sp < 0.015), 0] = np.inf
    im[(sp > 0.015) & (sp < 0.02), 2] = -np.inf
    n = rows * cols
    nn, nb = rng.choice([0.001, 0.01, 0.1]), rng.choice([0.001, 0.05, 0.5, 2.0])
    return bg, im, nn * n / 1.2e6, nb * n / 1.2e6


def grid_scene(first_small=True, speck=True):
    """176 x 176: 16 x 16 blocks of 10 x 10 pixels between zero-depth lines, each block its own component (> 254 of
    them); block 0 cut to 5 x 5 (too small), a one-pixel speck in the last gap column, past the cap"""
    im = np.zeros((176, 176, 3), F)
    for bi in range(16):
        for bj in range(16):
            im[11 * bi:11 * bi + 10, 11 * bj:11 * bj + 10] = (0.1 * bj, 0.1 * bi, 1.0 + 0.5 * ((bi + bj) % 2))
    if first_small:
        im[0:10, 5:10, 2] = 0
        im[5:10, 0:5, 2] = 0
    if speck:
        im[170, 175] = (5, 5, 5)
    return np.full_like(im, 0.0), im


# ---- the known-answer scenes of test_bgsub_cpu.py

def tie_scene():
    """12 x 12 at (0.002, 0.001): squared distance 16.666666f against the threshold 16.666668f, at a corner, the right
    border and inside"""
    bg, im = _flat(12, 12, (0, 0, 5.082483))
    bg[0, 0] = (0, 0, 1)                          # (5.082483 - 1)^2 = 16.666666f exactly
    bg[11, 11] = (0, 0, 1)                        # a corner: the window is clipped, not wrapped
    bg[5, 11] = (0, 0, 1)                         # the right border
    return bg, im, 0.002, 0.001, PREV


def zero_bg_scene(bgz):
    """the whole background at depth bgz, the image next to it: 0 and -0.0 are skipped, 1e-30 is a neighbour"""
    bg, im = _flat(12, 12, (3, 0, 0.001), (3, 0, bgz))
    return bg, im, 0.002, 0.001, PREV


def hole_scene():
    bg, im = _flat(12, 12, (3, 0, 0.001))
    im[4, 7, 2] = 0                               # a sensor hole is 255 and splits nothing here
    return bg, im, 0.002, 0.001, PREV


def nan_inf_scene(kind=None):
    """two halves of 72 pixels, 64 apart; kind "nan" or "inf" puts that coordinate on the pixel left of the seam"""
    bg, im = _flat(12, 12, (0, 0, 1))
    im[:, 6:] = (0, 0, 9)
    if kind == "nan":
        im[0, 5] = (np.nan, 0, 1)
    elif kind == "inf":
        im[0, 5] = (np.inf, 0, 1)
    return bg, im, 0.002, 0.001, PREV


def min_pts_scene(missing=False):
    """exactly min_pts = 100 pixels, or 99 when missing"""
    bg, im = _flat(12, 12, (0, 0, 0))
    im[1:11, 1:11] = (0, 0, 1)
    if missing:
        im[5, 5, 2] = 0
    return bg, im, 0.005, 0.005, PREV


def tiny_scene(v):
    """3 x 4: never min_pts pixels"""
    bg, im = _flat(3, 4, v)
    return bg, im, 0.005, 0.005, PREV


def cap_scene(exact=False):
    """grid_scene past the cap; exact: exactly 254 kept components, nothing left unvisited but the speck"""
    if not exact:
        bg, im = grid_scene()
    else:
        bg, im = grid_scene(first_small=False, speck=True)
        im[165:175, 154:175, 2] = 0
    return bg, im, 0.005, 0.005, PREV


def ids_scene(equal=False):
    """135 pixels from (1, 0) and the rest, which reaches row 0 (id 0); equal: 200 / 200"""
    bg, im = _flat(20, 20, (0, 0, 9))
    im[1:10, 0:15] = (0, 0, 1)
    if equal:
        im[0:10] = (0, 0, 1)
    return bg, im, 0.005, 0.001, PREV


def denormal_scene():
    """image depth 1e-40 (an f32 denormal, nonzero): every pixel a candidate, one component; a background of the same
    point with depth 1e-40 (nonzero, so not skipped) in the middle: the pixels around it are near the background"""
    bg, im = _flat(12, 12, (0, 0, 1e-40))
    bg[5:7, 5:7] = (0, 0, 1e-40)
    return bg, im, 0.005, 0.005, PREV


def known_answer_scenes():
    """(name, builder output) of every known-answer scene"""
    out = [("tie", tie_scene())]
    out += [(f"zero_bg_{z!r}", zero_bg_scene(z)) for z in (0.0, -0.0, 1e-30)]
    out += [("hole", hole_scene())]
    out += [(f"nan_inf_{k}", nan_inf_scene(k)) for k in (None, "nan", "inf")]
    out += [("min_pts", min_pts_scene(False)), ("min_pts_minus_1", min_pts_scene(True))]
    out += [(f"tiny_{i}", tiny_scene(v)) for i, v in enumerate(((0, 0, 0), (0, 0, 1)))]
    out += [("cap", cap_scene(False)), ("cap_exact", cap_scene(True))]
    out += [("ids", ids_scene(False)), ("ids_equal", ids_scene(True)), ("denormal", denormal_scene())]
    return out


# ---- scenes at size

def blocky_scene(rows, cols, seed, k=None):
    """avatar-free: blocks of k x k pixels at one of three levels (equal neighbouring levels merge; k grows with the
    size so that components reach min_pts), noise well below the join threshold, sensor holes, a few NaN / inf
    coordinates, a background near the image on a hundredth of the frame (each such point takes its 3 x 3 window
    out) and with holes of its own.  Thresholds are
    absolute (nn 0.01, neighb 0.05), whatever the size."""
    rng = np.random.default_rng(seed)
    if k is None:
        k = int(rng.integers(3, 13)) * max(1, int(round(np.sqrt(R.min_points(rows, cols)) / 10)))
    lv = rng.choice([1.0, 1.5, 2.5], size=((rows + k - 1) // k + 1, (cols + k - 1) // k + 1))
    levels = np.stack([0.1 * lv, -0.1 * lv, lv], -1).astype(F)
    im = np.repeat(np.repeat(levels, k, 0), k, 1)[:rows, :cols].copy()
    im += rng.uniform(-0.01, 0.01, im.shape).astype(F)
    bg = np.full_like(im, 10.0)
    near = rng.random((rows, cols)) < 0.01
    bg[near] = im[near] + rng.normal(0, 0.02, (int(near.sum()), 3)).astype(F)
    bg[rng.random((rows, cols)) < 0.05, 2] = 0
    im[rng.random((rows, cols)) < 0.03, 2] = 0
    sp = rng.random((rows, cols))
    im[sp < 0.001] = np.nan
    im[(sp > 0.001) & (sp < 0.002), 0] = np.inf
    n = rows * cols
    return bg, im, 0.01 * n / 1.2e6, 0.05 * n / 1.2e6, PREV


def _on(rows, cols):
    """zero background, zero-depth image: shapes are drawn on it with _draw"""
    return np.zeros((rows, cols, 3), F), np.zeros((rows, cols, 3), F)


def _draw(im, pix, v):
    rr, cc = np.asarray(pix).T
    im[rr, cc] = v


def serpentine_scene(rows=100, cols=130):
    """one 1-pixel path through every tile row: along row 2i, down at the right or left end"""
    bg, im = _on(rows, cols)
    pix = []
    for i, r in enumerate(range(0, rows, 2)):
        pix += [(r, c) for c in range(cols)]
        if r + 1 < rows:
            pix.append((r + 1, cols - 1 if i % 2 == 0 else 0))
    _draw(im, pix, (0.5, 0.5, 2.0))
    return bg, im, 0.005, 0.005, PREV


def spiral_scene(rows=100, cols=130):
    """an inward rectangular spiral of 1-pixel wall with 1-pixel gaps between its turns: one component"""
    bg, im = _on(rows, cols)
    on = np.zeros((rows, cols), bool)
    inside = lambda r, c: 0 <= r < rows and 0 <= c < cols
    r, c, d = 0, 0, 0
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    on[0, 0] = True
    while True:
        for turn in (0, 1):                       # straight on, else turn right; stop when neither is free
            dr, dc = dirs[(d + turn) % 4]
            nr, nc = r + dr, c + dc
            if inside(nr, nc) and not on[nr, nc] and not (inside(nr + dr, nc + dc) and on[nr + dr, nc + dc]):
                d, r, c = (d + turn) % 4, nr, nc
                on[r, c] = True
                break
        else:
            break
    im[on] = (0.2, 0.3, 2.0)
    return bg, im, 0.005, 0.005, PREV


def comb_scene(rows=100, cols=130):
    """vertical teeth on every other column from row 0, joined only by a bar on the last row (the last tile row)"""
    bg, im = _on(rows, cols)
    im[:, 0::2] = (0.1, 0.1, 1.5)
    im[rows - 1, :] = (0.1, 0.1, 1.5)
    return bg, im, 0.005, 0.005, PREV


def u_scene(rows=100, cols=130):
    """two interleaved U shapes: the first pixel of each is the top of its right arm, in a tile right of most of it;
    the inner U reaches row 0, so its id is 0 though the outer U starts left of it and below"""
    bg, im = _on(rows, cols)
    b0, b1 = rows - 10, rows - 5                  # the bottoms: inner, outer
    c0, c1 = cols - 10, cols - 5                  # the right arms: inner, outer
    inner = np.zeros((rows, cols), bool)          # left arm at col 10 from row 20, bottom on row b0, right arm c0 from row 0
    inner[20:b0 + 1, 10] = True
    inner[b0, 10:c0 + 1] = True
    inner[0:b0 + 1, c0] = True
    outer = np.zeros((rows, cols), bool)          # left arm col 5 from row 30, bottom row b1, right arm c1 from row 2
    outer[30:b1 + 1, 5] = True
    outer[b1, 5:c1 + 1] = True
    outer[2:b1 + 1, c1] = True
    im[inner] = (0.0, 0.0, 2.0)
    im[outer] = (0.0, 0.0, 2.0)
    return bg, im, 0.005, 0.005, PREV


def checker_scene(rows=100, cols=130, block=11):
    """a checkerboard of block x block squares (one pixel when block == 1): squares meet only at corners, which do not
    join"""
    bg, im = _on(rows, cols)
    r, c = np.meshgrid(np.arange(rows) // block, np.arange(cols) // block, indexing="ij")
    on = (r + c) % 2 == 0
    im[on] = (0.3, 0.3, 2.0)
    return bg, im, 0.005, 0.005, PREV


def staircase_scene(rows=100, cols=130):
    """4-connected 1-pixel staircases (r, r + s), (r, r + s + 1) every 3 columns, each touching the next only at
    corners, and a pure diagonal (corner contacts only) in the lower left"""
    bg, im = _on(rows, cols)
    on = np.zeros((rows, cols), bool)
    r = np.arange(rows)
    for s in range(0, cols, 3):
        for dc in (0, 1):
            c = r + s + dc
            ok = c < cols
            on[r[ok], c[ok]] = True
    for s in range(4, rows, 6):                   # diagonals below the main staircase: (s + i, i)
        i = np.arange(rows - s)
        on[s + i, i] = True
    im[on] = (0.4, 0.1, 2.0)
    return bg, im, 0.005, 0.005, PREV


def full_frame_scene(rows=720, cols=1280, seed=0):
    """one component over the whole frame: noise far below the join threshold, a zero background"""
    rng = np.random.default_rng(seed)
    im = np.empty((rows, cols, 3), F)
    im[:] = (0.25, -0.5, 2.0)
    im += rng.uniform(-0.004, 0.004, im.shape).astype(F)
    return np.zeros_like(im), im, 0.005, 0.005, PREV


def hard_shape_scenes(rows=100, cols=130):
    return [("serpentine", serpentine_scene(rows, cols)), ("spiral", spiral_scene(rows, cols)), ("comb", comb_scene(rows, cols)),
            ("u", u_scene(rows, cols)), ("checker_1", checker_scene(rows, cols, 1)), ("checker_11", checker_scene(rows, cols, 11)),
            ("staircase", staircase_scene(rows, cols))]


# ---- near-threshold fields: squared distances within +-2 ulp of the threshold, in float32, in the reference order

def _sq3(d0, d1, d2):
    d0, d1, d2 = F(d0), F(d1), F(d2)
    return (d0 * d0 + d1 * d1) + d2 * d2


def _ulp_off(sq, t):
    return sq.view(np.int32).astype(np.int64) - np.asarray(t, F).view(np.int32).astype(np.int64)


def near_background_field(rows, cols, seed=0, rel=0.005):
    """a constant background (0, 0, 0.5); 60% of the pixels at squared distance t + k ulp from it (t the near threshold,
    k drawn from -2..2: k < 0 near the background, k >= 0 a candidate), the rest clearly candidates.  Every candidate
    lies within sqrt(t) / 2 in z and 0.1 sqrt(t) in x, y of the others, so they join (neighb threshold = t).
    Returns the scene and the offset k of every placed pixel (99 for the clear candidates)."""
    rng = np.random.default_rng(seed)
    t, _ = R.thresholds(rows, cols, rel, rel)
    s = float(np.sqrt(t))
    m = 400000
    x = (rng.uniform(-0.1, 0.1, m) * s).astype(F)
    y = (rng.uniform(-0.1, 0.1, m) * s).astype(F)
    z0 = F(0.5) - (np.sqrt(np.maximum(float(t) - x.astype(np.float64) ** 2 - y.astype(np.float64) ** 2, 0.0))).astype(F)
    pool = {k: [] for k in range(-2, 3)}
    for step in range(-12, 13):
        z = (z0.view(np.int32) + step).view(F)
        off = _ulp_off(_sq3(F(0) - x, F(0) - y, F(0.5) - z), t)
        for k in range(-2, 3):
            sel = off == k
            pool[k].append(np.stack([x[sel], y[sel], z[sel]], -1))
    pool = {k: np.concatenate(v) for k, v in pool.items()}
    n = rows * cols
    ks = np.where(rng.random(n) < 0.6, rng.integers(-2, 3, n), 99)
    im = np.empty((n, 3), F)
    for k in range(-2, 3):
        sel = np.nonzero(ks == k)[0]
        im[sel] = pool[k][rng.integers(0, len(pool[k]), len(sel))]
    sel = ks == 99
    im[sel, 0] = (rng.uniform(-0.1, 0.1, int(sel.sum())) * s).astype(F)
    im[sel, 1] = (rng.uniform(-0.1, 0.1, int(sel.sum())) * s).astype(F)
    im[sel, 2] = F(0.5) - F(1.5 * s)
    bg = np.empty((rows, cols, 3), F)
    bg[:] = (0, 0, 0.5)
    return (bg, im.reshape(rows, cols, 3), rel, rel, PREV), ks.reshape(rows, cols)


def _pick_step(a, t, rng, k, two_d):
    """a next value b after a (x, z when two_d, else one coordinate) with squared distance t + k ulp, or the nearest
    offset reachable; moving back toward the start keeps the chain's ulps fine.  Returns (b, offset)."""
    s = float(np.sqrt(t))
    m = 4000
    if two_d:
        sx = -1.0 if a[0] > 0.3 else 1.0
        sz = -1.0 if a[1] > 0.7 else 1.0
        u = rng.uniform(0.3, 0.7, m)
        bx = (a[0] + sx * u * s).astype(F)
        dx = F(a[0]) - bx
        bz0 = (a[1] + sz * np.sqrt(np.maximum(float(t) - dx.astype(np.float64) ** 2, 0.0))).astype(F)
        best = None
        for step in range(-12, 13):
            bz = (bz0.view(np.int32) + step).view(F)
            off = _ulp_off(_sq3(dx, F(0), F(a[1]) - bz), t)
            hit = np.nonzero(off == k)[0]
            if len(hit):
                return (bx[hit[0]], bz[hit[0]]), k
            j = int(np.argmin(np.abs(off - k)))
            if best is None or abs(off[j] - k) < abs(best[1] - k):
                best = ((bx[j], bz[j]), int(off[j]))
        return best
    sy = -1.0 if a > 0.0 else 1.0
    b0 = F(a + sy * s)
    cand = (np.array([b0], F).view(np.int32) + np.arange(-40, 41)).view(F)
    off = _ulp_off(_sq3(F(0), F(a) - cand, F(0)), t)
    ok = np.nonzero(np.abs(off) <= 2)[0]
    prefer = ok[(off[ok] <= 0) == (k <= 0)]
    j = int(rng.choice(prefer if len(prefer) else ok))
    return cand[j], int(off[j])


def near_neighbour_field(rows, cols, seed=0, rel=0.005):
    """a zero background (every pixel a candidate); the image (X[c], Y[r], Z[c]) in bands of 16..44 columns and rows
    with constant values inside a band.  Across a column band boundary the squared distance (dX, 0, dZ) is placed at
    t + k ulp (t the join threshold, k cycling through 0, 1, -1, 2, -2; k <= 0 joins), across a row boundary (0, dY, 0) at the reachable
    offset within 2 ulp on the drawn side.  Components are the rectangles between the boundaries that do not join.
    Returns the scene and the offsets of the column and of the row boundaries."""
    rng = np.random.default_rng(seed)
    _, t = R.thresholds(rows, cols, rel, rel)

    def bands(n):
        cuts, c = [], int(rng.integers(16, 45))
        while c < n:
            cuts.append(c)
            c += int(rng.integers(16, 45))
        return cuts

    ccuts, rcuts = bands(cols), bands(rows)
    X, Z, Y = np.empty(cols, F), np.empty(cols, F), np.empty(rows, F)
    cur, coff, edges = (F(0.3), F(0.7)), [], [0] + ccuts + [cols]
    for i in range(len(edges) - 1):
        if i:
            cur, o = _pick_step(cur, t, rng, (0, 1, -1, 2, -2)[(i - 1) % 5], True)
            coff.append(o)
        X[edges[i]:edges[i + 1]], Z[edges[i]:edges[i + 1]] = cur
    cur, roff, edges = F(0.0), [], [0] + rcuts + [rows]
    for i in range(len(edges) - 1):
        if i:
            cur, o = _pick_step(float(cur), t, rng, (0, 1, -1, 2, -2)[(i - 1) % 5], False)
            roff.append(o)
        Y[edges[i]:edges[i + 1]] = cur
    im = np.empty((rows, cols, 3), F)
    im[:, :, 0] = X[None, :]
    im[:, :, 1] = Y[:, None]
    im[:, :, 2] = Z[None, :]
    return (np.zeros_like(im), im, rel, rel, PREV), (np.array(coff), np.array(roff), ccuts, rcuts)


# ---- cap and list boundaries across tiles

def cap_blocks_scene(n_kept, small_before=True, small_after=True):
    """130 x 260 (min_pts 100): abutting 10 x 10 blocks, each its own component by a value jump.  Block rows 0-9 hold
    253 kept blocks (7 of the 260 cut to 90 pixels by a zero-depth column when small_before, else lost to zero depth),
    so the 253rd kept root starts on row 90 (tile row 2); block row 10 (from row 100, tile row 3) holds the kept
    blocks past 253, n_kept - 253 of them, first; a small block follows them when small_after"""
    rows, cols = 130, 260
    bg = np.zeros((rows, cols, 3), F)
    im = np.zeros((rows, cols, 3), F)

    def block(bi, bj):
        im[10 * bi:10 * bi + 10, 10 * bj:10 * bj + 10] = (0.1 * (bj % 3), 0.1 * (bi % 3), 1.0 + 0.5 * ((bi + 2 * bj) % 5))

    for bi in range(10):
        for bj in range(26):
            block(bi, bj)
    for j in range(7):                            # 7 blocks of block row 1 are not kept
        bj = 3 * j + 1
        if small_before:
            im[10:20, 10 * bj + 9, 2] = 0         # 90 pixels: small, before the cap
        else:
            im[10:20, 10 * bj:10 * bj + 10, 2] = 0
    extra = n_kept - 253
    for bj in range(extra):
        block(10, bj)
    if small_after:
        block(10, extra + 1)
        im[100:110, 10 * (extra + 1) + 9, 2] = 0  # 90 pixels after the last kept block
    return bg, im, 0.005, 0.0005, PREV


def columns_scene(cols=1009, rows=100):
    """rows x cols of one-column components of exactly rows pixels each (min_pts 100 at 100 x 1009): every kept root
    on row 0, cols of them in the kept list"""
    im = np.empty((rows, cols, 3), F)
    c = np.arange(cols)
    im[:, :, 0] = (0.5 * (c % 2)).astype(F)[None, :]
    im[:, :, 1] = (0.01 * (c % 7)).astype(F)[None, :]
    im[:, :, 2] = (1.0 + 0.25 * (c % 3)).astype(F)[None, :]
    return np.zeros_like(im), im, 0.005, 0.0005, PREV
