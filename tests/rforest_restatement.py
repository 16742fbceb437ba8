"""Plain-numpy restatement of a forest of several trees (include/avt_rforest.h), TEST INFRASTRUCTURE.

Per pixel: the walk of every tree with the reference's float32 sequence (scoreByFeature / getDepth, RTree.cpp:39-68: offset /
depth per component, round half away from zero, int32 cast, a probe outside the bound or on zero depth reads 20 m, zu - zv <
thresh goes left), then sum[p] = ((d_0[p] + d_1[p]) + d_2[p]) + ... in np.float32 in tree order, then the arg-max of
rtree-run-dataset.cpp:143-158: the first p with sum[p] > best, best starting at 0; 255 when none.  Two walking rules:

  predict(trees, depth)            RTree::predict (RTree.cpp:3156-3182): every pixel with depth > 0, probes bounded by the image
  predict_best(trees, depth, ...)  RTree::predictBest (:3184-3262): the interval grid inside the box, first row skipped,
                                   depth == 0 skipped, probes bounded by the box, upscaleGrid's fill clamped to the row

The pixels are walked together, one tree level per trip; every pixel's arithmetic is its own.  A tree is (feature (n, 5)
float32 [u.x u.y v.x v.y thresh], links (n, 3) int32 [lnode rnode leafid], leaf_data (nl, num_parts) float32)."""
import numpy as np

BACKGROUND_DEPTH = np.float32(20.0)


def _round_to_int(q):
    """(int32)std::round(q) for float32 q, as int64; a quotient that leaves int32 (or is not finite) lands far outside any image."""
    x = q.astype(np.float64)
    with np.errstate(invalid="ignore"):
        r = np.trunc(x + np.copysign(0.5, x))           # exact in float64: half away from zero
    bad = ~np.isfinite(r) | (np.abs(r) >= 2.0 ** 31)
    return np.where(bad, -(2 ** 40), r).astype(np.int64)


def _probe(depth, x, y, lox, loy, hix, hiy):
    inside = (x >= lox) & (y >= loy) & (x <= hix) & (y <= hiy)
    z = np.full(x.shape, BACKGROUND_DEPTH, np.float32)
    z[inside] = depth[y[inside], x[inside]]
    z[z == 0.0] = BACKGROUND_DEPTH
    return z


def walk(tree, depth, rr, cc, lox, loy, hix, hiy):
    """Leaf ids reached by the pixels (rr[i], cc[i]) of `depth` in one tree, probes bounded by [lox, hix] x [loy, hiy]."""
    feature, links, _ = tree
    feature = np.asarray(feature, np.float32); links = np.asarray(links, np.int64)
    depth = np.asarray(depth, np.float32)
    node = np.zeros(len(rr), np.int64)
    sample = depth[rr, cc]
    while True:
        act = np.nonzero(links[node, 2] < 0)[0]
        if len(act) == 0:
            return links[node, 2]
        f = feature[node[act]]
        s = sample[act]
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            ux = _round_to_int(f[:, 0] / s) + cc[act]; uy = _round_to_int(f[:, 1] / s) + rr[act]
            vx = _round_to_int(f[:, 2] / s) + cc[act]; vy = _round_to_int(f[:, 3] / s) + rr[act]
            score = _probe(depth, ux, uy, lox, loy, hix, hiy) - _probe(depth, vx, vy, lox, loy, hix, hiy)      # float32
        node[act] = np.where(score < f[:, 4], links[node[act], 0], links[node[act], 1])


def sums(trees, leaves):
    """(n_pixels, num_parts) float32: tree 0's distribution, then + tree 1's, + tree 2's, ... (leaves[t][i]: pixel i's leaf in tree t)."""
    s = np.asarray(trees[0][2], np.float32)[leaves[0]].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(1, len(trees)):
            s = (s + np.asarray(trees[t][2], np.float32)[leaves[t]]).astype(np.float32)
    return s


def argmax(s):
    """The first p with s[p] > best, best starting at 0 and following the winner; 255 when none.  NaN never wins."""
    lab = np.full(len(s), 255, np.uint8)
    best = np.zeros(len(s), np.float32)
    with np.errstate(invalid="ignore"):
        for p in range(s.shape[1]):
            win = s[:, p] > best
            best[win] = s[win, p]
            lab[win] = p
    return lab


def predict(trees, depth):
    depth = np.ascontiguousarray(depth, np.float32)
    rows, cols = depth.shape
    num_parts = np.asarray(trees[0][2]).shape[1]
    out = np.zeros((num_parts, rows, cols), np.float32)
    rr, cc = np.nonzero(depth > 0)
    if len(rr):
        leaves = [walk(t, depth, rr, cc, 0, 0, cols - 1, rows - 1) for t in trees]
        out[:, rr, cc] = sums(trees, leaves).T
    return out


def predict_best(trees, depth, interval=1, top_left=(0, 0), bot_right=(-1, -1), fill_in_gaps=True):
    depth = np.ascontiguousarray(depth, np.float32)
    rows, cols = depth.shape
    (tlx, tly), (brx, bry) = top_left, bot_right
    if brx == -1:
        brx, bry = cols - 1, rows - 1
    out = np.full((rows, cols), 255, np.uint8)
    gr, gc = np.meshgrid(np.arange(tly + interval, bry + 1, interval), np.arange(tlx, brx + 1, interval), indexing="ij")
    gr, gc = gr.ravel(), gc.ravel()
    keep = depth[gr, gc] != 0 if len(gr) else np.zeros(0, bool)
    rr, cc = gr[keep], gc[keep]
    if len(rr):
        leaves = [walk(t, depth, rr, cc, tlx, tly, brx, bry) for t in trees]
        out[rr, cc] = argmax(sums(trees, leaves))
    if fill_in_gaps and interval > 1:                    # upscaleGrid (RTree.cpp:70-99), width clamped to the row
        for r0 in range(tly + interval, bry + 1, interval):
            for r in range(r0, min(r0 + interval, bry + 1)):
                for c in range(tlx, brx + 1, interval):
                    out[r, c:min(c + interval, cols)] = out[r0, c]
    return out


def predict_best_box_on_device(trees, depth, box, interval, fill_in_gaps=True):
    """The box-per-image forms: a box that does not lie inside the image labels nothing."""
    rows, cols = depth.shape
    tlx, tly, brx, bry = (int(v) for v in box)
    if not (0 <= tlx <= brx < cols and 0 <= tly <= bry < rows):
        return np.full((rows, cols), 255, np.uint8)
    return predict_best(trees, depth, interval, (tlx, tly), (brx, bry), fill_in_gaps)
