"""Plain-numpy restatement of the forest's score (include/avt_rforest.h, THE SCORE), TEST INFRASTRUCTURE, on top of
tests/rforest_restatement.py.

Let P = num_parts.  confusion(trees, depth, mask, stride) is the (P + 1, P + 1) int64 matrix conf[truth][predicted], index P
meaning "none" (255), of every pixel (r, c) with r % stride == 0 and c % stride == 0 of every image:

  predicted  the distribution form's rule: the pixels with depth > 0 are walked in every tree (`walk`, probes bounded by the
             whole image, whatever the stride), summed in tree order (`sums`) and the first part whose sum exceeds a best that
             starts at 0 wins (`argmax`); a pixel that is not walked, or that no part wins, is P
  truth      the mask byte, 255 -> P; a byte >= P that is not 255 is refused (ValueError, nothing is returned)
  counting   np.add.at on the (truth, predicted) pairs, the both-none pairs removed: conf[P][P] is always 0"""
import numpy as np

import rforest_restatement as rr


def predicted(trees, depth):
    """(rows, cols) uint8 arg-max of one image, 255 where nothing is predicted: RTree::predict's walk, not predictBest's"""
    depth = np.ascontiguousarray(depth, np.float32)
    rows, cols = depth.shape
    out = np.full((rows, cols), 255, np.uint8)
    with np.errstate(invalid="ignore"):
        r, c = np.nonzero(depth > 0)                     # zero, negative and NaN depths are not walked
    if len(r):
        leaves = [rr.walk(t, depth, r, c, 0, 0, cols - 1, rows - 1) for t in trees]
        out[r, c] = rr.argmax(rr.sums(trees, leaves))
    return out


def predicted_batch(trees, depth):
    """`predicted` of every image of (n, rows, cols): the part of the score that does not depend on the mask or the stride"""
    return np.stack([predicted(trees, d) for d in np.asarray(depth, np.float32)])


def confusion(trees, depth, mask, stride=1, pred=None):
    """depth (n, rows, cols) or (rows, cols) float32, mask the same shape uint8 -> ((P + 1, P + 1) int64, pixels selected).
    `pred`: predicted_batch(trees, depth), when the caller scores the same images more than once."""
    depth = np.asarray(depth, np.float32)
    mask = np.asarray(mask, np.uint8)
    if depth.ndim == 2:
        depth, mask = depth[None], mask[None]
        pred = None if pred is None else np.asarray(pred).reshape(depth.shape)
    assert depth.shape == mask.shape and stride >= 1
    P = np.asarray(trees[0][2]).shape[1]
    if pred is None:
        pred = predicted_batch(trees, depth)
    if ((mask >= P) & (mask != 255)).any():
        raise ValueError("a part-mask label is >= num_parts (%d) and not 255" % P)
    conf = np.zeros((P + 1, P + 1), np.int64)
    n_pixels = 0
    for m, pr in zip(mask, pred):
        q = pr[::stride, ::stride].astype(np.int64).ravel()
        t = m[::stride, ::stride].astype(np.int64).ravel()
        n_pixels += len(t)
        q[q == 255] = P
        t[t == 255] = P
        keep = (t != P) | (q != P)
        np.add.at(conf, (t[keep], q[keep]), 1)
    return conf, n_pixels
