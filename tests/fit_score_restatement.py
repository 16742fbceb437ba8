"""Plain-numpy restatement of the fit score (include/avt_fitscore.h, THE RULE), TEST INFRASTRUCTURE.

tables(R, M, D, boxes, tol, stride, P) is the (n, P + 1, 7) int64 stack of per-image tables, columns AGREE, IN_FRONT, BEHIND,
MODEL_ONLY, DATA_ONLY, ABS_UM, ABS_UM_AGREE, of every pixel (r, c) with r % stride == 0 and c % stride == 0:

  m      R > 0 (NaN is not)
  d      inside the box and D > 0 (zero, negative, NaN are not data, +inf is); a box with br.x == -1 is the whole image, an empty
         box or one that does not lie inside the image selects nothing
  row    M where m and M < P, else P
  bad    a selected pixel with P <= M < 255 raises ValueError naming num_parts, whatever R is
  delta  float64(R) - float64(D); tol is the float32 argument promoted to float64; AGREE if |delta| <= tol, else IN_FRONT if
         delta < -tol, else BEHIND (a NaN delta, +inf against +inf, lands there)
  um     int64(rint(fmin(|delta|, 1000.0) * 1e6)), added to ABS_UM and, for AGREE pixels, to ABS_UM_AGREE

float64 subtraction, np.rint (to nearest even), int64 sums by np.add.at."""
import numpy as np

AGREE, IN_FRONT, BEHIND, MODEL_ONLY, DATA_ONLY, ABS_UM, ABS_UM_AGREE = range(7)


def box_mask(box, rows, cols):
    """(rows, cols) bool: the pixels the inclusive box tl.x tl.y br.x br.y holds, by the header's rule"""
    inside = np.zeros((rows, cols), bool)
    tlx, tly, brx, bry = (int(v) for v in box)
    if brx == -1:
        tlx, tly, brx, bry = 0, 0, cols - 1, rows - 1
    if 0 <= tlx <= brx < cols and 0 <= tly <= bry < rows:
        inside[tly:bry + 1, tlx:brx + 1] = True
    return inside


def table(R, M, D, box=None, tol=0.05, stride=1, P=24):
    """one image's (P + 1, 7) int64 table"""
    R, M, D = np.asarray(R, np.float32), np.asarray(M, np.uint8), np.asarray(D, np.float32)
    rows, cols = R.shape
    assert M.shape == R.shape and D.shape == R.shape and stride >= 1 and 1 <= P <= 254
    tol = np.float64(np.float32(tol))
    assert tol >= 0
    inside = box_mask((0, 0, -1, -1) if box is None else box, rows, cols)
    sel = (slice(None, None, stride), slice(None, None, stride))
    R, M, D, inside = R[sel].ravel(), M[sel].ravel().astype(np.int64), D[sel].ravel(), inside[sel].ravel()
    if ((M >= P) & (M != 255)).any():
        raise ValueError("a part-mask label at a selected pixel is >= num_parts (%d) and not 255" % P)
    with np.errstate(invalid="ignore"):
        m = R > 0
        d = inside & (D > 0)
        delta = R.astype(np.float64) - D.astype(np.float64)
        a = np.abs(delta)
        um = np.rint(np.fmin(a, 1000.0) * 1e6)
        cls = np.where(a <= tol, AGREE, np.where(delta < -tol, IN_FRONT, BEHIND))
    cls = np.where(m & d, cls, np.where(m, MODEL_ONLY, DATA_ONLY))
    row = np.where(m & (M < P), M, P)
    keep, both = m | d, m & d
    out = np.zeros((P + 1, 7), np.int64)
    np.add.at(out, (row[keep], cls[keep]), 1)
    um = np.where(both, um, 0).astype(np.int64)
    np.add.at(out, (row[both], ABS_UM), um[both])
    agree = both & (cls == AGREE)
    np.add.at(out, (row[agree], ABS_UM_AGREE), um[agree])
    return out


def tables(R, M, D, boxes=None, tol=0.05, stride=1, P=24):
    """(n, P + 1, 7) int64 of stacks (n, rows, cols); boxes (n, 4) or None"""
    R, M, D = np.asarray(R, np.float32), np.asarray(M, np.uint8), np.asarray(D, np.float32)
    if R.ndim == 2:
        R, M, D = R[None], M[None], D[None]
    return np.stack([table(R[i], M[i], D[i], None if boxes is None else np.asarray(boxes).reshape(-1, 4)[i], tol, stride, P) for i in range(len(R))])
