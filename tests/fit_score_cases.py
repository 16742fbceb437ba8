"""The cases the fit-score tests share (TEST INFRASTRUCTURE): a 3 x 4 image that holds every class with its tables worked out by
hand, and the generator of the random batches the GPU tests score."""
import numpy as np

nan, inf = np.nan, np.inf
F = np.float32

# ---- by hand: P = 2, tol = 0.1 (float32 0.1 is a little above 0.1), box rows 0-1 of the image (tl.x tl.y br.x br.y)
HAND_P, HAND_TOL, HAND_BOX = 2, 0.1, (0, 0, 3, 1)
HAND_R = np.array([[1.5, 1.5, 1.5, 1.5],
                   [2.0, 0.0, 0.0, 1.0],
                   [1.0, 0.0, nan, 3.0]], F)
HAND_M = np.array([[0, 1, 255, 0],
                   [1, 0, 255, 1],
                   [0, 255, 1, 255]], np.uint8)
HAND_D = np.array([[1.5625, 1.75, 1.0, 0.0],
                   [inf, 2.0, 0.0, -1.0],
                   [1.0, 5.0, 2.0, nan]], F)
# (0,0) delta -0.0625: AGREE, part 0, 62500 um            (0,1) delta -0.25: IN_FRONT, part 1, 250000 um
# (0,2) delta +0.5, mask 255: BEHIND, row P, 500000 um    (0,3) D = 0: MODEL_ONLY, part 0
# (1,0) D = +inf: IN_FRONT, part 1, clamped 1e9 um        (1,1) R = 0 under a label, D = 2: DATA_ONLY, row P
# (1,2) neither: nothing                                  (1,3) D = -1 is no data: MODEL_ONLY, part 1
# (2,0) outside the box, D ignored: MODEL_ONLY, part 0    (2,1) outside the box, no model: nothing
# (2,2) R = NaN is no model, outside the box: nothing     (2,3) mask 255, D = NaN: MODEL_ONLY, row P
#                        AGREE IN_FRONT BEHIND MODEL_ONLY DATA_ONLY ABS_UM ABS_UM_AGREE
HAND_TABLE = np.array([[1, 0, 0, 2, 0, 62500, 62500],
                       [0, 2, 0, 1, 0, 1000250000, 0],
                       [0, 0, 1, 1, 1, 500000, 0]], np.int64)
# stride 2 selects (0,0), (0,2), (2,0), (2,2)
HAND_TABLE_STRIDE2 = np.array([[1, 0, 0, 1, 0, 62500, 62500],
                               [0, 0, 0, 0, 0, 0, 0],
                               [0, 0, 1, 0, 0, 500000, 0]], np.int64)
# tol = 0.25 is exactly |delta| of (0,1): it agrees (<=); (1,0) stays IN_FRONT
HAND_TABLE_TOL_QUARTER = np.array([[1, 0, 0, 2, 0, 62500, 62500],
                                   [1, 1, 0, 1, 0, 1000250000, 250000],
                                   [0, 0, 1, 1, 1, 500000, 0]], np.int64)
# tol = 0: (0,0) is IN_FRONT too
HAND_TABLE_TOL_ZERO = np.array([[0, 1, 0, 2, 0, 62500, 0],
                                [0, 2, 0, 1, 0, 1000250000, 0],
                                [0, 0, 1, 1, 1, 500000, 0]], np.int64)
# tol = +inf: every pixel with both agrees, the clamped one included
HAND_TABLE_TOL_INF = np.array([[1, 0, 0, 2, 0, 62500, 62500],
                               [2, 0, 0, 1, 0, 1000250000, 1000250000],
                               [1, 0, 0, 1, 1, 500000, 500000]], np.int64)
# the whole image as the box: (2,0) D = R bit for bit agrees with 0 um, (2,1) becomes DATA_ONLY, (2,2) R = NaN, D = 2: DATA_ONLY
HAND_TABLE_WHOLE = np.array([[2, 0, 0, 1, 0, 62500, 62500],
                             [0, 2, 0, 1, 0, 1000250000, 0],
                             [0, 0, 1, 1, 3, 500000, 0]], np.int64)

# ---- random batches for the GPU: the smallest shapes that cross the 64 x 16 tile of a workgroup in both axes
BATCHES = ((1, 1, 1), (1, 40, 3), (17, 33, 3), (37, 53, 5), (5, 130, 2))     # rows, cols, images
STRIDES = (1, 2, 3, 5, 1000)                                                   # the last is larger than any image: pixel (0, 0) alone
PARTS = (1, 24, 254)
DENORMAL = F(1e-40)


def images(rng, n, H, W, P):
    """R: 40 % no model, a few at 255 (renderDepth's clamp), one NaN; M: mostly a part under the model and 255 elsewhere, with
    M == 255 where R > 0 and M < P where R == 0 both present; D: R plus centimetres of noise, or one of 0, -1, NaN, +inf, a
    denormal, R itself bit for bit, or an unrelated depth"""
    shape = (n, H, W)
    R = np.where(rng.random(shape) < 0.4, 0.0, rng.uniform(0.5, 3.0, shape)).astype(F)
    R[rng.random(shape) < 0.03] = 255.0
    M = np.where(R > 0, rng.integers(0, P, shape), 255)
    M = np.where(rng.random(shape) < 0.15, np.where(R > 0, 255, rng.integers(0, P, shape)), M).astype(np.uint8)
    D = (R + F(0.08) * rng.standard_normal(shape).astype(F)).astype(F)
    kind = rng.integers(0, 16, shape)
    for k, v in enumerate((0.0, -1.0, nan, inf, DENORMAL)):
        D[kind == k] = v
    D[kind == 5] = R[kind == 5]
    far = kind == 6
    D[far] = rng.uniform(0.3, 6.0, shape).astype(F)[far]
    D[kind == 7] = 0.0
    if H * W > 1:
        R.reshape(-1)[int(rng.integers(R.size))] = nan
    return R, M, D


def boxes(rng, n, H, W):
    """one box per image, in turn: whole by -1, a random inner box, one pixel, the inclusive edges, empty, partly outside"""
    out = []
    for i in range(n):
        x0, x1 = sorted(int(v) for v in rng.integers(0, W, 2))
        y0, y1 = sorted(int(v) for v in rng.integers(0, H, 2))
        out.append([(0, 0, -1, -1), (x0, y0, x1, y1), (x0, y0, x0, y0), (0, 0, W - 1, H - 1), (x1 + 1, y0, x0, y1), (x0, y0, W, y1)][i % 6])
    return np.array(out, np.int32)
