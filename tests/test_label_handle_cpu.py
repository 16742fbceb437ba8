"""The labelling handle the tree and the forest share (avatar_amd/csrc/avt_label.h, avatar_amd/labelhandle.py): every check of
the image side that fires before the device is touched, on null handles and on host-only ones (device = -1), with the text
avt_last_error() must give, byte for byte, for both kinds.  The table was written against the two separate copies of the host
code; the one copy must give the same strings."""
import ctypes as C

import numpy as np
import pytest

from avatar_amd import capi, rforest, rtree


class _Slot:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name


H = _Slot("H")          # the host-only handle of the row's kind
F = _Slot("F")          # a float buffer
B = _Slot("B")          # a byte buffer
I = _Slot("I")          # an int buffer
D = _Slot("D")          # a double buffer
X = _Slot("X")          # a non-null pointer that the call must not follow: a context or a background subtractor behind a check that fires first
W = C.c_double(0.001)   # dist_to_pre_weight

T_HOST = "rtree: created host-only (device < 0): inference needs a GPU"
F_HOST = "rforest: created host-only (device < 0): inference needs a GPU"
T_ROI = "rtree: bad image size, interval or region of interest"
F_ROI = "rforest: bad image size, interval or region of interest"
UPLOAD = ": bad arguments (1 to 65535 images of 1 to 32767 rows and columns)"
STAGE = ": created host-only (device < 0): the device stage needs a GPU"

# (kind, entry point, arguments, avt_last_error())
TABLE = [
    # ---- predict_best: null arguments, then size, interval and region of interest, then the device
    ("rtree", "avt_rtree_predict_best", (None, F, 4, 6, 1, 0, 0, -1, -1, 1, B), "avt_rtree_predict_best: null argument"),
    ("rtree", "avt_rtree_predict_best", (H, None, 4, 6, 1, 0, 0, -1, -1, 1, B), "avt_rtree_predict_best: null argument"),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 6, 1, 0, 0, -1, -1, 1, None), "avt_rtree_predict_best: null argument"),
    ("rforest", "avt_rforest_predict_best", (None, F, 4, 6, 1, 0, 0, -1, -1, 1, B), "avt_rforest_predict_best: null argument"),
    ("rforest", "avt_rforest_predict_best", (H, None, 4, 6, 1, 0, 0, -1, -1, 1, B), "avt_rforest_predict_best: null argument"),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 6, 1, 0, 0, -1, -1, 1, None), "avt_rforest_predict_best: null argument"),
    ("rtree", "avt_rtree_predict_best", (H, F, 0, 6, 1, 0, 0, -1, -1, 1, B), T_ROI),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 0, 1, 0, 0, -1, -1, 1, B), T_ROI),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 6, 0, 0, 0, -1, -1, 1, B), T_ROI),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 6, 1, -1, 0, 5, 3, 1, B), T_ROI),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 6, 1, 0, -1, 5, 3, 1, B), T_ROI),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 6, 1, 0, 0, 6, 3, 1, B), T_ROI),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 6, 1, 0, 0, 5, 4, 1, B), T_ROI),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 6, 1, 3, 0, 2, 3, 1, B), T_ROI),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 6, 1, 0, 3, 5, 2, 1, B), T_ROI),
    ("rtree", "avt_rtree_predict_best", (H, F, 32768, 6, 1, 0, 0, -1, -1, 1, B), T_ROI),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 32768, 1, 0, 0, -1, -1, 1, B), T_ROI),
    ("rforest", "avt_rforest_predict_best", (H, F, 0, 6, 1, 0, 0, -1, -1, 1, B), F_ROI),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 0, 1, 0, 0, -1, -1, 1, B), F_ROI),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 6, 0, 0, 0, -1, -1, 1, B), F_ROI),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 6, 1, -1, 0, 5, 3, 1, B), F_ROI),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 6, 1, 0, -1, 5, 3, 1, B), F_ROI),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 6, 1, 0, 0, 6, 3, 1, B), F_ROI),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 6, 1, 0, 0, 5, 4, 1, B), F_ROI),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 6, 1, 3, 0, 2, 3, 1, B), F_ROI),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 6, 1, 0, 3, 5, 2, 1, B), F_ROI),
    ("rforest", "avt_rforest_predict_best", (H, F, 32768, 6, 1, 0, 0, -1, -1, 1, B), F_ROI),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 32768, 1, 0, 0, -1, -1, 1, B), F_ROI),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 6, 1, 0, 0, -1, -1, 1, B), T_HOST),
    ("rtree", "avt_rtree_predict_best", (H, F, 4, 6, 2, 1, 1, 5, 3, 0, B), T_HOST),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 6, 1, 0, 0, -1, -1, 1, B), F_HOST),
    ("rforest", "avt_rforest_predict_best", (H, F, 4, 6, 2, 1, 1, 5, 3, 0, B), F_HOST),
    # ---- predict (the distributions): only the forest looks at the 32767 limit before the upload
    ("rtree", "avt_rtree_predict", (None, F, 4, 6, F), "avt_rtree_predict: bad arguments"),
    ("rtree", "avt_rtree_predict", (H, None, 4, 6, F), "avt_rtree_predict: bad arguments"),
    ("rtree", "avt_rtree_predict", (H, F, 4, 6, None), "avt_rtree_predict: bad arguments"),
    ("rtree", "avt_rtree_predict", (H, F, 0, 6, F), "avt_rtree_predict: bad arguments"),
    ("rtree", "avt_rtree_predict", (H, F, 4, -1, F), "avt_rtree_predict: bad arguments"),
    ("rtree", "avt_rtree_predict", (H, F, 4, 6, F), T_HOST),
    ("rtree", "avt_rtree_predict", (H, F, 32768, 1, F), T_HOST),
    ("rtree", "avt_rtree_predict", (H, F, 1, 32768, F), T_HOST),
    ("rforest", "avt_rforest_predict", (None, F, 4, 6, F), "avt_rforest_predict: bad arguments"),
    ("rforest", "avt_rforest_predict", (H, None, 4, 6, F), "avt_rforest_predict: bad arguments"),
    ("rforest", "avt_rforest_predict", (H, F, 4, 6, None), "avt_rforest_predict: bad arguments"),
    ("rforest", "avt_rforest_predict", (H, F, 0, 6, F), "avt_rforest_predict: bad arguments"),
    ("rforest", "avt_rforest_predict", (H, F, 4, -1, F), "avt_rforest_predict: bad arguments"),
    ("rforest", "avt_rforest_predict", (H, F, 4, 6, F), F_HOST),
    ("rforest", "avt_rforest_predict", (H, F, 32768, 1, F), F_ROI),
    ("rforest", "avt_rforest_predict", (H, F, 1, 32768, F), F_ROI),
    # ---- images_upload: only the forest has the 65535 limit
    ("rtree", "avt_rtree_images_upload", (None, 1, 4, 6, F), "avt_rtree_images_upload: bad arguments"),
    ("rtree", "avt_rtree_images_upload", (H, 0, 4, 6, F), "avt_rtree_images_upload: bad arguments"),
    ("rtree", "avt_rtree_images_upload", (H, 1, 0, 6, F), "avt_rtree_images_upload: bad arguments"),
    ("rtree", "avt_rtree_images_upload", (H, 1, 4, 0, F), "avt_rtree_images_upload: bad arguments"),
    ("rtree", "avt_rtree_images_upload", (H, 1, 4, 6, None), "avt_rtree_images_upload: bad arguments"),
    ("rtree", "avt_rtree_images_upload", (H, 1, 4, 6, F), T_HOST),
    ("rtree", "avt_rtree_images_upload", (H, 65535, 1, 1, F), T_HOST),
    ("rtree", "avt_rtree_images_upload", (H, 65536, 1, 1, F), T_HOST),
    ("rforest", "avt_rforest_images_upload", (None, 1, 4, 6, F), "avt_rforest_images_upload: bad arguments"),
    ("rforest", "avt_rforest_images_upload", (H, 0, 4, 6, F), "avt_rforest_images_upload: bad arguments"),
    ("rforest", "avt_rforest_images_upload", (H, 1, 0, 6, F), "avt_rforest_images_upload: bad arguments"),
    ("rforest", "avt_rforest_images_upload", (H, 1, 4, 0, F), "avt_rforest_images_upload: bad arguments"),
    ("rforest", "avt_rforest_images_upload", (H, 1, 4, 6, None), "avt_rforest_images_upload: bad arguments"),
    ("rforest", "avt_rforest_images_upload", (H, 1, 4, 6, F), F_HOST),
    ("rforest", "avt_rforest_images_upload", (H, 65535, 1, 1, F), F_HOST),
    ("rforest", "avt_rforest_images_upload", (H, 65536, 1, 1, F), "rforest: at most 65535 images per call"),
    # ---- the two label downloads: nothing is labelled behind a fresh handle
    ("rtree", "avt_rtree_labels_download", (None, 0, B), "avt_rtree_labels_download: bad arguments"),
    ("rtree", "avt_rtree_labels_download", (H, 0, None), "avt_rtree_labels_download: bad arguments"),
    ("rtree", "avt_rtree_labels_download", (H, -1, B), "avt_rtree_labels_download: bad arguments"),
    ("rtree", "avt_rtree_labels_download", (H, 0, B), "avt_rtree_labels_download: bad arguments"),
    ("rtree", "avt_rtree_labels_download", (H, 1, B), "avt_rtree_labels_download: bad arguments"),
    ("rforest", "avt_rforest_labels_download", (None, 0, B), "avt_rforest_labels_download: bad arguments"),
    ("rforest", "avt_rforest_labels_download", (H, 0, None), "avt_rforest_labels_download: bad arguments"),
    ("rforest", "avt_rforest_labels_download", (H, -1, B), "avt_rforest_labels_download: bad arguments"),
    ("rforest", "avt_rforest_labels_download", (H, 0, B), "avt_rforest_labels_download: bad arguments"),
    ("rforest", "avt_rforest_labels_download", (H, 1, B), "avt_rforest_labels_download: bad arguments"),
    ("rtree", "avt_rtree_labels_download_all", (None, B), "avt_rtree_labels_download_all: bad arguments or no labelled images"),
    ("rtree", "avt_rtree_labels_download_all", (H, None), "avt_rtree_labels_download_all: bad arguments or no labelled images"),
    ("rtree", "avt_rtree_labels_download_all", (H, B), "avt_rtree_labels_download_all: bad arguments or no labelled images"),
    ("rforest", "avt_rforest_labels_download_all", (None, B), "avt_rforest_labels_download_all: bad arguments or no labelled images"),
    ("rforest", "avt_rforest_labels_download_all", (H, None), "avt_rforest_labels_download_all: bad arguments or no labelled images"),
    ("rforest", "avt_rforest_labels_download_all", (H, B), "avt_rforest_labels_download_all: bad arguments or no labelled images"),
    # ---- the resident forms
    ("rtree", "avt_rtree_predict_best_resident", (None, 1, 0, 0, -1, -1, 1), "avt_rtree_predict_best_resident: no images resident"),
    ("rtree", "avt_rtree_predict_best_resident", (H, 1, 0, 0, -1, -1, 1), "avt_rtree_predict_best_resident: no images resident"),
    ("rtree", "avt_rtree_predict_best_resident_boxes", (None, 1, I, 1), "avt_rtree_predict_best_resident_boxes: null argument"),
    ("rtree", "avt_rtree_predict_best_resident_boxes", (H, 1, None, 1), "avt_rtree_predict_best_resident_boxes: null argument"),
    ("rtree", "avt_rtree_predict_best_resident_boxes", (H, 1, I, 1), T_HOST),
    ("rforest", "avt_rforest_predict_best_resident_boxes", (None, 1, I, 1), "avt_rforest_predict_best_resident_boxes: null argument"),
    ("rforest", "avt_rforest_predict_best_resident_boxes", (H, 1, None, 1), "avt_rforest_predict_best_resident_boxes: null argument"),
    ("rforest", "avt_rforest_predict_best_resident_boxes", (H, 1, I, 1), F_HOST),
    ("rtree", "avt_rtree_predict_best_from_bgsub", (None, None, 1, 1), "avt_rtree_predict_best_from_bgsub: null tree"),
    ("rtree", "avt_rtree_predict_best_from_bgsub", (None, X, 1, 1), "avt_rtree_predict_best_from_bgsub: null tree"),
    ("rtree", "avt_rtree_predict_best_from_bgsub", (H, None, 1, 1), T_HOST),
    ("rtree", "avt_rtree_predict_best_from_bgsub", (H, X, 1, 1), T_HOST),
    ("rforest", "avt_rforest_predict_best_from_bgsub", (None, None, 1, 1), "avt_rforest_predict_best_from_bgsub: null forest"),
    ("rforest", "avt_rforest_predict_best_from_bgsub", (None, X, 1, 1), "avt_rforest_predict_best_from_bgsub: null forest"),
    ("rforest", "avt_rforest_predict_best_from_bgsub", (H, None, 1, 1), F_HOST),
    ("rforest", "avt_rforest_predict_best_from_bgsub", (H, X, 1, 1), F_HOST),
    # ---- sync: only the forest refuses a host-only handle
    ("rtree", "avt_rtree_sync", (None,), "avt_rtree_sync: null tree"),
    ("rforest", "avt_rforest_sync", (None,), "avt_rforest_sync: null forest"),
    ("rforest", "avt_rforest_sync", (H,), F_HOST),
    # ---- the device post-processing and its memory
    ("rtree", "avt_rtree_post_process_resident", (None, 1, None, W), "avt_rtree_post_process_resident: null handle"),
    ("rtree", "avt_rtree_post_process_resident", (H, 1, None, W), "avt_rtree_post_process_resident" + STAGE),
    ("rtree", "avt_rtree_post_process_resident", (H, 0, I, W), "avt_rtree_post_process_resident" + STAGE),
    ("rforest", "avt_rforest_post_process_resident", (None, 1, None, W), "avt_rforest_post_process_resident: null handle"),
    ("rforest", "avt_rforest_post_process_resident", (H, 1, None, W), "avt_rforest_post_process_resident" + STAGE),
    ("rforest", "avt_rforest_post_process_resident", (H, 0, I, W), "avt_rforest_post_process_resident" + STAGE),
    ("rtree", "avt_rtree_post_process_from_bgsub", (None, None, 1, W), "avt_rtree_post_process_from_bgsub: null handle"),
    ("rtree", "avt_rtree_post_process_from_bgsub", (H, None, 1, W), "avt_rtree_post_process_from_bgsub" + STAGE),
    ("rtree", "avt_rtree_post_process_from_bgsub", (H, X, 1, W), "avt_rtree_post_process_from_bgsub" + STAGE),
    ("rforest", "avt_rforest_post_process_from_bgsub", (None, None, 1, W), "avt_rforest_post_process_from_bgsub: null handle"),
    ("rforest", "avt_rforest_post_process_from_bgsub", (H, None, 1, W), "avt_rforest_post_process_from_bgsub" + STAGE),
    ("rforest", "avt_rforest_post_process_from_bgsub", (H, X, 1, W), "avt_rforest_post_process_from_bgsub" + STAGE),
    ("rtree", "avt_rtree_com_pre_set", (None, 0, 1, D, None), "avt_rtree_com_pre_set: null or host-only tree"),
    ("rtree", "avt_rtree_com_pre_set", (H, 0, 1, D, B), "avt_rtree_com_pre_set: null or host-only tree"),
    ("rtree", "avt_rtree_com_pre_get", (None, 0, 1, D, B), "avt_rtree_com_pre_get: null or host-only tree"),
    ("rtree", "avt_rtree_com_pre_get", (H, 0, 1, D, B), "avt_rtree_com_pre_get: null or host-only tree"),
    ("rforest", "avt_rforest_com_pre_set", (None, 0, 1, D, None), "avt_rforest_com_pre_set: null or host-only forest"),
    ("rforest", "avt_rforest_com_pre_set", (H, 0, 1, D, B), "avt_rforest_com_pre_set: null or host-only forest"),
    ("rforest", "avt_rforest_com_pre_get", (None, 0, 1, D, B), "avt_rforest_com_pre_get: null or host-only forest"),
    ("rforest", "avt_rforest_com_pre_get", (H, 0, 1, D, B), "avt_rforest_com_pre_get: null or host-only forest"),
    ("rtree", "avt_rtree_labels_upload", (None, 1, 4, 6, B), "avt_rtree_labels_upload" + UPLOAD),
    ("rtree", "avt_rtree_labels_upload", (H, 1, 4, 6, None), "avt_rtree_labels_upload" + UPLOAD),
    ("rtree", "avt_rtree_labels_upload", (H, 0, 4, 6, B), "avt_rtree_labels_upload" + UPLOAD),
    ("rtree", "avt_rtree_labels_upload", (H, 65536, 1, 1, B), "avt_rtree_labels_upload" + UPLOAD),
    ("rtree", "avt_rtree_labels_upload", (H, 1, 0, 6, B), "avt_rtree_labels_upload" + UPLOAD),
    ("rtree", "avt_rtree_labels_upload", (H, 1, 4, 32768, B), "avt_rtree_labels_upload" + UPLOAD),
    ("rtree", "avt_rtree_labels_upload", (H, 1, 4, 6, B), "avt_rtree_labels_upload" + STAGE),
    ("rforest", "avt_rforest_labels_upload", (None, 1, 4, 6, B), "avt_rforest_labels_upload" + UPLOAD),
    ("rforest", "avt_rforest_labels_upload", (H, 1, 4, 6, None), "avt_rforest_labels_upload" + UPLOAD),
    ("rforest", "avt_rforest_labels_upload", (H, 0, 4, 6, B), "avt_rforest_labels_upload" + UPLOAD),
    ("rforest", "avt_rforest_labels_upload", (H, 65536, 1, 1, B), "avt_rforest_labels_upload" + UPLOAD),
    ("rforest", "avt_rforest_labels_upload", (H, 1, 0, 6, B), "avt_rforest_labels_upload" + UPLOAD),
    ("rforest", "avt_rforest_labels_upload", (H, 1, 4, 32768, B), "avt_rforest_labels_upload" + UPLOAD),
    ("rforest", "avt_rforest_labels_upload", (H, 1, 4, 6, B), "avt_rforest_labels_upload" + STAGE),
    # ---- the subsampling entry points (ctx, handle, bgsub, boxes, intervals, want_centroid, counts, centroid, boxes_out)
    ("rtree", "avt_frames_subsample_rtree", (None, H, X, None, I, None, I, None, None), "avt_frames_subsample_rtree: null context"),
    ("rtree", "avt_frames_subsample_rtree", (X, None, X, None, I, None, I, None, None), "avt_frames_subsample_rtree: null forest handle"),
    ("rtree", "avt_frames_subsample_rtree", (X, H, None, None, I, None, I, None, None), "avt_frames_subsample_rtree: null background subtractor"),
    ("rtree", "avt_frames_subsample_rtree", (X, H, X, None, None, None, I, None, None), "avt_frames_subsample_rtree: null argument (intervals, counts_out)"),
    ("rtree", "avt_frames_subsample_rtree", (X, H, X, None, I, None, None, None, None), "avt_frames_subsample_rtree: null argument (intervals, counts_out)"),
    ("rtree", "avt_frames_subsample_rtree", (X, H, X, None, I, None, I, None, None), "avt_frames_subsample_rtree: the forest handle was created host-only (device < 0)"),
    ("rforest", "avt_frames_subsample_rforest", (None, H, X, None, I, None, I, None, None), "avt_frames_subsample_rforest: null context"),
    ("rforest", "avt_frames_subsample_rforest", (X, None, X, None, I, None, I, None, None), "avt_frames_subsample_rforest: null forest handle"),
    ("rforest", "avt_frames_subsample_rforest", (X, H, None, None, I, None, I, None, None), "avt_frames_subsample_rforest: null background subtractor"),
    ("rforest", "avt_frames_subsample_rforest", (X, H, X, None, None, None, I, None, None), "avt_frames_subsample_rforest: null argument (intervals, counts_out)"),
    ("rforest", "avt_frames_subsample_rforest", (X, H, X, None, I, None, None, None, None), "avt_frames_subsample_rforest: null argument (intervals, counts_out)"),
    ("rforest", "avt_frames_subsample_rforest", (X, H, X, None, I, None, I, None, None), "avt_frames_subsample_rforest: the forest handle was created host-only (device < 0)"),
]


@pytest.fixture(scope="module")
def handles():
    """A host-only tree whose root is a leaf, the host-only forest of two of it, and the buffers the rows point at."""
    tree = rtree.RTree.from_arrays(np.zeros((1, 5), np.float32), np.array([[-1, -1, 0]], np.int32), np.array([[0.5, 0.25, 0.25]], np.float32), 3,
                                   device=-1)
    forest = rforest.RForest([tree, tree], device=-1)
    bufs = {F: np.ones(3 * 4 * 6, np.float32), B: np.zeros(64, np.uint8), I: np.ones(16, np.int32), D: np.zeros(16, np.float64),
            X: np.zeros(1 << 16, np.uint8)}
    return {"rtree": tree, "rforest": forest}, bufs


@pytest.mark.parametrize("row", range(len(TABLE)), ids=lambda i: "%s-%d" % (TABLE[i][1], i))
def test_error_text_before_the_device_is_touched(handles, row):
    kinds, bufs = handles
    kind, name, args, want = TABLE[row]
    lib = capi.load_library()
    real = []
    for a in args:
        if a is H:
            real.append(kinds[kind]._h)
        elif isinstance(a, _Slot):
            real.append(C.c_void_p(bufs[a].ctypes.data))
        else:
            real.append(a)
    fn = getattr(lib, name)
    fn.restype = C.c_int
    assert fn(*real) == 1
    assert lib.avt_last_error() == want.encode()


def test_the_table_covers_both_kinds_alike():
    """Every shared entry point is in the table for both kinds, with as many rows; only the tree has the one-box resident form."""
    count = {}
    for kind, name, _, _ in TABLE:
        stem = name.replace("avt_rtree_", "").replace("avt_rforest_", "").replace("avt_frames_subsample_rtree", "subsample").replace(
            "avt_frames_subsample_rforest", "subsample")
        count.setdefault(stem, {}).setdefault(kind, 0)
        count[stem][kind] += 1
    assert count.pop("predict_best_resident") == {"rtree": 2}
    assert count.pop("sync") == {"rtree": 1, "rforest": 2}
    for stem, c in count.items():
        assert c.get("rtree") == c.get("rforest"), stem
    assert set(count) == {"predict_best", "predict", "images_upload", "labels_download", "labels_download_all", "predict_best_resident_boxes",
                          "predict_best_from_bgsub", "post_process_resident", "post_process_from_bgsub", "com_pre_set", "com_pre_get", "labels_upload",
                          "subsample"}


def test_both_classes_derive_from_the_one_base():
    from avatar_amd import labelhandle
    assert issubclass(rtree.RTree, labelhandle.LabelHandle) and issubclass(rforest.RForest, labelhandle.LabelHandle)
    assert not issubclass(rforest.RForest, rtree.RTree) and not issubclass(rtree.RTree, rforest.RForest)
    for name in ("predictBest", "predict", "upload_images", "predict_resident_boxes", "predict_from_bgsub", "upload_labels", "post_process_resident",
                 "post_process_from_bgsub", "com_pre_get", "com_pre_set", "sync", "download_labels", "download_all_labels", "__del__"):
        assert name in vars(labelhandle.LabelHandle), name
        assert name not in vars(rtree.RTree) and name not in vars(rforest.RForest), name
