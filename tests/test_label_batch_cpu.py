"""The batch labelling entry points of include/avt_rtree.h without a GPU: every declared avt_rtree_* function is in
avatar_amd/rtree.py's symbol list and exported by the built library, the three entry points of the stream-batch labelling among
them, and a host-only tree refuses them with the text of every other inference call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from avatar_amd import capi, rtree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "forest_small.srtr")
NEW = ["avt_rtree_predict_best_resident_boxes", "avt_rtree_predict_best_from_bgsub", "avt_rtree_labels_download_all"]
HOST_ONLY = "rtree: created host-only (device < 0): inference needs a GPU"


def _declared():
    text = open(os.path.join(ROOT, "include", "avt_rtree.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(avt_rtree_[a-z_]+)\s*\(", text)))


def test_every_declared_function_is_listed_and_exported():
    names = _declared()
    assert len(names) >= 16
    lib = C.CDLL(capi.LIB_PATH)
    for n in names:
        assert n in rtree.RTREE_SYMBOLS, n
        getattr(lib, n)
    for n in NEW:
        assert n in names, n


def test_host_only_tree_refuses_the_batch_calls():
    t = rtree.RTree(GOLD, device=-1)

    class NoBGSub:                       # predict_from_bgsub reads the handle only; a host-only tree fails before it is looked at
        _h, _n, _shape = None, 0, (0, 0, 3)

    with pytest.raises(capi.AvtError) as e:
        t.predict_resident_boxes(2, np.array([[0, 0, -1, -1]], np.int32))
    assert str(e.value) == HOST_ONLY
    with pytest.raises(capi.AvtError) as e:
        t.predict_from_bgsub(NoBGSub(), 2)
    assert str(e.value) == HOST_ONLY
