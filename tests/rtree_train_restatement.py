"""ctypes binding of tests/cpp/rtree_train_restatement.cpp: the reference's forest trainer (AvatarTrainerV3, RTree.cpp:2338-2950)
and RTree::trainTransfer (:3332-3420) restated on the CPU with the port's documented draws, compiled on first use with
g++ -ffp-contract=off into a temporary directory.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "rtree_train_restatement.cpp")
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(tempfile.mkdtemp(prefix="rtree_train_rst"), "librtree_train_rst.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", so, SRC])
        L = C.CDLL(so)
        L.rst_train.restype = C.c_void_p
        L.rst_train.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                                C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.rst_sizes.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.rst_get.argtypes = [C.c_void_p] + [C.c_void_p] * 7
        L.rst_near.restype = C.c_int
        L.rst_near.argtypes = [C.c_void_p]
        L.rst_free.argtypes = [C.c_void_p]
        L.rst_transfer.restype = C.c_int
        L.rst_transfer.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.rst_component.restype = C.c_float
        L.rst_component.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_float]
        L.rst_hash.restype = C.c_uint64
        L.rst_hash.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
        L.rst_bucket.restype = C.c_longlong
        L.rst_bucket.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int]
        L.rst_scan.restype = C.c_int
        L.rst_scan.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rst_root_hist.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_int,
                                    C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def train(depth, mask, num_parts, num_points_per_image, num_features, max_probe_offset, min_samples, max_tree_depth, T, seed,
          nthreads=1, device_tree=None, train=True):
    """dict: samples (img, x, y, label), feature (n,5), links (n,3), leaf (nl,P), ties (near ties that took the device's choice),
    near (nodes with two gains that are not bit-equal within 1e-12 relative, counted without a device tree: ties <= near).
    device_tree: (feature, links) of the GPU's tree; at a node whose two best gains (of two features, or of two thresholds of the
    chosen feature) lie within 1e-12 relative, the restatement takes the device's choice."""
    d = np.ascontiguousarray(depth, np.float32)
    m = np.ascontiguousarray(mask, np.uint8)
    n, rows, cols = d.shape
    L = lib()
    df = dl = None
    dn = 0
    if device_tree is not None:
        df = np.ascontiguousarray(device_tree[0], np.float32)
        dl = np.ascontiguousarray(device_tree[1], np.int32)
        dn = len(dl)
    h = L.rst_train(n, rows, cols, _ptr(d), _ptr(m), num_parts, num_points_per_image, num_features, max_probe_offset, min_samples, max_tree_depth,
                    T, seed, nthreads, dn, _ptr(df), _ptr(dl), 1 if train else 0)
    ns, nn, nl, ties = C.c_longlong(), C.c_int(), C.c_int(), C.c_int()
    L.rst_sizes(h, C.addressof(ns), C.addressof(nn), C.addressof(nl), C.addressof(ties))
    out = dict(img=np.empty(ns.value, np.int32), x=np.empty(ns.value, np.int32), y=np.empty(ns.value, np.int32), label=np.empty(ns.value, np.uint8),
               feature=np.empty((nn.value, 5), np.float32), links=np.empty((nn.value, 3), np.int32),
               leaf=np.empty((nl.value, num_parts), np.float32), ties=ties.value)
    L.rst_get(h, *(_ptr(out[k]) for k in ("img", "x", "y", "label", "feature", "links", "leaf")))
    out["near"] = L.rst_near(h)
    L.rst_free(h)
    return out


def transfer(feature, links, leaf, depth, mask):
    """(new leaf data, unvisited leaves) of trainTransfer on the fixed tree."""
    f = np.ascontiguousarray(feature, np.float32); l = np.ascontiguousarray(links, np.int32)
    lf = np.array(leaf, np.float32, copy=True, order="C")
    d = np.ascontiguousarray(depth, np.float32); m = np.ascontiguousarray(mask, np.uint8)
    n, rows, cols = d.shape
    z = lib().rst_transfer(len(l), _ptr(f), _ptr(l), lf.shape[0], lf.shape[1], _ptr(lf), n, rows, cols, _ptr(d), _ptr(m))
    return lf, z


def component(seed, key, f, c, max_probe_offset):
    return lib().rst_component(seed, key, f, c, max_probe_offset)


def bucket(score, mn, mx, T):
    return lib().rst_bucket(score, mn, mx, T)


def scan(hist, tot):
    """(best bucket index or -1, gain) of the threshold scan over a (P, T) histogram and the node's per-part totals."""
    h = np.ascontiguousarray(hist, np.int64); t = np.ascontiguousarray(tot, np.int64)
    g = C.c_double()
    i = lib().rst_scan(h.shape[0], h.shape[1], _ptr(h), _ptr(t), C.addressof(g))
    return i, g.value


def root_histograms(depth, mask, num_parts, num_points_per_image, max_probe_offset, T, seed, n_features):
    """(n_features, P, T) int32 root histograms and (n_features, 2) min / max, as the restatement counts them"""
    d = np.ascontiguousarray(depth, np.float32); m = np.ascontiguousarray(mask, np.uint8)
    n, rows, cols = d.shape
    h = np.empty((n_features, num_parts, T), np.int32)
    mm = np.empty((n_features, 2), np.float32)
    lib().rst_root_hist(n, rows, cols, _ptr(d), _ptr(m), num_parts, num_points_per_image, max_probe_offset, T, seed, n_features, _ptr(h), _ptr(mm))
    return h, mm
