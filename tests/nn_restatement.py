"""A CPU restatement of the correspondence search (findNN(..., invert=true), AvatarOptimizer.cpp:841-907, with nanoflann's
L2_Simple_Adaptor::evalMetric and KNNResultSet::addPoint) and of the bookkeeping the GPU kernels keep beside it, in plain
numpy: the yardstick of tests/test_gpu_nn_edges.py.  A helper module of the tests, not a test file.

  nn_ref(...)       for every query with a valid label whose part has a visible vertex: the part's visible vertices in
                    ascending id, r = d0*d0; r = r + d1*d1; r = r + d2*d2 as separate float64 array operations (numpy
                    does not fuse them), the FIRST minimum - i.e. one ascending scan with strict '<'.  -1 otherwise.
  nn_sums_ref(...)  per model vertex the number of queries matched to it and the exact integer sums of
                    rint((data - centre) * 2**40), centre = the frame's first point whatever its label.

tests/test_nn_edges_cpu.py ties nn_ref to the CPU oracle (orc_nn) on every case of tests/nn_cases.py."""
from __future__ import annotations

import numpy as np

FIX_SCALE = 2.0 ** 40
_CHUNK = 512           # queries per block of the distance matrix (4097 x 6890 doubles at once would be 225 MB)


def dist2(q, c):
    """(Q, 3) queries against (C, 3) candidates -> (Q, C) squared distances, each product and sum rounded separately."""
    d0 = q[:, None, 0] - c[None, :, 0]
    d1 = q[:, None, 1] - c[None, :, 1]
    d2 = q[:, None, 2] - c[None, :, 2]
    r = d0 * d0
    r = r + d1 * d1
    r = r + d2 * d2
    return r


def nn_ref(part_of_vertex, num_parts, cloud, vis, data, labels):
    part_of_vertex = np.asarray(part_of_vertex)
    cloud = np.asarray(cloud, np.float64); data = np.asarray(data, np.float64).reshape(-1, 3)
    labels = np.asarray(labels, np.int64); vis = np.asarray(vis)
    out = np.full(len(labels), -1, np.int32)
    for q in range(num_parts):
        qi = np.nonzero(labels == q)[0]
        ids = np.nonzero((part_of_vertex == q) & (vis != 0))[0]          # ascending vertex id
        if len(qi) == 0 or len(ids) == 0:
            continue
        cand = cloud[ids]
        for b in range(0, len(qi), _CHUNK):
            sel = qi[b:b + _CHUNK]
            out[sel] = ids[np.argmin(dist2(data[sel], cand), axis=1)]     # argmin: the first minimum
    return out


def tie_counts(part_of_vertex, num_parts, cloud, vis, data, labels):
    """For every query: the number of candidates of its part at exactly the minimum distance (0: no candidate)."""
    part_of_vertex = np.asarray(part_of_vertex)
    cloud = np.asarray(cloud, np.float64); data = np.asarray(data, np.float64).reshape(-1, 3)
    labels = np.asarray(labels, np.int64); vis = np.asarray(vis)
    out = np.zeros(len(labels), np.int64)
    for q in range(num_parts):
        qi = np.nonzero(labels == q)[0]
        ids = np.nonzero((part_of_vertex == q) & (vis != 0))[0]
        if len(qi) == 0 or len(ids) == 0:
            continue
        for b in range(0, len(qi), _CHUNK):
            sel = qi[b:b + _CHUNK]
            r = dist2(data[sel], cloud[ids])
            out[sel] = (r == r.min(axis=1, keepdims=True)).sum(axis=1)
    return out


def nn_sums_ref(corr, data, num_vertices=6890):
    """(cnt int32[V], fsum int64[3, V], centre float64[3]) of the correspondences `corr` of the frame `data`."""
    corr = np.asarray(corr); data = np.asarray(data, np.float64).reshape(-1, 3)
    centre = data[0].copy() if len(data) else np.zeros(3)
    m = corr >= 0
    cnt = np.bincount(corr[m], minlength=num_vertices).astype(np.int32)
    fsum = np.zeros((3, num_vertices), np.int64)
    for k in range(3):
        fx = np.rint((data[m, k] - centre[k]) * FIX_SCALE).astype(np.int64)      # |x| < 2^51 for every frame of a few metres: exact
        np.add.at(fsum[k], corr[m], fx)
    return cnt, fsum, centre
