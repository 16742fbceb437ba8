"""A CPU restatement of the correspondence gate (include/avt.h avt_set_corr_gate) in plain numpy, on top of
tests/nn_restatement.py: the yardstick of tests/test_gpu_nn_gate.py.  A helper module of the tests, not a test file.

  gate_ref(...)      a query of part q matched to model point m at squared distance d2 keeps m iff d2 <= g[q] * g[q], else -1;
                     d2 = d0*d0; d2 = d2 + d1*d1; d2 = d2 + e2*e2 of (query - model point) as separate float64 array operations,
                     i.e. the search's own minimum; g[q] * g[q] is one float64 multiplication.  Returns the gated indices and
                     the number of matches dropped.
  median_gates(...)  per part sqrt(median d2 of the part's matched queries), +inf for a part without matches: gates that drop
                     and keep in almost every case, whatever its scale."""
from __future__ import annotations

import numpy as np


def matched_d2(corr, cloud, data):
    """(indices of the matched queries, their squared distances to their model points)."""
    corr = np.asarray(corr); cloud = np.asarray(cloud, np.float64); data = np.asarray(data, np.float64).reshape(-1, 3)
    m = np.nonzero(corr >= 0)[0]
    d0 = data[m, 0] - cloud[corr[m], 0]
    d1 = data[m, 1] - cloud[corr[m], 1]
    d2 = data[m, 2] - cloud[corr[m], 2]
    r = d0 * d0
    r = r + d1 * d1
    r = r + d2 * d2
    return m, r


def gate_ref(corr, cloud, data, labels, g):
    """(corr_gated int32, gated_count) of the ungated correspondences `corr` under the gates g (None / a scalar / one per part)."""
    corr = np.asarray(corr)
    labels = np.asarray(labels, np.int64)
    g = np.atleast_1d(np.asarray(np.inf if g is None else g, np.float64)).reshape(-1)
    assert not np.isnan(g).any() and (g >= 0).all()
    g2 = g * g
    m, r = matched_d2(corr, cloud, data)
    drop = r > (g2[0] if len(g2) == 1 else g2[labels[m]])      # a matched query has a label in [0, num_parts)
    out = corr.astype(np.int32).copy()
    out[m[drop]] = -1
    return out, int(drop.sum())


def median_gates(corr, cloud, data, labels, num_parts):
    labels = np.asarray(labels, np.int64)
    m, r = matched_d2(corr, cloud, data)
    g = np.full(num_parts, np.inf)
    for q in range(num_parts):
        rq = r[labels[m] == q]
        if len(rq):
            g[q] = np.sqrt(np.median(rq))
    return g


def on_gate(corr, cloud, data, labels, g):
    """How many matched queries sit exactly on d2 == g2 of their part (g: one gate per part)."""
    g = np.asarray(g, np.float64)
    m, r = matched_d2(corr, cloud, data)
    return int((r == (g * g)[np.asarray(labels, np.int64)[m]]).sum())
