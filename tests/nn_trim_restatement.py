"""A CPU restatement of trimmed ICP (include/avt.h avt_set_corr_trim) in plain numpy, on top of
tests/nn_restatement.py and tests/nn_gate_restatement.matched_d2: the yardstick of tests/test_gpu_nn_trim.py.  A helper module of the
tests, not a test file.

  trim_ref(...)   per part q with a finite factor: Q = the part's queries that hold a match (after the search and the fixed gate),
                  n = |Q|; n == 0 or n < min_matches: T = +inf.  Else k = int(ceil(rho * float(n))) clamped to [1, n], t = the k-th
                  smallest squared distance (np.sort of the part's d2, the order statistic - not a median), T = max(k2 * t, f2) with
                  k2 = kappa * kappa and f2 = floor * floor, one float64 multiplication each; a match is dropped iff d2 > T.
                  Returns (indices, total dropped, dropped per part, T per part).
  on_threshold(...)  how many matches sit exactly on d2 == T of their part."""
from __future__ import annotations

import numpy as np

import nn_gate_restatement as ng


def _per_part(v, num_parts):
    a = np.atleast_1d(np.asarray(v, np.float64)).reshape(-1)
    assert len(a) in (1, num_parts)
    return np.full(num_parts, a[0]) if len(a) == 1 else a.copy()


def thresholds(d2, part, num_parts, rho, kappa, floor=0.0, min_matches=1):
    """T float64[num_parts] of matches with squared distances d2 in parts `part`."""
    rho, kappa, floor = (_per_part(v, num_parts) for v in (rho, kappa, floor))
    assert ((rho > 0) & (rho <= 1)).all() and (kappa >= 0).all() and (floor >= 0).all() and np.isfinite(floor).all() and min_matches >= 1
    k2 = kappa * kappa
    f2 = floor * floor
    assert (np.isfinite(k2) | np.isinf(kappa)).all()
    assert not np.isnan(d2).any() and (d2 >= 0).all()          # where the order of the bit patterns is the numeric order
    T = np.full(num_parts, np.inf)
    for q in range(num_parts):
        if np.isinf(kappa[q]):
            continue
        rq = np.sort(d2[part == q])
        n = len(rq)
        if n == 0 or n < min_matches:
            continue
        k = min(max(int(np.ceil(rho[q] * float(n))), 1), n)
        with np.errstate(over="ignore"):                        # (k2 t may round to +inf: then nothing is dropped)
            T[q] = np.maximum(k2[q] * rq[k - 1], f2[q])
    return T


def trim_ref(corr, cloud, data, labels, num_parts, rho, kappa, floor=0.0, min_matches=1):
    corr = np.asarray(corr)
    labels = np.asarray(labels, np.int64)
    m, r = ng.matched_d2(corr, cloud, data)
    part = labels[m]                                            # a matched query has a label in [0, num_parts)
    T = thresholds(r, part, num_parts, rho, kappa, floor, min_matches)
    drop = r > T[part]
    out = corr.astype(np.int32).copy()
    out[m[drop]] = -1
    per_part = np.bincount(part[drop], minlength=num_parts).astype(np.int32)
    return out, int(drop.sum()), per_part, T


def on_threshold(corr, cloud, data, labels, T):
    m, r = ng.matched_d2(corr, cloud, data)
    return int((r == np.asarray(T)[np.asarray(labels, np.int64)[m]]).sum())
