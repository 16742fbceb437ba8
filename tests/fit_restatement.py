"""One Levenberg-Marquardt step restated in numpy.longdouble: the damped solve (H + lambda diag(H)) delta = -g (oracle/avatar_oracle.cpp:895)
by an unblocked LDL^T, and the decrease the quadratic model predicts for that step (:1081-1108).  A helper module of the tests, not a test
file; needs neither a GPU nor the oracle (OracleModel.retract applies the step)."""
import numpy as np

LD = np.longdouble


def lm_step_ld(H, g, lam):
    """(delta, pivots, predicted decrease 1/2 delta^T (lam D delta - g)), all float64 rounded from long double; D = diag(H)."""
    H = np.asarray(H, LD)
    g = np.asarray(g, LD)
    n = len(g)
    D = np.diag(H).copy()
    A = H + LD(lam) * np.diag(D)
    L = np.eye(n, dtype=LD)
    d = np.zeros(n, LD)
    for k in range(n):
        d[k] = A[k, k] - (L[k, :k] ** 2 * d[:k]).sum()
        if k + 1 < n:
            L[k + 1:, k] = (A[k + 1:, k] - (L[k + 1:, :k] * L[k, :k] * d[:k]).sum(1)) / d[k]
    y = np.zeros(n, LD)
    for k in range(n):
        y[k] = -g[k] - (L[k, :k] * y[:k]).sum()
    z = y / d
    x = np.zeros(n, LD)
    for k in range(n - 1, -1, -1):
        x[k] = z[k] - (L[k + 1:, k] * x[k + 1:]).sum()
    pred = LD(0.5) * (x * (LD(lam) * D * x - g)).sum()
    return np.asarray(x, np.float64), np.asarray(d, np.float64), float(pred)
