"""Plain numpy restatement of the pose error (include/avt_poseerr.h, THE RULE) on float64, for the tests.  The alignment comes in
two independent formulations: Umeyama's, through np.linalg.svd with the reflection correction (`align_svd`, the one the tests
compare the device against), and Horn's, through the largest eigenvector of his symmetric 4 x 4 matrix with np.linalg.eigh
(`align_horn`).  Their difference on a case measures how well the case's 3 x 3 problem is conditioned, and sets the tolerance of
the alignment figures on that case (`alignment_tolerance`)."""
import numpy as np

COLUMNS = ("V_SUM", "V_SQ", "V_MAX", "VPA_SUM", "VPA_SQ", "VPA_SCALE", "J_SUM", "J_MAX", "JR_SUM", "JPA_SUM", "JPA_SQ", "JPA_SCALE")
EPS = 2.0 ** -52


def errors(x, y):
    """d_k = |x_k - y_k| of two (n, 3) point sets"""
    d = np.asarray(x, np.float64) - np.asarray(y, np.float64)
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def coincident(x):
    """the rule's degenerate estimate: every point equals the first (compared with ==)"""
    return bool((x == x[0]).all())


def align_svd(x, y):
    """(s, R, c) minimising sum |s R x_k + c - y_k|^2 over proper rotations and s >= 0: Umeyama 1991, eqs. 34-43"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mx, my = x.mean(0), y.mean(0)
    if coincident(x):
        return 0.0, np.eye(3), my.copy()
    xc, yc = x - mx, y - my
    sigma = yc.T @ xc / len(x)
    U, D, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    s = max(float((D * S).sum() / ((xc * xc).sum() / len(x))), 0.0)
    return s, R, my - s * R @ mx


def align_horn(x, y):
    """the same optimum by Horn 1987: the rotation of the largest eigenvector of N, s = its eigenvalue / sum |x'|^2"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mx, my = x.mean(0), y.mean(0)
    if coincident(x):
        return 0.0, np.eye(3), my.copy()
    xc, yc = x - mx, y - my
    M = xc.T @ yc                                      # M[a, b] = sum x'_a y'_b
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = M
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    lam, vec = np.linalg.eigh(N)
    w, a, b, c = vec[:, 3] / np.linalg.norm(vec[:, 3])
    R = np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b)],
                  [2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a)],
                  [2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)]])
    s = max(float(lam[3] / (xc * xc).sum()), 0.0)
    return s, R, my - s * R @ mx


def aligned(x, y, form=align_svd):
    """dict(sum, sq, scale, err (n,), R, spread): the aligned figures of one point set; spread = S = sum |y_k - mean y|"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    s, R, c = form(x, y)
    a = s * (x - x.mean(0)) @ R.T - (y - y.mean(0))
    q = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]
    return dict(sum=float(np.sqrt(q).sum()), sq=float(q.sum()), scale=float(s), err=np.sqrt(q), R=R, spread=float(errors(y, y.mean(0)[None]).sum()))


def alignment_tolerance(x, y):
    """Per figure of one point set, dict(sum, sq, scale, err): tol = max(16 |svd form - quaternion form|, (n + 16) 2^-52 S) with
    S = sum |y_k - mean y|, the problem's scale: figures near zero are compared on it.  `forms` is the largest difference of the
    two formulations over the four figures."""
    a, b = aligned(x, y, align_svd), aligned(x, y, align_horn)
    floor = (len(x) + 16) * EPS * a["spread"]
    diff = dict(sum=abs(a["sum"] - b["sum"]), sq=abs(a["sq"] - b["sq"]), scale=abs(a["scale"] - b["scale"]), err=float(np.abs(a["err"] - b["err"]).max()))
    out = {k: max(16 * v, floor) for k, v in diff.items()}
    out["forms"] = max(diff.values())
    return out


def pair(est_cloud, truth_cloud, est_joints=None, truth_joints=None, vertex_part=None, num_parts=1):
    """One pair: dict(summary (12,), per_joint (2, J), per_part (2, P), argmax (2,), bad) as avt_poseerr_get lays them out"""
    E, T = np.asarray(est_cloud, np.float64), np.asarray(truth_cloud, np.float64)
    V = len(E)
    J = 0 if est_joints is None else len(est_joints)
    vp = np.zeros(V, np.int64) if vertex_part is None else np.asarray(vertex_part, np.int64)
    out = dict(summary=np.full(12, np.nan), per_joint=np.zeros((2, J)), per_part=np.zeros((2, num_parts)), argmax=np.array([-1, -1], np.int32))
    bad = not (np.isfinite(E).all() and np.isfinite(T).all())
    if J:
        bad |= not (np.isfinite(np.asarray(est_joints, np.float64)).all() and np.isfinite(np.asarray(truth_joints, np.float64)).all())
    out["bad"] = bad
    if bad:                                              # the figures are unspecified
        return out
    d = errors(E, T)
    pa = aligned(E, T)
    out["summary"][:6] = d.sum(), (d * d).sum(), d.max(), pa["sum"], pa["sq"], pa["scale"]
    out["argmax"][0] = int(np.argmax(d))                 # the first of equal maxima
    for q in range(num_parts):
        sel = d[vp == q]
        if len(sel):
            out["per_part"][:, q] = sel.sum(), sel.max()
    if J:
        A, B = np.asarray(est_joints, np.float64), np.asarray(truth_joints, np.float64)
        e = errors(A, B)
        r = errors(A - A[0], B - B[0])
        pj = aligned(A, B)
        out["summary"][6:] = e.sum(), e.max(), r.sum(), pj["sum"], pj["sq"], pj["scale"]
        out["per_joint"][0], out["per_joint"][1] = e, pj["err"]
        out["argmax"][1] = int(np.argmax(e))
    return out


def pairs(est_clouds, truth_clouds, est_joints=None, truth_joints=None, vertex_part=None, num_parts=1):
    """n pairs stacked: what poseerror.PoseError.get returns (status: 1 for a non-finite pair)"""
    n = len(est_clouds)
    rs = [pair(est_clouds[i], truth_clouds[i], None if est_joints is None else est_joints[i], None if truth_joints is None else truth_joints[i],
               vertex_part, num_parts) for i in range(n)]
    return dict(summary=np.stack([r["summary"] for r in rs]), per_joint=np.stack([r["per_joint"] for r in rs]),
                per_part=np.stack([r["per_part"] for r in rs]), argmax=np.stack([r["argmax"] for r in rs]),
                status=np.array([1 if r["bad"] else 0 for r in rs], np.uint32))
