"""Inputs of the pose-error tests (tests/test_pose_error_cpu.py, tests/test_gpu_pose_error.py): four families of (estimate, truth)
point sets, the sizes at which the kernel's workgroup of 256 lanes and its waves of 64 begin and end, and vertex-to-part tables.
Coordinates are of order one metre about a centre away from the origin, as posed avatars in front of a camera are."""
import numpy as np

FAMILIES = ("noise_shift", "similarity", "reflected", "unrelated")
V_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 513)
J_SIZES = (0, 1, 2, 3, 24)
ARGMAX_MARGIN = 1e-6
CENTRE = np.array([0.3, -0.2, 2.5])


def rotation(rng):
    """a proper rotation, uniformly drawn"""
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def margin(d):
    """how far the largest of d exceeds the runner-up, relative; inf for fewer than two"""
    if len(d) < 2:
        return np.inf
    s = np.sort(d)
    return (s[-1] - s[-2]) / s[-1] if s[-1] > 0 else 0.0


def family(name, n, seed):
    """(estimate (n, 3), truth (n, 3)) of one family; the largest raw error leads the runner-up by ARGMAX_MARGIN at least"""
    rng = np.random.default_rng([20261020, FAMILIES.index(name), n, seed])
    est = CENTRE + 0.5 * rng.standard_normal((n, 3))
    if name == "noise_shift":
        truth = est + 0.01 * rng.standard_normal((n, 3)) + np.array([0.05, -0.02, 0.08])
    elif name == "similarity":
        truth = 1.7 * est @ rotation(rng).T + np.array([-0.4, 0.1, 0.6])
    elif name == "reflected":
        truth = (est - CENTRE) * np.array([1.0, 1.0, -1.0]) + CENTRE + 0.003 * rng.standard_normal((n, 3))
    elif name == "unrelated":
        truth = CENTRE + 0.5 * rng.standard_normal((n, 3))
    else:
        raise ValueError(name)
    d = np.linalg.norm(est - truth, axis=1)
    if margin(d) < 10 * ARGMAX_MARGIN:                       # never seen with these seeds; kept so that a new seed cannot break the promise
        k = int(np.argmax(d))
        truth[k] += 1e-3 * (truth[k] - est[k])
    return est, truth


def pair_case(V, J, name, seed=0):
    """dict(E, T (V, 3), A, B (J, 3) or None) of one family"""
    E, T = family(name, V, seed)
    A, B = family(name, J, seed + 1000) if J else (None, None)
    return dict(E=E, T=T, A=A, B=B)


def batch(V, J, names=FAMILIES, seed=0):
    """the families stacked as one call: dict(E, T (n, V, 3), A, B (n, J, 3) or None)"""
    cs = [pair_case(V, J, nm, seed) for nm in names]
    return dict(E=np.stack([c["E"] for c in cs]), T=np.stack([c["T"] for c in cs]), A=np.stack([c["A"] for c in cs]) if J else None,
                B=np.stack([c["B"] for c in cs]) if J else None)


def part_tables(V):
    """{name: (P, vertex_part or None)}: one part; 24 parts with several empty; a part of one vertex; a part of all but one; 254 parts"""
    rng = np.random.default_rng([20261020, 77, V])
    sparse = rng.choice(np.array([0, 2, 3, 7, 11, 12, 19, 23]), V).astype(np.int32)       # 16 of 24 parts stay empty
    single = np.zeros(V, np.int32); single[V // 2] = 1                                  # part 1 holds one vertex, part 0 the rest
    return {"one": (1, None), "sparse24": (24, sparse), "single": (2, single), "all_but_one": (3, 2 - 2 * single),
            "p254": (254, (rng.permutation(V) % 254).astype(np.int32))}
