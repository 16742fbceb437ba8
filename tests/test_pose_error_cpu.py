"""CPU tests of the pose error (include/avt_poseerr.h): the numpy restatement against values worked by hand, its two alignment
formulations against each other on the cases the GPU tests use, poseerror.metrics against ark::PoseErrorResult::derive through
tests/cpp/pose_error_demo (the same doubles, NaN cases included), the ABI's names in the built library and in the Python binding,
and the argument refusals that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pose_error_cases as pc
import pose_error_restatement as pr
from avatar_amd import capi, poseerror

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEMO = os.path.join(HERE, "cpp", "pose_error_demo")


def test_restatement_pure_translation():
    rng = np.random.default_rng(1)
    E = rng.standard_normal((7, 3))
    A = rng.standard_normal((4, 3))
    shift = np.array([3.0, -4.0, 12.0])                                      # |shift| = 13
    r = pr.pair(E, E + shift, A, A + shift, vertex_part=[0, 1, 1, 0, 0, 1, 0], num_parts=3)
    s = dict(zip(pr.COLUMNS, r["summary"]))
    assert abs(s["V_SUM"] - 7 * 13) < 1e-12 and abs(s["V_SQ"] - 7 * 169) < 1e-11 and abs(s["V_MAX"] - 13) < 1e-13
    assert abs(s["J_SUM"] - 4 * 13) < 1e-12 and abs(s["J_MAX"] - 13) < 1e-13 and np.allclose(r["per_joint"][0], 13, atol=1e-13)
    assert s["JR_SUM"] < 1e-13                                               # the root-relative form removes the shift
    for k in ("VPA_SUM", "VPA_SQ", "JPA_SUM", "JPA_SQ"):
        assert s[k] < 1e-13, k
    assert abs(s["VPA_SCALE"] - 1) < 1e-14 and abs(s["JPA_SCALE"] - 1) < 1e-14 and (r["per_joint"][1] < 1e-14).all()
    assert np.allclose(r["per_part"][0], [4 * 13, 3 * 13, 0], atol=1e-12) and np.allclose(r["per_part"][1], [13, 13, 0], atol=1e-13)
    assert not r["bad"]


def test_restatement_rotation_and_scale():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((9, 3))
    R = pc.rotation(rng)
    y = 1.7 * x @ R.T + np.array([0.5, -1.0, 2.0])
    for form in (pr.align_svd, pr.align_horn):
        a = pr.aligned(x, y, form)                                           # estimate x, truth y: s = 1.7
        assert abs(a["scale"] - 1.7) < 1e-14 and a["sum"] < 1e-13 and np.allclose(a["R"], R, atol=1e-14)
        b = pr.aligned(y, x, form)                                           # roles swapped: s = 1 / 1.7, the rotation inverted
        assert abs(b["scale"] - 1 / 1.7) < 1e-14 and b["sum"] < 1e-13 and np.allclose(b["R"], R.T, atol=1e-14)
        assert abs(np.linalg.det(a["R"]) - 1) < 1e-14


def test_restatement_reflection_stays_a_rotation():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((12, 3))
    y = x * np.array([1.0, 1.0, -1.0])                                       # a mirror image: no rotation maps one onto the other
    for form in (pr.align_svd, pr.align_horn):
        a = pr.aligned(x, y, form)
        assert abs(np.linalg.det(a["R"]) - 1) < 1e-14 and a["sum"] > 0.1 and a["sq"] > 0.01
    assert abs(pr.aligned(x, y)["sq"] - pr.aligned(x, y, pr.align_horn)["sq"]) < 1e-13
    # the degenerate estimate: s = 0 and the errors are the truth's distances from its centroid
    one = np.tile(x[:1], (12, 1))
    a = pr.aligned(one, y)
    assert a["scale"] == 0.0 and np.array_equal(a["err"], pr.errors(y - y.mean(0), np.zeros((1, 3))))
    assert pr.aligned(x[:1], y[:1])["sum"] == 0.0
    bad = x.copy()
    bad[3, 1] = np.nan
    assert pr.pair(bad, y)["bad"] and pr.pair(x, y, x[:2], np.array([[0, np.inf, 0], [0, 0, 0.0]]))["bad"] and not pr.pair(x, y)["bad"]


def test_the_two_formulations_agree_on_the_gpu_cases():
    """what the issue measured while the tolerance was chosen: about 1.4e-15 S sqrt(n) between the two CPU forms"""
    worst = 0.0
    for V in pc.V_SIZES + (24, 6890):
        for nm in pc.FAMILIES:
            E, T = pc.family(nm, V, 0)
            assert V == 1 or pc.margin(pr.errors(E, T)) >= pc.ARGMAX_MARGIN
            S = pr.aligned(E, T)["spread"]
            if S > 0:
                worst = max(worst, pr.alignment_tolerance(E, T)["forms"] / (S * np.sqrt(V)))
    assert worst < 1e-14, worst
    for V in (3, 65, 513):
        sizes = {nm: np.bincount(vp, minlength=P) if vp is not None else np.array([V]) for nm, (P, vp) in pc.part_tables(V).items()}
        assert (sizes["sparse24"] == 0).sum() >= 16 and sizes["single"].tolist() == [V - 1, 1] and sizes["all_but_one"].tolist() == [1, 0, V - 1]
        assert len(sizes["p254"]) == 254


def _derive_cpp(V, J, summary, part_sum, part_sizes, tmp_path):
    P = len(part_sizes)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as fh:
        np.array([V, J, P], np.int32).tofile(fh)
        np.ascontiguousarray(summary, np.float64).tofile(fh)
        np.ascontiguousarray(part_sum, np.float64).tofile(fh)
        np.ascontiguousarray(part_sizes, np.int32).tofile(fh)
    r = subprocess.run([DEMO, "derive", inp, outp], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    v = np.fromfile(outp, np.float64)
    assert len(v) == 10 + P
    return v[:10], v[10:]


def test_metrics_equal_the_cpp_derive(tmp_path):
    assert os.path.exists(DEMO), "tests/cpp/pose_error_demo not built (make -C avatar_amd/csrc facade)"
    rng = np.random.default_rng(5)
    keys = ("pve", "pve_rms", "pve_max", "pa_pve", "pa_pve_scale", "mpjpe", "mpjpe_max", "mpjpe_root", "pa_mpjpe", "pa_mpjpe_scale")
    same = lambda a, b: np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)
    for V, J, sizes in ((6890, 24, rng.integers(1, 900, 24)), (7, 3, np.array([4, 0, 3])), (5, 0, np.array([5])), (3, 1, np.array([0, 0, 3, 0]))):
        summary = rng.uniform(0.0, 50.0, 12)
        if J == 0:
            summary[6:] = np.nan                                             # what the device writes without joints
        psum = rng.uniform(0.0, 9.0, len(sizes))
        res = dict(summary=summary[None], per_part=np.stack([psum, psum])[None])
        m = poseerror.metrics(res, V, J, sizes)
        fig, part = _derive_cpp(V, J, summary, psum, sizes, tmp_path)
        assert same(fig, [m[k][0] for k in keys]), (V, J)
        assert same(part, m["pve_part"][0]) and np.array_equal(np.isnan(part), sizes == 0)
        assert m["pve"][0] == summary[0] / V and m["pve_rms"][0] == np.sqrt(summary[1] / V)
        if J == 0:
            assert all(np.isnan(m[k][0]) for k in keys[5:])
        else:
            assert m["mpjpe"][0] == summary[6] / J and m["mpjpe_root"][0] == summary[8] / J and m["pa_mpjpe"][0] == summary[9] / J
    assert poseerror.COLUMNS == pr.COLUMNS and len(poseerror.COLUMNS) == 12 and poseerror.COLUMNS[poseerror.JPA_SCALE] == "JPA_SCALE"


def test_every_declared_function_is_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "avt_poseerr.h")).read()
    declared = re.findall(r"^(?:int|void) (avt_poseerr_\w+)\(", header, re.M)
    assert len(declared) == 9 and sorted(declared) == sorted(poseerror.POSEERR_SYMBOLS)
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    enum = re.search(r"enum \{ (AVT_POSEERR_V_SUM = 0,[^}]*) \}", header).group(1)
    names = [x.strip().split(" ")[0].replace("AVT_POSEERR_", "") for x in enum.split(",")]
    assert tuple(names[:-1]) == poseerror.COLUMNS and names[-1] == "COLS"


def test_argument_refusals_that_need_no_device():
    lib = capi.load_library()
    err = lambda: lib.avt_last_error()
    h = ctypes.c_void_p()
    i32 = ctypes.c_int
    vp = np.array([0, 1, 2, 1], np.int32)
    vpp = capi.ptr(vp, i32)
    for V in (0, -3):
        assert lib.avt_poseerr_create(-1, V, 2, 1, None, 4, ctypes.byref(h)) != 0 and b"V >= 1" in err()
    assert lib.avt_poseerr_create(-1, 4, -1, 1, None, 4, ctypes.byref(h)) != 0 and b"J >= 0" in err()
    for P in (0, -1, 255):
        assert lib.avt_poseerr_create(-1, 4, 2, P, vpp, 4, ctypes.byref(h)) != 0 and b"num_parts" in err()
    assert lib.avt_poseerr_create(-1, 4, 2, 3, None, 4, ctypes.byref(h)) != 0 and b"num_parts == 1" in err()
    assert lib.avt_poseerr_create(-1, 4, 2, 2, vpp, 4, ctypes.byref(h)) != 0 and b"vertex_part[2] = 2" in err()
    neg = np.array([0, -1, 0, 0], np.int32)
    assert lib.avt_poseerr_create(-1, 4, 2, 2, capi.ptr(neg, i32), 4, ctypes.byref(h)) != 0 and b"vertex_part[1] = -1" in err()
    assert lib.avt_poseerr_create(-1, 4, 2, 3, vpp, 0, ctypes.byref(h)) != 0 and b"max_pairs" in err()
    assert lib.avt_poseerr_create(-1, 4, 2, 3, vpp, 4, None) != 0 and b"null" in err()
    assert lib.avt_poseerr_create_for_model(-1, None, 3, None, 4, ctypes.byref(h)) != 0 and b"null" in err()
    for call in (lambda: lib.avt_poseerr_upload(None, 0, 1, None, None), lambda: lib.avt_poseerr_from_ctx(None, 0, None, 1, None),
                 lambda: lib.avt_poseerr_run(None), lambda: lib.avt_poseerr_get(None, None, None, None, None, None, None),
                 lambda: lib.avt_poseerr_part_sizes(None, None, None, None, None), lambda: lib.avt_poseerr_sync(None)):
        assert call() != 0 and b"null" in err()
    lib.avt_poseerr_destroy(None)
    # a host-only handle: checks arguments, keeps counts, refuses to score
    pe = poseerror.PoseError(4, 2, 3, vp, max_pairs=2, device=-1)
    assert (pe.V, pe.J, pe.numParts) == (4, 2, 3) and pe.part_sizes.tolist() == [1, 2, 1]
    assert poseerror.PoseError(5, 0, 1, None, 1, device=-1).part_sizes.tolist() == [5]
    assert poseerror.PoseError(3, 1, 254, [253, 0, 253], 1, device=-1).part_sizes[253] == 2
    E, A = np.zeros((3, 4, 3)), np.zeros((3, 2, 3))
    with pytest.raises(capi.AvtError, match="no result"):
        pe.get()
    with pytest.raises(capi.AvtError, match="created for 2"):
        pe.upload(poseerror.ESTIMATE, E, A)
    with pytest.raises(capi.AvtError, match="no pairs"):
        pe.run()
    with pytest.raises(capi.AvtError, match="joints may be null only if J == 0"):
        pe.upload(poseerror.ESTIMATE, E[:1], None)
    with pytest.raises(capi.AvtError, match="side"):
        pe.upload(2, E[:1], A[:1])
    assert lib.avt_poseerr_upload(pe._h, 0, 0, capi.ptr(E, ctypes.c_double), capi.ptr(A, ctypes.c_double)) != 0 and b"n >= 1" in err()
    assert lib.avt_poseerr_from_ctx(pe._h, 0, None, 1, None) != 0 and b"null context" in err()
    pe.upload(poseerror.ESTIMATE, E[:2], A[:2])
    pe.upload(poseerror.TRUTH, E[:1], A[:1])
    with pytest.raises(capi.AvtError, match="estimate side holds 2 pairs, the truth side 1"):
        pe.run()
    pe.upload(poseerror.TRUTH, E[:2], A[:2])
    with pytest.raises(capi.AvtError, match="host-only"):
        pe.run()
    with pytest.raises(capi.AvtError, match="host-only"):
        pe.sync()
    with pytest.raises(capi.AvtError, match="no result"):
        pe.get()
    with pytest.raises(ValueError):
        pe.upload(poseerror.ESTIMATE, np.zeros((1, 5, 3)), A[:1])
    with pytest.raises(ValueError):
        pe.upload(poseerror.ESTIMATE, E[:1], np.zeros((1, 3, 3)))
    with pytest.raises(ValueError):
        poseerror.PoseError(4, 2, 3, vp[:3], device=-1)
