"""The cases of tests/data_term_cases.py, on the CPU: every case is what its name promises - matched vertices M, data points N, batches, the
batches every evaluation workgroup gets under the strided deal, the matched entries per segment of the moment form's pair lists - and the
oracle alone stays inside every bar tests/test_gpu_data_term_grid.py holds the device to: its two summation orders (aggregate 0 and 1)
agree to 1e-12 in H, g and the cost, and the cost's cancellation factor leaves the 1e-9 of the cost bar a factor 4 in hand."""
import ctypes

import numpy as np
import pytest

import data_term_cases as dc
import fit_models as fm

CASES = [(n, k) for n in dc.MODELS for k in dc.case_keys(n)]
IDS = [f"{n}-{dc.key_id(k)}" for n, k in CASES]
STRIDED = [G for G in dc.GRIDS if G >= dc.STRIDED_MIN]


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def test_per_joint_leaves_the_table_of_fit_models_alone():
    """fit_model without per_joint returns the models it returned before: V = 12 J, and the object the table's cache holds"""
    m = fm.fit_model(9, 4, "star", 3, fm.SEEDS[(9, 4, "star", 3)])
    assert m["v_template"].shape[0] == 12 * 9 == fm.PER_JOINT * 9 and m is fm.case_model((9, 4, "star", 3))
    assert fm.fit_model(9, 4, "star", 3, 2, per_joint=fm.PER_JOINT) is m
    big = fm.fit_model(9, 4, "star", 3, 2, per_joint=232)
    assert big is not m and big["v_template"].shape[0] == 2088 and fm.fit_model(9, 4, "star", 3, 2)["v_template"].shape[0] == 108
    assert np.array_equal(big["kintree_table"], m["kintree_table"])


@pytest.mark.parametrize("name", dc.MODELS)
def test_model_and_full_frame(name):
    """The model has the size its row says and avt_model_create takes it (host side); the full frame's correspondences are those of the
    oracle's optimize(); every vertex of a small model is matched; the batch counts the cases stand on; the moment form where promised."""
    from avatar_amd import capi
    b = dc.base(name)
    om, fr = b["om"], b["frame"]
    lib = capi.load_library()
    desc = (arr := capi.ModelArrays(b["model"])).desc()
    h = ctypes.c_void_p()
    assert lib.avt_model_create(ctypes.byref(desc), ctypes.byref(h)) == 0, lib.avt_last_error()
    dims = [ctypes.c_int() for _ in range(5)]
    assert lib.avt_model_dims(h, *[ctypes.byref(d) for d in dims]) == 0
    lib.avt_model_destroy(h)
    V, J, K, _, P = [d.value for d in dims]
    assert (V, J, K, P) == (om.V, om.J, om.K, 3 + 3 * om.J + om.K)
    assert dc.MOM_OK[name] == (K + 1 <= 16 and 4 * ((P + 4) // 4) // 4 <= 22)          # avt_model.cpp build_moment_tables: V does not enter
    assert np.array_equal(fr["data"], np.rint(fr["data"] * dc.FIX) / dc.FIX) and (fr["labels"] >= 0).all()
    ref = om.optimize(fr["part_map"], fr["num_parts"], fr["data"], fr["labels"], dc.options(fr, icp_iters=1, max_iters_per_icp=0), *fr["start"], aggregate=1)
    assert np.array_equal(ref["corr"], b["corr"])
    nb = (len(b["matched"]) + dc.EVAL_PTS - 1) // dc.EVAL_PTS
    if name == "smpl":
        assert (V, J, K) == (6890, 24, 10) and 64 < nb < 128       # a full frame leaves zero-batch workgroups at G = 127 and 128, a second batch at G = 64
    else:
        Jm, Km, _tree, _nc, per = dc.SMALL[name]
        assert (V, J, K) == (per * Jm, Jm, Km) and len(b["matched"]) == V
    if name == "j9k4":
        assert nb == 131 and dc.deal(nb, 64).max() == 3 and dc.deal(nb - 3, 64).max() == 2        # the third batch of a G = 64 workgroup
    if name == "j45k5":
        assert (P + 1 + 15) // 16 == 9 and 4 * ((P + 4) // 4) // 4 > 22
    if name == "j1k1":
        assert nb == 1026 > dc.ERANGE_CAP > dc.ERANGE_ROOM_HS8 and 4 * ((P + 4) // 4) == 8
    if name == "j2k2":
        pl = dc.pair_lists(b["model"])
        assert {k: len(v) for k, v in pl.items()} == {(0, 0): 1374, (0, 1): 344, (1, 1): 1030}
        assert np.array_equal(pl[(0, 0)][:1030], np.arange(1030)) and np.array_equal(pl[(0, 1)], 1030 + 3 * np.arange(344))


@pytest.mark.parametrize("name,key", CASES, ids=IDS)
def test_case_is_what_its_name_promises(name, key):
    b, c = dc.base(name), dc.case(name, key)
    om, fr = b["om"], c["frame"]
    corr, M, N, nb = c["corr"], c["M"], c["N"], c["nb"]
    # the correspondences the case expects are the oracle's for the case's own data points
    assert np.array_equal(dc._nn(b, c["data"], c["labels"]), corr)
    assert N == len(c["labels"]) == len(c["data"]) and M == len(np.unique(corr[corr >= 0])) and nb == -(-M // 16)
    assert np.array_equal(c["data"][0], b["centre"]) or key[0] == "one"
    cnt = np.bincount(corr[corr >= 0], minlength=om.V)
    for G in STRIDED:             # the strided deal: every batch dealt once, G - nb idle workgroups, the busiest with ceil(nb / G)
        d = dc.deal(nb, G)
        assert d.sum() == nb and (d == 0).sum() == max(0, G - nb) and d.max() == -(-nb // G) and (np.diff(d) <= 0).all()
    if key[0] == "M":
        _, want, how, G = key
        assert M == want and N == int(b["count"][np.unique(corr[corr >= 0])].sum()) + int(corr[0] < 0)
        if how == "first":
            assert np.array_equal(np.unique(corr[corr >= 0]), b["matched"][:M])
        if M <= 16:
            assert nb == (M > 0) and all((dc.deal(nb, g) == 0).sum() == g - nb for g in STRIDED)        # one batch (none): every other workgroup idle
        if M == 17:
            assert nb == 2 and all(list(dc.deal(nb, g)[:3]) == [1, 1, 0] for g in STRIDED)
        if G:
            d = dc.deal(nb, G)
            want_deal = {16 * G - 1: [1] * G, 16 * G: [1] * G, 16 * G + 1: [2] + [1] * (G - 1), 32 * G + 1: [3] + [2] * (G - 1)}[M]
            assert list(d) == want_deal
            assert (M % 16) == {16 * G - 1: 15, 16 * G: 0, 16 * G + 1: 1, 32 * G + 1: 1}[M]          # the last batch: 15, 16 and 1 records
    elif key[0] == "all":
        assert M == len(b["matched"]) and N == len(b["corr"])
    elif key[0] == "mult":
        v = corr[-1]
        assert M == len(b["matched"]) and cnt[v] == key[1] and (corr[-key[1]:] == v).all() and N == len(b["corr"]) - b["count"][v] + key[1]
        d = c["data"][-key[1]:]
        assert np.abs(d - d[0]).max() <= 1e-4 + 2.0 ** -40 and np.array_equal(d, np.rint(d * dc.FIX) / dc.FIX)
        assert key[1] < 3 or len(np.unique(d, axis=0)) == key[1]
    elif key[0] == "one":
        assert (M, N) == (1, 2049) and cnt.max() == 2049 and np.abs(c["data"] - c["data"][0]).max() <= 1e-4 + 2.0 ** -40
    elif key[0] == "N":
        t = dc.tail_of(N)
        assert N == key[1] and (c["labels"][N - t:] == -1).all() and (c["labels"][:N - t] >= 0).all() and M > 16
        for blk in (dc.CONST_ROWS, dc.CONST_MOMENTS):      # the last cost-constant block of either form holds no matched point
            assert (corr[(N - 1) // blk * blk:] < 0).all() or (N - 1) // blk == 0
        assert (N - 1) // dc.CONST_ROWS == {255: 0, 256: 0, 257: 1, 2047: 7, 2048: 7, 2049: 8}[N] and (N - 1) // dc.CONST_MOMENTS == (N == 2049)
    elif key[0] == "seg":
        lst = dc.pair_lists(b["model"])[(0, 0)]
        assert dc.segment_counts(lst, cnt) == key[1] and M == sum(key[1])
        pad = [-(-s // dc.MOM_PAD) * dc.MOM_PAD - s for s in key[1]]           # weight-zero entries k_moments pads a segment with
        assert pad == {(0, 8, 0): [0, 0, 0], (1, 0, 7): [7, 0, 1], (9, 512, 6): [7, 0, 2], (511, 0, 1): [1, 0, 7], (512, 512, 6): [0, 0, 2]}[key[1]]


@pytest.mark.parametrize("name,key", CASES, ids=IDS)
def test_oracle_alone_stays_inside_the_bars(name, key):
    """The oracle's two summation orders agree to 1e-12 in H, g and cost at the state behind its LM step; the cost's cancellation factor is
    under the cap; H has a scale wherever there is a matched vertex."""
    c, s = dc.case(name, key), dc.one_step(name, key)
    assert np.array_equal(s["run"]["corr"], c["corr"])
    (c0, g0, H0, _), (c1, g1, H1, _) = s["rows"], s["agg"]
    if c["M"] == 0:
        assert c0 == 0.0 and not H0.any() and not g0.any() and s["run"]["stats"].accepted_steps == 0
        return
    assert np.abs(H1).max() > 0.0
    eh, eg, ec = _rel(H0, H1), float(np.abs(g0 - g1).max() / max(1.0, np.abs(g1).max())), abs(c0 - c1) / c1
    print(f"DATATERM cpu {name}-{dc.key_id(key)} M {c['M']} N {c['N']} aggregate 0/1 H {eh:.1e} g {eg:.1e} cost {ec:.1e} kappa_c {s['kappa_c']:.2e}")
    assert eh <= 1e-12 and eg <= 1e-12 and ec <= 1e-12, (eh, eg, ec)
    assert 0.0 < s["kappa_c"] <= dc.KAPPA_C_MAX, s["kappa_c"]
    assert s["cost_full"] >= c1 > 0.0


SHORT = dc.short_fit_cases()


@pytest.mark.parametrize("name,key,G", SHORT, ids=[f"{n}-{dc.key_id(k)}" for n, k, _ in SHORT])
def test_short_fits_are_fit_to_compare(name, key, G):
    """The fits of tests/test_gpu_data_term_grid.py d (2 ICP x 3 GN iterations): the same accept / reject sequence with both summation orders,
    and lambda determined by the fit, not by the last bits of the costs (fit_models.replay_fit, KAPPA_MAX)."""
    b, c = dc.base(name), dc.case(name, key)
    om, fr = b["om"], c["frame"]
    opt = dc.options(fr, **dc.SHORT_FIT)
    fits = [om.optimize(fr["part_map"], fr["num_parts"], fr["data"], fr["labels"], opt, *fr["start"], aggregate=a) for a in (0, 1)]
    assert np.array_equal(fits[0]["trace_acc"], fits[1]["trace_acc"])
    r = fm.replay_fit(om, fr, dc.SHORT_FIT["max_iters_per_icp"])
    assert r["kappa"] <= fm.KAPPA_MAX, r["kappa"]
    assert abs(r["lam"] / fits[1]["stats"].lambda_ - 1.0) <= r["kappa"] * 64 * 2.0 ** -53 + 1e-15
    assert G is None or G in dc.GRIDS
