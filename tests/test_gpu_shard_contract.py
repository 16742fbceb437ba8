"""The contract of a shard handle (avatar_amd/csrc/avt_shard.cpp, include/avt_shard.h) as a caller sees it, on the smallest inputs at which
its host paths can go wrong: the models (9, 4, "star") and (5, 16, "star") of tests/fit_models.py, contexts of max_points = 512, frames of
fit_frame.  Loop-back ranks are threads of this process, the RCCL handle has one rank, the shared-memory ranks are two fresh processes.

  1  every refusal of every entry point, to its text: null and range checks, "nothing was gathered", the collective rejections of the
     scatter on every rank, the refusals of the three creates
  2  loop-back scatter, optimize and gather at W in {1, 2, 3, 8} and B in {1, W - 1, W, W + 1, 2 W + 1}: every rank's resident frames are
     its share, every rank's gathered rows are the bits of plain contexts holding each rank's share
  3  the gather through the shard's own send block (a context with fewer frame slots than the rank block has rows)
  4  avt_shard_set_self_exchange(1): the same bits as with it off
  5  the gathered block is a snapshot of the call the gather was enqueued behind
  6  a rank that never arrives fails its peer after the time-out, and a fresh group under the same name works
  7  the shared-memory transport at a message that ends 16 bytes under a chunk's end and one that needs 8 bytes of a second chunk"""
import ctypes as C
import os
import subprocess
import sys
import threading
import time
import uuid

import numpy as np
import pytest

import fit_models as fm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_POINTS = 512
MOM, ROWS_ONLY = (9, 4, "star"), (5, 16, "star")
NFRAMES = 17                      # the largest batch: 2 W + 1 at W = 8
TIMEOUT_TEXT = "loop-back transport: a rank did not arrive (time-out); the group is broken"
# (W, B) -> the frames of the batch that have no points: one batch with an empty frame, one with a rank all of whose frames are empty
EMPTY = {(2, 5): (2,), (3, 7): (1, 4)}
WB = [(W, B) for W in (1, 2, 3, 8) for B in sorted({1, W - 1, W, W + 1, 2 * W + 1}) if B > 0]


@pytest.fixture(autouse=True)
def _timeout_of_new_groups(monkeypatch):
    monkeypatch.setenv("AVT_SHARD_LOOPBACK_TIMEOUT_S", "20")      # read once, when a group is created


class Rig:
    """a model on the device, its oracle and the frames of the largest batch (frame f without its last f % 3 points: ragged counts)"""

    def __init__(self, key):
        from avatar_amd import api, capi
        from oracle import oracle as orc
        self.key = key
        self.m = fm.fit_model(*key)
        self.gm = api.AvatarModel(self.m)
        self.om = orc.OracleModel(self.m)
        self.J, self.K, self.V = self.om.J, self.om.K, self.om.V
        self.frs = []
        for f in range(NFRAMES):
            fr = fm.fit_frame(self.m, self.om, f)
            n = self.V - f % 3
            self.frs.append(dict(fr, data=np.ascontiguousarray(fr["data"][:n]), labels=np.ascontiguousarray(fr["labels"][:n])))
        self.lib = capi.load_library()
        self.opt = fm.options(self.frs[0], icp_iters=2, max_iters_per_icp=3)
        self._plain = {}

    def ctx(self, max_frames, max_points=MAX_POINTS, model=None):
        from avatar_amd import api
        fr = self.frs[0]
        return api.Context(model or self.gm, fr["num_parts"], fr["part_map"], max_points, max_frames, device=0)

    def batch(self, B, empty=()):
        """(datas, labels, p, q, w) of the first B frames, those of `empty` without points"""
        frs = self.frs[:B]
        datas = [fr["data"] if f not in empty else np.zeros((0, 3)) for f, fr in enumerate(frs)]
        labels = [fr["labels"] if f not in empty else np.zeros(0, np.int32) for f, fr in enumerate(frs)]
        return (datas, labels) + tuple(np.stack([fr["start"][k] for fr in frs]) for k in range(3))

    def plain(self, W, B, empty=(), again=False):
        """the yard-stick: every rank's share fitted by one ordinary context holding exactly those frames (results are bit-reproducible for a
        launch shape); rows in global frame order.  again: a second optimize() on the resident states behind the first (the warm restart)"""
        from avatar_amd import shard
        k = (W, B, tuple(empty), again)
        if k not in self._plain:
            datas, labels, p0, q0, w0 = self.batch(B, empty)
            per = (B + W - 1) // W
            p, q, w, st = np.empty((B, 3)), np.empty((B, self.J, 4)), np.empty((B, self.K)), [None] * B
            for r in range(W):
                mine = shard.frames_of_rank(B, r, W)
                if not mine:
                    continue
                c = self.ctx(per)
                c.frames_upload([datas[f] for f in mine], [labels[f] for f in mine])
                c.state_upload(p0[mine], q0[mine], w0[mine])
                c.optimize_resident(self.opt)
                if again:
                    c.optimize_resident(self.opt)
                pr, qr, wr, sr = c.state_download()
                p[mine], q[mine], w[mine] = pr, qr, wr
                for i, f in enumerate(mine):
                    st[f] = sr[i]
            self._plain[k] = (p, q, w, _stats(st))
            for a in self._plain[k]:
                a.setflags(write=False)
        return self._plain[k]

    def err(self):
        return self.lib.avt_last_error().decode()


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(key):
        if key not in made:
            made[key] = Rig(key)
        return made[key]
    return get


@pytest.fixture(scope="module")
def rccl_shard():
    """the one-rank RCCL handle (RCCL refuses two ranks on one device)"""
    from avatar_amd import capi, shard
    lib = capi.load_library()
    buf = C.create_string_buffer(shard.ID_BYTES)
    assert lib.avt_shard_unique_id(buf) == 0, lib.avt_last_error()
    s = shard.Shard(0, 0, 1, buf.raw)
    yield s
    s.close()


def _stats(st):
    return np.array([[s.initial_cost, s.final_cost, s.lambda_, s.num_correspondences, s.matched_model_points, s.gn_iterations, s.accepted_steps] for s in st])


def _same(got, want):
    """the entries of (p, q, w, stats) that differ (NaN equals NaN: the same bits are wanted)"""
    return [n for n, a, b in zip("pqws", got, want) if not np.array_equal(np.asarray(a).reshape(np.shape(b)), b, equal_nan=True)]


def _run_ranks(W, fn, limit=120):
    """fn(rank) on W threads; the results, the first exception re-raised after all threads ended"""
    out, err = [None] * W, [None] * W

    def body(r):
        try:
            out[r] = fn(r)
        except BaseException as e:      # noqa: BLE001 - re-raised below
            err[r] = e
    th = [threading.Thread(target=body, args=(r,)) for r in range(W)]
    for t in th:
        t.start()
    for t in th:
        t.join(limit)
    assert not any(t.is_alive() for t in th), "a rank hangs in an exchange"
    for e in err:
        if e is not None:
            raise e
    return out


def _group():
    return "c-" + uuid.uuid4().hex


def _scatter(sh, ctx, rig, B, empty=(), root=0):
    """the scatter as rank sh.rank calls it, then: this rank's resident frames are its share of the batch, bit for bit"""
    from avatar_amd import shard
    datas, labels, p0, q0, w0 = rig.batch(B, empty)
    if sh.rank == root:
        sh.scatter_frames(ctx, B, datas, labels, p0, q0, w0, root=root)
    else:
        sh.scatter_frames(ctx, B, root=root)
    mine = shard.frames_of_rank(B, sh.rank, sh.world)
    ctx._N = np.array([len(labels[f]) for f in mine], np.int32)
    for i, f in enumerate(mine):
        d, l = ctx.frame_download(i)
        assert np.array_equal(d, datas[f]) and np.array_equal(l, labels[f]), f"rank {sh.rank}: resident frame {i} is not frame {f} of the batch"
    return mine


def _gathered(res):
    p, q, w, st = res
    return p, q, w, _stats(st)


def _loopback(rig, W, B, empty=(), max_frames=None, self_exchange=False, snapshot=False, root=0):
    """W loop-back ranks: create, scatter, optimize, gather (snapshot: enqueue, optimize again, download), barrier.  Every rank's rows."""
    from avatar_amd import shard
    group, per = _group(), (B + W - 1) // W

    def rank_main(r):
        sh = shard.Shard(0, r, W, loopback_group=group)
        assert sh.backend == "loop-back (threads of one process), group " + group and (sh.world, sh.rank) == (W, r)
        assert (rig.lib.avt_shard_world(sh.h), rig.lib.avt_shard_rank(sh.h)) == (W, r)
        if self_exchange:
            sh.set_self_exchange(True)
        ctx = rig.ctx(max_frames(r) if max_frames else per)
        mine = _scatter(sh, ctx, rig, B, empty, root)
        if mine:
            ctx.optimize_resident(rig.opt)
        if snapshot:
            sh.gather_enqueue(ctx, B)
            if mine:
                ctx.optimize_resident(rig.opt)
            res = sh.gather_download(ctx, B)
        else:
            res = sh.gather_results(ctx, B)
        sh.gather_wait()
        sh.barrier(ctx)
        sh.barrier()
        sh.close()
        return _gathered(res)
    return _run_ranks(W, rank_main)


# ---- 2. loop-back scatter, optimize and gather --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", [MOM, ROWS_ONLY], ids=["J9K4", "J5K16"])
@pytest.mark.parametrize("W,B", WB)
def test_loopback_scatter_optimize_gather_gives_the_bits_of_plain_contexts(rigs, key, W, B):
    rig = rigs(key)
    empty = EMPTY.get((W, B), ())
    want = rig.plain(W, B, empty)
    for r, got in enumerate(_loopback(rig, W, B, empty)):
        assert _same(got, want) == [], f"rank {r} of {W}, {B} frames"


def test_loopback_broadcast_model_and_a_root_other_than_rank_0(rigs):
    """the model every rank builds from the broadcast bytes fits like the one built from the arrays, and the scatter's root may be any rank"""
    from avatar_amd import api, shard
    rig = rigs(MOM)
    W, B, root, group = 3, 4, 2, _group()
    want = rig.plain(W, B)

    def rank_main(r):
        sh = shard.Shard(0, r, W, loopback_group=group)
        h = sh.broadcast_model(rig.gm.arrays if r == root else None, root=root)
        ctx = rig.ctx(2, model=api.AvatarModel(rig.m, handle=h))
        _scatter(sh, ctx, rig, B, root=root)
        ctx.optimize_resident(rig.opt)
        res = _gathered(sh.gather_results(ctx, B))
        sh.close()
        return res
    for r, got in enumerate(_run_ranks(W, rank_main)):
        assert _same(got, want) == [], f"rank {r}"


# ---- 3. the d_send path of the gather ------------------------------------------------------------------------------------------------------

def test_gather_through_the_send_block_when_the_context_has_fewer_slots_than_the_rank_block(rigs):
    """B = 5 over W = 2: a rank block has 3 rows; rank 1 owns 2 frames and its context has 2 slots, so its result records cannot be the send
    block.  The rows are those of the other path."""
    rig = rigs(MOM)
    want = rig.plain(2, 5)
    for r, got in enumerate(_loopback(rig, 2, 5, max_frames=lambda r: 2 if r == 1 else 3)):
        assert _same(got, want) == [], f"rank {r}"


# ---- 4. avt_shard_set_self_exchange ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,B", [(1, 3), (2, 5)])
def test_self_exchange_on_loopback_gives_the_same_bits(rigs, W, B):
    rig = rigs(MOM)
    want = rig.plain(W, B)
    for r, got in enumerate(_loopback(rig, W, B, self_exchange=True)):
        assert _same(got, want) == [], f"rank {r}"
    if W == 2:      # ... and with a root that is not rank 0 sending its share to itself
        for r, got in enumerate(_loopback(rig, W, B, self_exchange=True, root=1)):
            assert _same(got, want) == [], f"rank {r}, root 1"


@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
def test_self_exchange_on_the_rccl_handle_gives_the_same_bits(rigs, rccl_shard, on):
    rig = rigs(MOM)
    B = 3
    want = rig.plain(1, B)
    assert rccl_shard.backend.startswith("rccl ") and "librccl" in rccl_shard.backend
    rccl_shard.set_self_exchange(on)
    try:
        ctx = rig.ctx(B)
        _scatter(rccl_shard, ctx, rig, B)
        ctx.optimize_resident(rig.opt)
        assert _same(_gathered(rccl_shard.gather_results(ctx, B)), want) == []
        rccl_shard.barrier(ctx)
        rccl_shard.barrier()
    finally:
        rccl_shard.set_self_exchange(False)


# ---- 5. the gather is a snapshot ------------------------------------------------------------------------------------------------------------

def test_gather_is_a_snapshot_on_loopback(rigs):
    rig = rigs(MOM)
    want, later = rig.plain(2, 5), rig.plain(2, 5, again=True)
    assert _same(later, want) != [], "the second optimize() moves nothing: the case shows nothing"
    for r, got in enumerate(_loopback(rig, 2, 5, snapshot=True)):
        assert _same(got, want) == [], f"rank {r}"


@pytest.mark.parametrize("on", [False, True], ids=["direct", "all-gather"])
def test_gather_is_a_snapshot_on_the_rccl_handle(rigs, rccl_shard, on):
    rig = rigs(MOM)
    B = 3
    want, later = rig.plain(1, B), rig.plain(1, B, again=True)
    rccl_shard.set_self_exchange(on)
    try:
        ctx = rig.ctx(B)
        _scatter(rccl_shard, ctx, rig, B)
        ctx.optimize_resident(rig.opt)
        rccl_shard.gather_enqueue(ctx, B)
        ctx.optimize_resident(rig.opt)
        assert _same(_gathered(rccl_shard.gather_download(ctx, B)), want) == []
        ctx._F = B
        p, q, w, st = ctx.state_download()
        assert _same((p, q, w, _stats(st)), later) == []
    finally:
        rccl_shard.set_self_exchange(False)


# ---- 1. refusals --------------------------------------------------------------------------------------------------------------------------------

def _refused(rig, rc, text, status=1):
    assert rc == status and rig.err() == text, f"returned {rc} with {rig.err()!r}, wanted {status} with {text!r}"


def test_null_and_range_refusals_of_every_entry_point(rigs, rccl_shard):
    from avatar_amd.capi import Stats, dptr, iptr
    rig = rigs(MOM)
    lib, s = rig.lib, rccl_shard.h
    ctx = rig.ctx(2)
    c, out, n = ctx.h, C.c_void_p(), C.c_size_t()
    desc = rig.gm.arrays.desc()
    d, i, st = dptr(np.zeros(4096)), iptr(np.zeros(4096, np.int32)), (Stats * 4)()
    assert lib.avt_shard_rank(None) == -1 and lib.avt_shard_world(None) == 0 and lib.avt_shard_backend(None) == b""
    lib.avt_shard_destroy(None)
    for call, text in (
            (lambda: lib.avt_model_pack_size(None, C.byref(n)), "avt_model_pack_size: bad model description"),
            (lambda: lib.avt_model_pack_size(C.byref(desc), None), "avt_model_pack_size: bad model description"),
            (lambda: lib.avt_model_pack(None, d, 1 << 20), "avt_model_pack: bad model description"),
            (lambda: lib.avt_model_pack(C.byref(desc), None, 1 << 20), "avt_model_pack: bad model description"),
            (lambda: lib.avt_model_pack(C.byref(desc), d, 64), "avt_model_pack: buffer too small"),
            (lambda: lib.avt_model_unpack(None, 1 << 20, C.byref(out)), "avt_model_unpack: block too small"),
            (lambda: lib.avt_model_unpack(d, 1 << 10, None), "avt_model_unpack: block too small"),
            (lambda: lib.avt_model_unpack(d, 8, C.byref(out)), "avt_model_unpack: block too small"),
            (lambda: lib.avt_model_unpack(d, 1 << 10, C.byref(out)), "avt_model_unpack: not a packed model (magic / version / size mismatch)"),
            (lambda: lib.avt_shard_unique_id(None), "avt_shard_unique_id: null argument"),
            (lambda: lib.avt_shard_broadcast_model(None, 0, C.byref(desc), C.byref(out)), "avt_shard_broadcast_model: bad argument"),
            (lambda: lib.avt_shard_broadcast_model(s, 0, C.byref(desc), None), "avt_shard_broadcast_model: bad argument"),
            (lambda: lib.avt_shard_broadcast_model(s, -1, C.byref(desc), C.byref(out)), "avt_shard_broadcast_model: bad argument"),
            (lambda: lib.avt_shard_broadcast_model(s, 1, C.byref(desc), C.byref(out)), "avt_shard_broadcast_model: bad argument"),
            (lambda: lib.avt_shard_broadcast_model(s, 0, None, C.byref(out)), "avt_model_pack_size: bad model description"),
            (lambda: lib.avt_shard_scatter_frames(None, c, 0, 1, d, i, i, d, d, d), "avt_shard_scatter_frames: bad argument"),
            (lambda: lib.avt_shard_scatter_frames(s, None, 0, 1, d, i, i, d, d, d), "avt_shard_scatter_frames: bad argument"),
            (lambda: lib.avt_shard_scatter_frames(s, c, -1, 1, d, i, i, d, d, d), "avt_shard_scatter_frames: bad argument"),
            (lambda: lib.avt_shard_scatter_frames(s, c, 1, 1, d, i, i, d, d, d), "avt_shard_scatter_frames: bad argument"),
            (lambda: lib.avt_shard_scatter_frames(s, c, 0, 0, d, i, i, d, d, d), "avt_shard_scatter_frames: bad argument"),
            (lambda: lib.avt_shard_scatter_frames(s, c, 0, -3, d, i, i, d, d, d), "avt_shard_scatter_frames: bad argument"),
            (lambda: lib.avt_shard_gather_enqueue(None, c, 1), "avt_shard_gather_enqueue: bad argument"),
            (lambda: lib.avt_shard_gather_enqueue(s, None, 1), "avt_shard_gather_enqueue: bad argument"),
            (lambda: lib.avt_shard_gather_enqueue(s, c, 0), "avt_shard_gather_enqueue: bad argument"),
            (lambda: lib.avt_shard_gather_download(None, c, 1, d, d, d, st), "avt_shard_gather_download: bad argument"),
            (lambda: lib.avt_shard_gather_download(s, None, 1, d, d, d, st), "avt_shard_gather_download: bad argument"),
            (lambda: lib.avt_shard_gather_download(s, c, 0, d, d, d, st), "avt_shard_gather_download: bad argument"),
            (lambda: lib.avt_shard_gather_results(None, c, 1, d, d, d, st), "avt_shard_gather_enqueue: bad argument"),
            (lambda: lib.avt_shard_gather_results(s, None, 1, d, d, d, st), "avt_shard_gather_enqueue: bad argument"),
            (lambda: lib.avt_shard_gather_results(s, c, 0, d, d, d, st), "avt_shard_gather_enqueue: bad argument"),
            (lambda: lib.avt_shard_gather_wait(None), "avt_shard_gather_wait: null argument"),
            (lambda: lib.avt_shard_set_self_exchange(None, 1), "avt_shard_set_self_exchange: null argument"),
            (lambda: lib.avt_shard_barrier(None, c), "avt_shard_barrier: null argument"),
            (lambda: lib.avt_shard_barrier(None, None), "avt_shard_barrier: null argument")):
        _refused(rig, call(), text)
    # a description with a required array missing
    bad = rig.gm.arrays.desc()
    bad.jreg_val = None
    assert lib.avt_model_pack_size(C.byref(bad), C.byref(n)) == 0
    buf = C.create_string_buffer(n.value)
    _refused(rig, lib.avt_model_pack(C.byref(bad), buf, n), "avt_model_pack: a required array of the model description is NULL")


def test_nothing_was_gathered_and_a_context_without_its_share(rigs):
    """a handle that has gathered nothing refuses the download; a gather over a context that does not hold the rank's share reports it at once,
    and the download then names the frame and the rank whose rows are faulty (status 3)"""
    from avatar_amd import shard
    from avatar_amd.capi import Stats, dptr
    rig = rigs(MOM)
    lib = rig.lib
    sh = shard.Shard(0, 0, 1, loopback_group=_group())
    try:
        ctx = rig.ctx(2)
        d, st = dptr(np.zeros(4096)), (Stats * 4)()
        assert lib.avt_shard_gather_wait(sh.h) == 0                   # nothing enqueued: nothing to wait for
        _refused(rig, lib.avt_shard_gather_download(sh.h, ctx.h, 2, d, d, d, st), "avt_shard_gather_download: nothing was gathered")
        _refused(rig, lib.avt_shard_gather_enqueue(sh.h, ctx.h, 2),
                 "avt_shard_gather_enqueue: resident frames differ from this rank's share of the batch (its rows were gathered as faulty)")
        _refused(rig, lib.avt_shard_gather_download(sh.h, ctx.h, 2, d, d, d, st),
                 "avt_shard_gather_download: frame 0 carries a device fault (rank 0); its result is not valid", status=3)
        _refused(rig, lib.avt_shard_gather_download(sh.h, ctx.h, 4, d, d, d, st), "avt_shard_gather_download: nothing was gathered")   # a larger batch than was gathered
        # the same handle and context then serve a sound batch
        _scatter(sh, ctx, rig, 2)
        ctx.optimize_resident(rig.opt)
        assert _same(_gathered(sh.gather_results(ctx, 2)), rig.plain(1, 2)) == []
    finally:
        sh.close()


def _raw_scatter(rig, sh, ctx, B, arrays, root=0):
    """avt_shard_scatter_frames through ctypes: (status, text).  arrays: (data, labels, offs, p, q, w) or None"""
    from avatar_amd.capi import dptr, iptr
    if arrays is None:
        args = (None,) * 6
    else:
        data, lab, offs, p, q, w = arrays
        args = (dptr(data) if data is not None else None, iptr(lab), iptr(offs), dptr(p), dptr(q), dptr(w))
    rc = rig.lib.avt_shard_scatter_frames(sh.h, ctx.h, root, B, *args)
    return rc, rig.err() if rc else ""      # (the last error is per thread)


def _flat(rig, B):
    datas, labels, p0, q0, w0 = rig.batch(B)
    offs = np.zeros(B + 1, np.int32)
    offs[1:] = np.cumsum([len(l) for l in labels])
    return [np.ascontiguousarray(np.concatenate(datas)), np.ascontiguousarray(np.concatenate(labels)), offs,
            np.ascontiguousarray(p0), np.ascontiguousarray(q0.reshape(B, -1)), np.ascontiguousarray(w0)]


ROOT_REJECTED = "avt_shard_scatter_frames: the root rank rejected the batch"
SHARE = "avt_shard_scatter_frames: this rank's share exceeds the context's max_frames"
POINTS = "avt_shard_scatter_frames: a frame has more points than max_points_per_frame"


def _peer(r):
    return f"avt_shard_scatter_frames: rank {r} rejected the batch; nothing was exchanged"


# what is wrong -> (how the root's arrays are spoilt, max_frames of rank r, max_points of rank r, the text on rank r); W = 3, B = 6, root 0
def _no_data(a): a[0] = None
def _not_monotone(a): a[2][3] = a[2][2] - 1
COLLECTIVE = {
    "root without its arrays": (_no_data, lambda r: 2, lambda r: MAX_POINTS,
                                lambda r: "avt_shard_scatter_frames: root needs all host arrays" if r == 0 else ROOT_REJECTED),
    "offsets not monotone": (_not_monotone, lambda r: 2, lambda r: MAX_POINTS,
                             lambda r: "avt_shard_scatter_frames: frame_offsets not monotone" if r == 0 else ROOT_REJECTED),
    "a share above max_frames": (None, lambda r: 2 if r == 0 else 1, lambda r: MAX_POINTS, lambda r: _peer(1) if r == 0 else SHARE),
    "a share above max_frames on the last rank": (None, lambda r: 1 if r == 2 else 2, lambda r: MAX_POINTS, lambda r: SHARE if r == 2 else _peer(2)),
    "a frame above max_points": (None, lambda r: 2, lambda r: 64 if r == 1 else MAX_POINTS, lambda r: POINTS if r == 1 else _peer(1)),
    "a frame above max_points on the root": (None, lambda r: 2, lambda r: 64 if r == 0 else MAX_POINTS, lambda r: POINTS if r == 0 else _peer(0)),
}


@pytest.mark.parametrize("what", list(COLLECTIVE))
def test_collective_rejections_of_the_scatter_on_every_rank(rigs, what):
    """what one rank alone can see is agreed on before any cloud moves: every rank returns 1 with its own text, the peers' names the lowest
    bad rank, no context holds frames afterwards, and the same handles then scatter a sound batch"""
    from avatar_amd import shard
    rig = rigs(MOM)
    spoil, max_frames, max_points, text = COLLECTIVE[what]
    W, B, group = 3, 6, _group()

    def rank_main(r):
        sh = shard.Shard(0, r, W, loopback_group=group)
        ctx = rig.ctx(max_frames(r), max_points(r))
        arrays = None
        if r == 0:
            arrays = _flat(rig, B)
            if spoil:
                spoil(arrays)
        got = _raw_scatter(rig, sh, ctx, B, arrays)
        opt_rc = rig.lib.avt_optimize_resident(ctx.h, C.byref(rig.opt))
        opt_text = rig.err()
        good = rig.ctx(2)
        _scatter(sh, good, rig, B)
        sh.close()
        return got, (opt_rc, opt_text)
    for r, (got, after) in enumerate(_run_ranks(W, rank_main)):
        assert got == (1, text(r)), f"rank {r}"
        assert after[0] == 1 and "no frames resident" in after[1], f"rank {r}: {after}"


def test_refusals_of_the_three_creates(rigs):
    from avatar_amd import shard
    rig = rigs(MOM)
    lib, out = rig.lib, C.c_void_p()
    uid = C.create_string_buffer(shard.ID_BYTES)
    assert lib.avt_shard_unique_id(uid) == 0, rig.err()
    uid = uid.raw
    g = _group().encode()
    for name, fn, rv in (("avt_shard_create", lib.avt_shard_create, uid), ("avt_shard_create_loopback", lib.avt_shard_create_loopback, g),
                         ("avt_shard_create_shm", lib.avt_shard_create_shm, os.urandom(shard.ID_BYTES))):
        for args in ((0, 0, 1, None, C.byref(out)), (0, 0, 1, rv, None), (0, 0, 0, rv, C.byref(out)), (0, 0, -2, rv, C.byref(out)),
                     (0, -1, 2, rv, C.byref(out)), (0, 2, 2, rv, C.byref(out))):
            _refused(rig, fn(*args), name + ": bad argument")
        for device in (-1, 4096):
            _refused(rig, fn(device, 0, 1, rv, C.byref(out)), name + ": device index out of range", status=2)
        assert not out.value
    _refused(rig, lib.avt_shard_create_shm(0, 0, 65, os.urandom(shard.ID_BYTES), C.byref(out)), "avt_shard_create_shm: bad argument")
    _refused(rig, lib.avt_shard_create_shm(0, 64, 65, os.urandom(shard.ID_BYTES), C.byref(out)), "avt_shard_create_shm: bad argument")
    # the group registry of the loop-back create
    a = shard.Shard(0, 0, 2, loopback_group=g.decode())
    try:
        _refused(rig, lib.avt_shard_create_loopback(0, 0, 3, g, C.byref(out)), "avt_shard_create_loopback: group exists with another world size, or is full")
        _refused(rig, lib.avt_shard_create_loopback(0, 0, 2, g, C.byref(out)), "avt_shard_create_loopback: this rank is already a member of the group")
        b = shard.Shard(0, 1, 2, loopback_group=g.decode())
        try:
            for r in (0, 1):
                _refused(rig, lib.avt_shard_create_loopback(0, r, 2, g, C.byref(out)), "avt_shard_create_loopback: group exists with another world size, or is full")
        finally:
            b.close()
        c = shard.Shard(0, 1, 2, loopback_group=g.decode())      # a rank that left may come again
        c.close()
    finally:
        a.close()
    assert not out.value
    shard.Shard(0, 0, 3, loopback_group=g.decode()).close()       # the last member took the group with it: the name is free for another shape


# ---- 6. a rank that never arrives ---------------------------------------------------------------------------------------------------------------

def test_a_rank_that_never_arrives_fails_its_peer_after_the_time_out(rigs, monkeypatch):
    """W = 2, time-out 2 s, rank 1 makes no call: rank 0's model broadcast returns 1 with the time-out text after one time-out (not at once, and
    not after a second wait: under 4 s), the group stays broken for its members, and a fresh group under the same name works"""
    from avatar_amd import api, shard
    rig = rigs(MOM)
    monkeypatch.setenv("AVT_SHARD_LOOPBACK_TIMEOUT_S", "2")
    group = _group()
    a, b = shard.Shard(0, 0, 2, loopback_group=group), shard.Shard(0, 1, 2, loopback_group=group)
    try:
        desc, out = rig.gm.arrays.desc(), C.c_void_p()
        t0 = time.monotonic()
        rc = rig.lib.avt_shard_broadcast_model(a.h, 0, C.byref(desc), C.byref(out))
        dt = time.monotonic() - t0
        assert rc == 1 and rig.err().endswith(": " + TIMEOUT_TEXT), (rc, rig.err())
        assert 1.9 <= dt < 4.0, f"the call returned after {dt:.2f} s"
        t0 = time.monotonic()      # broken: the late rank is refused at once
        rc = rig.lib.avt_shard_broadcast_model(b.h, 0, None, C.byref(out))
        assert rc == 1 and rig.err().endswith(": " + TIMEOUT_TEXT) and time.monotonic() - t0 < 1.0, (rc, rig.err())
        monkeypatch.setenv("AVT_SHARD_LOOPBACK_TIMEOUT_S", "20")

        def rank_main(r):
            sh = shard.Shard(0, r, 2, loopback_group=group)
            h = sh.broadcast_model(rig.gm.arrays if r == 0 else None, root=0)
            api.AvatarModel(rig.m, handle=h)
            sh.barrier()
            sh.close()
            return True
        assert _run_ranks(2, rank_main) == [True, True]
    finally:
        a.close(); b.close()


# ---- 7. shared memory across a chunk boundary ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rank1_points", [43690, 43691], ids=["one-chunk-1048560-bytes", "second-chunk-of-8-bytes"])
def test_shared_memory_ranks_at_a_chunk_boundary(rank1_points):
    env = dict(os.environ, AVT_SHARD_LOOPBACK_TIMEOUT_S="20")
    script = os.path.join(ROOT, "tests", "shard_shm_rank.py")
    uid = os.urandom(128).hex()
    ranks = [subprocess.Popen([sys.executable, script, str(r), uid, str(rank1_points)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT)
             for r in (0, 1)]
    outs = []
    try:
        for p in ranks:
            outs.append(p.communicate(timeout=120))
    finally:
        for p in ranks:
            if p.poll() is None:
                p.kill()
    for r, (p, (so, se)) in enumerate(zip(ranks, outs)):
        assert p.returncode == 0, f"rank {r} ended with {p.returncode}\n{so[-500:]}\n{se[-2000:]}"
    assert f"rank 0: 161 points in 6 frames, verdict ok" in outs[0][0]
    assert f"rank 1: {rank1_points} points in 6 frames, verdict ok" in outs[1][0]
