"""MultiFrameTracker's protocol without a GPU: the budget vector and the re-installed streams of every step are what S separate
FrameTracker decisions give (stub context; no fitting happens)."""
import numpy as np
import pytest

from avatar_amd.tracker import FrameTracker, MultiFrameTracker

J, K, PARTS, H, W = 24, 10, 24, 48, 48
POLICY = dict(interval=2, frame_icp_iters=3, reinit_icp_iters=5, reinit_cnz=40, initial_per_part_cnz=8, initial_icp_iters=6)


def _frame(kind, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.0, 1.0, (H, W, 3)).astype(np.float32)
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mask = ((rr // 2 * (W // 2) + cc // 2) % PARTS).astype(np.uint8)     # every part on the interval-2 grid, 24 points each
    if kind == "empty":
        mask[:] = 255
    elif kind == "sparse":                    # 5 points at interval 2: below reinit_cnz // 4
        keep = np.zeros_like(mask, bool)
        keep[0, 0:10:2] = True
        mask[~keep] = 255
    elif kind == "missing":                   # part 7 absent: only the first fit asks for every part
        mask[mask == 7] = 255
    return xyz, mask, None


# stream -> the kind of frame it sees at each of the six steps
SCRIPT = [
    ["full", "full", "full", "full", "full", "full"],
    ["empty", "full", "full", "empty", "full", "full"],
    ["missing", "full", "missing", "sparse", "full", "full"],
    ["full", "sparse", "full", "full", "empty", "full"],
]


class _Ava:
    def __init__(self):
        self.p = np.zeros(3); self.w = np.zeros(K); self.r = np.tile(np.eye(3), (J, 1, 1))
        self.model = type("M", (), {"numJoints": staticmethod(lambda: J)})()
        self.updates = 0

    def update(self):
        self.updates += 1


class _Opt:
    """The attributes FrameTracker reads of an AvatarOptimizer; optimize() records its ICP budget."""
    numParts = PARTS

    def __init__(self):
        self.ava = _Ava()
        self.calls = []

    def optimize(self, data, labels, icp_iters, num_threads):
        self.calls.append(icp_iters)


class _Ctx:
    """The Context calls MultiFrameTracker makes, recorded; the device state is a host copy."""
    num_parts = PARTS
    model = type("M", (), {"numJoints": staticmethod(lambda: J), "numShapeKeys": staticmethod(lambda: K)})()

    def __init__(self):
        self.log = []
        self.p = self.q = self.w = None

    def frames_upload(self, datas, labels):
        self.log.append(("frames", [len(l) for l in labels]))

    def state_upload(self, p, q, w):
        self.p, self.q, self.w = np.array(p), np.array(q), np.array(w)
        self.log.append(("state", None))

    def state_upload_frames(self, frames, p, q, w):
        for i, f in enumerate(frames):
            self.p[f], self.q[f], self.w[f] = p[i], q[i], w[i]
        self.log.append(("state_frames", list(frames)))

    def optimize_resident_budgets(self, opt, budgets):
        self.log.append(("fit", (opt.icp_iters, list(np.asarray(budgets)))))

    def state_download(self):
        return self.p.copy(), self.q.copy(), self.w.copy(), [None] * len(self.p)


def _reference():
    """Per step: the budget vector (0 = lost) and the reinitialised streams of four separate FrameTrackers."""
    trackers = []
    for _ in SCRIPT:
        tr = FrameTracker(_Opt(), **{k: v for k, v in POLICY.items()})
        trackers.append(tr)
    steps = []
    for t in range(6):
        budgets, reinit = [], []
        for s, tr in enumerate(trackers):
            n_calls, n_upd = len(tr.opt.calls), tr.ava.updates
            fitted = tr.process(*_frame(SCRIPT[s][t], 100 * s + t))
            budgets.append(tr.opt.calls[-1] if fitted else 0)
            assert fitted == (len(tr.opt.calls) == n_calls + 1)
            if tr.ava.updates > n_upd:
                reinit.append(s)
        steps.append((budgets, reinit))
    return steps


def test_budgets_and_reinstalls_follow_frame_tracker():
    ref = _reference()
    # the script exercises: first fit -> initialICPIters, a loss -> 0 and a reinit at the next step (reinitICPIters), the per-part rule
    # only before the first fit
    assert ref[0] == ([6, 0, 0, 6], [0, 3])
    assert ref[1] == ([3, 6, 6, 0], [1, 2])
    assert ref[2] == ([3, 3, 3, 5], [3])
    assert ref[3] == ([3, 0, 0, 3], [])
    assert ref[4] == ([3, 5, 5, 0], [1, 2])
    assert ref[5] == ([3, 3, 3, 5], [3])
    ctx = _Ctx()
    mt = MultiFrameTracker(ctx, 4, **POLICY)
    for t in range(6):
        ctx.log.clear()
        fitted = mt.process([_frame(SCRIPT[s][t], 100 * s + t) for s in range(4)])
        budgets, reinit = ref[t]
        assert fitted == [b > 0 for b in budgets]
        assert list(mt.last_budgets) == budgets and mt.last_reinit == reinit
        kinds = [e[0] for e in ctx.log]
        if t == 0:       # the first step installs every stream's state
            assert kinds == ["frames", "state", "fit"]
        else:
            assert kinds == (["frames", "state_frames", "fit"] if reinit else ["frames", "fit"])
            if reinit:
                assert ctx.log[1][1] == reinit
        assert ctx.log[-1][1] == (max(budgets), budgets)
        frames_n = ctx.log[0][1]
        assert all(n == 0 for n, b in zip(frames_n, budgets) if b == 0)      # a lost stream's frame rides empty
        for s in reinit:     # the installed start state: the data centroid, zero shape, identity joints, root AngleAxis(pi, y)
            xyz, mask, _ = _frame(SCRIPT[s][t], 100 * s + t)
            sub = mask[::2, ::2] != 255
            pts = xyz[::2, ::2][sub].astype(np.float64); pts[:, 1] *= -1
            assert np.allclose(ctx.p[s], pts.mean(0), rtol=0, atol=1e-12)
            assert np.array_equal(ctx.w[s], np.zeros(K))
            assert np.allclose(ctx.q[s][0], [0.0, 1.0, 0.0, 0.0], atol=1e-15) or np.allclose(ctx.q[s][0], [0.0, -1.0, 0.0, 0.0], atol=1e-15)
            assert np.array_equal(ctx.q[s][1:], np.tile([0.0, 0.0, 0.0, 1.0], (J - 1, 1)))
    assert [st.framesFitted for st in mt.streams] == [6, 4, 4, 4]


def test_all_lost_step_runs_nothing():
    ctx = _Ctx()
    mt = MultiFrameTracker(ctx, 2, **POLICY)
    assert mt.process([_frame("empty", 0), _frame("sparse", 1)]) == [False, False]
    assert ctx.log == [] and all(st.reinit for st in mt.streams)


def test_out_of_range_label_raises():
    ctx = _Ctx()
    mt = MultiFrameTracker(ctx, 2, **POLICY)
    xyz, mask, _ = _frame("full", 0)
    bad = mask.copy(); bad[0, 0] = PARTS
    with pytest.raises(ValueError):
        mt.process([(xyz, mask, None), (xyz, bad, None)])


def test_wrong_stream_count_raises():
    mt = MultiFrameTracker(_Ctx(), 3, **POLICY)
    with pytest.raises(ValueError):
        mt.process([_frame("full", 0)] * 2)
