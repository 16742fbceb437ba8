"""What the pose error of a tracker-sized batch costs (include/avt_poseerr.h), beside the only route there was before it.  n = 64
and 512 SMPL-sized pairs (V = 6890, J = 24, 24 parts), both sides resident in contexts: truths put there by avt_lbs_update from the
synthetic ground-truth states, estimates by avt_lbs_update from the perturbed start states (a skinning like the one that ends
optimize(); the scorer reads the same buffers either way).  In the same process and alternately:

  device_path    PoseError.from_context of both sides, run, get: two device copies per side, one kernel, one small table back
  run_get        run + get alone on the pairs the scorer already holds: the kernel, the download of the tables and the wait
  download_path  what a caller had before: avt_get_posed of every frame of both contexts and the numpy restatement of the rule
                 (tests/pose_error_restatement.py); `download_only` is its avt_get_posed part alone

The handles' streams are their own, so the clock is the host's around calls that end in a wait for the device; every path is
warmed up at the timed shapes; medians with min and max over the repeats.  The two paths' figures are compared before anything
is timed.

Usage: python tools/pose_error_measure.py [out.txt] [repeats]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from avatar_amd import api, poseerror, synth  # noqa: E402
import pose_error_restatement as pr  # noqa: E402

P = 24
DISTINCT = 16                 # distinct states; a batch repeats them


def ms(v):
    return "median %9.3f ms  min %9.3f  max %9.3f" % (float(np.median(v)) * 1e3, min(v) * 1e3, max(v) * 1e3)


def contexts(gm, smpl, pm, n):
    gts = [synth.sample_ground_truth(smpl, s) for s in range(DISTINCT)]
    starts = [synth.perturb_start(*gt, s) for s, gt in enumerate(gts)]
    pick = lambda states, k: np.stack([states[i % DISTINCT][k] for i in range(n)])
    out = []
    for states in (starts, gts):
        c = api.Context(gm, P, pm, 1000, n, device=0)
        c.lbs_update(pick(states, 0), pick(states, 1), pick(states, 2))
        out.append(c)
    return out


def download(est, truth, n):
    return [[c.posed(f)[:2] for f in range(n)] for c in (est, truth)]


def download_path(est, truth, n, vp):
    e, t = download(est, truth, n)
    return pr.pairs([x[0] for x in e], [x[0] for x in t], [x[1] for x in e], [x[1] for x in t], vp, P)


def main():
    args = sys.argv[1:]
    out = args[0] if args else os.path.join(ROOT, "profiles", "pose_error_measure.txt")
    repeats = int(args[1]) if len(args) > 1 else 9
    smpl = synth.load_model(0)
    gm = api.AvatarModel(smpl)
    pm = synth.identity_part_map()
    vp = np.asarray(pm)[gm.mainJoint]
    lines = ["pose error, V = %d, J = %d, %d parts; host clock around calls that end in a wait for the device, paths in turn, %d repeats after 2 warm-up rounds"
             % (gm.numPoints(), gm.numJoints(), P, repeats)]
    for n in (64, 512):
        est, truth = contexts(gm, smpl, pm, n)
        pe = poseerror.PoseError.for_model(gm, P, pm, max_pairs=n)

        def device_path():
            pe.from_context(poseerror.ESTIMATE, est, None, n=n)
            pe.from_context(poseerror.TRUTH, truth, None, n=n)
            pe.run()
            return pe.get()

        def run_get():
            pe.run()
            return pe.get()

        got, ref = device_path(), download_path(est, truth, n, vp)
        assert (got["status"] == 0).all() and np.array_equal(got["argmax"], ref["argmax"])
        rel = float(np.max(np.abs(got["summary"] - ref["summary"]) / np.abs(ref["summary"])))
        assert rel < 1e-9, rel
        paths = {"device_path": device_path, "run_get": run_get, "download_path": lambda: download_path(est, truth, n, vp),
                 "download_only": lambda: download(est, truth, n)}
        for fn in paths.values():
            for _ in range(2):
                fn()
        tm = {k: [] for k in paths}
        for _ in range(repeats):                            # alternately: what else runs on the host hits all alike
            for k, fn in paths.items():
                t = time.perf_counter()
                fn()
                tm[k].append(time.perf_counter() - t)
        m = pe.metrics(got)
        byts = n * 2 * 3 * (gm.numPoints() + gm.numJoints()) * 8
        lines.append("n = %d pairs (%.1f MB of points on the two sides; %d distinct states, for reference only: pve %.4f m, pa_pve %.4f m, mpjpe %.4f m, pa_mpjpe %.4f m)"
                     % (n, byts / 1e6, DISTINCT, m["pve"].mean(), m["pa_pve"].mean(), m["mpjpe"].mean(), m["pa_mpjpe"].mean()))
        for k in paths:
            lines.append("  %-14s %s" % (k, ms(tm[k])))
        lines.append("  download_path / device_path %.1f   run_get reads its points three times: %.1f GB/s of the call   largest relative difference of the two paths' summaries %.1e"
                     % (np.median(tm["download_path"]) / np.median(tm["device_path"]), 3 * byts / float(np.median(tm["run_get"])) / 1e9, rel))
        del pe, est, truth
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
