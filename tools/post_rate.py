"""postProcess of a batch of label images, on the host per stream against the device stage (include/avt_rtree.h:
avt_rtree_post_process_from_bgsub), and what the deliberate difference of the device rule above interval 1 does to the labels.
Workload: tools/label_rate.py's 64 streams at 1280x720, the forest of tests/golden at interval 2 inside each image's box.

  host_post_ms          RTree.postProcess of the 64 label images, one thread, the labels already on the host
  device_post_ms        post_process_from_bgsub alone: the call and its one wait, between two points where the stream is idle
                        (the labelling that feeds it is waited for first; nothing is downloaded)
  step_host_ms          MultiFrameTracker.process_depth, the step of 64 streams, post-processing on the host
  step_device_ms        the same with attach_front_end(..., device_post_process=True)
  differing_fg_share    share of the pixels that are foreground under either rule whose label differs between the host rule (the
                        reference's, scan-order bound at interval 2) and the grid rule, first frame (no memory)
  fit_score_host / fit_score_device   MultiFrameTracker.fit_score tables summed over the streams after each of 12 steps, both ways

Every timed path is warmed up; the figures are medians over the timed repeats with (min, max).

Usage: python tools/post_rate.py [out.json] [streams] [repeats]   (default profiles/post_rate.json, 64, 7)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from avatar_amd import api, bgsub, rtree, synth  # noqa: E402
from avatar_amd.tracker import MultiFrameTracker  # noqa: E402
import label_rate as L  # noqa: E402
import test_gpu_bgsub as T  # noqa: E402

W, H = 1280, 720
INTRIN = {k: synth.K4A_INTRIN[k] for k in ("fx", "fy", "cx", "cy")}
WEIGHT = 0.001


def ms(v):
    return {"median_ms": round(float(np.median(v)) * 1e3, 3), "min_ms": round(min(v) * 1e3, 3), "max_ms": round(max(v) * 1e3, 3)}


def front_end(bgs):
    b = bgsub.BGSubtractor(bgs)
    b.nnDistThreshRel, b.neighbThreshRel = T.LIVE
    return b


def tracker(gm, bgs, n, device):
    A = MultiFrameTracker.create(gm, n, 24, synth.identity_part_map(), max_points=H * W // 16 + 1, beta_pose=0.05, beta_shape=0.12,
                                 interval=4, frame_icp_iters=2, reinit_icp_iters=3, reinit_cnz=1000)
    A.attach_front_end(front_end(bgs), rtree.RTree(L.GOLD), rtree_interval=L.INTERVAL, dist_to_pre_weight=WEIGHT, device_post_process=device)
    return A


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "post_rate.json")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    smpl = synth.load_model(0)
    bgs, imgs = L.scenes(smpl, n)
    b, tree = front_end(bgs), rtree.RTree(L.GOLD)
    b.upload(imgs)
    b.run_resident()
    tree.predict_from_bgsub(b, L.INTERVAL)
    raw = tree.download_all_labels()
    boxes = [(b.info(s).topLeft, b.info(s).botRight) for s in range(n)]

    # the host rule and the device rule on the same labels, no memory
    host = raw.copy()
    t_host = []
    for rep in range(reps + 1):
        work = raw.copy()
        t = time.perf_counter()
        for s in range(n):
            tree.postProcess(work[s], None, L.INTERVAL, 1, *boxes[s], WEIGHT)
        t_host.append(time.perf_counter() - t)
        host = work
    t_dev = []
    for rep in range(reps + 1):
        tree.com_pre_set(0, np.zeros((n, 2, tree.numParts)), np.zeros(n, bool))
        tree.predict_from_bgsub(b, L.INTERVAL)
        tree.sync()
        t = time.perf_counter()
        tree.post_process_from_bgsub(b, L.INTERVAL, WEIGHT)
        t_dev.append(time.perf_counter() - t)
    dev = tree.download_all_labels()
    fg = (host != 255) | (dev != 255)
    differing = float(((host != dev) & fg).sum()) / max(1, int(fg.sum()))

    # a labelled tracker step both ways, alternately; then 12 steps each with the fit score after every step
    gm = api.AvatarModel(smpl)
    A, B = tracker(gm, bgs, n, False), tracker(gm, bgs, n, True)
    t_a, t_b, score_a, score_b = [], [], [], []
    streams = list(range(n))
    for step in range(12):
        frame = np.roll(imgs, 4, axis=0) if step % 2 else imgs             # odd steps: another avatar in front of the same room
        t = time.perf_counter(); A.process_depth(frame); t_a.append(time.perf_counter() - t)
        t = time.perf_counter(); B.process_depth(frame); t_b.append(time.perf_counter() - t)
        score_a.append(A.fit_score(streams, (W, H), INTRIN).sum(0).sum(0).tolist())
        score_b.append(B.fit_score(streams, (W, H), INTRIN).sum(0).sum(0).tolist())
    rec = {"streams": n, "size": "1280x720", "interval": L.INTERVAL, "repeats": reps,
           "host_post": ms(t_host[1:]), "device_post": ms(t_dev[1:]),
           "host_over_device": round(float(np.median(t_host[1:]) / np.median(t_dev[1:])), 2),
           "step_host": ms(t_a[2:]), "step_device": ms(t_b[2:]),
           "foreground_pixels": int(fg.sum()), "differing_fg_share": round(differing, 5),
           "fit_score_columns": "the 7 columns of avatar_amd.fitscore tables, summed over streams and parts",
           "fit_score_host": score_a, "fit_score_device": score_b}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
