"""What the fit score of a tracker step costs (include/avt_fitscore.h), beside the only route there was before it.  64 streams at
1280x720 (tools/label_rate.py's scenes: a room per stream with the avatar pasted over it), one MultiFrameTracker step through
the attached front end, then, in the same process and alternately:

  device_path   MultiFrameTracker.fit_score of all streams: depth and part mask rendered from the context, scored against the
                background subtractor's masked depth and boxes where they lie (k_fit_score), the tables fetched
  download_path what a caller had before: MultiFrameTracker.render's download of the two images per stream, the download of
                every stream's masked depth, and the numpy restatement of the rule (tests/fit_score_restatement.py)
  score_call    FitScorer.score_rendered_from_bgsub alone on the images the render left: two memsets, the kernel, the download
                of the tables and the wait

The handles' streams are their own, so the clock is the host's around calls that end in a wait for the device; every path is
warmed up at the timed shapes; medians with min and max over the repeats.  The tables of the two paths are compared before
anything is timed.  The kernel alone is read from a kernel trace of `--loop` (this script's second mode: the score call alone,
100 times) taken in a run of its own; `--kernel-us X` writes that figure and the rate it means into the record.

Usage: python tools/fitscore_measure.py [out.json] [streams] [repeats] [--kernel-us X] | --loop [streams]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from avatar_amd import bgsub, fitscore, render, rtree, synth  # noqa: E402
from avatar_amd.tracker import MultiFrameTracker  # noqa: E402
import fit_score_restatement as fr  # noqa: E402
import label_rate as L  # noqa: E402
import test_gpu_bgsub as T  # noqa: E402

W, H = 1280, 720
INTRIN = {k: synth.K4A_INTRIN[k] for k in ("fx", "fy", "cx", "cy")}
TOL = fitscore.DEFAULT_TOL
P = 24


def ms(v):
    return {"median_ms": round(float(np.median(v)) * 1e3, 3), "min_ms": round(min(v) * 1e3, 3), "max_ms": round(max(v) * 1e3, 3)}


def stepped_tracker(n):
    """a tracker of n streams with one fitted step behind its front end"""
    from avatar_amd import api
    smpl = synth.load_model(0)
    bgs, imgs = L.scenes(smpl, n)
    front = bgsub.BGSubtractor(bgs)
    front.nnDistThreshRel, front.neighbThreshRel = T.LIVE
    A = MultiFrameTracker.create(api.AvatarModel(smpl), n, P, synth.identity_part_map(), max_points=H * W // 16 + 1, beta_pose=0.05, beta_shape=0.12,
                                 interval=4, frame_icp_iters=2, reinit_icp_iters=3, reinit_cnz=1000)
    A.attach_front_end(front, rtree.RTree(L.GOLD), rtree_interval=2)
    fitted = A.process_depth(imgs)
    return A, front, fitted


def download_path(A, front, streams, pm):
    imgs = A.render(streams, (W, H), INTRIN, render.DEPTH | render.PART_MASK, pm)
    R, M = np.stack([x["depth"] for x in imgs]), np.stack([x["mask"] for x in imgs])
    D = np.stack([front.download(s).masked_depth for s in streams])
    return fr.tables(R, M, D, [A.boxes[s][0] + A.boxes[s][1] for s in streams], TOL, 1, P)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--loop":
        n = int(args[1]) if len(args) > 1 else 64
        A, front, _ = stepped_tracker(n)
        streams, pm = list(range(n)), synth.identity_part_map()
        A.fit_score(streams, (W, H), INTRIN, TOL, 1, pm)
        for _ in range(100):
            A._fit_scorer.score_rendered_from_bgsub(A._renderer, front, streams, TOL, 1)
        return
    kernel_us = None
    if "--kernel-us" in args:
        i = args.index("--kernel-us")
        kernel_us = float(args[i + 1])
        del args[i:i + 2]
    out = args[0] if args else os.path.join(ROOT, "profiles", "fitscore.json")
    n = int(args[1]) if len(args) > 1 else 64
    repeats = int(args[2]) if len(args) > 2 else 9
    A, front, fitted = stepped_tracker(n)
    streams, pm = list(range(n)), synth.identity_part_map()
    got = A.fit_score(streams, (W, H), INTRIN, TOL, 1, pm)
    ref = download_path(A, front, streams, pm)
    assert np.array_equal(got, ref), "the device path and the download path count differently"
    paths = {"device_path": lambda: A.fit_score(streams, (W, H), INTRIN, TOL, 1, pm),
             "download_path": lambda: download_path(A, front, streams, pm),
             "score_call": lambda: A._fit_scorer.score_rendered_from_bgsub(A._renderer, front, streams, TOL, 1),
             "score_call_stride_2": lambda: A._fit_scorer.score_rendered_from_bgsub(A._renderer, front, streams, TOL, 2)}
    for fn in paths.values():
        for _ in range(2):
            fn()
    tm = {k: [] for k in paths}
    for _ in range(repeats):                                # alternately: what else runs on the host hits all alike
        for k, fn in paths.items():
            t = time.perf_counter()
            fn()
            tm[k].append(time.perf_counter() - t)
    selected = n * H * W
    table_bytes = 2 * n * (P + 1) * 7 * 8                   # cleared once, fetched once
    byts = 9 * selected + table_bytes
    total = fitscore.metrics(got.sum(0))
    per = fitscore.metrics(got)
    rec = {"workload": {"streams": n, "size": "%dx%d" % (W, H), "scenes": "tools/label_rate.py", "fitted": int(sum(fitted)), "num_parts": P, "tol_m": TOL,
                        "repeats": repeats, "timing": "host clock around calls that end in a wait for the device, paths in turn"},
           "device_path": ms(tm["device_path"]), "download_path": dict(ms(tm["download_path"]), bytes_over_the_host=int(9 * selected)),
           "download_over_device": round(float(np.median(tm["download_path"]) / np.median(tm["device_path"])), 1),
           "score_call": dict(ms(tm["score_call"]), pixels_selected=selected, bytes=byts,
                              GB_per_s_of_the_call=round(byts / float(np.median(tm["score_call"])) / 1e9, 1)),
           "score_call_stride_2": ms(tm["score_call_stride_2"]),
           "tables_equal_the_download_path": True,
           "synthetic_run_for_reference_only": {"iou": round(total["iou"], 4), "agree": round(total["agree"], 4), "violation": round(total["violation"], 4),
                                                "unexplained": round(total["unexplained"], 4), "mean_abs_err_m": round(total["mean_abs_err"], 5),
                                                "per_stream_iou_min_max": [round(min(m["iou"] for m in per), 4), round(max(m["iou"] for m in per), 4)],
                                                "counted_pixels": int(got[:, :, :5].sum())}}
    if kernel_us is not None:
        rec["k_fit_score"] = {"source": "kernel trace of --loop in a run of its own, mean of 100 launches", "us": kernel_us,
                              "GB_per_s": round(byts / (kernel_us * 1e-6) / 1e9, 1),
                              "bytes": "9 per selected pixel + the tables cleared and fetched; the observed depth is not read outside the box, so fewer move"}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
