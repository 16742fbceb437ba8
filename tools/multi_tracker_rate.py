#!/usr/bin/env python3
"""Tracking throughput of the batched tracker: tests/cpp/multi_tracker_demo at S = 1, 8 and 64 streams against the single-stream
tests/cpp/tracker_demo, on the same seeded rendered sequence at the tracker stage's size (1280 x 720, interval 3, ICP budgets 3 / 6).
Stream s plays the sequence starting s frames in, so the streams are staggered.  Two sequences: one without losses, and one in which
one frame of the cycle is empty - every stream then loses tracking once per cycle and reinitialises (budget 6) on the next step, at
different steps for different streams.  Each program runs in a process of its own under `timeout -k`.

usage: python tools/multi_tracker_rate.py [--out profiles/multi_tracker_rate.json] [--frames 12] [--reps 20]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avatar_amd import synth  # noqa: E402
from tests.test_gpu_facade import write_model_dir  # noqa: E402
from tests.test_gpu_tracker import write_sequence  # noqa: E402


def clip(smpl, n, seed=7):
    w, p, R = synth.sample_ground_truth(smpl, seed, use_gmm=False)
    w = 0.5 * w
    out = []
    for k in range(n):
        ph = 2 * np.pi * k / n          # a cycle: the last frame leads back to the first
        Rk = R.copy()
        Rk[16] = R[16] @ synth.rodrigues([0.0, 0.0, 0.3 * np.sin(ph)])
        Rk[4] = R[4] @ synth.rodrigues([0.3 * (1 - np.cos(ph)), 0.0, 0.0])
        pk = p + np.array([0.05 * np.sin(ph), 0.0, 0.0])
        xyz, mask, _ = synth.render_images(smpl, synth.pose_vertices(smpl, w, pk, Rk), synth.identity_part_map())
        ys, xs = np.nonzero(mask != 255)
        out.append((xyz, mask, (ys.min(), xs.min(), ys.max(), xs.max())))
    return out


def run(cmd, tlimit):
    r = subprocess.run(["timeout", "-k", "10", str(tlimit)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"{os.path.basename(cmd[0])} exited with {r.returncode}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--streams", default="1,8,64")
    ap.add_argument("--keep", default=None, help="write the model directory and the sequences here instead of a temporary directory")
    a = ap.parse_args()
    smpl = synth.load_model(0)
    cpp = os.path.join(ROOT, "tests", "cpp")
    res = {"size": "1280x720", "interval": 3, "frame_icp_iters": 3, "reinit_icp_iters": 6, "frames_per_cycle": a.frames, "reps": a.reps, "runs": []}
    base = clip(smpl, a.frames)
    with tempfile.TemporaryDirectory() as tmpd:
        tmp = tmpd
        if a.keep:
            os.makedirs(a.keep, exist_ok=True)
            tmp = a.keep
        mdir = os.path.join(tmp, "model")
        write_model_dir(smpl, mdir)
        for losses in (False, True):
            frames = list(base)
            if losses:
                xyz, mask, _ = frames[-1]
                frames[-1] = (xyz, np.full_like(mask, 255), (0, 0, mask.shape[0] - 1, mask.shape[1] - 1))
            seq = os.path.join(tmp, f"seq{int(losses)}.bin")
            write_sequence(seq, frames, 3, 3, 6, 1000)
            out = run([os.path.join(cpp, "tracker_demo"), mdir, seq, os.path.join(tmp, "o.bin"), str(a.reps)], 600)
            m = re.search(r"(\d+) frames, ([\d.]+) ms per frame, ([\d.]+) GN", out)
            single = {"program": "tracker_demo", "losses": losses, "streams": 1, "frames": int(m.group(1)),
                      "frames_per_s": 1000.0 / float(m.group(2)), "gn_per_frame": float(m.group(3))}
            res["runs"].append(single)
            print(json.dumps(single), flush=True)
            for S in [int(s) for s in a.streams.split(",")]:
                for posed in (0, 1):
                    out = run([os.path.join(cpp, "multi_tracker_demo"), mdir, os.path.join(tmp, "o.bin"), str(S), str(a.reps), str(posed), "-1", seq], 900)
                    m = re.search(r"(\d+) steps, (\d+) frames, ([\d.]+) frames/s, ([\d.]+) ms per step, ([\d.]+) GN", out)
                    row = {"program": "multi_tracker_demo", "losses": losses, "streams": S, "posed": posed, "steps": int(m.group(1)),
                           "frames": int(m.group(2)), "frames_per_s": float(m.group(3)), "ms_per_step": float(m.group(4)),
                           "gn_per_frame": float(m.group(5)), "vs_single_stream": float(m.group(3)) / single["frames_per_s"]}
                    res["runs"].append(row)
                    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
