"""Rate of the GPU background subtraction (include/avt_bgsub.h) on 1280x720 scenes of tests/test_gpu_bgsub.py (a wall
and a floor, the avatar pasted over them, 1 mm noise, 1 % sensor holes):

  resident      avt_bgsub_run_resident on 1 / 8 / 64 uploaded images, `reps` runs queued back to back, then one sync:
                wall time per run and per image (launch sequence included, no host copies)
  host_to_host  avt_bgsub_run: upload of one XYZ map, the run, download of mask + masked depth + result record
  restatement   tests/bgsub_restatement.fast on the host CPU: a numpy / scipy restatement, NOT the reference's C++

Usage: python tools/bgsub_rate.py [out.json]   (default profiles/bgsub_rate.json)
       python tools/bgsub_rate.py --trace N    only N resident runs of the 64-image batch (under rocprofv3 --kernel-trace)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from avatar_amd import bgsub, synth  # noqa: E402
import bgsub_restatement as R  # noqa: E402
import test_gpu_bgsub as T  # noqa: E402


def images(smpl, bg, n):
    base = [T.scene(smpl, 80 + i, bg, holes=0.01, noise=0.001) for i in range(min(n, 8))]
    return np.stack([base[i % len(base)] for i in range(n)])


def resident(b, imgs, reps):
    b.upload(imgs, np.zeros(len(imgs), np.int32))
    for _ in range(3):
        b.run_resident()
    b.sync()
    t = time.perf_counter()
    for _ in range(reps):
        b.run_resident()
    b.sync()
    return (time.perf_counter() - t) / reps


def main():
    smpl = synth.load_model(0)
    bg = T.room()
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        b = bgsub.BGSubtractor(bg)
        b.upload(images(smpl, bg, 64), np.zeros(64, np.int32))
        for _ in range(int(sys.argv[2])):
            b.run_resident()
        b.sync()
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bgsub_rate.json")
    rec = {"size": "1280x720", "scene": "wall + floor, avatar pasted, 1 mm noise, 1 % holes; defaults 0.005 / 0.005", "resident": []}
    for n, reps in ((1, 200), (8, 50), (64, 10)):
        b = bgsub.BGSubtractor(bg)
        s = resident(b, images(smpl, bg, n), reps)
        rec["resident"].append({"images": n, "reps": reps, "ms_per_run": round(s * 1e3, 4), "us_per_image": round(s * 1e6 / n, 2)})
        print(rec["resident"][-1], flush=True)
    b = bgsub.BGSubtractor(bg)
    im = images(smpl, bg, 1)[0]
    for _ in range(5):
        b.run(im)
    ts = []
    for _ in range(50):
        t = time.perf_counter()
        b.run(im)
        ts.append(time.perf_counter() - t)
    rec["host_to_host"] = {"call": "avt_bgsub_run (upload 11 MB, run, download mask + depth + record)", "reps": 50,
                           "median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(float(np.min(ts)) * 1e3, 4)}
    print(rec["host_to_host"], flush=True)
    ref = R.fast(bg, im)
    assert np.array_equal(ref["mask"], b.run(im))
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        R.fast(bg, im)
        ts.append(time.perf_counter() - t)
    rec["restatement_cpu"] = {"what": "tests/bgsub_restatement.fast (numpy + scipy connected_components), a Python restatement, not the reference",
                              "threads": 1, "median_ms": round(float(np.median(ts)) * 1e3, 1)}
    print(rec["restatement_cpu"], flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
