"""One labelling step of the tracker's front end for 64 streams, from XYZ maps on the host to body-part labels on the host,
two ways in the same process (include/avt_bgsub.h, include/avt_rtree.h).  Scenes: tests/test_gpu_bgsub.py's room with the
avatar pasted over it (1 mm noise, 1 % sensor holes) at 1280x720, one background per stream, the live demo's thresholds, the
forest of tests/golden at interval 2 inside each image's box.

  per_image   per stream avt_bgsub_run (upload the XYZ map, run, download mask + masked depth + record) and
              avt_rtree_predict_best (upload the masked depth, label, download): two blocking calls and 20.3 MB per image
  chain       avt_bgsub_images_upload of all streams, avt_bgsub_run_resident, avt_rtree_predict_best_from_bgsub (masked depth
              and boxes read on the device), avt_rtree_labels_download_all: two blocking calls per step, 12.0 MB per image
  post        RTree.postProcess of the 64 label images on the host, the same in both paths: what neither path can shorten

Each path is warmed up, then the two are timed alternately step by step; the figures are medians over the timed steps.  The
labels of the two paths are compared before anything is timed.

Usage: python tools/label_rate.py [out.json] [streams] [steps]   (default profiles/label_rate.json, 64, 9)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from avatar_amd import bgsub, rtree, synth  # noqa: E402
import test_gpu_bgsub as T  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "forest_small.srtr")
INTERVAL = 2


def scenes(smpl, n):
    walls = [(4.5, 1.0), (3.8, 1.2), (4.2, 1.1), (5.0, 0.9)]
    rooms = [T.room(*w) for w in walls]
    bgs = np.stack([rooms[i % len(rooms)] for i in range(n)])
    base = [T.scene(smpl, 80 + i, rooms[i % len(rooms)], holes=0.01, noise=0.001) for i in range(min(n, 8))]
    return bgs, np.stack([base[i % len(base)] for i in range(n)])


def per_image(b, tree, imgs):
    out, boxes = [], []
    for s in range(len(imgs)):
        b.topLeft, b.botRight = (0, 0), (0, 0)
        b.run(imgs[s], background_index=s)
        out.append(tree.predictBest(b.maskedDepth, 0, INTERVAL, b.topLeft, b.botRight))
        boxes.append((b.topLeft, b.botRight))
    return out, boxes


def chain(b, tree, imgs):
    b.upload(imgs)
    b.run_resident()
    tree.predict_from_bgsub(b, INTERVAL)
    return tree.download_all_labels()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "label_rate.json")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    smpl = synth.load_model(0)
    bgs, imgs = scenes(smpl, n)
    ba, bb = bgsub.BGSubtractor(bgs), bgsub.BGSubtractor(bgs)
    for b in (ba, bb):
        b.nnDistThreshRel, b.neighbThreshRel = T.LIVE
    ta, tb = rtree.RTree(GOLD), rtree.RTree(GOLD)
    la, boxes = per_image(ba, ta, imgs)
    lb = chain(bb, tb, imgs)
    assert all(np.array_equal(la[s], lb[s]) for s in range(n)), "the two paths label differently"
    labelled = int(sum((x != 255).sum() for x in la))
    for _ in range(2):                                  # warm-up of both paths at the timed shapes
        per_image(ba, ta, imgs)
        chain(bb, tb, imgs)
    t_a, t_b = [], []
    for _ in range(steps):                              # alternately: what else runs on the host hits both alike
        t = time.perf_counter()
        per_image(ba, ta, imgs)
        t_a.append(time.perf_counter() - t)
        t = time.perf_counter()
        chain(bb, tb, imgs)
        t_b.append(time.perf_counter() - t)
    t_p = []
    for _ in range(3):
        work = lb.copy()
        t = time.perf_counter()
        for s in range(n):
            ta.postProcess(work[s], None, INTERVAL, 1, *boxes[s])
        t_p.append(time.perf_counter() - t)
    a, b_, p = (float(np.median(v)) * 1e3 for v in (t_a, t_b, t_p))
    rec = {"streams": n, "size": "1280x720", "forest": "tests/golden/forest_small.srtr, interval 2, each image's own box",
           "steps": steps, "labelled_pixels_per_step": labelled,
           "per_image_ms": round(a, 3), "per_image_min_max_ms": [round(min(t_a) * 1e3, 3), round(max(t_a) * 1e3, 3)],
           "chain_ms": round(b_, 3), "chain_min_max_ms": [round(min(t_b) * 1e3, 3), round(max(t_b) * 1e3, 3)],
           "per_image_over_chain": round(a / b_, 3), "post_process_host_ms": round(p, 3)}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
