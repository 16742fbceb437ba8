"""One labelling step of the tracker's front end for 64 streams, from the host to body-part labels on the host, fed two ways in
the same process (include/avt_bgsub.h, include/avt_rtree.h).  Scenes and forest are tools/label_rate.py's, built as depth
images: the z channel of every scene and background with the K4A camera; the XYZ path gets depth.depth_to_xyz of them, so
both paths see the same maps and must label alike (asserted, with the boxes, before anything is timed).

  xyz     avt_bgsub_images_upload of the 64 XYZ maps (11.06 MB each), avt_bgsub_run_resident,
          avt_rtree_predict_best_from_bgsub, avt_rtree_labels_download_all: label_rate.py's chain
  depth   the same with avt_bgsub_depth_upload: 3.69 MB per image cross the bus, k_bgs_backproject builds the maps

Both are warmed up, then timed alternately step by step; the figures are medians over the timed steps with min and max.
`--depth-only` runs the depth path alone (warm-up and steps, nothing written): the run to put under a kernel trace.

Usage: python tools/depth_in_rate.py [out.json] [streams] [steps] [--depth-only]   (default profiles/depth_in_rate.json, 64, 9)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from avatar_amd import bgsub, rtree, synth  # noqa: E402
from avatar_amd.depth import CameraIntrin, depth_to_xyz  # noqa: E402
import label_rate as L  # noqa: E402
import test_gpu_bgsub as T  # noqa: E402

COPY_RATE = 6.29e12          # B/s: the measured rate of a streaming copy on the MI355X


def labels_of(b, tree, upload):
    upload()
    b.run_resident()
    tree.predict_from_bgsub(b, L.INTERVAL)
    return tree.download_all_labels()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    depth_only = "--depth-only" in sys.argv
    out = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "depth_in_rate.json")
    n = int(args[1]) if len(args) > 1 else 64
    steps = int(args[2]) if len(args) > 2 else 9
    k = synth.K4A_INTRIN
    cam = CameraIntrin(k["fx"], k["fy"], k["cx"], k["cy"])
    bgs, imgs = L.scenes(synth.load_model(0), n)
    bgz, z = np.ascontiguousarray(bgs[..., 2]), np.ascontiguousarray(imgs[..., 2])
    rows, cols = z.shape[1:]
    del bgs, imgs
    distinct = {}                                       # the scenes repeat (label_rate.scenes): expand each once
    def xyz_of(a):
        key = a.tobytes()
        if key not in distinct:
            distinct[key] = depth_to_xyz(a, cam)
        return distinct[key]
    bg_xyz = np.stack([xyz_of(a) for a in bgz])
    ba, bb = bgsub.BGSubtractor(bg_xyz), bgsub.BGSubtractor(bg_xyz)
    for b in (ba, bb):
        b.nnDistThreshRel, b.neighbThreshRel = T.LIVE
    ta, tb = rtree.RTree(L.GOLD), rtree.RTree(L.GOLD)
    path_b = lambda: labels_of(bb, tb, lambda: bb.upload_depth(z, cam))
    if depth_only:
        for _ in range(2 + steps):
            path_b()
        return
    xyz = np.stack([xyz_of(a) for a in z])
    distinct.clear()
    path_a = lambda: labels_of(ba, ta, lambda: ba.upload(xyz))
    la, lb = path_a(), path_b()
    assert np.array_equal(la, lb), "the two paths label differently"
    for s in range(n):
        ra, rb = ba.info(s), bb.info(s)
        assert (ra.topLeft, ra.botRight, ra.capped, ra.fg_count) == (rb.topLeft, rb.botRight, rb.capped, rb.fg_count), "the two paths box differently"
    labelled = int((la != 255).sum())
    for _ in range(2):                                  # warm-up of both paths at the timed shapes
        path_a()
        path_b()
    t_a, t_b = [], []
    for _ in range(steps):                              # alternately: what else runs on the host hits both alike
        t = time.perf_counter()
        path_a()
        t_a.append(time.perf_counter() - t)
        t = time.perf_counter()
        path_b()
        t_b.append(time.perf_counter() - t)
    a, b_ = (float(np.median(v)) * 1e3 for v in (t_a, t_b))
    npix = rows * cols
    rec = {"streams": n, "size": f"{cols}x{rows}", "forest": "tests/golden/forest_small.srtr, interval 2, each image's own box",
           "steps": steps, "labelled_pixels_per_step": labelled,
           "xyz_ms": round(a, 3), "xyz_min_max_ms": [round(min(t_a) * 1e3, 3), round(max(t_a) * 1e3, 3)],
           "depth_ms": round(b_, 3), "depth_min_max_ms": [round(min(t_b) * 1e3, 3), round(max(t_b) * 1e3, 3)],
           "xyz_over_depth": round(a / b_, 3),
           "xyz_bytes_per_image": {"up": npix * 12, "down": npix}, "depth_bytes_per_image": {"up": npix * 4 + 16, "down": npix},
           "backproject_bytes": 16 * n * npix, "backproject_copy_bound_ms": round(16 * n * npix / COPY_RATE * 1e3, 4)}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
