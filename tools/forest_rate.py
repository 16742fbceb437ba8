"""What a forest of several trees costs and gives (include/avt_rforest.h), three measurements in one process on one image set:
T trees from the GPU trainer (RForest.train_from_images, seeds seed .. seed + 7) on synthetic renders at 1280x720.

  step      the labelling step of 64 streams at interval 2 behind one background-subtraction batch, the images left on the
            device: RTree.predict_from_bgsub (one tree, the capability before forests), RForest.predict_from_bgsub for T in
            1, 2, 4, 8 (one launch, the trees walked in lock step), and T single trees one after the other on the same batch
            (T launches, each waited for).  Every call ends in a wait for the stream.  T x the single tree's time is what a
            T-tree method has to beat.
  image     one 1280x720 image, T = 4, host image in and host labels out: RForest.predictBest against the route there was
            before, T x RTree.predict (num_parts float planes down per tree), summed in tree order and arg-maxed with numpy.
            The labels of the two routes are compared first.
  accuracy  per-pixel agreement of RForest.predictBest (interval 1) with the rendered part mask on renders that are not in the
            training set, T in 1, 2, 4, 8.  Reported, not promised: the feature is the mechanism.

Every timed path is warmed up, the paths of one measurement are timed alternately repeat by repeat, the figures are medians with
min and max over the repeats.

Usage: python tools/forest_rate.py [out.json] [streams] [repeats] [training images]   (default profiles/forest_rate.json, 64, 15, 16)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from avatar_amd import bgsub, rforest, rtree, synth, synth_forest  # noqa: E402
import test_gpu_bgsub as T  # noqa: E402

INTERVAL = 2
SIZES = (1, 2, 4, 8)
LIVE = (0.002, 0.001)                                    # live-demo.cpp:96-100


def render(smpl, seed):
    w, p, R = synth.sample_ground_truth(smpl, seed)
    xyz, mask, _ = synth.render_images(smpl, synth.pose_vertices(smpl, w, p, R), synth.identity_part_map())
    return synth_forest.depth_of(xyz), mask


def scenes(smpl, n):
    walls = [(4.5, 1.0), (3.8, 1.2), (4.2, 1.1), (5.0, 0.9)]
    rooms = [T.room(*w) for w in walls]
    bgs = np.stack([rooms[i % len(rooms)] for i in range(n)])
    base = [T.scene(smpl, 80 + i, rooms[i % len(rooms)], holes=0.01, noise=0.001) for i in range(min(n, 8))]
    return bgs, np.stack([base[i % len(base)] for i in range(n)])


def timed(paths, warmup, repeats):
    """{name: [seconds per repeat]}: every path warmed up, then all of them once per repeat, in turn"""
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in paths}
    for _ in range(repeats):
        for k, fn in paths.items():
            t = time.perf_counter()
            fn()
            out[k].append(time.perf_counter() - t)
    return out


def ms(v):
    return {"median_ms": round(float(np.median(v)) * 1e3, 3), "min_ms": round(min(v) * 1e3, 3), "max_ms": round(max(v) * 1e3, 3)}


def host_route(trees, depth):
    """T x RTree.predict, then the sum in tree order and the arg-max of rtree-run-dataset.cpp:128-158 on the host"""
    s = trees[0].predict(depth)
    for t in trees[1:]:
        s = s + t.predict(depth)
    lab = np.full(depth.shape, 255, np.uint8)
    best = np.zeros(depth.shape, np.float32)
    for p in range(len(s)):
        win = s[p] > best
        best[win] = s[p][win]
        lab[win] = p
    return lab


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "forest_rate.json")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 15
    n_train = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    smpl = synth.load_model(0)
    train = [render(smpl, 400 + i) for i in range(n_train)]
    d, m = np.stack([x[0] for x in train]), np.stack([x[1] for x in train])
    t0 = time.perf_counter()
    full = rforest.RForest.train_from_images(max(SIZES), d, m, 24, num_points_per_image=2000, num_features=400, max_probe_offset=170.0,
                                             min_samples=10, max_tree_depth=16, seed=3, part_map=synth.identity_part_map())
    train_s = time.perf_counter() - t0
    trees = full.trees                                    # device trees: the single-tree paths run them
    forests = {k: rforest.RForest(trees[:k]) for k in SIZES}
    rec = {"trees": {"trainer": "RForest.train_from_images, 2000 points per image, 400 features, min_samples 10, depth 16, seeds 3..10",
                     "training_images": n_train, "train_all_s": round(train_s, 2), "nodes": [len(t.links) for t in trees]}}

    # ---- step: 64 streams behind one background-subtraction batch
    bgs, imgs = scenes(smpl, n)
    b = bgsub.BGSubtractor(bgs)
    b.nnDistThreshRel, b.neighbThreshRel = LIVE
    b.upload(imgs)
    b.run_resident()
    b.sync()

    def one(tree):
        tree.predict_from_bgsub(b, INTERVAL)
        tree.sync()

    def back_to_back(k):
        for t in trees[:k]:
            one(t)

    one(trees[0]); one(forests[1])
    same = bool(np.array_equal(trees[0].download_all_labels(), forests[1].download_all_labels()))
    paths = {"tree": lambda: one(trees[0]), "tree_again": lambda: one(trees[0])}
    for k in SIZES:
        paths["forest_%d" % k] = (lambda f: lambda: one(f))(forests[k])
        if k > 1:
            paths["trees_back_to_back_%d" % k] = (lambda kk: lambda: back_to_back(kk))(k)
    tm = timed(paths, 3, repeats)
    tree_ms = float(np.median(tm["tree"])) * 1e3
    one(forests[max(SIZES)])
    labelled = int((forests[max(SIZES)].download_all_labels() != 255).sum())
    step = {"streams": n, "size": "1280x720", "interval": INTERVAL, "repeats": repeats, "labelled_pixels": labelled,
            "forest_1_labels_equal_tree": same, "tree": ms(tm["tree"]), "tree_again": ms(tm["tree_again"])}
    for k in SIZES:
        f_ms = float(np.median(tm["forest_%d" % k])) * 1e3
        step["forest_%d" % k] = dict(ms(tm["forest_%d" % k]), over_tree=round(f_ms / tree_ms, 3), over_T_x_tree=round(f_ms / (k * tree_ms), 3))
        if k > 1:
            bb = float(np.median(tm["trees_back_to_back_%d" % k])) * 1e3
            step["trees_back_to_back_%d" % k] = dict(ms(tm["trees_back_to_back_%d" % k]), forest_over_back_to_back=round(f_ms / bb, 3))
    rec["step"] = step
    print(json.dumps({"step": step}), flush=True)
    del b

    # ---- image: one image, T = 4, forest against T x predict + host sum and arg-max
    depth, mask = render(smpl, 21)
    got, ref = forests[4].predictBest(depth, 0, 1, fill_in_gaps=False), host_route(trees[:4], depth)
    walked = depth > 0
    walked[0] = False
    equal = bool(np.array_equal(got[walked], ref[walked]))
    tm = timed({"forest": lambda: forests[4].predictBest(depth, 0, 1, fill_in_gaps=False), "host_route": lambda: host_route(trees[:4], depth)},
               2, max(3, repeats // 3))
    rec["image"] = {"size": "1280x720", "T": 4, "labels_equal": equal, "forest": ms(tm["forest"]), "host_route": ms(tm["host_route"]),
                    "host_route_over_forest": round(float(np.median(tm["host_route"]) / np.median(tm["forest"])), 2),
                    "plane_bytes_per_tree": int(24 * depth.size * 4)}
    print(json.dumps({"image": rec["image"]}), flush=True)

    # ---- accuracy on renders outside the training set
    acc = {}
    for seed in (21, 22):
        depth, mask = render(smpl, seed)
        fg = mask != 255
        fg[0] = False
        for k in SIZES:
            lab = forests[k].predictBest(depth, 0, 1, fill_in_gaps=False)
            acc.setdefault("T_%d" % k, []).append(round(float((lab[fg] == mask[fg]).mean()), 4))
    rec["accuracy"] = {"renders": "synth seeds 21, 22 (1280x720), foreground pixels below row 0", "agreement_with_part_mask": acc}
    print(json.dumps({"accuracy": rec["accuracy"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
