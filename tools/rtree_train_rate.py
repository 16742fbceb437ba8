"""Forest training rate on the GPU (include/avt_rtree_train.h) -> profiles/rtree_train_rate.json.

Configurations: `rtree-train`'s command-line defaults (100 images at 1280x720, 2000 px per image, 5000 features, T 20,
depth 20, probe 170, min_samples 1) and one larger set (--large: 2000 images, 2000 features).  Images are synthetic
renders (avatar_amd/synth.py).  Per level: open / searched nodes, feature evaluations, wall time, evaluations per second.
--cpu-threads N also times the CPU restatement (tests/cpp/rtree_train_restatement.cpp) at the first configuration and
checks that it trains the same tree (near ties settled by the device's choice are counted).  Every entry of the output
comes from one invocation.  Kernel statistics: run under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from avatar_amd import rtree_train, synth, synth_forest  # noqa: E402


def renders(smpl, n, first=1000):
    d = np.empty((n, 720, 1280), np.float32)
    m = np.empty((n, 720, 1280), np.uint8)
    for i in range(n):
        w, p, R = synth.sample_ground_truth(smpl, first + i)
        xyz, mask, _ = synth.render_images(smpl, synth.pose_vertices(smpl, w, p, R), synth.identity_part_map())
        d[i] = synth_forest.depth_of(xyz)
        m[i] = mask
    return d, m


def run(smpl, n_images, F, batch, reps=1):
    cfg = dict(num_parts=24, num_points_per_image=2000, num_features=F, max_probe_offset=170.0, min_samples=1, max_tree_depth=20,
               min_samples_per_feature=20, seed=1)
    tr = rtree_train.Trainer(**cfg)
    t0 = time.perf_counter()
    for i0 in range(0, n_images, batch):
        d, m = renders(smpl, min(batch, n_images - i0), 1000 + i0)
        tr.add_images(d, m)
    ingest = time.perf_counter() - t0
    tree, st = tr.run()                       # warm-up (code objects)
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        tree, st = tr.run()
        runs.append(time.perf_counter() - t0)
    levels = [dict(level=l, open_nodes=st["level_nodes"][l], searched=st["level_searched"][l], feature_evals=st["level_evals"][l],
                   ms=st["level_ms"][l], evals_per_s=(st["level_evals"][l] / (st["level_ms"][l] / 1e3) if st["level_ms"][l] > 0 else 0.0))
              for l in range(st["n_levels"])]
    evals = sum(x["feature_evals"] for x in levels)
    return dict(config=dict(cfg, num_images=n_images), samples=st["n_samples"], nodes=st["n_nodes"], leaves=st["n_leafs"],
                levels=st["n_levels"], whole_tree_s=min(runs), whole_tree_runs_s=runs, ingest_and_render_s=ingest, feature_evals=evals,
                evals_per_s=evals / min(runs), per_level=levels), tree, tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rtree_train_rate.json"))
    a = ap.parse_args()
    smpl = synth.load_model(0)
    # one invocation writes every entry: derived fields (the CPU speedup) refer to the GPU runs beside them
    res = dict(device="MI355X (gfx950)", note="whole_tree_s: avt_rtree_trainer_run wall clock, samples resident; best of the timed runs")
    cli, tree, _ = run(smpl, 100, 5000, 50, reps=3)
    res["cli_defaults"] = cli
    print(f"CLI defaults: {cli['whole_tree_s']:.3f} s per tree, {cli['nodes']} nodes, {cli['evals_per_s']:.3g} feature evals/s", flush=True)
    if a.large:
        big, _, _ = run(smpl, 2000, 2000, 100, reps=1)
        res["large_2000_images_2000_features"] = big
        print(f"2000 images x 2000 features: {big['whole_tree_s']:.2f} s per tree, {big['nodes']} nodes", flush=True)
    if a.cpu_threads:
        import rtree_train_restatement as rst
        d, m = renders(smpl, 100, 1000)
        t0 = time.perf_counter()
        ref = rst.train(d, m, 24, 2000, 5000, 170.0, 1, 20, 20, seed=1, nthreads=a.cpu_threads, device_tree=(tree.feature, tree.links))
        cpu = time.perf_counter() - t0
        same = bool(np.array_equal(ref["links"], tree.links) and ref["feature"].tobytes() == tree.feature.tobytes()
                    and ref["leaf"].tobytes() == tree.leafData.tobytes())
        res["cpu_restatement"] = dict(threads=a.cpu_threads, whole_tree_s=cpu, same_tree=same, near_ties=ref["ties"],
                                      speedup_vs_cli_defaults=cpu / cli["whole_tree_s"])
        print(f"CPU restatement, {a.cpu_threads} threads: {cpu:.1f} s (same tree: {same}, near ties {ref['ties']})", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
