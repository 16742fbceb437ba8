"""What scoring a forest against ground-truth part masks costs (include/avt_rforest.h, THE SCORE): the inner step of
RForest.scoreFromAvatar, render excluded, beside the route there was before it.  One batch of 64 avatars (RForest.scoreFromAvatar's
poses, image 32 onwards of seed 3: none of them trained on) rendered at 1280x720 and left on the device; forests of T = 1, 3, 8
trees from RForest.trainFromAvatar at small settings (32 images, 500 points per image, 100 features, depth 12, seeds 3..10).

  score_rendered  route A, this feature: RForest.score_rendered on the batch, stride 1 and 2.  One call = two memsets, the fused
                  kernel (walk, sum, arg-max, compare, count), the download of the (P + 1)^2 matrix and the wait for the stream.
  old_route       route B, what a user had before: Renderer.download of the 64 depth images and masks, RForest.upload_images,
                  predict_resident_boxes at interval 1 over the whole image, download_all_labels, numpy.bincount of the (mask,
                  label) pairs.  ITS RULE DIFFERS: the label form skips the first row of every image, so its matrix is the
                  score's without row 0 of the images; `old_route_matrix_equals_score` says whether that changed a count here.
  wave_merge      when avatar_amd/csrc/libavatar_hip_rf_score_merge.so is there (make -C avatar_amd/csrc
                  libavatar_hip_rf_score_merge.so): route A with the in-wave merge of equal cells in front of the LDS atomics,
                  timed in child processes that alternate with child processes on the shipped library, same images, same trees;
                  "not tried" otherwise.

Every timed path is warmed up; the paths of one measurement are timed alternately, repeat by repeat; every timed call ends in a
wait for the device, and the clock is the host's around it; the figures are medians with min and max over the repeats.

Usage: python tools/rforest_score_measure.py [out.json] [images] [repeats]      (default profiles/rforest_score.json, 64, 15)"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from avatar_amd import api, capi, render, rforest, rtree, rtree_train, synth  # noqa: E402

SIZES = (1, 3, 8)
STRIDES = (1, 2)
W, H = 1280, 720
INTRIN = {k: synth.K4A_INTRIN[k] for k in ("fx", "fy", "cx", "cy")}
TRAIN = dict(num_images=32, num_points_per_image=500, num_features=100, max_probe_offset=170, min_samples=10, max_tree_depth=12, seed=3, batch=32)
MERGE_LIB = os.path.join(ROOT, "avatar_amd", "csrc", "libavatar_hip_rf_score_merge.so")


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


def held_out_clouds(model, n, first, seed):
    """the posed avatars of RForest.scoreFromAvatar's images first .. first + n - 1"""
    key = rtree_train.xor_key(seed)
    ava = api.Avatar(model)
    clouds = []
    for idx in range(first, first + n):
        ava.randomize(True, True, True, (idx ^ key) & 0xFFFFFFFF)
        ava.update()
        clouds.append(ava.cloud.copy())
    return np.stack(clouds)


def rendered(model, clouds, part_map):
    rend = render.Renderer(model, W, H, INTRIN, max_images=len(clouds))
    rend.set_part_map(part_map)
    rend.upload(clouds)
    rend.run(render.DEPTH | render.PART_MASK)
    rend.sync()
    return rend


def score_step(forest, rend, stride):
    forest.score_reset()
    forest.score_rendered(rend, stride)             # returns after the forest's stream has finished


def old_route(forest, rend, n):
    """the confusion matrix by the calls there were before the score: images to the host and back, labels to the host"""
    imgs = [rend.download(i, render.DEPTH | render.PART_MASK) for i in range(n)]
    depth, mask = np.stack([x["depth"] for x in imgs]), np.stack([x["mask"] for x in imgs])
    forest.upload_images(depth)
    forest.predict_resident_boxes(1, [(0, 0, -1, -1)] * n, False)
    lab = forest.download_all_labels()
    P = forest.numParts
    t = np.where(mask == 255, P, mask).astype(np.int64).ravel()
    q = np.where(lab == 255, P, lab).astype(np.int64).ravel()
    conf = np.bincount(t * (P + 1) + q, minlength=(P + 1) * (P + 1)).reshape(P + 1, P + 1)
    conf[P, P] = 0
    return conf


def child(work, out, repeats):
    """route A alone on the library AVT_LIB names, on the trees and clouds the parent left in `work`"""
    model = api.AvatarModel(synth.load_model(0))
    clouds = np.load(os.path.join(work, "clouds.npy"))
    rend = rendered(model, clouds, synth.identity_part_map())
    rec = {"library": os.path.basename(capi.LIB_PATH)}
    for k in SIZES:
        forest = rforest.RForest([os.path.join(work, "tree_%d.srtr" % t) for t in range(k)])
        tm = timed({"stride_%d" % s: (lambda s: lambda: score_step(forest, rend, s))(s) for s in STRIDES}, 3, repeats)
        rec["T_%d" % k] = {name: ms(v) for name, v in tm.items()}
        rec["T_%d" % k]["matrix_sum"] = int(forest.score_get().conf.sum())
    with open(out, "w") as fh:
        json.dump(rec, fh)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rforest_score.json")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 15
    model = api.AvatarModel(synth.load_model(0))
    pm = synth.identity_part_map()
    t0 = time.perf_counter()
    full = rforest.RForest.trainFromAvatar(max(SIZES), model, INTRIN, (W, H), part_map=pm, **TRAIN)
    train_s = time.perf_counter() - t0
    forests = {k: rforest.RForest(full.trees[:k]) for k in SIZES}
    clouds = held_out_clouds(model, n, TRAIN["num_images"], TRAIN["seed"])
    rend = rendered(model, clouds, pm)
    selected = {s: n * ((H - 1) // s + 1) * ((W - 1) // s + 1) for s in STRIDES}
    rec = {"workload": {"images": n, "size": "%dx%d" % (W, H), "poses": "scoreFromAvatar's images %d.. of seed %d" % (TRAIN["num_images"], TRAIN["seed"]),
                        "trainer": "RForest.trainFromAvatar " + json.dumps(TRAIN), "train_all_s": round(train_s, 2),
                        "nodes": [len(t.links) for t in full.trees], "num_parts": full.numParts, "repeats": repeats,
                        "timing": "host clock around calls that end in a wait for the device; render excluded"}}
    for k in SIZES:
        f = forests[k]
        paths = {"score_rendered_stride_%d" % s: (lambda s: lambda: score_step(f, rend, s))(s) for s in STRIDES}
        paths["old_route"] = lambda: old_route(f, rend, n)
        tm = timed(paths, 2, repeats)
        score_step(f, rend, 1)
        sc = f.score_get()
        conf_b = old_route(f, rend, n)
        r = {"route_A_score_rendered": {}, "route_B_old_route": dict(ms(tm["old_route"]), rule="label form: the first row of every image is skipped",
                                                                     bytes_over_the_host=int(n * W * H * (4 + 1 + 4 + 1)))}
        for s in STRIDES:
            v = tm["score_rendered_stride_%d" % s]
            r["route_A_score_rendered"]["stride_%d" % s] = dict(ms(v), pixels_selected=selected[s],
                                                                Mpixels_per_s=round(selected[s] / float(np.median(v)) / 1e6, 1))
        r["old_route_over_score_rendered_stride_1"] = round(float(np.median(tm["old_route"]) / np.median(tm["score_rendered_stride_1"])), 1)
        r["old_route_matrix_equals_score"] = bool(np.array_equal(conf_b, sc.conf))
        r["old_route_matrix_counts_differing"] = int(np.abs(conf_b - sc.conf).sum())
        r["held_out"] = {"accuracy": round(sc.accuracy, 4), "mean_iou": round(sc.mean_iou, 4), "missed": sc.missed, "spurious": sc.spurious,
                         "counted": int(sc.conf.sum())}
        rec["T_%d" % k] = r
        print(json.dumps({"T_%d" % k: r}), flush=True)

    # ---- the in-wave merge, if that library was built: child processes, the two libraries in turn, twice
    if os.path.exists(MERGE_LIB):
        with tempfile.TemporaryDirectory() as work:
            np.save(os.path.join(work, "clouds.npy"), clouds)
            for t, tree in enumerate(full.trees):
                assert tree.exportFile(os.path.join(work, "tree_%d.srtr" % t))
            runs = []
            for rnd in range(2):
                for lib in (capi.LIB_PATH, MERGE_LIB):
                    res = os.path.join(work, "child.json")
                    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", work, res, str(repeats)], env=dict(os.environ, AVT_LIB=lib),
                                          timeout=600)
                    runs.append(dict(json.load(open(res)), round=rnd))
        rec["wave_merge"] = {"tried": True, "how": "child processes, shipped library and merge library in turn, two rounds; route A only", "runs": runs}
    else:
        rec["wave_merge"] = {"tried": False, "why": "libavatar_hip_rf_score_merge.so not built"}
    print(json.dumps({"wave_merge": rec["wave_merge"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
