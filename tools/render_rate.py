"""Rate of the avatar renderer on the GPU (include/avt_render.h): wall time of one run (projections, painter order, the selected
images) for 1, 8 and 64 posed SMPL avatars at 1280x720, with the per-image sort and with the O(F^2) rank count; and the Lambert
overlays end to end (taken from a context, rendered, every image downloaded to the host).  Prints one JSON
object; with --out also writes it.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel breakdown."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avatar_amd import api, render, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    smpl = synth.load_model(0)
    gm = api.AvatarModel(smpl)
    k = synth.K4A_INTRIN
    batches = [int(x) for x in a.batches.split(",")]
    nmax = max(batches)
    gts = [synth.sample_ground_truth(smpl, s) for s in range(nmax)]
    ctx = api.Context(gm, 24, synth.identity_part_map(), 1000, nmax, device=0)
    cloud, jp, _ = ctx.lbs_update(np.array([g[0] for g in gts]), np.array([g[1] for g in gts]), np.array([g[2] for g in gts]))
    res = {"width": k["width"], "height": k["height"], "faces": gm.numFaces(), "reps": a.reps, "runs": []}
    for n in batches:
        r = render.Renderer(gm, k["width"], k["height"], k, n)
        r.upload(cloud[:n], jp[:n])
        for ordering, oname in ((render.ORDER_SORT, "sort"), (render.ORDER_RANK, "rank")):
            r.set_ordering(ordering)
            for what, wname in ((render.LAMBERT, "lambert"), (render.ALL, "all"), (0, "order_only")):
                r.run(what)
                r.sync()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    r.run(what)
                    r.sync()
                    ts.append(time.perf_counter() - t0)
                ms = float(np.median(ts) * 1e3)
                res["runs"].append({"images": n, "ordering": oname, "outputs": wname, "median_ms": round(ms, 4),
                                    "us_per_image": round(ms * 1e3 / n, 2)})
                print(f"{n:3d} images  {oname:4s}  {wname:10s}  {ms:8.3f} ms  {ms * 1e3 / n:8.1f} us/image", file=sys.stderr)
        # what a displayed overlay costs after a fit: the posed clouds taken from the context on the device, the run, and the
        # download of every image's Lambert overlay to the host (avt_renderer_download: pageable memory, one wait per image)
        r.set_ordering(render.ORDER_SORT)
        ts = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            r.from_context(ctx, n=n)
            r.run(render.LAMBERT)
            for i in range(n):
                r.download(i, render.LAMBERT)
            if rep:
                ts.append(time.perf_counter() - t0)
        ms = float(np.median(ts) * 1e3)
        res["runs"].append({"images": n, "ordering": "sort", "outputs": "lambert, from context + download", "median_ms": round(ms, 4),
                            "us_per_image": round(ms * 1e3 / n, 2)})
        print(f"{n:3d} images  sort  lambert from the context, downloaded  {ms:8.3f} ms  {ms * 1e3 / n:8.1f} us/image", file=sys.stderr)
        del r
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
