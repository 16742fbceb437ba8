"""What the device subsampling (include/avt_subsample.h, MultiFrameTracker.attach_front_end(..., device_subsample=True)) does
to a depth-in tracking step, against the path it replaces, in one process on one GPU:
python tools/subsample_measure.py [out.json] [streams] [timed steps]      (default profiles/subsample_measure.json, 64, 9)

Workload: tools/label_rate.py's streams at 1280x720 as depth images (their z channel, the K4A camera), one background per stream,
the forest of tests/golden at rtree_interval 2, tracker interval 12, device_post_process=True in both trackers.  Tracker A has
device_subsample on, tracker B off (the parent commit's path: all labels down, numpy subsampling per stream, the clouds up).
The two take the same steps alternately; step 0 (every stream reinitialises: all centroids) and one more warm-up step are reported
apart, the timed steps after them as median (min - max).  Host clocks around calls that end in a stream wait.

  step_on / step_off            MultiFrameTracker.process_depth_images, ms
  first_step_on / _off          step 0: allocations, graph capture, 64 start states; on: the 64 serial centroid sums
  subsample_commit              frames_subsample + frames_commit alone inside A's timed steps, ms
  bytes_*                       what crosses the bus per step in either direction, both ways, computed from the shapes and the
                                steps' point counts (the copies the code makes; not a counter reading)
  one_stream_interval_1         one stream at tracker interval 1, the largest frame the serial sum meets: step 0 (reinitialising)
                                and the next step, both ways, and the subsample + commit calls of both steps
  same_results                  every step's fitted flags, budgets and states are equal between A and B (they must be)"""
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
CAM = tuple(synth.K4A_INTRIN[k] for k in ("fx", "fy", "cx", "cy"))


def ms(v):
    return {"median_ms": round(float(np.median(v)) * 1e3, 3), "min_ms": round(min(v) * 1e3, 3), "max_ms": round(max(v) * 1e3, 3)}


def tracker(gm, bgz, interval, device_subsample, max_points):
    n = len(bgz)
    A = MultiFrameTracker.create(gm, n, 24, synth.identity_part_map(), max_points=max_points, beta_pose=0.05, beta_shape=0.12,
                                 interval=interval, frame_icp_iters=2, reinit_icp_iters=3, reinit_cnz=1000)
    front = bgsub.BGSubtractor(np.zeros(bgz.shape + (3,), np.float32))
    for i in range(n):
        front.set_background_depth(bgz[i], CAM, i)
    front.nnDistThreshRel, front.neighbThreshRel = T.LIVE
    A.attach_front_end(front, rtree.RTree(L.GOLD), rtree_interval=L.INTERVAL, dist_to_pre_weight=0.001, device_post_process=True,
                       device_subsample=device_subsample)
    A.sub_times = []
    if device_subsample:                       # the two calls alone: a clock around each
        ctx = A.ctx
        sub, commit = ctx.frames_subsample, ctx.frames_commit

        def timed_sub(*a, **k):
            t = time.perf_counter(); out = sub(*a, **k); A.sub_times.append(time.perf_counter() - t); A.last_counts = out[0]
            return out

        def timed_commit(*a, **k):
            t = time.perf_counter(); commit(*a, **k); A.sub_times[-1] += time.perf_counter() - t

        ctx.frames_subsample, ctx.frames_commit = timed_sub, timed_commit
    return A


def run(A, B, frames_of, steps):
    t_a, t_b, same = [], [], True
    for step in range(steps):
        depths = frames_of(step)
        t = time.perf_counter(); fa = A.process_depth_images(depths, CAM); t_a.append(time.perf_counter() - t)
        t = time.perf_counter(); fb = B.process_depth_images(depths, CAM); t_b.append(time.perf_counter() - t)
        same = same and fa == fb and np.array_equal(A.last_budgets, B.last_budgets) and all(np.array_equal(x, y) for x, y in ((A.p, B.p), (A.q, B.q), (A.w, B.w)))
    return t_a, t_b, same


def bus_bytes(n, parts, J, K, points, reinit):
    """per step and direction: the copies each path makes (the depth images and the state download are common to both)"""
    depth_up = n * H * W * 4 + n * 16
    state_down = n * ((3 + 4 * J + K) * 8 + 64)                         # p, q, w and the statistics of every frame
    com_down = n * parts * 2 * 8 + n
    start_up = reinit * (3 + 4 * J + K) * 8
    off = {"up": depth_up + points * 28 + (n + 1) * 4 + n * 4 + start_up, "down": n * H * W + com_down + n * 64 + state_down}
    on = {"up": depth_up + n * 6 * 4 + n + n * 4 + start_up, "down": n * (24 + (1 + parts) * 4 + 4 + 16) + com_down + 64 + state_down}
    return on, off


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "subsample_measure.json")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    timed = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    smpl = synth.load_model(0)
    gm = api.AvatarModel(smpl)
    bgs, imgs = L.scenes(smpl, n)
    bgz, z = np.ascontiguousarray(bgs[..., 2]), np.ascontiguousarray(imgs[..., 2])
    other = np.ascontiguousarray(np.roll(z, 4, axis=0))                 # odd steps: another avatar in front of the same room
    A, B = tracker(gm, bgz, 12, True, -(-H // 12) * -(-W // 12)), tracker(gm, bgz, 12, False, -(-H // 12) * -(-W // 12))
    t_a, t_b, same = run(A, B, lambda step: other if step % 2 else z, 2 + timed)
    points = int(A.last_counts[:, 0].sum())
    on, off = bus_bytes(n, 24, 24, 10, points, 0)
    rec = {"streams": n, "size": "1280x720", "tracker_interval": 12, "rtree_interval": L.INTERVAL, "timed_steps": timed,
           "points_per_step": points, "same_results": bool(same),
           "step_on": ms(t_a[2:]), "step_off": ms(t_b[2:]), "first_step_on_ms": round(t_a[0] * 1e3, 3), "first_step_off_ms": round(t_b[0] * 1e3, 3),
           "second_step_on_ms": round(t_a[1] * 1e3, 3), "second_step_off_ms": round(t_b[1] * 1e3, 3),
           "first_step_subsample_commit_ms": round(A.sub_times[0] * 1e3, 3), "subsample_commit": ms(A.sub_times[2:]),
           "bytes_on": on, "bytes_off": off}
    print(json.dumps(rec), flush=True)
    del A, B
    # one stream at interval 1: the largest frame the serial centroid sum meets
    A1, B1 = tracker(gm, bgz[:1], 1, True, H * W // 2), tracker(gm, bgz[:1], 1, False, H * W // 2)
    t_a1, t_b1, same1 = run(A1, B1, lambda step: z[:1], 4)
    A1.streams[0].reinit = B1.streams[0].reinit = True                  # a reinitialisation with everything warm: the sum alone
    t_a2, t_b2, same2 = run(A1, B1, lambda step: z[:1], 1)
    rec["one_stream_interval_1"] = {"points": int(A1.last_counts[0, 0]), "same_results": bool(same1 and same2),
                                    "first_step_on_ms": round(t_a1[0] * 1e3, 3), "first_step_off_ms": round(t_b1[0] * 1e3, 3),
                                    "warm_step_on": ms(t_a1[1:]), "warm_step_off": ms(t_b1[1:]),
                                    "warm_reinit_step_on_ms": round(t_a2[0] * 1e3, 3), "warm_reinit_step_off_ms": round(t_b2[0] * 1e3, 3),
                                    "subsample_commit_ms": [round(v * 1e3, 3) for v in A1.sub_times]}
    print(json.dumps(rec["one_stream_interval_1"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
