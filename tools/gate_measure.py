"""What the correspondence gate (include/avt.h, avt_set_corr_gate) costs and what it does to a fit, in one process on one GPU:
python tools/gate_measure.py [cost] [effect]

cost:   the benchmark's headline workload (one 38 k-point frame rendered on the GPU, Options.counted(icp_iters=1), avt_state_reset +
        avt_optimize_resident per step, 5 warm-up and 50 timed steps) with the gate off and with a finite gate that drops nothing
        (g = 10 m), three rounds each, alternating; ms per step of every round.  (The comparison with the parent commit is
        `python bench.py` on the two trees)
effect: the contaminated frame of tests/test_gpu_nn_gate.py (every 6th pixel of synth.make_frame(smpl, 3) plus 300 points planted
        0.6 m off the surface) and the clean frame it was made from, Options.demo(icp_iters=3), from the frame's start state: mean vertex
        distance of the fitted avatar to the generating one ungated and at g = 0.1, 0.2 and 0.3 m, with the correspondences kept and
        dropped by the last search.  Reported only: no default follows from it."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from avatar_amd import api, synth
from avatar_amd.capi import Options


def cost(smpl, gm):
    pm = synth.identity_part_map()
    gt = synth.sample_ground_truth(smpl, 0)
    w0, p0, R0 = synth.perturb_start(*gt, 0)
    ctx = api.Context(gm, 24, pm, 65536, 1, device=0)
    n = ctx.render_frames(gt[0][None], gt[1][None], gt[2][None])
    ctx.state_upload(p0[None], api.rot_to_quat(R0)[None], w0[None])
    opt = Options.counted(icp_iters=1)
    print(f"one frame of {int(n[0])} points, icp_iters 1, 10 iterations, 5 warm-up + 50 timed steps per round")
    print("| round | gate off: ms per step | g = 10 m: ms per step | gated at g = 10 |")
    print("|---|---|---|---|")
    for rnd in range(3):
        row = []
        for g in (None, 10.0):
            ctx.set_corr_gate(g)
            for _ in range(5):
                ctx.state_reset(); ctx.optimize_resident(opt)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(50):
                ctx.state_reset(); ctx.optimize_resident(opt)
            ctx.sync()
            row.append((time.perf_counter() - t0) / 50 * 1e3)
        print(f"| {rnd + 1} | {row[0]:.4f} | {row[1]:.4f} | {ctx.gated(0)} |", flush=True)


def contaminated_frame(smpl):
    """The frame of tests/test_gpu_nn_gate.py: (clean data, clean labels, contaminated data, contaminated labels, the frame)."""
    fr = synth.make_frame(smpl, 3)
    sel = np.arange(0, len(fr["labels"]), 6)
    data, labels = fr["data"][sel], fr["labels"][sel]
    N = len(labels)
    rng = np.random.default_rng(5)
    idx = rng.integers(1, N, 300)
    nrm = rng.normal(size=(300, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    D = np.concatenate([data, data[idx] + 0.6 * nrm])
    L = np.concatenate([labels, labels[idx]]).astype(np.int32)
    perm = np.concatenate([[0], 1 + rng.permutation(len(L) - 1)])
    return data, labels, np.ascontiguousarray(D[perm]), np.ascontiguousarray(L[perm]), fr


def effect(smpl, gm):
    pm = synth.identity_part_map()
    data, labels, D, L, fr = contaminated_frame(smpl)
    w0, p0, R0 = fr["start"]
    q0 = api.rot_to_quat(R0)
    opt = Options.demo(icp_iters=3)
    ctx = api.Context(gm, 24, pm, len(L), 1, device=0)
    start_err = np.linalg.norm(synth.pose_vertices(smpl, w0, p0, R0) - fr["gt_verts"], axis=1).mean()
    print(f"start state: {1e3 * start_err:.2f} mm mean vertex distance to the generating avatar")
    print("| frame | gate | mean vertex distance (mm) | final objective | correspondences of the last search | gated by it |")
    print("|---|---|---|---|---|---|")
    for name, d, l in (("contaminated (5 201 + 300 planted)", D, L), ("clean (5 201)", data, labels)):
        for g in (None, 0.1, 0.2, 0.3):
            ctx.set_corr_gate(g)
            _, _, _, st = ctx.optimize_batch([d], [l], opt, p0[None], q0[None], w0[None])
            err = np.linalg.norm(ctx.posed(0)[0] - fr["gt_verts"], axis=1).mean()
            print(f"| {name} | {'off' if g is None else g} | {1e3 * err:.2f} | {st[0].final_cost:.4f} | {st[0].num_correspondences} | {ctx.gated(0)} |", flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["cost", "effect"]
    smpl = synth.load_model(0)
    gm = api.AvatarModel(smpl)
    if "cost" in what:
        cost(smpl, gm)
    if "effect" in what:
        effect(smpl, gm)
