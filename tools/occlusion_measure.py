"""What the render occlusion (include/avt.h, avt_set_occlusion_render) costs and what it buys, in one process on one GPU:
python tools/occlusion_measure.py [cost] [fit] [frames=N ...]

cost: optimize() time per call with occlusion off, with the back-face test and with the face-id render at 1280 x 720 and 320 x 180, one
      38 k-point frame and 64 frames, icp_iters 1 and 3, and the share of the visibility class in the profiled time.
fit:  on the benchmark's twelve seeds and on a set of self-occluding poses (forearms in front of the torso), per mode: mean vertex
      distance of the fitted avatar to the generating one, final objective, and how many correspondences of the first ICP iteration
      land on vertices that tests/occlusion_restatement.py calls hidden."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from avatar_amd import api, synth
from avatar_amd.capi import Options

K4A = synth.K4A_INTRIN
FRAMES = tuple(int(a[7:]) for a in sys.argv[1:] if a.startswith("frames=")) or (1, 64)      # frames=N (repeatable): the batch sizes of `cost`
SMALL = dict(fx=K4A["fx"] / 4, fy=K4A["fy"] / 4, cx=K4A["cx"] / 4, cy=K4A["cy"] / 4, width=320, height=180)
MODES = (("off", 0, None), ("back-face", 1, None), ("render 1280x720", 1, K4A), ("render 320x180", 1, SMALL))


def set_mode(ctx, cam):
    ctx.set_occlusion_render(None if cam is None else (cam["width"], cam["height"]), cam)


def upload(ctx, frs):
    ctx.frames_upload([f["data"] for f in frs], [f["labels"] for f in frs])
    ctx.state_upload(np.array([f["start"][1] for f in frs]), np.array([api.rot_to_quat(f["start"][2]) for f in frs]), np.array([f["start"][0] for f in frs]))


def cost(smpl, gm):
    pm = synth.identity_part_map()
    base = [synth.make_frame(smpl, s) for s in range(4)]
    print("| frames | icp_iters | mode | ms per optimize() | visibility ms (launches) | share |")
    print("|---|---|---|---|---|---|")
    for F in FRAMES:
        frs = [base[s % 4] for s in range(F)]
        ctx = api.Context(gm, 24, pm, max(len(f["labels"]) for f in frs), F, device=0)
        upload(ctx, frs)
        for icp in (1, 3):
            for name, enable, cam in MODES:
                set_mode(ctx, cam)
                opt = Options.demo(icp_iters=icp, enable_occlusion=enable)
                for _ in range(3):
                    ctx.state_reset(); ctx.optimize_resident(opt)
                ctx.sync()
                steps = 30 if F == 1 else 10
                t0 = time.perf_counter()
                for _ in range(steps):
                    ctx.state_reset(); ctx.optimize_resident(opt)
                ctx.sync()
                ms = (time.perf_counter() - t0) / steps * 1e3
                ctx.profile_begin(); ctx.state_reset(); ctx.optimize_resident(opt); ctx.sync(); prof = ctx.profile_end()
                tot = sum(v[0] for v in prof.values())
                vis = prof.get("visibility", (0.0, 0))
                print(f"| {F} | {icp} | {name} | {ms:.3f} | {vis[0]:.4f} ({vis[1]}) | {100 * vis[0] / tot:.1f} % |", flush=True)


ARMS = [(1.8, 1.5), (1.6, 1.5), (2.0, 1.3), (1.8, 1.1), (1.5, 1.7), (2.1, 1.6)]      # (shoulder about y, elbow about z) in rad, both arms


def arm_frame(smpl, i):
    sh, el = ARMS[i]
    R = np.tile(np.eye(3), (24, 1, 1))
    R[0] = synth.rodrigues(np.array([0.0, np.pi + 0.15 * (i - 2.5), 0.0]))
    for j, aa in {16: (0.0, sh, 0.0), 18: (0.0, 0.0, -el), 17: (0.0, -sh, 0.0), 19: (0.0, 0.0, el)}.items():
        R[j] = synth.rodrigues(np.array(aa))
    w, p = np.zeros(10), np.array([0.1 * (i - 2.5), 0.0, 2.4])
    verts = synth.pose_vertices(smpl, w, p, R)
    data, labels = synth.render_cloud(smpl, verts, synth.identity_part_map())
    w0, p0, R0 = synth.perturb_start(w, p, R, 100 + i)
    return dict(data=data, labels=labels, gt=(w, p, R), start=(w0, p0, R0), gt_verts=verts)


def fit(smpl, gm):
    import occlusion_restatement as occ
    pm = synth.identity_part_map()
    mesh = np.asarray(smpl["f"])
    sets = {"twelve seeds": [synth.make_frame(smpl, s) for s in range(12)], "self-occluding": [arm_frame(smpl, i) for i in range(len(ARMS))]}
    print("| set | mode | mean vertex error (mm) | final objective (mean) | first-iteration correspondences on hidden vertices (of all) |")
    print("|---|---|---|---|---|")
    for sname, frs in sets.items():
        F = len(frs)
        ctx = api.Context(gm, 24, pm, max(len(f["labels"]) for f in frs), F, device=0)
        hidden = None
        for name, enable, cam in MODES[:3]:
            set_mode(ctx, cam)
            upload(ctx, frs)
            ctx.optimize_resident(Options.demo(icp_iters=1, max_iters_per_icp=0, enable_occlusion=enable))
            if hidden is None:          # the start clouds are the same in every mode
                hidden = [occ.visible(ctx.posed(f)[0], mesh, K4A, K4A["width"], K4A["height"]) == 0 for f in range(F)]
            on_hidden = tot = 0
            for f in range(F):
                c = ctx.correspondences(f, len(frs[f]["labels"]))
                on_hidden += int(hidden[f][c[c >= 0]].sum()); tot += int((c >= 0).sum())
            upload(ctx, frs)
            ctx.optimize_resident(Options.demo(icp_iters=3, enable_occlusion=enable))
            p, q, w, st = ctx.state_download()
            err = np.mean([np.linalg.norm(ctx.posed(f)[0] - frs[f]["gt_verts"], axis=1).mean() for f in range(F)])
            obj = np.mean([st[f].final_cost for f in range(F)])
            print(f"| {sname} | {name} | {1e3 * err:.2f} | {obj:.4f} | {on_hidden} ({tot}) |", flush=True)


if __name__ == "__main__":
    what = [a for a in sys.argv[1:] if not a.startswith("frames=")] or ["cost", "fit"]
    smpl = synth.load_model(0)
    gm = api.AvatarModel(smpl)
    if "cost" in what:
        cost(smpl, gm)
    if "fit" in what:
        fit(smpl, gm)
