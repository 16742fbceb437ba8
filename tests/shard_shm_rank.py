"""One rank of tests/test_gpu_shard_contract.py's shared-memory case, run as a fresh process (a helper, not a test file):

    python shard_shm_rank.py RANK ID_HEX RANK1_POINTS

Two ranks on device 0 over avt_shard_create_shm.  Rank 0 scatters a batch of 12 frames whose odd frames - rank 1's share - total
RANK1_POINTS points (five frames of 8192 and the rest in the sixth), so that the coordinate block rank 1 receives is RANK1_POINTS x 24
bytes: 43690 points fill one 1 MiB chunk of the segment to 16 bytes under its end, 43691 need a second chunk of 8 bytes.  Each rank
compares every frame it then holds with the batch, bit for bit, and prints its verdict; a rank that saw a difference exits with 1."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import fit_models as fm  # noqa: E402

W, B, MAX_FRAMES, MAX_POINTS = 2, 12, 6, 8192
RANK0_COUNTS = (7, 0, 100, 3, 1, 50)
MODEL = (9, 4, "star")


def batch(rank1_points):
    """(datas, labels, p, q, w) of the 12 frames, the same on every rank"""
    J, K = MODEL[:2]
    rest = rank1_points - 5 * MAX_POINTS
    assert 0 <= rest <= MAX_POINTS
    counts = [0] * B
    counts[0::2] = RANK0_COUNTS
    counts[1::2] = [MAX_POINTS] * 5 + [rest]
    rng = np.random.default_rng([20261020, rank1_points])
    datas = [rng.standard_normal((n, 3)) for n in counts]
    labels = [rng.integers(0, J, n).astype(np.int32) for n in counts]
    q = np.zeros((B, J, 4)); q[:, :, 3] = 1.0
    return datas, labels, np.zeros((B, 3)), q, np.zeros((B, K))


def main():
    from avatar_amd import api, shard
    rank, unique_id, rank1_points = int(sys.argv[1]), bytes.fromhex(sys.argv[2]), int(sys.argv[3])
    J, K, tree = MODEL
    gm = api.AvatarModel(fm.fit_model(J, K, tree))
    ctx = api.Context(gm, J, np.arange(J, dtype=np.int32), MAX_POINTS, MAX_FRAMES, device=0)
    sh = shard.Shard(0, rank, W, unique_id, shm=True)
    assert "shared memory" in sh.backend
    datas, labels, p, q, w = batch(rank1_points)
    if rank == 0:
        sh.scatter_frames(ctx, B, datas, labels, p, q, w, root=0)
    else:
        sh.scatter_frames(ctx, B, root=0)
    mine = shard.frames_of_rank(B, rank, W)
    ctx._N = np.array([len(labels[f]) for f in mine], np.int32)
    bad = []
    for i, f in enumerate(mine):
        d, l = ctx.frame_download(i)
        if not (np.array_equal(d, datas[f]) and np.array_equal(l, labels[f])):
            bad.append(f)
    sh.barrier(ctx)
    sh.close()
    print(f"rank {rank}: {sum(len(labels[f]) for f in mine)} points in {len(mine)} frames, " + (f"frames {bad} differ" if bad else "verdict ok"), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
