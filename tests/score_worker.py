"""Worker of tests/test_scores_cpu.py and tests/test_scores_gpu.py (not collected by pytest).

    python -m torch.distributed.run --nproc-per-node N tests/score_worker.py gather OUT.npy
        no GPU: N ranks over gloo hand their `frames_of` shares of `gather_row(j)` to parallel.gather_frame_rows.
    python [-m torch.distributed.run --nproc-per-node 2] tests/score_worker.py head OUT.npy DATASET_DIR
        the head dataset at DATASET_DIR (clip_worker.head_dataset wrote it) through clip.score_head_clip, alone or as two
        ranks sharing GPU 0 over gloo.

Rank 0 saves what it received to OUT.npy; every rank prints one JSON line {"rank": r, "got": "rows" | "none", ...}.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GATHER_FRAMES, GATHER_K = 10, 7
SCORE_FRAMES = 5


def gather_row(j):
    """Row of frame j: a function of j and of the column, so order, loss and duplication all show."""
    return np.arange(GATHER_K, dtype=np.float64) * 0.5 + 100.0 * j + 1.0 / (j + 3)


def gather(rank, world):
    from idealnerf_amd.parallel import frames_of, gather_frame_rows
    mine = np.stack([gather_row(j) for j in frames_of(rank, world, GATHER_FRAMES)])
    return gather_frame_rows(torch.from_numpy(mine), GATHER_FRAMES, None)


def head(datadir):
    import clip_worker as cw
    from types import SimpleNamespace
    from idealnerf_amd import clip, dataset
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    args = SimpleNamespace(gt_dirs="head_imgs", testskip=1, N_rand=64, sample_rate=0.95, mouth_rays=8, torso_rays=4)
    frames = dataset.ResidentFrames(datadir, "aud.npy", "val", args, skip=1, device=dev)
    net = cw.head_network(dev, frames.focal)
    res = clip.score_head_clip(net, frames, net.args.nosmo_iters, latent_code=torch.ones(32), frame_ids=range(SCORE_FRAMES))
    return None if res is None else (res["table"], {k: res[k] for k in ("frames", "n_frames", "nonfinite_frames", "world")})


def main():
    import torch.distributed as dist
    mode, out = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import datetime
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=int(os.environ.get("IDN_DIST_TIMEOUT_S", "120"))))
    try:
        info = {}
        if mode == "gather":
            rows = gather(rank, world)
        else:
            res = head(sys.argv[3])
            rows, info = res if res is not None else (None, {})
        if rows is not None:
            np.save(out, rows.cpu().numpy())
        sys.stdout.write(json.dumps({"rank": rank, "got": "none" if rows is None else "rows", **info}) + "\n")   # one write per line
        sys.stdout.flush()
    finally:
        if world > 1:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
