"""``python tests/golden/make_golden_torso_sample_rays.py`` -> tests/golden/torso_sample_rays.npz.

The torso stage's region-weighted ray sampler from the reference's own code: ``GetData.sample_rays`` of
NeRFs/TorsoNeRF/train_torso.py (:130-183), imported with the stand-ins of ``make_golden.install_shims`` (as ``make_golden.py
headtorso`` imports that module), called under a fixed numpy seed on one H = 96, W = 128 frame: face_rect = [8, 8, 40, 40],
mouth landmarks inside [30, 34] on both axes, N_rand = 64, sample_rate = 0.95 -- once with ``use_highlight`` off, once on.

By arithmetic the mouth box is at most 45 x 45 = 2025 pixels (rows / columns 10 .. 54), the outside population is
96 * 128 - 41 * 41 = 10 607, so upstream's mouth indexing (``coords_norect[select_inds_mouth]``) stays in range; the rect minus
the box keeps at least 41 * 41 - 39 * 39 = 160 pixels against the 45 drawn.

Stored: the inputs, and per case (suffix ``_off`` / ``_on``) the selected coordinates and the four outputs.  ``sample_rays`` does
not return the coordinates: they are read off a second call under the same seed whose `target` image holds every pixel's own
(row, col).  Data only.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

H, W, FOCAL, N_RAND, RATE, SEED = 96, 128, 1200.0 * 128 / 450.0, 64, 0.95, 11


def main():
    mg.install_shims()
    sys.argv = [sys.argv[0], "--perturb", "0", "--dim_aud", "64", "--dim_aud_body", "64", "--N_samples", "64",
                "--N_importance", "128", "--near", str(mg.NEAR), "--far", str(mg.FAR), "--chunk", "512",
                "--vis_path", "/tmp/idealnerf_golden_vis"]
    for p in (mg.REPO, mg.REF, os.path.join(mg.REF, "NeRFs", "TorsoNeRF")):
        sys.path.insert(0, p)
    import oracle
    import functools
    helpers = importlib.import_module("NeRFs.TorsoNeRF.run_nerf_helpers")
    real_get_embedder = helpers.get_embedder   # (its default device is 'cuda': the module builds three embedders at import)
    helpers.get_embedder = functools.wraps(real_get_embedder)(lambda multires, i=0, device="cpu": real_get_embedder(multires, i, device))
    mg.torso_raw2outputs()      # imports NeRFs.TorsoNeRF.run_nerf and supplies its missing `F`
    tt = importlib.import_module("NeRFs.TorsoNeRF.train_torso")
    torch.autograd.set_detect_anomaly(False)

    rs = np.random.RandomState(SEED)
    pose = oracle.synthetic_frame(H, W, seed=6)["c2w"].numpy().astype(np.float64)[:3, :4]
    pose0 = oracle.synthetic_frame(H, W, seed=7)["c2w"].numpy().astype(np.float64)[:3, :4]
    rect = np.array([8, 8, 40, 40], dtype=np.int32)
    lms = rs.uniform(6, 90, size=(68, 2))
    lms[48:] = rs.uniform(30, 34, size=(20, 2))
    image = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    background = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    target = torch.as_tensor(torch.tensor(image)).float() / 255.0        # train_torso.py:97
    bc_img = torch.tensor(background / 255.0)                            # :61-62, float64
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    where = torch.from_numpy(np.stack([rows, cols, np.zeros_like(rows)], -1))

    ds = object.__new__(tt.GetData)
    ds.H, ds.W, ds.focal, ds.cx, ds.cy = H, W, FOCAL, W / 2.0, H / 2.0
    ds.args = types.SimpleNamespace(N_rand=N_RAND, sample_rate=RATE)
    ds.all_poses = [np.concatenate([pose0, [[0.0, 0.0, 0.0, 1.0]]], 0)]
    fx = dict(pose=pose, pose_torso=pose0, rect=rect, landmark=lms, image=image, background=background, focal=FOCAL, cx=W / 2.0,
              cy=H / 2.0, N_rand=N_RAND, sample_rate=RATE, seed=SEED)
    for tag, highlight in (("off", False), ("on", True)):
        tt.args.use_highlight = highlight
        with torch.no_grad():
            np.random.seed(SEED)
            rays, rays_torso, target_s, bc_s = ds.sample_rays(pose, rect, target, bc_img, lms)
            np.random.seed(SEED)
            _, _, coords, _ = ds.sample_rays(pose, rect, where, bc_img, lms)
        fx.update({f"coords_{tag}": coords[:, :2].numpy().astype(np.int64), f"batch_rays_{tag}": rays.numpy(),
                   f"batch_rays_torso_{tag}": rays_torso.numpy(), f"target_s_{tag}": target_s.numpy(), f"bc_s_{tag}": bc_s.numpy()})
    np.savez_compressed(os.path.join(HERE, "torso_sample_rays.npz"), **fx)
    print({k: getattr(v, "shape", v) for k, v in fx.items()})


if __name__ == "__main__":
    main()
