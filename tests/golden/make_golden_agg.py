#!/usr/bin/env python3
"""Golden fixtures of the feature-aggregation model, from the REFERENCE itself on the CPU (build container only, like
make_golden.py, whose stand-ins for the optional imports this script uses):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_agg.py

``configs_agg_parsed.json``  the two shipped ``configs/agg_aud_expr_nerf/*/feat_agg.txt``: their lines, whether the
                             reference's parser rejects them as shipped (it does: ``use_highlight`` is not one of its flags,
                             although the agg trainer reads ``args.use_highlight``), and the values it resolves once that
                             switch is added to it.
``agg_train_step.npz``       one training step of the reference's agg ``Network`` (NeRFs/HeadNeRF/train/agg_aud_exp_nerf.py):
                             64 rays of the 32 x 32 scene, perturb 0 -- loss, rgb maps and the tensor selection of
                             train_step.npz plus the four ``agg_linears`` gradients of each network (of the weight
                             gradients with 128 rows or more every second row: the file stays under 1 MiB).  Weights are not stored:
                             Xavier-uniform from numpy RandomState(seed) in state_dict order, bias 0.01, the density head
                             scaled by 300 with bias 0.3 (seeds 6 / 7: both volumes are
                             occupied), as the tests rebuild them.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import NEAR, FAR, REF, REPO, install_shims  # noqa: E402

GRAD_KEYS = ("pts_linears.0.weight", "pts_linears.0.bias", "pts_linears.5.weight", "pts_linears.7.weight",
             "views_linears.0.weight", "views_linears.2.bias", "alpha_linear.weight", "alpha_linear.bias",
             "rgb_linear.weight", "rgb_linear.bias",
             "agg_linears.0.weight", "agg_linears.0.bias", "agg_linears.1.weight", "agg_linears.1.bias")


SEEDS = (6, 7)
ROW_STEP = 2   # weight gradients with 128 rows or more are stored as their rows [::2]: the fixture stays under 1 MiB


def recipe(module, seed, gain, bias):
    rs = np.random.RandomState(seed)
    sd = {}
    for k, v in module.state_dict().items():
        if k.endswith(".weight"):
            bound = float(np.sqrt(6.0 / (v.shape[0] + v.shape[1])))
            sd[k] = torch.from_numpy(rs.uniform(-bound, bound, size=tuple(v.shape)).astype(np.float32))
        else:
            sd[k] = torch.full(tuple(v.shape), 0.01, dtype=torch.float32)
    sd["alpha_linear.weight"] = sd["alpha_linear.weight"] * gain
    sd["alpha_linear.bias"] = torch.full_like(sd["alpha_linear.bias"], bias)
    module.load_state_dict(sd)


def configs(helper):
    import glob
    out = {}
    for path in sorted(glob.glob(os.path.join(REF, "NeRFs/HeadNeRF/configs/agg_aud_expr_nerf/*/feat_agg.txt"))):
        lines = [l.strip() for l in open(path) if l.strip() and l.strip()[0] not in "#;"]
        argv = []
        for l in lines:
            if "=" in l:
                k, v = [t.strip() for t in l.split("=", 1)]
                argv += ["--" + k, v]
            else:
                argv += ["--" + l]
        rejected = False
        try:
            with contextlib.redirect_stderr(io.StringIO()):
                helper.config_parser().parse_args(argv)
        except SystemExit:
            rejected = True
        parser = helper.config_parser()
        parser.add_argument("--use_highlight", action="store_true")
        ns = parser.parse_args(argv)
        out[os.path.relpath(path, REF)] = {"lines": lines, "rejected_by_head_parser": rejected,
                                           "parsed": {k: v for k, v in vars(ns).items() if k != "config"}}
    with open(os.path.join(HERE, "configs_agg_parsed.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)


def train_step():
    import importlib
    import oracle
    agg = importlib.import_module("NeRFs.HeadNeRF.train.agg_aud_exp_nerf")
    helper = importlib.import_module("NeRFs.HeadNeRF.helper")
    dims = oracle.facenerf_dims(dim_aud=64, dim_expr=79, dim_latent=32)
    syn = oracle.synthetic_frame(32, 32, seed=0, dims=dims)
    torch.manual_seed(1234)
    net = agg.Network(32, 32, syn["focal"], NEAR, FAR, 512, None, 64, 128)
    recipe(net.face_nerf_coarse, SEEDS[0], 300.0, 0.3)
    recipe(net.face_nerf_fine, SEEDS[1], 300.0, 0.3)
    net.train()
    rays = torch.from_numpy(np.load(os.path.join(HERE, "frame32.npz"))["rays"])
    sel = torch.from_numpy(np.load(os.path.join(HERE, "train_step.npz"))["sel"])
    rs = np.random.RandomState(79)
    tgt = torch.from_numpy(rs.uniform(0, 1, size=(sel.numel(), 3)).astype(np.float32))
    aud = syn["aud"].clone().requires_grad_(True)
    lat = syn["latent"].clone().requires_grad_(True)
    ret = net.render_rays(rays[sel], syn["bc"].reshape(-1, 3)[sel], aud, syn["c2w"], lat, syn["expr"])
    img_loss = helper.img2mse(ret["rgb_map"], tgt)
    loss = img_loss + helper.img2mse(ret["rgb0"], tgt) + 10 * (torch.norm(lat) * 0.0005)
    loss.backward()
    fx = dict(sel=sel.numpy(), target=tgt.numpy(), loss=loss.detach().numpy(), img_loss=img_loss.detach().numpy(),
              rgb_map=ret["rgb_map"].detach().numpy(), rgb0=ret["rgb0"].detach().numpy(), g_aud=aud.grad.numpy(),
              g_latent=lat.grad.numpy(), seed_coarse=np.int64(SEEDS[0]), seed_fine=np.int64(SEEDS[1]))
    for tag, m in (("c", net.face_nerf_coarse), ("f", net.face_nerf_fine)):
        named = dict(m.named_parameters())
        for k in GRAD_KEYS:
            grad = named[k].grad.numpy()
            fx[f"g_{tag}_{k}"] = grad[::ROW_STEP] if grad.ndim == 2 and grad.shape[0] >= 128 else grad
    fx["row_step"] = np.int64(ROW_STEP)
    np.savez_compressed(os.path.join(HERE, "agg_train_step.npz"), **fx)
    print("agg_train_step.npz", os.path.getsize(os.path.join(HERE, "agg_train_step.npz")) // 1024, "KiB")


def main():
    install_shims()
    sys.argv = [sys.argv[0], "--perturb", "0", "--dim_aud", "64", "--N_samples", "64", "--N_importance", "128",
                "--near", str(NEAR), "--far", str(FAR), "--vis_path", "/tmp/idealnerf_golden_vis", "--chunk", "512"]
    sys.path.insert(0, REF)
    sys.path.insert(0, REPO)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import importlib
    helper = importlib.import_module("NeRFs.HeadNeRF.helper")
    configs(helper)
    train_step()


if __name__ == "__main__":
    main()
