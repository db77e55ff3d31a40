#!/usr/bin/env python3
"""Frame and train-step times of a narrow-encoding network next to the 10 / 4 network (profiles/multires.json: "timing").

    python tools/multires_timing.py [--out profiles/multires.json] [--pair 5 2]

One process, both arms alternating, HIP events around each window after a warm-up, the median over the windows and their
spread (max - min).  The forward kernels evaluate all ten / four octaves whatever the width (a narrow network's missing
columns are zeros in its weight stream), so the frame times are expected to be equal within the spread; the record tells a
later change whether skipping the unused octaves is worth touching those kernels for.

frame: one 450 x 450 frame, 64 + 128 samples, perturb 0, through ``Network.render_dynamic_face`` in "f32" and "bf16".
train: ``render_rays`` with gradients on 3072 rays, the reference's loss (mse(rgb) + mse(rgb0) + the latent norm term),
       backward and an Adam step -- the compute of one step at N_rand 3072, without a loader.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from idealnerf_amd import autograd  # noqa: E402
import oracle  # noqa: E402
from idealnerf_amd.audio_exp_nerf import Network, init_weights  # noqa: E402
from idealnerf_amd.helper import RenderConfig, img2mse  # noqa: E402
from idealnerf_amd.models.face_nerf import set_render_precision  # noqa: E402

H = W = 450
N_RAND = 3072


def build(pair, dev):
    cfg = RenderConfig(perturb=0.0, chunk=8192, multires=pair[0], multires_views=pair[1])
    dims = oracle.facenerf_dims(input_ch=3 + 6 * pair[0], input_ch_views=3 + 6 * pair[1])
    syn = oracle.synthetic_frame(H, W, seed=0, dims=dims)
    torch.manual_seed(0)
    net = Network(H, W, syn["focal"], cfg.near, cfg.far, cfg.chunk, None, 64, 128, args=cfg)
    net.apply(init_weights)
    for m, seed in ((net.face_nerf_coarse, 2), (net.face_nerf_fine, 3)):
        p = oracle.xavier_facenerf_params(seed, dims)
        p["alpha_linear.weight"] = p["alpha_linear.weight"] * 300.0
        p["alpha_linear.bias"] = torch.full_like(p["alpha_linear.bias"], 0.3)
        m.load_state_dict(p)
    return net.to(dev), syn


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summary(xs):
    return dict(median_ms=statistics.median(xs), spread_ms=max(xs) - min(xs), windows_ms=xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multires.json"))
    ap.add_argument("--pair", type=int, nargs=2, default=[5, 2])
    ap.add_argument("--windows", type=int, default=5)
    ns = ap.parse_args()
    dev = torch.device("cuda:0")
    arms = {f"{ns.pair[0]}_{ns.pair[1]}": tuple(ns.pair), "10_4": (10, 4)}
    nets = {k: build(p, dev) for k, p in arms.items()}
    g = lambda t: t.to(dev)
    rec = dict(device=torch.cuda.get_device_name(0), size=[H, W], N_samples=64, N_importance=128, N_rand=N_RAND, windows=ns.windows,
               frame={}, train={})

    def frame_fn(net, syn):
        def run():
            with torch.no_grad():
                net.render_dynamic_face(H, W, syn["focal"], expr=g(syn["expr"]), poses=syn["c2w"], latent_code=g(syn["latent"]),
                                        render_poses=syn["c2w"][:3, :4], chunk=8192, near=syn["near"], far=syn["far"],
                                        bc_rgb=g(syn["bc"]), aud_para=g(syn["aud"]))
        return run

    for mode in ("f32", "bf16"):
        fns = {}
        for k, (net, syn) in nets.items():
            net.eval()
            set_render_precision(net, mode)
            fns[k] = frame_fn(net, syn)
            fns[k]()                                     # warm-up: packs the stream, sizes the workspace
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(ns.windows):
            for k in fns:                                # the arms alternate
                times[k].append(timed(fns[k], 3))
        rec["frame"][mode] = {k: summary(v) for k, v in times.items()}

    steps = {}
    for k, (net, syn) in nets.items():
        net.train()
        gen = torch.Generator().manual_seed(1)
        ro, rd = oracle.camera_rays(H, W, syn["focal"], syn["c2w"])
        sel = torch.randperm(H * W, generator=gen)[:N_RAND]
        rays = g(oracle.ray_records(ro, rd, syn["near"], syn["far"])[sel].contiguous())
        bc, tgt = g(syn["bc"].reshape(-1, 3)[sel].contiguous()), g(torch.rand(N_RAND, 3, generator=gen))
        lat = g(syn["latent"]).clone().requires_grad_(True)
        opt = torch.optim.Adam(list(net.parameters()) + [lat], lr=5e-4)
        aud, expr = g(syn["aud"]), g(syn["expr"])

        def step(net=net, rays=rays, bc=bc, tgt=tgt, lat=lat, opt=opt, aud=aud, expr=expr):
            opt.zero_grad()
            ret = net.render_rays(rays, bc, aud, None, lat, expr)
            loss = img2mse(ret["rgb_map"], tgt) + img2mse(ret["rgb0"], tgt) + 10 * (torch.norm(lat) * 0.0005)
            loss.backward()
            opt.step()
        steps[k] = step
        for _ in range(5):
            step()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(ns.windows):
        for k in steps:
            times[k].append(timed(steps[k], 30))
    rec["train"] = {k: summary(v) for k, v in times.items()}
    rec["train"]["precision"] = autograd.TRAIN_PRECISION

    old = json.load(open(ns.out)) if os.path.exists(ns.out) else {}
    old["timing"] = rec
    os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
    json.dump(old, open(ns.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
