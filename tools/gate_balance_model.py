#!/usr/bin/env python3
"""CPU model of the colour gate's gain on the benchmark's frame, by the order in which the persistent workgroups take tiles.

    python tools/gate_balance_model.py [--size 512] [--cus 256] [--skews 1,33,97,...] [--dead-map FILE.npy]

The coarse pass of `synthetic.frame(size, size, seed=0)` with the bench's coarse network (seed 2, sigma gain 300, bias 0.3)
is run through the CPU oracle, pass by pass as the render does it (32 768 rays each), and every 128-point tile is marked
all-dead by the gate's predicate (csrc/mlp_common.h: gate_point_dead).  A dead tile costs 1 - 1088 / 8768 of a live one (the
colour branch's share of a pass's MFMAs), a launch ends with its slowest CU, and the figure per order is the launch's time
relative to the ungated launch (every tile live).  Orders: the plain grid-stride walk, contiguous blocks, the skewed walk of
csrc/tile_order.h for a list of strides, tiles handed out in order to whichever CU is free (what an atomic counter would do),
and the ideal balance.  No fine tile of this frame is dead (98.8 % of its points have sigma > 0), so only the coarse launches
are modelled.  About two minutes on 16 threads; writes profiles/gate_balance_model.json.  Not part of the test suite.
"""
import argparse
import heapq
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S = 64
PASS_RAYS = 32768
DEAD_COST = 1.0 - 1088.0 / 8768.0


def header_skew():
    src = open(os.path.join(ROOT, "ideal-nerf_amd", "csrc", "tile_order.h")).read()
    return int(re.search(r"#define IDN_TILE_SKEW (\d+)", src).group(1))


def dead_tiles(size):
    """-> list of bool arrays, one per pass: tile t of the pass is all dead"""
    import idealnerf_amd
    import oracle
    from idealnerf_amd import synthetic
    from oracle import render_oracle
    kmax = float(idealnerf_amd._lib.load().idealnerf_colour_gate_max_dist())
    syn = synthetic.frame(size, size, seed=0)
    net = synthetic.xavier_state_dict(idealnerf_amd.FaceNeRF(dim_aud=64, dim_latent=32, dim_expr=76), 2, 300.0, 0.3)
    params = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    ro, rd = oracle.camera_rays(size, size, syn["focal"], syn["c2w"])
    rays = oracle.ray_records(ro, rd, syn["near"], syn["far"]).reshape(-1, 11)
    dims = oracle.facenerf_dims()
    out = []
    with torch.no_grad():
        for i in range(0, rays.shape[0], PASS_RAYS):
            r = rays[i:i + PASS_RAYS]
            o, d, view = r[:, 0:3], r[:, 3:6], r[:, -3:]
            z = oracle.coarse_depths(r[:, 6:7], r[:, 7:8], S)
            raw = render_oracle._query(params, o[:, None, :] + d[:, None, :] * z[:, :, None], view,
                                              syn["aud"], syn["expr"], syn["latent"], dims)
            dn = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            dist = (z[:, 1:] - z[:, :-1]) * dn[:, None]
            dead = torch.ones(z.shape, dtype=torch.bool)
            dead[:, :-1] = (raw[:, :-1, 3] <= 0.0) & (dist.abs() <= kmax)
            flat = dead.reshape(-1)
            pad = (-flat.numel()) % 128
            if pad:
                flat = torch.cat([flat, torch.ones(pad, dtype=torch.bool)])   # points beyond n_points are dead
            out.append(flat.reshape(-1, 128).all(1).numpy())
            print(f"pass {len(out)}: {out[-1].mean():.3f} of {out[-1].size} coarse tiles all dead", flush=True)
    return out


def launch_time(cost, cu_of_tile, G):
    """slowest CU's load over the ungated launch's (every tile live, plain order)"""
    load = np.bincount(cu_of_tile, weights=cost, minlength=G)
    return float(load.max() / np.ceil(cost.size / G))


def orders(dead, G, skews):
    n = dead.size
    g = min(G, n)
    cost = np.where(dead, DEAD_COST, 1.0)
    t = np.arange(n)
    r, pos = t // g, t % g
    res = {"grid_stride": launch_time(cost, pos, g), "contiguous": launch_time(cost, t // int(np.ceil(n / g)), g)}
    for k in skews:
        res[f"skew_{k}"] = launch_time(cost, (pos - r * k) % g, g)   # tile(r, c) = r g + (c + r k) mod g
    free = [(0.0, c) for c in range(g)]
    heapq.heapify(free)
    for c in cost:   # tiles in order to the CU that is free first
        at, cu = heapq.heappop(free)
        heapq.heappush(free, (at + c, cu))
    res["dynamic"] = float(max(a for a, _ in free) / np.ceil(n / g))
    res["ideal"] = float(cost.sum() / g / np.ceil(n / g))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--skews", default="", help="comma-separated strides to tabulate beside the header's (default: a spread of odd ones)")
    ap.add_argument("--dead-map", help="load the per-pass dead-tile map from this .npy if it exists, else write it there")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_balance_model.json"))
    args = ap.parse_args()
    shipped = header_skew()
    skews = [int(x) for x in args.skews.split(",") if x] or [1, 3, 17, 33, 65, 97, 127, 129, 161, 193, 225, 255]
    skews = sorted(set(skews) | {shipped})
    if args.dead_map and os.path.exists(args.dead_map):
        dead = list(np.load(args.dead_map, allow_pickle=True))
    else:
        dead = dead_tiles(args.size)
        if args.dead_map:
            np.save(args.dead_map, np.array(dead, dtype=object), allow_pickle=True)
    per_pass = [orders(d, args.cus, skews) for d in dead]
    names = list(per_pass[0])
    mean = {k: float(np.mean([p[k] for p in per_pass])) for k in names}
    # every odd stride, for the record of how the header's constant was chosen (mean and worst pass)
    odd = {}
    for k in range(1, args.cus, 2):
        v = [orders_one(d, args.cus, k) for d in dead]
        odd[k] = (float(np.mean(v)), float(np.max(v)))
    best = sorted(odd, key=lambda k: odd[k])[:8]
    print(f"\n{args.size} x {args.size}, {args.cus} CUs, {len(dead)} coarse passes; launch time / ungated launch")
    print("pass  dead    " + "  ".join(f"{k:>11s}" for k in names))
    for i, (d, p) in enumerate(zip(dead, per_pass)):
        print(f"{i:4d}  {d.mean():.3f}   " + "  ".join(f"{p[k]:11.4f}" for k in names))
    print("mean  {:.3f}   ".format(float(np.mean([d.mean() for d in dead]))) + "  ".join(f"{mean[k]:11.4f}" for k in names))
    print("best odd strides (mean, worst pass): " + ", ".join(f"{k}: {odd[k][0]:.4f} / {odd[k][1]:.4f}" for k in best))
    print(f"header's IDN_TILE_SKEW = {shipped}: {odd[shipped][0]:.4f} / {odd[shipped][1]:.4f}" if shipped in odd else f"header's IDN_TILE_SKEW = {shipped}")
    coarse_share = S / (S + S + 128.0)   # the fine network runs the coarse depths again beside the 128 new ones
    print(f"frame (coarse = {coarse_share:.3f} of the samples): plain order {1 - coarse_share * (1 - mean['grid_stride']):.4f}, "
          f"skew {shipped} {1 - coarse_share * (1 - mean[f'skew_{shipped}']):.4f}, ideal {1 - coarse_share * (1 - mean['ideal']):.4f} of ungated")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"size": args.size, "cus": args.cus, "dead_tile_cost": DEAD_COST, "header_skew": shipped,
                   "dead_share_per_pass": [float(d.mean()) for d in dead], "per_pass": per_pass, "mean": mean,
                   "odd_strides_mean_and_worst": {str(k): odd[k] for k in odd}}, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(args.out, ROOT))


def orders_one(dead, G, k):
    n = dead.size
    g = min(G, n)
    cost = np.where(dead, DEAD_COST, 1.0)
    t = np.arange(n)
    return launch_time(cost, (t % g - (t // g) * k) % g, g)


if __name__ == "__main__":
    main()
