#!/usr/bin/env python
"""Train a head model with ``idealnerf_amd.train.train`` -- the reference's ``train()`` (NeRFs/HeadNeRF/train/audio_exp_nerf.py)
-- and measure what the two loaders cost.

    python tools/train_head.py --config <file> [upstream's flags] [--loader resident|reference] [--steps N] [--sample-seed S]
    python tools/train_head.py --timing-json profiles/train_loop.json [--generate 300] [--steps 60]

Upstream's flags go through ``helper.config_parser``.  ``--timing-json`` (needs a GPU; no fallback) measures on ONE device, in
one process, the two loaders alternating round by round:

    reference   wall time per step of the loop fed by dataset.GetData   (decode, numpy draw, full-frame rays, gather)
    resident    wall time per step of the loop fed by dataset.ResidentFrames
    floor       the bare train_step on batches prepared in advance
    sampler     HIP-event time of one ResidentFrames.batch (both launches), and the host's time inside that call

Every window ends in a device synchronise and follows warm-up steps of its own shape.  ``--generate N`` writes an N-frame
450 x 450 directory (synthetic.write_clip_directory) under ``--datadir`` when that directory does not exist.  Prints one JSON
line; with a path, writes the same object there (merged over what the file already holds).
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv):
    from idealnerf_amd.helper import config_parser
    p = config_parser()
    p.add_argument("--loader", type=str, default="resident", choices=("resident", "reference"))
    p.add_argument("--steps", type=int, default=None, help="stop after this many steps (timing: steps per window, default 60)")
    p.add_argument("--sample-seed", type=int, default=0)
    p.add_argument("--timing-json", type=str, default=None)
    p.add_argument("--generate", type=int, default=0, help="frames of the generated 450 x 450 directory (timing)")
    return p.parse_args(argv)


ROUNDS, WARMUP, SIZE = 3, 10, 450    # timing: rounds of (reference, resident, floor) windows; warm-up steps before each window


def timing(args):
    import numpy as np
    import torch
    from idealnerf_amd import dataset, synthetic, train as T_
    from idealnerf_amd.audio_exp_nerf import Network, init_weights
    from idealnerf_amd.config import to_render_config
    if not torch.cuda.is_available():
        raise SystemExit("--timing-json measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    if args.generate and not os.path.isdir(args.datadir):
        os.makedirs(args.datadir)
        synthetic.write_clip_directory(args.datadir, SIZE, args.generate, seed=0)
    steps = args.steps or 60
    t0 = time.perf_counter()
    frames = dataset.ResidentFrames(args.datadir, args.aud_file, "train", args, device=dev, seed=args.sample_seed)
    load_s = time.perf_counter() - t0
    ds = dataset.GetData(args.datadir, args.aud_file, "train", args, device=dev)
    n = len(frames)
    torch.manual_seed(0)
    net = Network(frames.H, frames.W, frames.focal, near=args.near, far=args.far, chunk=args.chunk, intrinsic=None,
                  N_samlpes=args.N_samples, N_importance=args.N_importance, args=to_render_config(args)).to(dev)
    lat = torch.ones(n, 32, dtype=torch.float32, device=dev)
    net.apply(init_weights)
    lat.requires_grad = True
    opt = T_.make_optimizer(net, lat, args.lrate)
    net.train()
    prepared = []
    for i in range(16):                          # batches prepared in advance: the three sampled tensors copied out of the loader
        b = frames.batch(i % n, i)
        prepared.append(tuple(t.clone() for t in b[:3]) + b[3:])
    feeds = {"reference": lambda s: T_._as_loader_item(ds[s % n]),
             "resident": lambda s: frames.batch(s % n, s),
             "floor": lambda s: prepared[s % len(prepared)]}
    step = [0]

    def window(feed, count):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            data = feed(step[0])
            T_.train_step(net, opt, data, lat, step[0], n, lrate=args.lrate, lrate_decay=args.lrate_decay)
            step[0] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count * 1e3

    np.random.seed(0)
    per_round = {k: [] for k in feeds}
    for _ in range(ROUNDS):
        for name, feed in feeds.items():         # the same order in every round: reference, resident, floor
            window(feed, WARMUP)
            per_round[name].append(window(feed, steps))

    # the sampler alone: device time by events around one batch() on an idle stream, and the host's time inside the call
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
    host = []
    for i in range(10):
        frames.batch(i % n, i)
    for i, (a, b) in enumerate(ev):
        torch.cuda.synchronize()
        a.record()
        t = time.perf_counter()
        frames.batch(i % n, 1000 + i)
        host.append((time.perf_counter() - t) * 1e3)
        b.record()
    torch.cuda.synchronize()
    device = [a.elapsed_time(b) for a, b in ev]
    # ... and behind a busy stream: how far ahead of the device the host leaves batch() inside a running loop
    lead = []
    for i in range(20):
        T_.train_step(net, opt, prepared[i % len(prepared)], lat, step[0], n, lrate=args.lrate, lrate_decay=args.lrate_decay)
        step[0] += 1
        done = torch.cuda.Event()
        frames.batch(i % n, 2000 + i)
        done.record()
        t = time.perf_counter()
        done.synchronize()
        lead.append((time.perf_counter() - t) * 1e3)

    med = lambda v: float(statistics.median(v))
    out = {"timing": {
        "device": torch.cuda.get_device_name(0), "size": [frames.H, frames.W], "frames": n, "N_rand": args.N_rand,
        "mouth_rays": args.mouth_rays, "torso_rays": args.torso_rays, "N_samples": args.N_samples, "N_importance": args.N_importance,
        "perturb": args.perturb, "steps_per_window": steps, "warmup_steps": WARMUP, "rounds": ROUNDS,
        "resident_load_s": load_s, "resident_bytes": int(frames.maps.numel() + frames.imgs.numel() + frames.background.numel()),
        "step_ms_reference": per_round["reference"], "step_ms_resident": per_round["resident"], "step_ms_floor": per_round["floor"],
        "step_ms_reference_median": med(per_round["reference"]), "step_ms_resident_median": med(per_round["resident"]),
        "step_ms_floor_median": med(per_round["floor"]),
        "sampler_device_ms_median": med(device), "sampler_device_ms_max": max(device),
        "batch_host_ms_median": med(host), "batch_host_ms_max": max(host),
        "host_wait_for_batch_after_return_ms_median": med(lead),
    }}
    return out


def main(argv=None):
    args = parse(argv)
    if args.timing_json is not None:
        if args.generate:                        # the reference's size and split on the generated directory
            args.N_rand, args.mouth_rays, args.dim_aud, args.dim_expr = 3072, 256, 64, 76
        out = timing(args)
        if args.timing_json not in ("", "-"):
            old = json.load(open(args.timing_json)) if os.path.exists(args.timing_json) else {}
            old.update(out)
            os.makedirs(os.path.dirname(os.path.abspath(args.timing_json)), exist_ok=True)
            json.dump(old, open(args.timing_json, "w"), indent=1)
        print(json.dumps(out))
        return out
    import torch
    from idealnerf_amd import train as T_
    t0 = time.perf_counter()
    run = T_.train(args, loader=args.loader, sample_seed=args.sample_seed, steps=args.steps)
    torch.cuda.synchronize()
    out = {"loader": args.loader, "global_step": run["global_step"], "frames": run["data_size"], "seconds": time.perf_counter() - t0}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
