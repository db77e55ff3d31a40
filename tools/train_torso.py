#!/usr/bin/env python
"""Train the torso stage with ``idealnerf_amd.train_torso.train`` -- the reference's ``train()`` of
NeRFs/TorsoNeRF/train_torso.py -- and measure what the loaders and the frozen head pass cost.

    python tools/train_torso.py --config <file> [upstream's torso flags] [--loader resident|reference] [--steps N] [--sample-seed S]
    python tools/train_torso.py --timing-json profiles/torso_train_loop.json [--generate 300] [--steps 60]

Upstream's flags go through ``train_torso.config_parser``; the run directory ``basedir/expname`` is expected to hold the head
stage's ``head.tar`` (tools/train_head.py), as upstream's.  ``--timing-json`` (needs a GPU; no fallback) measures on ONE
device, in one process, four arms alternating round by round:

    reference   wall time per step of the loop fed by dataset.TorsoGetData
    resident    wall time per step of the loop fed by dataset.ResidentTorsoFrames
    floor       the bare torso_train_step on batches prepared in advance (head pair frozen: the conditioning-only backward)
    full_plan   the same bare step with the head pair's parameters left requiring gradients: the full backward of the head
                passes, whose weight gradients nobody reads -- the baseline the frozen plan has to beat

Every window ends in a device synchronise and follows warm-up steps of its own shape.  After the last window one held-out
frame is rendered and its whole-frame PSNR recorded (not asserted).  ``--generate N`` writes an N-frame 450 x 450 directory
(synthetic.write_clip_directory, expression width 79) under ``--datadir`` when that directory does not exist.  Prints one
JSON line; with a path, writes the same object there (merged over what the file already holds).
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv):
    from idealnerf_amd.train_torso import config_parser
    p = config_parser()
    p.add_argument("--loader", type=str, default="resident", choices=("resident", "reference"))
    p.add_argument("--steps", type=int, default=None, help="stop after this many steps (timing: steps per window, default 60)")
    p.add_argument("--sample-seed", type=int, default=0)
    p.add_argument("--timing-json", type=str, default=None)
    p.add_argument("--generate", type=int, default=0, help="frames of the generated 450 x 450 directory (timing)")
    return p.parse_args(argv)


ROUNDS, WARMUP, SIZE = 3, 10, 450    # timing: rounds of the four windows; warm-up steps before each window


def timing(args):
    import numpy as np
    import torch
    from idealnerf_amd import dataset, synthetic, train as T_, train_torso as TT
    from idealnerf_amd.audio_exp_nerf import init_weights
    from idealnerf_amd.config import to_render_config
    if not torch.cuda.is_available():
        raise SystemExit("--timing-json measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    if args.generate and not os.path.isdir(args.datadir):
        os.makedirs(args.datadir)
        synthetic.write_clip_directory(args.datadir, SIZE, args.generate, seed=0, dim_expr=79)
    steps = args.steps or 60
    t0 = time.perf_counter()
    frames = dataset.ResidentTorsoFrames(args.datadir, args.aud_file, "train", args, device=dev, seed=args.sample_seed)
    load_s = time.perf_counter() - t0
    ds = dataset.TorsoGetData(args.datadir, args.aud_file, "train", args, device=dev)
    n = len(frames)
    torch.manual_seed(0)
    cfg = to_render_config(args)
    cfg.dim_expr = frames.exprs.shape[1]
    net = TT.Network(frames.H, frames.W, frames.focal, near=args.near, far=args.far, chunk=args.chunk, N_samlpes=args.N_samples,
                     N_importance=args.N_importance, args=cfg, dim_aud_body=args.dim_aud_body, dim_expr_head=cfg.dim_expr).to(dev)
    lat = torch.ones(n, 32, dtype=torch.float32, device=dev)
    net.apply(init_weights)
    opt = torch.optim.Adam([p for m in (net.torso_coarse_nerf, net.torso_fine_nerf, net.aud_net, net.aud_att_net) for p in m.parameters()],
                           lr=args.lrate, betas=(0.9, 0.999))
    head = [p for m in (net.face_nerf_coarse, net.face_nerf_fine) for p in m.parameters()]
    net.train()

    def freeze(on):
        for p in head:
            p.requires_grad_(not on)
            p.grad = None

    prepared = []
    for i in range(16):                          # batches prepared in advance: the four sampled tensors copied out of the loader
        b = frames.batch(i % n, i)
        prepared.append(tuple(t.clone() for t in b[:4]) + b[4:])
    feeds = {"reference": (lambda s: T_._as_loader_item(ds[s % n]), True),
             "resident": (lambda s: frames.batch(s % n, s), True),
             "floor": (lambda s: prepared[s % len(prepared)], True),
             "full_plan": (lambda s: prepared[s % len(prepared)], False)}
    step = [0]

    def window(feed, count):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            T_.torso_train_step(net, opt, feed(step[0]), lat, step[0], n, lrate=args.lrate, lrate_decay=args.lrate_decay)
            step[0] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count * 1e3

    np.random.seed(0)
    per_round = {k: [] for k in feeds}
    for _ in range(ROUNDS):
        for name, (feed, frozen) in feeds.items():   # the same order in every round
            freeze(frozen)
            window(feed, WARMUP)
            per_round[name].append(window(feed, steps))
    freeze(True)
    _, scores = T_.resident_validation_frame(net, frames, lat, step[0], args.sample_seed, flip=False)

    med = lambda v: float(statistics.median(v))
    full = per_round["full_plan"]
    out = {"timing": {
        "device": torch.cuda.get_device_name(0), "size": [frames.H, frames.W], "frames": n, "N_rand": args.N_rand,
        "use_highlight": bool(args.use_highlight), "N_samples": args.N_samples, "N_importance": args.N_importance,
        "perturb": args.perturb, "steps_per_window": steps, "warmup_steps": WARMUP, "rounds": ROUNDS,
        "resident_load_s": load_s, "resident_bytes": int(frames.maps.numel() + frames.imgs.numel() + frames.background.numel()),
        **{f"step_ms_{k}": v for k, v in per_round.items()}, **{f"step_ms_{k}_median": med(v) for k, v in per_round.items()},
        "full_plan_round_spread_ms": max(full) - min(full),
        "frozen_plan_gain_ms": med(full) - med(per_round["floor"]),
        "composite_psnr_after_last_window": scores["psnr"][0], "composite_psnr_frame": scores["frame"], "steps_trained": step[0],
    }}
    return out


def main(argv=None):
    args = parse(argv)
    if args.timing_json is not None:
        out = timing(args)
        if args.timing_json not in ("", "-"):
            old = json.load(open(args.timing_json)) if os.path.exists(args.timing_json) else {}
            old.update(out)
            os.makedirs(os.path.dirname(os.path.abspath(args.timing_json)), exist_ok=True)
            json.dump(old, open(args.timing_json, "w"), indent=1)
        print(json.dumps(out))
        return out
    import torch
    from idealnerf_amd import train_torso as TT
    t0 = time.perf_counter()
    run = TT.train(args, loader=args.loader, sample_seed=args.sample_seed, steps=args.steps)
    torch.cuda.synchronize()
    out = {"loader": args.loader, "global_step": run["global_step"], "frames": run["data_size"], "seconds": time.perf_counter() - t0}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
