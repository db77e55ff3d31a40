#!/usr/bin/env python
"""Train a head model with ``idealnerf_amd.train.train`` -- the reference's ``train()`` (NeRFs/HeadNeRF/train/audio_exp_nerf.py)
-- and measure what the two loaders cost.

    python tools/train_head.py --config <file> [upstream's flags] [--loader resident|reference] [--steps N] [--sample-seed S]
    python tools/train_head.py --model agg --config <feat_agg.txt> ...      # the feature-aggregation model: train_agg.train
    python tools/train_head.py --config <file> --refine_poses [--pose_lrate R]   # refine the training cameras with the model
    python tools/train_head.py --config <file> --generate 300 --pose_noise 1.0,0.01 --refine_poses   # on noised generated cameras
    python tools/train_head.py --timing-json profiles/train_loop.json [--generate 300] [--steps 60]
    python tools/train_head.py --model agg --timing-json profiles/agg_train_loop.json --generate 300
    python tools/train_head.py --model baseline --config <adnerf_baseline.txt> ...   # the AD-NeRF baseline: train_baseline.train
    python tools/train_head.py --model baseline --timing-json profiles/baseline_train_loop.json --generate 300
    python tools/train_head.py --refine_poses --timing-json profiles/pose_refine.json --generate 300   # the option's cost per step
    python tools/train_head.py --config <file> --refine_expr [--expr_lrate R] --learn_background [--bg_lrate R]
    python tools/train_head.py --refine_expr --learn_background --timing-json profiles/cond_refine.json --generate 40 --steps 40
    python tools/train_head.py --config <file> --ssim_weight 0.2 --patches 1x32 [--patch_region rect|frame]   # an SSIM term on patches
    python tools/train_head.py --ssim_weight 0.2 --patches 1x32 --timing-json profiles/ssim_loss.json --generate 40 --steps 40

``--model agg`` trains ``agg_aud_exp_nerf.Network`` (NeRFs/HeadNeRF/train/agg_aud_exp_nerf.py) with its own loaders, flags
(the head stage's plus ``use_highlight``) and ``{epoch:06d}_head.tar`` checkpoints.  Its ``--timing-json`` measures what the
model's per-frame host arithmetic costs: the agg network and a head network at the same N_rand (2048, feat_agg.txt's)
alternate, window by window, in one process on batches prepared in advance -- ``step_ms_agg``, ``step_ms_head`` and their
difference, the whole cost of computing the fused feature and its gradient terms outside the kernels.

``--model baseline`` trains ``head_baseline.Network`` (NeRFs/HeadNeRF/train/head_baseline.py: audio only, no expression, no
latent codes) with its own loaders, the head stage's flags and ``{epoch:06d}_head.tar`` checkpoints; ``--ft_path`` takes an
AD-NeRF checkpoint whole.  Its ``--timing-json`` records the baseline step beside the head model's in the same way
(``step_ms_baseline``, ``step_ms_head``): one process, the same prepared batches, the head arm with the directory's expressions
and a latent code on top.

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
    import argparse
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--model", choices=("head", "agg", "baseline"), default="head")
    model = pre.parse_known_args(argv)[0].model
    if model == "agg":
        from idealnerf_amd.agg_aud_exp_nerf import config_parser
    else:
        from idealnerf_amd.helper import config_parser
    p = config_parser()
    p.add_argument("--model", choices=("head", "agg", "baseline"), default="head",
                   help="agg: the feature-aggregation model (train_agg.train); baseline: the AD-NeRF baseline (train_baseline.train)")
    p.add_argument("--loader", type=str, default="resident", choices=("resident", "reference"))
    p.add_argument("--steps", type=int, default=None, help="stop after this many steps (timing: steps per window, default 60)")
    p.add_argument("--sample-seed", type=int, default=0)
    p.add_argument("--timing-json", type=str, default=None)
    p.add_argument("--generate", type=int, default=0, help="frames of the generated 450 x 450 directory (timing, or a training run on a directory that does not exist yet)")
    p.add_argument("--refine_poses", action="store_true",
                   help="refine the training cameras jointly with the model (pose_refine.PoseRefiner); head.tar gains pose_deltas")
    p.add_argument("--pose_lrate", type=float, default=None, help="Adam rate of the pose deltas (default 0.1 * lrate, untuned)")
    p.add_argument("--refine_expr", action="store_true",
                   help="refine the per-frame expressions jointly with the model (cond_refine.ExprRefiner); head.tar gains expr_deltas")
    p.add_argument("--expr_lrate", type=float, default=None, help="Adam rate of the expression deltas (default 0.1 * lrate, untuned)")
    p.add_argument("--learn_background", action="store_true",
                   help="train the background image with the model (cond_refine.Background; resident loader); head.tar gains background")
    p.add_argument("--bg_lrate", type=float, default=None, help="Adam rate of the background (default lrate, untuned)")
    p.add_argument("--ssim_weight", type=float, default=0.0,
                   help="weight of the patch SSIM term, 1 - mean SSIM on the fine image (ssim_loss.ssim_patch_loss; needs --patches; untuned)")
    p.add_argument("--patches", type=str, default=None, metavar="KxP",
                   help="K contiguous P x P patches ride in every batch, out of the rect region's share (resident loader)")
    p.add_argument("--patch_region", type=str, default="rect", choices=("rect", "frame"), help="where the patches' corners are drawn")
    p.add_argument("--pose_noise", type=str, default=None, metavar="DEG,LEN",
                   help="with --generate: seeded noise of this size (degrees, scene units) on the generated TRAINING cameras; "
                        "the clean poses are kept as transforms_exp_train_clean.json")
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


def agg_timing(args):
    """The agg network against a head network at the same N_rand, alternating in one process: warmed windows of bare
    train_step on prepared batches, each ended by one synchronise."""
    import torch
    from idealnerf_amd import dataset, synthetic, train as T_
    from idealnerf_amd.agg_aud_exp_nerf import build_head_network, init_weights
    if not torch.cuda.is_available():
        raise SystemExit("--timing-json measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    if args.generate and not os.path.isdir(args.datadir):
        os.makedirs(args.datadir)
        synthetic.write_clip_directory(args.datadir, SIZE, args.generate, seed=0, dim_expr=79)
    steps = args.steps or 60
    frames = dataset.ResidentAggFrames(args.datadir, args.aud_file, "train", args, device=dev, seed=args.sample_seed)
    n = len(frames)
    arms = {}
    for model in ("agg", "head"):
        torch.manual_seed(0)
        net = build_head_network(args, frames.H, frames.W, frames.focal, model).to(dev)
        lat = torch.ones(n, 32, dtype=torch.float32, device=dev)
        net.apply(init_weights)
        lat.requires_grad = True
        net.train()
        arms[model] = (net, T_.make_optimizer(net, lat, args.lrate), lat)
    prepared = []
    for i in range(16):                          # one set of batches for both arms
        b = frames.batch(i % n, i)
        prepared.append(tuple(t.clone() for t in b[:3]) + b[3:])
    step = {k: 0 for k in arms}

    def window(model, count):
        net, opt, lat = arms[model]
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            T_.train_step(net, opt, prepared[step[model] % len(prepared)], lat, step[model], n, lrate=args.lrate,
                          lrate_decay=args.lrate_decay)
            step[model] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count * 1e3

    per_round = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for model in arms:                       # the same order in every round: agg, head
            window(model, WARMUP)
            per_round[model].append(window(model, steps))
    med = lambda v: float(statistics.median(v))
    return {"agg_timing": {
        "device": torch.cuda.get_device_name(0), "size": [frames.H, frames.W], "frames": n, "N_rand": args.N_rand,
        "use_highlight": bool(args.use_highlight), "N_samples": args.N_samples, "N_importance": args.N_importance,
        "perturb": args.perturb, "dim_expr_head_arm": args.dim_expr, "steps_per_window": steps, "warmup_steps": WARMUP, "rounds": ROUNDS,
        "step_ms_agg": per_round["agg"], "step_ms_head": per_round["head"],
        "step_ms_agg_median": med(per_round["agg"]), "step_ms_head_median": med(per_round["head"]),
        "agg_minus_head_ms": med(per_round["agg"]) - med(per_round["head"]),
    }}


def baseline_timing(args):
    """The baseline network against a head network at the same N_rand, alternating in one process: warmed windows of the bare
    steps (train.baseline_train_step / train.train_step) on one set of prepared batches, each ended by one synchronise.  The head
    arm's 8-tuples are the baseline's 7-tuples with the frame's expression put in."""
    import torch
    from idealnerf_amd import dataset, synthetic, train as T_
    from idealnerf_amd.agg_aud_exp_nerf import build_head_network, init_weights
    if not torch.cuda.is_available():
        raise SystemExit("--timing-json measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    if args.generate and not os.path.isdir(args.datadir):
        os.makedirs(args.datadir)
        synthetic.write_clip_directory(args.datadir, SIZE, args.generate, seed=0)
    steps = args.steps or 60
    frames = dataset.ResidentBaselineFrames(args.datadir, args.aud_file, "train", args, device=dev, seed=args.sample_seed)
    n = len(frames)
    exprs = torch.tensor([f["exp"] for f in frames.meta["frames"]], dtype=torch.float32, device=dev)
    arms = {}
    for model in ("baseline", "head"):
        torch.manual_seed(0)
        net = build_head_network(args, frames.H, frames.W, frames.focal, model).to(dev)
        net.apply(init_weights)
        net.train()
        if model == "head":
            lat = torch.ones(n, 32, dtype=torch.float32, device=dev)
            lat.requires_grad = True
            arms[model] = (net, T_.make_optimizer(net, lat, args.lrate), lat)
        else:
            arms[model] = (net, torch.optim.Adam(list(net.parameters()), lr=args.lrate, betas=(0.9, 0.999)), None)
    prepared = []
    for i in range(16):                          # one set of batches for both arms
        b = frames.batch(i % n, i)
        prepared.append(tuple(t.clone() for t in b[:3]) + b[3:])
    step = {k: 0 for k in arms}

    def window(model, count):
        net, opt, lat = arms[model]
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            data = prepared[step[model] % len(prepared)]
            if model == "head":
                T_.train_step(net, opt, (*data[:6], exprs[data[6]], data[6]), lat, step[model], n, lrate=args.lrate,
                              lrate_decay=args.lrate_decay)
            else:
                T_.baseline_train_step(net, opt, data, step[model], n, lrate=args.lrate, lrate_decay=args.lrate_decay)
            step[model] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count * 1e3

    per_round = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for model in arms:                       # the same order in every round: baseline, head
            window(model, WARMUP)
            per_round[model].append(window(model, steps))
    med = lambda v: float(statistics.median(v))
    return {"baseline_timing": {
        "device": torch.cuda.get_device_name(0), "size": [frames.H, frames.W], "frames": n, "N_rand": args.N_rand,
        "N_samples": args.N_samples, "N_importance": args.N_importance, "perturb": args.perturb, "dim_aud": args.dim_aud,
        "dim_expr_head_arm": args.dim_expr, "steps_per_window": steps, "warmup_steps": WARMUP, "rounds": ROUNDS,
        "step_ms_baseline": per_round["baseline"], "step_ms_head": per_round["head"],
        "step_ms_baseline_median": med(per_round["baseline"]), "step_ms_head_median": med(per_round["head"]),
        "baseline_minus_head_ms": med(per_round["baseline"]) - med(per_round["head"]),
    }}


def pose_timing(args):
    """What --refine_poses costs per step: the head model's bare train_step on prepared batches, without and with the frame's
    pose correction (pose_refine.PoseRefiner, its deltas a parameter group of the same Adam), the two arms alternating window
    by window in one process from equal initial weights, each window warmed and ended by one synchronise."""
    import torch
    from idealnerf_amd import dataset, synthetic, train as T_
    from idealnerf_amd.agg_aud_exp_nerf import build_head_network, init_weights
    from idealnerf_amd.pose_refine import PoseRefiner
    if not torch.cuda.is_available():
        raise SystemExit("--timing-json measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    if args.generate and not os.path.isdir(args.datadir):
        os.makedirs(args.datadir)
        synthetic.write_clip_directory(args.datadir, SIZE, args.generate, seed=0)
    steps = args.steps or 60
    frames = dataset.ResidentFrames(args.datadir, args.aud_file, "train", args, device=dev, seed=args.sample_seed)
    n = len(frames)
    pose_lrate = 0.1 * args.lrate if args.pose_lrate is None else args.pose_lrate
    arms = {}
    for arm in ("plain", "refine"):
        torch.manual_seed(0)
        net = build_head_network(args, frames.H, frames.W, frames.focal, "head").to(dev)
        lat = torch.ones(n, 32, dtype=torch.float32, device=dev)
        net.apply(init_weights)
        lat.requires_grad = True
        net.train()
        opt = T_.make_optimizer(net, lat, args.lrate)
        refiner = None
        if arm == "refine":
            refiner = PoseRefiner(n).to(dev)
            opt.add_param_group({"params": [refiner.deltas], "lr": pose_lrate, "lr_scale": pose_lrate / args.lrate})
        arms[arm] = (net, opt, lat, refiner)
    prepared = []
    for i in range(16):                          # one set of batches for both arms
        b = frames.batch(i % n, i)
        prepared.append(tuple(t.clone() for t in b[:3]) + b[3:])
    step = {k: 0 for k in arms}

    def window(arm, count):
        net, opt, lat, refiner = arms[arm]
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            data = prepared[step[arm] % len(prepared)]
            if refiner is not None:
                data = (refiner(int(data[-1]), data[0]), *data[1:])
            T_.train_step(net, opt, data, lat, step[arm], n, lrate=args.lrate, lrate_decay=args.lrate_decay)
            step[arm] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count * 1e3

    per_round = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for arm in arms:                         # the same order in every round: plain, refine
            window(arm, WARMUP)
            per_round[arm].append(window(arm, steps))
    med = lambda v: float(statistics.median(v))
    return {"step_cost": {
        "device": torch.cuda.get_device_name(0), "size": [frames.H, frames.W], "frames": n, "N_rand": args.N_rand,
        "mouth_rays": args.mouth_rays, "N_samples": args.N_samples, "N_importance": args.N_importance, "perturb": args.perturb,
        "steps_per_window": steps, "warmup_steps": WARMUP, "rounds": ROUNDS, "pose_lrate": pose_lrate,
        "step_ms_plain": per_round["plain"], "step_ms_refine": per_round["refine"],
        "step_ms_plain_median": med(per_round["plain"]), "step_ms_refine_median": med(per_round["refine"]),
        "refine_minus_plain_ms": med(per_round["refine"]) - med(per_round["plain"]),
        "refine_over_plain": med(per_round["refine"]) / med(per_round["plain"]),
    }}


def cond_timing(args):
    """What --refine_expr and --learn_background cost per step: the head model's bare train_step on prepared batches in four
    arms -- off, refine_expr, learn_background, both -- each with the option's parameter group in the same Adam, alternating
    window by window in one process from equal initial weights, each window warmed and ended by one synchronise.  The
    background arms render over ``Background.rows`` of the prepared batch's pixel indices."""
    import torch
    from idealnerf_amd import dataset, synthetic, train as T_
    from idealnerf_amd.agg_aud_exp_nerf import build_head_network, init_weights
    from idealnerf_amd.cond_refine import Background, ExprRefiner
    if not torch.cuda.is_available():
        raise SystemExit("--timing-json measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    if args.generate and not os.path.isdir(args.datadir):
        os.makedirs(args.datadir)
        synthetic.write_clip_directory(args.datadir, SIZE, args.generate, seed=0)
    steps = args.steps or 60
    frames = dataset.ResidentFrames(args.datadir, args.aud_file, "train", args, device=dev, seed=args.sample_seed)
    n = len(frames)
    expr_lrate = 0.1 * args.lrate if args.expr_lrate is None else args.expr_lrate
    bg_lrate = args.lrate if args.bg_lrate is None else args.bg_lrate
    arms = {}
    for arm, (with_expr, with_bg) in (("off", (False, False)), ("refine_expr", (True, False)), ("learn_background", (False, True)),
                                      ("both", (True, True))):
        torch.manual_seed(0)
        net = build_head_network(args, frames.H, frames.W, frames.focal, "head").to(dev)
        lat = torch.ones(n, 32, dtype=torch.float32, device=dev)
        net.apply(init_weights)
        lat.requires_grad = True
        net.train()
        opt = T_.make_optimizer(net, lat, args.lrate)
        refiner = background = None
        if with_expr:
            refiner = ExprRefiner(n, args.dim_expr).to(dev)
            opt.add_param_group({"params": [refiner.deltas], "lr": expr_lrate, "lr_scale": expr_lrate / args.lrate})
        if with_bg:
            background = Background(frames.background).to(dev)
            opt.add_param_group({"params": [background.image], "lr": bg_lrate, "lr_scale": bg_lrate / args.lrate})
        arms[arm] = (net, opt, lat, refiner, background)
    prepared = []
    for i in range(16):                          # one set of batches for all arms, each with its pixel indices
        b = frames.batch(i % n, i)
        prepared.append((tuple(t.clone() for t in b[:3]) + b[3:], frames.selection().clone()))
    step = {k: 0 for k in arms}

    def window(arm, count):
        net, opt, lat, refiner, background = arms[arm]
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            data, sel = prepared[step[arm] % len(prepared)]
            if refiner is not None:
                data = (*data[:-2], refiner(int(data[-1]), data[-2]), data[-1])
            if background is not None:
                data = (*data[:2], background.rows(sel), *data[3:])
            T_.train_step(net, opt, data, lat, step[arm], n, lrate=args.lrate, lrate_decay=args.lrate_decay)
            step[arm] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count * 1e3

    per_round = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for arm in arms:                         # the same order in every round: off, refine_expr, learn_background, both
            window(arm, WARMUP)
            per_round[arm].append(window(arm, steps))
    med = lambda v: float(statistics.median(v))
    out = {"device": torch.cuda.get_device_name(0), "size": [frames.H, frames.W], "frames": n, "N_rand": args.N_rand,
           "mouth_rays": args.mouth_rays, "N_samples": args.N_samples, "N_importance": args.N_importance, "perturb": args.perturb,
           "steps_per_window": steps, "warmup_steps": WARMUP, "rounds": ROUNDS, "expr_lrate": expr_lrate, "bg_lrate": bg_lrate}
    for arm in arms:
        out["step_ms_" + arm] = per_round[arm]
        out["step_ms_" + arm + "_median"] = med(per_round[arm])
        if arm != "off":
            out[arm + "_minus_off_ms"] = med(per_round[arm]) - med(per_round["off"])
    return {"step_cost": out}


def _patches(text):
    """"KxP" -> (K, P); None stays None."""
    if text is None:
        return None
    try:
        k, p = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise SystemExit(f"--patches takes KxP, e.g. 1x32 (got {text!r})") from None
    return k, p


def ssim_timing(args):
    """What --ssim_weight W --patches KxP costs per step: the head model's train_step fed by the resident loader in two arms --
    off, and the option on -- alternating window by window in one process from equal initial weights, each window warmed and
    ended by one synchronise; then the three new launches alone (patch_pixels, the loss's forward, its backward) by HIP events
    over repeated calls on one batch's patch rows."""
    import torch
    from idealnerf_amd import dataset, ops, synthetic, train as T_
    from idealnerf_amd.agg_aud_exp_nerf import build_head_network, init_weights
    if not torch.cuda.is_available():
        raise SystemExit("--timing-json measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    if args.generate and not os.path.isdir(args.datadir):
        os.makedirs(args.datadir)
        synthetic.write_clip_directory(args.datadir, SIZE, args.generate, seed=0)
    steps = args.steps or 60
    k, p = _patches(args.patches)
    arms = {}
    for arm, kw in (("off", {}), ("on", dict(patches=(k, p), patch_region=args.patch_region))):
        frames = dataset.ResidentFrames(args.datadir, args.aud_file, "train", args, device=dev, seed=args.sample_seed, **kw)
        torch.manual_seed(0)
        net = build_head_network(args, frames.H, frames.W, frames.focal, "head").to(dev)
        lat = torch.ones(len(frames), 32, dtype=torch.float32, device=dev)
        net.apply(init_weights)
        lat.requires_grad = True
        net.train()
        ssim = dict(ssim=(args.ssim_weight, frames.patch_rows(), k, p)) if kw else {}
        arms[arm] = (frames, net, T_.make_optimizer(net, lat, args.lrate), lat, ssim)
    n = len(arms["off"][0])
    step = {a: 0 for a in arms}

    def window(arm, count):
        frames, net, opt, lat, ssim = arms[arm]
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            s = step[arm]
            T_.train_step(net, opt, frames.batch(s % n, s), lat, s, n, lrate=args.lrate, lrate_decay=args.lrate_decay, **ssim)
            step[arm] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count * 1e3

    per_round = {a: [] for a in arms}
    for _ in range(ROUNDS):
        for arm in arms:                         # the same order in every round: off, on
            window(arm, WARMUP)
            per_round[arm].append(window(arm, steps))

    frames = arms["on"][0]
    batch = frames.batch(0, 0)
    rows = frames.patch_rows()
    truth = batch[1][rows].contiguous()
    pred = (truth + 0.05 * torch.randn_like(truth)).contiguous()
    origins, tail = frames.patch_origins_of(0, 0), torch.empty(k * p * p, dtype=torch.int64, device=dev)
    out64, d_pred = torch.empty(k + 1, dtype=torch.float64, device=dev), torch.empty_like(pred)

    def event_us(fn, reps=200):
        for _ in range(20):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    launches = {"patch_pixels_us": event_us(lambda: ops.patch_pixels(origins, p, frames.W, out=tail)),
                "ssim_patch_fwd_us": event_us(lambda: ops.ssim_patch_fwd(pred, truth, k, p, out=out64)),   # both of its launches
                "ssim_patch_bwd_us": event_us(lambda: ops.ssim_patch_bwd(pred, truth, k, p, g=args.ssim_weight, out=d_pred))}
    med = lambda v: float(statistics.median(v))
    out = {"device": torch.cuda.get_device_name(0), "size": [frames.H, frames.W], "frames": n, "N_rand": args.N_rand,
           "mouth_rays": args.mouth_rays, "N_samples": args.N_samples, "N_importance": args.N_importance, "perturb": args.perturb,
           "steps_per_window": steps, "warmup_steps": WARMUP, "rounds": ROUNDS, "ssim_weight": args.ssim_weight, "patches": [k, p],
           "patch_region": args.patch_region, "launches_back_to_back": launches}
    for arm in arms:
        out["step_ms_" + arm] = per_round[arm]
        out["step_ms_" + arm + "_median"] = med(per_round[arm])
    out["on_minus_off_ms"] = med(per_round["on"]) - med(per_round["off"])
    return {"step_cost": out}


def main(argv=None):
    args = parse(argv)
    if args.timing_json is not None:
        if args.generate and args.model == "agg":   # feat_agg.txt's batch on the generated directory; the head arm takes the 79-wide expression
            args.N_rand, args.dim_aud, args.dim_expr, args.use_highlight = 2048, 64, 79, True
        elif args.generate and args.model == "baseline":   # adnerf_baseline.txt's batch; the head arm takes the directory's 76-wide expression
            args.N_rand, args.dim_aud, args.dim_expr = 2048, 64, 76
        elif args.generate:                      # the reference's size and split on the generated directory
            args.N_rand, args.mouth_rays, args.dim_aud, args.dim_expr = 3072, 256, 64, 76
        if args.refine_poses and args.model != "head":
            raise SystemExit("--timing-json --refine_poses measures the head model")
        cond = args.refine_expr or args.learn_background   # either flag: the four arms off / refine_expr / learn_background / both
        if cond and (args.model != "head" or args.refine_poses):
            raise SystemExit("--timing-json --refine_expr / --learn_background measures the head model, without --refine_poses")
        if args.patches is not None:
            if cond or args.refine_poses or args.model != "head" or not args.ssim_weight > 0:
                raise SystemExit("--timing-json --patches measures the head model with --ssim_weight > 0 and no other option")
            out = ssim_timing(args)
        elif cond:
            out = cond_timing(args)
        else:
            out = pose_timing(args) if args.refine_poses else {"agg": agg_timing, "baseline": baseline_timing}.get(args.model, timing)(args)
        if args.timing_json not in ("", "-"):
            old = json.load(open(args.timing_json)) if os.path.exists(args.timing_json) else {}
            old.update(out)
            os.makedirs(os.path.dirname(os.path.abspath(args.timing_json)), exist_ok=True)
            json.dump(old, open(args.timing_json, "w"), indent=1)
        print(json.dumps(out))
        return out
    import torch
    from idealnerf_amd import train as T_
    clean = None
    if args.generate and not os.path.isdir(args.datadir):
        from idealnerf_amd import synthetic
        os.makedirs(args.datadir)
        synthetic.write_clip_directory(args.datadir, SIZE, args.generate, seed=0, dim_expr=79 if args.model == "agg" else 76)
        if args.pose_noise:
            deg, length = (float(v) for v in args.pose_noise.split(","))
            clean = synthetic.perturb_train_poses(args.datadir, deg, length, seed=0)
    elif args.pose_noise:
        raise SystemExit("--pose_noise perturbs a directory --generate writes; this one exists or --generate is missing")
    t0 = time.perf_counter()
    pose = dict(refine_poses=args.refine_poses, pose_lrate=args.pose_lrate, refine_expr=args.refine_expr, expr_lrate=args.expr_lrate,
                learn_background=args.learn_background, bg_lrate=args.bg_lrate, ssim_weight=args.ssim_weight,
                patches=_patches(args.patches), patch_region=args.patch_region)
    if args.model == "agg":
        from idealnerf_amd import train_agg
        run = train_agg.train(args, loader=args.loader, sample_seed=args.sample_seed, steps=args.steps, **pose)
    elif args.model == "baseline":
        from idealnerf_amd import train_baseline
        run = train_baseline.train(args, loader=args.loader, sample_seed=args.sample_seed, steps=args.steps, **pose)
    else:
        run = T_.train(args, loader=args.loader, sample_seed=args.sample_seed, steps=args.steps, **pose)
    torch.cuda.synchronize()
    out = {"model": args.model, "loader": args.loader, "global_step": run["global_step"], "frames": run["data_size"], "seconds": time.perf_counter() - t0}
    if clean is not None:   # camera error against the clean poses, before and after (degrees, scene units; mean over the frames)
        from idealnerf_amd.pose_refine import pose_errors, refined_c2w
        noisy, truth = clean
        before = pose_errors(noisy, truth)
        out["pose_error_before"] = [float(before[0].mean()), float(before[1].mean())]
        if "pose_refiner" in run:
            deltas = run["pose_refiner"].deltas.detach().double().cpu()
            after = pose_errors(torch.stack([refined_c2w(dl, m) for dl, m in zip(deltas, noisy)]), truth)
            out["pose_error_after"] = [float(after[0].mean()), float(after[1].mean())]
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
