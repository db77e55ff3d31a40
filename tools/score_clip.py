#!/usr/bin/env python3
"""Score a validation clip against its ground truth, once per arithmetic: the command line over
``idealnerf_amd.clip.score_head_clip`` (PSNR as the reference's helper.mse2psnr, SSIM; whole frame and per sampling region).

    python tools/score_clip.py --config <file> [--ckpt head.tar] [--frames N] [--precisions f32,bf16x6,bf16] [--avi out.avi]
                               [--gpus N] --out scores.json
    python tools/score_clip.py --out scores.json                                   # a generated clip, xavier weights
    python tools/score_clip.py --timing-json profiles/score_clip.json
    python tools/score_clip.py --config <file> --ckpt head.tar --learned_background --out scores.json   # over the learned background

The val split of the config's dataset directory goes to the device once (``dataset.ResidentFrames(mode="val")``) and is scored
once per entry of --precisions through ``set_render_precision``; the file holds, per arithmetic, the per-frame table, the
per-group means (with the number of frames a mean leaves out) and the pooled figures, and each arithmetic's dB / SSIM difference
from the first.  --avi also writes each arithmetic's clip (``out.<precision>.avi``).  --gpus N starts N ranks as fresh child
processes exactly as tools/render_clip.py does; this parent never opens the GPU (IDN_DIST_BACKEND=gloo IDN_FORCE_DEVICE=0
rehearses N > 1 on one GPU).  Without --config the clip is a ``synthetic.write_clip_directory`` one (--size, --frames), as in
tools/train_head.py's timing runs: the numbers then say what an arithmetic does to a render, not how good a model is.

--timing-json (one GPU, one process): HIP-event time of ``ops.frame_scores`` alone at 450 x 450 and 512 x 512, frames per second
of ``score_head_clip(path=None)`` next to ``render_head_clip`` to a raw file on the same generated clip in f32 and plain bf16, and
the HIP-event time of one plain-bf16 frame render.  Prints one JSON line.
"""
import json
import math
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)


def parse(argv):
    import argparse
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--model", choices=("head", "agg", "baseline"), default="head")
    if pre.parse_known_args(argv)[0].model == "agg":
        from idealnerf_amd.agg_aud_exp_nerf import config_parser   # the head stage's flags plus use_highlight
    else:
        from idealnerf_amd.helper import config_parser
    p = config_parser()
    p.add_argument("--ckpt", default=None, help="a head.tar of train.train; default: xavier weights")
    p.add_argument("--frames", type=int, default=None, help="score the first N frames of the val split (generated clip: its length, default 8)")
    p.add_argument("--precisions", default="f32,bf16x6,bf16")
    p.add_argument("--avi", default=None)
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--out", default=None)
    p.add_argument("--size", type=int, default=450, help="frame size of the generated clip")
    p.add_argument("--global-step", type=int, default=None, help="default: the checkpoint's, else nosmo_iters")
    p.add_argument("--generated", action="store_true", help="(set by the parent) --datadir is a generated clip")
    p.add_argument("--timing-json", default=None)
    p.add_argument("--model", choices=("head", "agg", "baseline"), default="head",
                   help="agg: the feature-aggregation network and its loader; baseline: the AD-NeRF baseline and its loader "
                        "(--ckpt: a {epoch:06d}_head.tar of train_baseline.train or an AD-NeRF four-dict file)")
    p.add_argument("--learned_background", action="store_true",
                   help="render over the checkpoint's `background` (train_head.py --learn_background) instead of bc.jpg; an error "
                        "without --ckpt or if the checkpoint holds none")
    from render_clip import cull_arguments
    cull_arguments(p)
    return p.parse_args(argv)


def plain(x):
    """numpy / torch values -> what json writes: nan as null, infinities as strings."""
    import numpy as np
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if hasattr(x, "tolist"):
        x = x.tolist()
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, (float, np.floating)):
        return None if math.isnan(x) else (str(x) if math.isinf(x) else float(x))
    return x


def generated_flags(args):
    """The generated clip's loader flags and the reference's widths on it (tools/train_head.py --generate); perturb 0, so that
    two arithmetics differ by their arithmetic alone."""
    args.perturb = 0.0
    args.gt_dirs, args.aud_file, args.testskip = "head_imgs", "aud.npy", 1
    args.N_rand, args.mouth_rays, args.torso_rays, args.sample_rate = 64, 8, 4, 0.95
    args.dim_aud, args.dim_expr, args.near, args.far = 64, 76, 0.3, 0.9
    return args


def build(args, dev):
    """-> (resident val frames, network, global_step, latent code)."""
    import torch
    from idealnerf_amd import checkpoint, dataset, synthetic
    from idealnerf_amd.agg_aud_exp_nerf import build_head_network
    resident = {"agg": dataset.ResidentAggFrames, "baseline": dataset.ResidentBaselineFrames}.get(args.model, dataset.ResidentFrames)
    frames = resident(args.datadir, args.aud_file, "val", args, skip=args.testskip, device=dev)
    if args.learned_background:   # what frame() hands the full-frame render as bg_img
        if not args.ckpt:
            raise SystemExit("--learned_background needs --ckpt")
        frames.background_unit = checkpoint.load_background(args.ckpt, map_location="cpu").to(dev)
    torch.manual_seed(0)   # the audio nets: every rank builds the same network
    net = build_head_network(args, frames.H, frames.W, frames.focal, args.model)
    step, latent = net.args.nosmo_iters, torch.ones(32)
    if args.ckpt and args.model == "baseline":
        ckpt = torch.load(args.ckpt, map_location="cpu", weights_only=False)
        if "model_state_dict" in ckpt:
            step = checkpoint.load_baseline_checkpoint(args.ckpt, net, map_location="cpu")
        else:
            step = checkpoint.load_adnerf(ckpt, net) or step
        latent = None
    elif args.ckpt:
        step, codes = checkpoint.load_checkpoint(args.ckpt, net, map_location="cpu")
        latent = codes[0]
    else:
        synthetic.xavier_state_dict(net.face_nerf_coarse, 2, 300.0, 0.3)
        synthetic.xavier_state_dict(net.face_nerf_fine, 3, 300.0, 0.3)
    return frames, net.to(dev).eval(), (step if args.global_step is None else args.global_step), latent


def score(args, dev, world):
    import numpy as np
    import idealnerf_amd
    from idealnerf_amd import clip, ops
    frames, net, step, latent = build(args, dev)
    ids = range(frames.data_size if args.frames is None else min(args.frames, frames.data_size))
    runs, first = {}, None
    for prec in [p.strip() for p in args.precisions.split(",") if p.strip()]:
        idealnerf_amd.set_render_precision(net, prec)
        path = None if args.avi is None else "{0}.{2}{1}".format(*os.path.splitext(args.avi), prec)
        from render_clip import cull_option
        res = clip.score_head_clip(net, frames, step, latent_code=latent, frame_ids=ids, path=path, seed=0 if args.perturb else None,
                                   codec="MJPG", model=args.model, cull=cull_option(args))
        if res is None:
            continue
        first = res if first is None else first
        delta = {k: res["mean"][k] - first["mean"][k] for k in ("psnr", "ssim")}
        pooled_delta = {k: res["pooled"][k] - first["pooled"][k] for k in ("psnr", "ssim")}
        runs[prec] = dict(mean=res["mean"], pooled=res["pooled"], per_frame=res["per_frame"], table=res["table"].numpy(),
                          mean_minus_first=delta, pooled_minus_first=pooled_delta, nonfinite_frames=res["nonfinite_frames"],
                          seconds=res["seconds"], frames_per_s=res["frames_per_s"], avi=path)
    if first is None:
        return None
    return dict(metric="PSNR (dB) / SSIM of the val clip per arithmetic, float render against uint8 / 255", groups=list(ops.SCORE_GROUPS),
                columns=list(ops.SCORE_COLUMNS), frames=first["frames"], size=[frames.H, frames.W], world=world, first=next(iter(runs)),
                generated_clip=bool(args.generated), ckpt=args.ckpt, global_step=int(step), perturb=args.perturb, precisions=runs,
                psnr_whole_frame={p: float(np.asarray(r["mean"]["psnr"])[0]) for p, r in runs.items()})


def events_us(fn, reps, rounds=5, warm=20):
    """Median over `rounds` of the HIP-event time per call of `reps` back-to-back calls, in microseconds."""
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return float(statistics.median(out)), out


def timing(args, dev):
    import torch
    import idealnerf_amd
    from idealnerf_amd import clip, dataset, ops, synthetic
    out = {"device": torch.cuda.get_device_name(dev), "method": "HIP events; warm-up calls first; median of 5 rounds (operator, render) "
           "or of 3 alternating clip runs (frames/s: wall time of the whole call, first render to the table / the closed file)"}
    op = {}
    for size in (450, 512):
        g = torch.Generator(device=dev).manual_seed(size)
        truth = torch.randint(0, 256, (size, size, 3), device=dev, generator=g, dtype=torch.uint8)
        pred = truth.float() / 255 + 0.05 * torch.randn((size, size, 3), device=dev, generator=g)
        regions = torch.randint(0, 16, (size, size), device=dev, generator=g, dtype=torch.uint8)
        res = torch.empty((5, 4), dtype=torch.float64, device=dev)
        ws = torch.empty(ops.frame_scores_workspace_doubles(size, size), dtype=torch.float64, device=dev)
        med, all_ = events_us(lambda: ops.frame_scores(pred, truth, regions, out=res, workspace=ws), 100)
        op[f"{size}x{size}"] = {"frame_scores_us": med, "rounds_us": all_, "calls_per_round": 100}
    out["operator"] = op

    d = tempfile.mkdtemp(prefix="score_clip_")
    try:
        n = args.frames or 8
        args.datadir = os.path.join(d, "clip")
        os.makedirs(args.datadir)
        synthetic.write_clip_directory(args.datadir, args.size, n, seed=0)
        generated_flags(args)
        frames, net, step, latent = build(args, dev)
        ds = dataset.GetData(args.datadir, args.aud_file, "val", args, skip=1, device=dev)
        loops = {}
        for prec in ("f32", "bf16"):
            idealnerf_amd.set_render_precision(net, prec)
            clip.score_head_clip(net, frames, step, latent_code=latent, frame_ids=range(1))      # warm-up of both loops
            clip.render_head_clip(net, ds, os.path.join(d, "w.avi"), step, latent_code=latent, frames=range(1), codec="raw")
            s_fps, r_fps = [], []
            for _ in range(3):
                s_fps.append(clip.score_head_clip(net, frames, step, latent_code=latent)["frames_per_s"])
                r_fps.append(clip.render_head_clip(net, ds, os.path.join(d, "r.avi"), step, latent_code=latent, codec="raw")["frames_per_s"])
            loops[prec] = {"score_head_clip_path_none_frames_per_s": float(statistics.median(s_fps)), "score_runs": s_fps,
                           "render_head_clip_raw_file_frames_per_s": float(statistics.median(r_fps)), "render_runs": r_fps,
                           "ms_per_frame_score_minus_render": 1e3 / statistics.median(s_fps) - 1e3 / statistics.median(r_fps)}
        data = frames.frame(0)

        def render():
            with torch.no_grad():
                net([(*data[:7], latent, data[7]), step, frames.data_size])
        med, all_ = events_us(render, 3, warm=3)      # net is in plain bf16 here
        out["clip"] = {"size": [frames.H, frames.W], "frames": n, "N_samples": args.N_samples, "N_importance": args.N_importance,
                       "perturb": args.perturb, "loops": loops, "bf16_frame_render_us": med, "bf16_frame_render_rounds_us": all_}
        at = f"{frames.H}x{frames.W}"
        if at in op:
            out["clip"]["frame_scores_share_of_bf16_render"] = op[at]["frame_scores_us"] / med
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse(argv)
    made = None
    try:
        if "RANK" not in os.environ and args.timing_json is None and args.config is None and not args.generated:
            made = tempfile.mkdtemp(prefix="score_clip_")     # by the parent, on the host: every rank reads the same directory
            from idealnerf_amd import synthetic
            os.makedirs(os.path.join(made, "clip"))
            synthetic.write_clip_directory(os.path.join(made, "clip"), args.size, args.frames or 8, seed=0,
                                           dim_expr=79 if args.model == "agg" else 76)   # the agg pair's expression width is 79
            argv += ["--datadir", os.path.join(made, "clip"), "--generated"]
            args = parse(argv)
        if args.gpus > 1 and "RANK" not in os.environ:
            from render_clip import launch
            return launch(args.gpus, argv, script=__file__)
        if args.generated:
            generated_flags(args)
        import torch
        import torch.distributed as dist
        from render_clip import init_ranks
        world, rank, dev, backend = init_ranks()
        try:
            if args.timing_json is not None:
                out = {"metric": "frame scoring: operator, scoring loop and render loop", "timing": timing(args, dev)}
                target = args.timing_json
            else:
                out, target = score(args, dev, world), args.out
            if out is not None:
                out = plain(out)
                if target and target != "-":
                    os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
                    with open(target, "w") as f:
                        json.dump(out, f, indent=1)
                brief = {k: v for k, v in out.items() if k != "precisions"}
                print(json.dumps(brief), flush=True)
        finally:
            if dist.is_available() and dist.is_initialized():
                dist.destroy_process_group()
    finally:
        if made is not None:
            shutil.rmtree(made, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
