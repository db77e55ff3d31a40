#!/usr/bin/env python3
"""Drive a trained model from an audio, pose and expression track and print one JSON line: the command line over
``idealnerf_amd.drive``.

    python tools/drive_clip.py --flow head  --config <file> [--gpus N] [--precision P] [--out PATH] [--codec raw] [--global-step S]
    python tools/drive_clip.py --flow torso --config <file> [--gpus N] [--precision P] [--out PATH] [--codec raw]
    python tools/drive_clip.py --flow head --model baseline --config <adnerf_baseline.txt> [--gpus N] ...
    python tools/drive_clip.py --flow head --config <file> --learned_background    # over the checkpoint's learned background

--flow head is ``drive.drive_head`` (the reference's eval script): the flags of the head stage's config file -- ``datadir``,
``aud_file``, ``evalExpr_path``, ``testskip``, ``basedir`` / ``expname`` or ``ft_path``, ``save_path`` --, the identity's val poses,
the audio from the start of the file, expressions and focal length of ``evalExpr_path``, the newest checkpoint of the run
directory (tools/train_head.py's ``head.tar``).  --flow torso is ``drive.drive_torso`` (the reference's ``test_torso.py
--with_test``): the torso stage's flags -- ``test_pose_file``, ``test_size``, ``aud_start``, ``evalExpr_path`` --, the ``head.tar``
/ ``*_torso.tar`` pair tools/train_torso.py leaves in the run directory.  Every other flag of the two parsers may follow on
the command line and ranks above the file, as in the reference.  --flow head --model baseline is ``drive.drive_baseline`` (the
reference's ``test/test_nerf.py``): the val poses with the audio rows by position, ``ft_path`` (an AD-NeRF checkpoint) or the
newest ``*tar`` of the run directory (tools/train_head.py --model baseline), always at global step 0.

--gpus N starts N ranks as fresh child processes exactly as tools/render_clip.py does; this parent never opens the GPU
(IDN_DIST_BACKEND=gloo IDN_FORCE_DEVICE=0 rehearses N > 1 on one GPU).  --global-step (head): the step ``Network.forward`` sees,
0 as upstream (the unsmoothed audio path); pass the checkpoint's for the smoothed one.

The line: {"metric": "frames/s (...)", "value", "path", "n_frames", "nonfinite_frames", "seconds", "frames_per_s", "world", ...}.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)


def parse(argv):
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--flow", choices=("head", "torso"), required=True)
    pre.add_argument("--model", choices=("head", "agg", "baseline"), default="head")
    known = pre.parse_known_args(argv)[0]
    flow = known.flow
    if flow == "head" and known.model == "agg":
        from idealnerf_amd.agg_aud_exp_nerf import config_parser   # the head stage's flags plus use_highlight
    elif flow == "head":
        from idealnerf_amd.helper import config_parser
    else:
        from idealnerf_amd.train_torso import config_parser
    p = config_parser()
    p.add_argument("--flow", choices=("head", "torso"), required=True)
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--precision", default=None, help="set_render_precision's; default: the shipped arithmetic")
    p.add_argument("--out", default=None, help="default: the reference's file name under save_path")
    p.add_argument("--codec", choices=("MJPG", "raw"), default="MJPG")
    p.add_argument("--global-step", type=int, default=0)
    p.add_argument("--still-every", type=int, default=10)
    p.add_argument("--seed", type=int, default=None, help="per-frame draws seeded with seed + frame (perturb > 0)")
    p.add_argument("--model", choices=("head", "agg", "baseline"), default="head",
                   help="--flow head: the run's model (agg: train_agg.train's; baseline: train_baseline.train's or an AD-NeRF ft_path)")
    p.add_argument("--learned_background", action="store_true",
                   help="--flow head: render over the checkpoint's `background` (train_head.py --learn_background) instead of bc.jpg; "
                        "an error if the checkpoint holds none")
    from render_clip import cull_arguments
    cull_arguments(p)
    return p.parse_args(argv)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse(argv)
    if args.config is None:
        sys.exit("drive_clip.py: --config <file> is required (the stage's config file)")
    if args.learned_background and args.flow != "head":
        sys.exit("drive_clip.py: --learned_background belongs to --flow head (the torso stage learns no background)")
    if args.gpus > 1 and "RANK" not in os.environ:
        from render_clip import launch
        return launch(args.gpus, argv, script=__file__)
    import torch
    import torch.distributed as dist
    from render_clip import init_ranks
    world, rank, dev, backend = init_ranks()
    try:
        from idealnerf_amd import drive
        from render_clip import cull_option
        common = dict(out=args.out, device=dev, codec=args.codec, still_every=args.still_every, seed=args.seed,
                      precision=args.precision, cull=cull_option(args))
        learned = dict(learned_background=True) if args.learned_background else {}
        if args.flow == "head" and args.model == "baseline":
            res = drive.drive_baseline(args, **common, **learned)
        elif args.flow == "head":
            res = drive.drive_head(args, global_step=args.global_step, model=args.model, **common, **learned)
        else:
            res = drive.drive_torso(args, **common)
        if res is not None:
            from idealnerf_amd.models.face_nerf import SHIPPED_DEFAULT_PRECISION
            what = "head + torso composite" if args.flow == "torso" else "head only"
            print(json.dumps(dict(res, metric=f"frames/s (driven {what} clip, render + convert + copy + file, whole job)",
                                  value=res["frames_per_s"], unit="frames/s", higher_is_better=True, n_gpus=world, backend=backend,
                                  shared_device="IDN_FORCE_DEVICE" in os.environ and world > 1, flow=args.flow,
                                  dtype=args.precision or os.environ.get("IDN_DEFAULT_PRECISION", SHIPPED_DEFAULT_PRECISION),
                                  perturb=args.perturb, codec=args.codec, config=args.config,
                                  device=torch.cuda.get_device_name(dev))), flush=True)
    finally:
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
