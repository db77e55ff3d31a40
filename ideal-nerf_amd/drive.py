"""A trained model on a track that is not its training clip: the reference's two test-time scripts as calls.

``drive_head``   NeRFs/HeadNeRF/test/eval_aud_exp_nerf.py::eval (:435-496) -- the identity's val poses, the audio file from its
                 start, expressions and focal length of ``--evalExpr_path`` (``dataset.DrivingFrames``), the newest checkpoint
                 of the run directory, ``clip.render_head_clip``.
``drive_torso``  NeRFs/TorsoNeRF/test_torso.py --with_test (:405-535) on ``train_torso.Network`` -- the track of
                 ``dataset.load_test_data``, one expression per frame (``dataset.load_test_exprs``), the ``head.tar`` /
                 ``*_torso.tar`` pair of the run directory, ``clip.render_torso_clip``.

Both are frame-parallel inside a process group like the clip calls they end in: every rank builds the same network and
reads the same files, rank 0 writes the clip and returns the dict, the other ranks return None.
"""
import os

import torch

from . import checkpoint, clip, dataset
from .config import to_render_config
from .helper import input_channels
from .models.face_nerf import set_render_precision


def _unset(value):
    return value is None or value == 'None'


def _same_on_every_rank(build):
    """`build()` under a generator seeded with 0 (layers without a checkpoint behind them are then the same on every rank);
    the caller's generator is left as it was."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        return build()


def _learned_background(frames, path, device):
    """The checkpoint's ``background`` (``train(learn_background=True)``) in place of the loader's ``bc.jpg``: the frames are
    rendered over it.  ValueError without a checkpoint, KeyError (``checkpoint.load_background``) for one that holds none."""
    if path is None:
        raise ValueError("learned_background: no checkpoint was loaded (no_reload, or none in the run directory)")
    frames.background_img = checkpoint.load_background(path, map_location=device).to(device)


def drive_head(args, *, out=None, global_step=0, device="cuda", codec="MJPG", still_every=10, seed=None, group=None,
               precision=None, model="head", learned_background=False, cull=None):
    """The eval script's ``eval()`` on the flags ``args`` (``helper.config_parser().parse_args()``): ``DrivingFrames(args.datadir,
    args.aud_file, "val", args, skip=args.testskip)``, a ``Network`` with ``to_render_config(args)`` and the loader's focal
    length, the checkpoint ``args.ft_path`` -- else the newest ``*.tar`` of ``basedir/expname`` --, read whole and without
    optimiser unless ``args.no_reload``, latent code row 0 of the checkpoint's (zeros [32] without one), every frame through
    ``clip.render_head_clip``.

    ``global_step`` is 0 as upstream, which selects the unsmoothed audio path of ``Network.forward``; pass the checkpoint's step
    for the smoothed one.  ``out`` defaults to upstream's ``V_{datadir[8:]}_{aud_file[-9:-4]}_N_ExpPose0.avi`` under
    ``args.save_path``; every ``still_every``-th frame is also written there as ``{datadir[8:]}_{aud_file[-9:-4]}_ExpPose_{i}.jpg``.
    ``precision``: ``set_render_precision``'s.  ``model``: "head", or "agg" for a run of ``train_agg.train``
    (``agg_aud_exp_nerf.Network``; its newest ``{epoch:06d}_head.tar``).  ValueError where the network's expression width --
    ``args.dim_expr``, the agg pair's 79 -- is not the expression track's.  ``learned_background``: render over the
    checkpoint's ``background`` instead of ``bc.jpg`` (it raises if the checkpoint holds none); off: nothing changes.
    ``cull``: ``render_head_clip``'s (None, or the occupancy grid's options: empty rays are not rendered; with ``samples=True`` neither are
    the live rays' samples in empty cells).
    -> ``render_head_clip``'s dict plus ``path`` on rank 0, None on the other ranks."""
    from .agg_aud_exp_nerf import DIM_EXPR, build_head_network
    frames = dataset.DrivingFrames(args.datadir, args.aud_file, "val", args, skip=args.testskip, device=device)
    width = len(frames.all_exprs[0])
    dim_expr = DIM_EXPR if model == "agg" else args.dim_expr
    if dim_expr != width:
        raise ValueError(f"dim_expr is {dim_expr}, the expression track {args.evalExpr_path} is {width} wide")
    network = _same_on_every_rank(lambda: build_head_network(args, frames.H, frames.W, frames.focal, model)).to(device)
    latent_code = torch.zeros(32, dtype=torch.float32)
    path = None
    if not args.no_reload:
        path = args.ft_path if not _unset(args.ft_path) else checkpoint.latest_checkpoint(os.path.join(args.basedir, args.expname))
        if path is not None:
            _, codes = checkpoint.load_checkpoint(path, network, map_location=device)
            latent_code = codes[0]
    if learned_background:
        _learned_background(frames, path, device)
    if precision is not None:
        set_render_precision(network, precision)
    name = f"{args.datadir[8:].lstrip(os.sep)}_{args.aud_file[-9:-4]}"
    out = os.path.join(args.save_path, f"V_{name}_N_ExpPose0.avi") if out is None else out
    stills = os.path.join(args.save_path, name + "_ExpPose_{i}.jpg") if still_every else None
    for d in {os.path.dirname(os.path.abspath(p)) for p in (out, stills) if p}:
        os.makedirs(d, exist_ok=True)
    res = clip.render_head_clip(network, frames, out, global_step, latent_code=latent_code, seed=seed, codec=codec,
                                still_every=still_every, still_path=stills, group=group, **({} if cull is None else dict(cull=cull)))
    return None if res is None else dict(res, path=out)


def head_expr_width(run_dir, input_ch_views=27):
    """The expression width of the head pair that the torso stage's checkpoints in ``run_dir`` hold: the input width of
    ``face_nerf_coarse.views_linears.0`` (``input_ch_views`` view columns -- 27 at ``multires_views = 4`` -- + 256 features +
    the expression) in the newest ``*head.tar*``, else in the newest ``*torso.tar*``.  FileNotFoundError without either."""
    path = checkpoint.latest_checkpoint(run_dir, contains="head.tar") or checkpoint.latest_checkpoint(run_dir, contains="torso.tar")
    if path is None:
        raise FileNotFoundError(f"no *head.tar* and no *torso.tar* in {run_dir}")
    state = torch.load(path, map_location="cpu", weights_only=False)["model_state_dict"]
    return int(state["face_nerf_coarse.views_linears.0.weight"].shape[1]) - input_ch_views - 256


def drive_torso(args, *, out=None, device="cuda", codec="MJPG", still_every=10, seed=None, group=None, precision=None, cull=None):
    """``test_torso.py --with_test`` on the flags ``args`` (``train_torso.config_parser().parse_args()``): the track of
    ``dataset.load_test_data(args.datadir, args.aud_file, args.test_pose_file, args.testskip, args.test_size, args.aud_start)``,
    a ``train_torso.Network`` whose head pair has the expression width of the run directory's head checkpoint
    (``head_expr_width``), the checkpoints as ``train_torso.train`` loads them (``train_torso.load_stage_checkpoints``, no
    optimiser), latent code row 0, and ``clip.render_torso_clip`` with the background as ``bc_img / 255``, ``swap_rb=True`` and
    the stills ``{aud_id}.jpg`` / ``{aud_id}_torso.jpg`` in ``args.save_path``; ``out`` defaults to ``result.avi`` there.

    Where the head pair takes an expression, frame j gets row j of ``dataset.load_test_exprs(args.evalExpr_path or
    args.test_pose_file, args.testskip, F)`` (ValueError where its width is not the head pair's); a head pair without
    expression columns gets none.  ``cull``: ``render_torso_clip``'s.  -> ``render_torso_clip``'s dict plus ``path`` on rank 0,
    None on the other ranks."""
    from .train_torso import Network, load_stage_checkpoints
    poses, auds, bc_img, (H, W, focal, _, _), aud_ids, torso_pose = dataset.load_test_data(
        args.datadir, args.aud_file, args.test_pose_file, args.testskip, args.test_size, args.aud_start)
    run_dir = os.path.join(args.basedir, args.expname)
    dim_expr_head = head_expr_width(run_dir, input_channels(args)[1])
    track = None
    if dim_expr_head > 0:
        expr_path = args.test_pose_file if _unset(args.evalExpr_path) else args.evalExpr_path
        track = dataset.load_test_exprs(expr_path, args.testskip, poses.shape[0])
        if track.shape[1] != dim_expr_head:
            raise ValueError(f"the head pair of {run_dir} takes {dim_expr_head} expression columns, the track {expr_path} is "
                             f"{track.shape[1]} wide")
    cfg = to_render_config(args)
    cfg.dim_expr = dim_expr_head
    network = _same_on_every_rank(lambda: Network(
        int(H), int(W), focal, near=args.near, far=args.far, chunk=args.chunk, N_samlpes=args.N_samples,
        N_importance=args.N_importance, args=cfg, dim_aud_body=args.dim_aud_body, dim_expr_head=dim_expr_head)).to(device)
    _, codes = load_stage_checkpoints(run_dir, network, None, device)
    if precision is not None:
        set_render_precision(network, precision)
    os.makedirs(args.save_path, exist_ok=True)
    out = os.path.join(args.save_path, "result.avi") if out is None else out
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = clip.render_torso_clip(network, poses, auds, bc_img / 255, out, expr=track, latent_code=codes[0], torso_pose=torso_pose,
                                 aud_ids=aud_ids, seed=seed, codec=codec, swap_rb=True, still_every=still_every,
                                 still_path=args.save_path, group=group, **({} if cull is None else dict(cull=cull)))
    return None if res is None else dict(res, path=out)


def baseline_names(args):
    """test_nerf.py:179,187 -> (the clip's file name, the stills' name pattern with ``{i}`` for the frame's position)."""
    name = f"{args.datadir[8:].lstrip(os.sep)}_{args.aud_file[:-4]}"
    return f"V_{name}_N_baseline.avi", name + "_ADNeRF_{i}.jpg"


def drive_baseline(args, *, out=None, device="cuda", codec="MJPG", still_every=10, seed=None, group=None, precision=None,
                   learned_background=False, cull=None):
    """The baseline tester's ``test()`` (NeRFs/HeadNeRF/test/test_nerf.py:140-190) on the flags ``args``
    (``helper.config_parser().parse_args()``): ``BaselineTestFrames(args.datadir, args.aud_file, "val", args,
    skip=args.testskip)`` -- the val poses, frame i with audio row i --, a ``head_baseline.Network`` with
    ``to_render_config(args)``, the weights of ``args.ft_path`` (an AD-NeRF four-dict file, ``checkpoint.load_adnerf``) -- else
    of the newest ``*tar`` of ``basedir/expname`` (``checkpoint.load_baseline_checkpoint``; none: the network as initialised,
    as upstream) --, every frame through ``clip.render_head_clip(model="baseline")`` at ``global_step = 0`` (:174: always the
    unsmoothed audio branch).

    ``out`` defaults to upstream's ``V_{datadir[8:]}_{aud_file[:-4]}_N_baseline.avi`` under ``args.save_path``; every
    ``still_every``-th frame is also written there as ``{datadir[8:]}_{aud_file[:-4]}_ADNeRF_{i}.jpg``.  Channels as upstream
    (:184-189): the red/blue-swapped bytes go to BOTH writers, the clip's (which takes them as BGR) and the stills' (which
    takes them as RGB).  Frame-parallel inside a process group like ``drive_head``.  ``learned_background``: as ``drive_head``
    (the run file of ``train_baseline.train(learn_background=True)``; an AD-NeRF ``ft_path`` holds none).  ``cull``: as ``drive_head``.
    -> ``render_head_clip``'s dict plus ``path`` on rank 0, None on the other ranks."""
    from .agg_aud_exp_nerf import build_head_network
    frames = dataset.BaselineTestFrames(args.datadir, args.aud_file, "val", args, skip=args.testskip, device=device)
    network = _same_on_every_rank(lambda: build_head_network(args, frames.H, frames.W, frames.focal, "baseline")).to(device)
    if not _unset(args.ft_path):
        path = args.ft_path
        checkpoint.load_adnerf(args.ft_path, network, map_location=device)
    else:
        path = checkpoint.latest_checkpoint(os.path.join(args.basedir, args.expname), contains="tar")
        if path is not None:
            checkpoint.load_baseline_checkpoint(path, network, map_location=device)
    if learned_background:
        _learned_background(frames, path, device)
    if precision is not None:
        set_render_precision(network, precision)
    clip_name, still_name = baseline_names(args)
    out = os.path.join(args.save_path, clip_name) if out is None else out
    stills = os.path.join(args.save_path, still_name) if still_every else None
    for d in {os.path.dirname(os.path.abspath(p)) for p in (out, stills) if p}:
        os.makedirs(d, exist_ok=True)
    res = clip.render_head_clip(network, frames, out, 0, latent_code=None, seed=seed, codec=codec, swap_rb=True,
                                still_every=still_every, still_path=stills, group=group, model="baseline", stills_as_rgb=True,
                                **({} if cull is None else dict(cull=cull)))
    return None if res is None else dict(res, path=out)
