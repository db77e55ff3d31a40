"""Whole clips: the reference's two render loops as functions.

``render_head_clip``   NeRFs/HeadNeRF/test/eval_aud_exp_nerf.py:435-496 -- ``GetData(val)`` -> loader ->
                       ``network([data, step, n])`` -> ``to8b`` -> writer.
``render_torso_clip``  NeRFs/TorsoNeRF/test_torso.py:474-535 -- one audio pass over the clip, then per frame the
                       head pair, the torso pair, ``rgbs * last_weights_torso[..., None] + rgb_fgs_torso``,
                       ``to8b``, ``vid_out.write``, stills every 10th frame.

Both are frame-parallel: inside an initialised process group rank r renders the frames
``parallel.frames_of(r, N, n)`` of the clip, converts each to bytes itself and hands it to a
``parallel.ClipAssembler``; rank 0 owns the ``frame_io.FrameSink`` and writes the clip in order.  There is no
collective until a frame is finished.  Without a process group the same code renders every frame and the
assembler is a pass-through, so a clip is the same file for any world size.

``score_head_clip`` / ``score_torso_clip`` are the same two loops with ground truth beside them: every rendered frame is
scored on the device where it was rendered (``ops.frame_scores``: squared error and SSIM, whole frame and per sampling
region) into this rank's rows of a table, and one gather at the end of the clip puts the rows in frame order on rank 0.
"""
import contextlib
import math
import os
import time

import torch
import torch.distributed as dist

from . import ops
from .frame_io import FrameSink, encode_jpeg
from .models.audio_net import clip_audio_features
from .parallel import ClipAssembler, frames_of, gather_frame_rows


def _ranks(group):
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


@contextlib.contextmanager
def _frame_rng(seed, frame, device):
    """seed is None: the live generators, as the per-frame API draws.  Else frame j draws from the CPU generator and the
    render device's generator, both seeded with seed + j, and the caller's generators are left as they were: a
    perturb > 0 clip does not depend on which rank renders a frame, in either draw mode (torch.rand tensors come
    from the device generator, the in-kernel draws' seed from the CPU generator)."""
    if seed is None:
        yield
        return
    with torch.random.fork_rng(devices=[device]):
        torch.default_generator.manual_seed(int(seed) + int(frame))
        with torch.cuda.device(device):
            torch.cuda.manual_seed(int(seed) + int(frame))
        yield


def _run(frames, render_one, network, path, group, seed, fps, codec, swap_rb, still_every, still_path, still_ids, write=True):
    """The loop every flow shares.  render_one(position, frame) -> (u8 [H, W, 3], int32 flag), both on the device; it is the
    per-frame hook: what else a flow does with a frame (scoring it) happens in there.  write=False: the frames are rendered
    and handed to nobody -- no sink, no assembler, no collective; render_one's return value is not looked at."""
    rank, world = _ranks(group)
    n = len(frames)
    if still_every and not still_path:
        raise ValueError("still_every needs still_path")
    device = next(network.parameters()).device
    was_training = network.training
    network.eval()
    assembler, t0 = None, time.perf_counter()
    try:
        with torch.no_grad():
            for k in range(math.ceil(n / world)):
                pos = k * world + rank
                u8 = flag = None
                if pos < n:
                    with _frame_rng(seed, frames[pos], device):
                        u8, flag = render_one(pos, frames[pos])
                if not write:
                    continue
                if assembler is None:   # rank 0 holds frame 0: its size is the clip's
                    sink = None
                    if rank == 0:
                        sink = FrameSink(path, u8.shape[1], u8.shape[0], fps=fps, swap_rb=swap_rb, device=device, codec=codec,
                                         still_every=still_every, still_path=still_path, still_ids=still_ids)
                    assembler = ClipAssembler(sink, n, group)
                assembler.push(u8, flag if u8 is not None else False)
        done = assembler.close() if assembler is not None else (dict(n_frames=0 if write else n, nonfinite_frames=[]) if rank == 0 else None)
    finally:
        network.train(was_training)
    if done is None:
        return None
    seconds = time.perf_counter() - t0
    return dict(done, seconds=seconds, frames_per_s=n / seconds if n else 0.0, world=world)


def _forward_tuple(data, latent_code, model):
    """A head-stage loader's item as ``Network.forward`` takes it: the latent code before the index -- the baseline's 7-tuple
    (``model="baseline"``: no expression, no latent code) as it is."""
    return tuple(data) if model == "baseline" else (*data[:7], latent_code, data[7])


def head_cull_conditioning(network, items, global_step, dataset_size, latent_code, model="head"):
    """What a cull grid of the head pair is built from (cull.build_grid): per item of `items` -- the tuples the loop hands to
    ``network([tuple, global_step, dataset_size])``, collated by a loader or not -- the (aud_para, expr, latent_code) triple
    ``Network.forward`` passes to the render, made by the functions it calls (``audio_feature`` and through it
    ``smoothed_audio_feature``, ``expr_feature``), and the camera.  -> (conds, cameras [n, 3, 4] on the host, H, W)."""
    dev = next(network.parameters()).device
    sq = lambda t: torch.squeeze(torch.as_tensor(t)).to(device=dev, dtype=torch.float32)
    conds, cameras, size = [], [], None
    was_training = network.training
    network.eval()
    try:
        with torch.no_grad():
            for data in items:
                data = _forward_tuple(data, latent_code, model)
                baseline = model == "baseline"
                auds, raw_img, pose, index = data[3], torch.as_tensor(data[4]), data[5], data[-1]
                aud = network.audio_feature(sq(auds), int(index), global_step, dataset_size)
                expr = None if baseline else network.expr_feature(sq(data[6]))
                latent = None if baseline else torch.squeeze(torch.as_tensor(data[7])).to(dev)
                conds.append((aud, expr, latent))
                cameras.append(torch.squeeze(torch.as_tensor(pose)).detach().to(device="cpu", dtype=torch.float32)[:3, :4])
                # (the frame size as the class's forward reads it off raw_img)
                size = tuple(torch.squeeze(raw_img).shape[:2]) if baseline else (raw_img.shape[1], raw_img.shape[1])
    finally:
        network.train(was_training)
    return conds, torch.stack(cameras), int(size[0]), int(size[1])


def torso_cull_conditioning(network, poses, auds, expr, latent_code, frames):
    """What the two cull grids of the head + torso flow are built from: for the clip's `frames`, the head pair's
    (aud_smo[j], expr row, latent_code) and the torso pair's (torso_signal(aud_smo[j], poses[j]), None, None) -- the tensors
    ``_torso_pairs`` passes, made by the functions it calls (``clip_audio_features``, ``torso_signal``).
    -> (head_conds, torso_conds, head cameras [n, 3, 4] on the host)."""
    device = next(network.parameters()).device
    f32 = lambda t: torch.as_tensor(t).to(device=device, dtype=torch.float32)
    poses_host = torch.as_tensor(poses).detach().to(device="cpu", dtype=torch.float32)
    poses_dev, latent_code = f32(poses), f32(latent_code)
    expr = None if expr is None else f32(expr)
    per_frame = expr is not None and expr.dim() == 2
    with torch.no_grad():
        aud_smo = clip_audio_features(network.aud_net, network.aud_att_net, f32(auds), network.args.smo_size)
        head = [(aud_smo[j], expr[j] if per_frame else expr, latent_code) for j in frames]
        torso = [(network.torso_signal(aud_smo[j], poses_dev[j]), None, None) for j in frames]
    return head, torso, torch.stack([poses_host[j][:3, :4] for j in frames])


@contextlib.contextmanager
def _culled(network, cull, build):
    """cull is None: nothing happens (the network is not touched).  Else `build(options)` -> dict(head=, torso=) of grids is
    run before the first frame, the grids are installed for the body and removed whatever happens in it."""
    if cull is None:
        yield None
        return
    from . import cull as cull_mod
    grids = build(cull_mod.options(cull))
    network.set_cull(**grids)
    try:
        yield grids
    finally:
        network.set_cull(head=None, torso=None)


def _with_cull_summary(done, grids):
    if done is not None and grids is not None:
        from . import cull as cull_mod
        done = dict(done, cull=cull_mod.summary(grids))
    return done


def _head_grid(network, items, global_step, dataset_size, latent_code, model, opts):
    from . import cull as cull_mod
    conds, cameras, H, W = head_cull_conditioning(network, items, global_step, dataset_size, latent_code, model)
    nets = (network.face_nerf_coarse, network.face_nerf_fine) if network.N_importance > 0 else (network.face_nerf_coarse,)
    return dict(head=cull_mod.build_grid(nets, conds, cameras, H, W, network.focal, network.near, network.far, **opts))


def _torso_grids(network, poses, auds, bc_img, expr, latent_code, torso_pose, frames, opts):
    from . import cull as cull_mod
    head_c, torso_c, cameras = torso_cull_conditioning(network, poses, auds, expr, latent_code, frames)
    H, W = int(bc_img.shape[0]), int(bc_img.shape[1])
    fine = network.N_importance > 0
    kw = dict(H=H, W=W, focal=network.focal, near=network.near, far=network.far, **opts)
    torso_cam = torch.as_tensor(torso_pose).detach().to(device="cpu", dtype=torch.float32)[:3, :4]
    return dict(head=cull_mod.build_grid((network.face_nerf_coarse, network.face_nerf_fine) if fine else (network.face_nerf_coarse,),
                                         head_c, cameras, **kw),
                torso=cull_mod.build_grid((network.torso_coarse_nerf, network.torso_fine_nerf) if fine else (network.torso_coarse_nerf,),
                                          torso_c, torso_cam[None], **kw))


def render_head_clip(network, dataset, path, global_step, *, latent_code, frames=None, seed=None, fps=25, codec="MJPG",
                     swap_rb=False, still_every=0, still_path=None, group=None, model="head", stills_as_rgb=False, cull=None):
    """The head-only eval loop: every frame of ``frames`` (default: the whole ``dataset``, a ``dataset.GetData`` in
    val mode) through ``network([data, global_step, dataset.data_size])`` in eval mode under no_grad, converted on
    the device and written to the AVI at ``path`` in order; ``still_path="dir/name_{i}.jpg"`` with
    ``still_every=10`` adds the reference's stills ({i}: position in the clip).  This rank reads only its own frames,
    through a batch-1 in-process loader, so every field is collated as the reference's loader collates it.
    ``model="baseline"``: a ``head_baseline.Network`` on a ``dataset.BaselineGetData`` (``latent_code`` is not read).
    ``stills_as_rgb``: the stills are written the way ``imageio.imwrite`` writes the frame's bytes -- taken as RGB, quality 75
    -- where the sink writes them as cv2 does (taken as BGR, quality 95): test_nerf.py:184-189 hands ONE array to both
    writers.  Each still is then written by the rank that rendered the frame.
    ``cull``: None, or ``dict(G=, dilate=, sigma_min=, frame_stride=, samples=)`` (any subset; cull.DEFAULTS; ``samples=True`` also
    skips the live rays' samples in empty cells, same bytes, and adds ``evaluated_share`` to the result's ``cull``) -- before the first frame every
    rank builds the head pair's occupancy grid from the WHOLE clip (it reads every frame's item once more for it), installs
    it (``network.set_cull``) and removes it at the end; the result gains ``cull = dict(build_seconds, network_seconds,
    occupied_share, live_share)``.

    Returns on rank 0 ``dict(n_frames, nonfinite_frames, seconds, frames_per_s, world)`` (seconds: first render to
    the file being closed), None on the other ranks.  A frame with a NaN/Inf is reported, not fatal."""
    from torch.utils.data import DataLoader, Subset
    frames = list(range(dataset.data_size) if frames is None else frames)
    rank, world = _ranks(group)
    share = [frames[p] for p in frames_of(rank, world, len(frames))]
    loader = iter(DataLoader(Subset(dataset, share), batch_size=1, shuffle=False, num_workers=0))
    device = next(network.parameters()).device

    def render_one(pos, frame):
        data = next(loader)
        rgb = network([_forward_tuple(data, latent_code, model), global_step, dataset.data_size])[0]
        flag = torch.zeros(1, dtype=torch.int32, device=device)
        u8 = ops.to8b(rgb, swap_rb, flag)
        if stills_as_rgb and still_every and pos % still_every == 0:
            with open(still_path.format(i=pos), "wb") as f:
                f.write(encode_jpeg(u8.cpu().numpy()[..., ::-1], quality=75))
        return u8, flag

    if stills_as_rgb and still_every and not still_path:
        raise ValueError("still_every needs still_path")
    whole_clip = lambda: iter(DataLoader(Subset(dataset, frames), batch_size=1, shuffle=False, num_workers=0))
    with _culled(network, cull, lambda o: _head_grid(network, whole_clip(), global_step, dataset.data_size, latent_code, model, o)) as grids:
        done = _run(frames, render_one, network, path, group, seed, fps, codec, swap_rb, 0 if stills_as_rgb else still_every,
                    still_path, None)
    return _with_cull_summary(done, grids)


def _torso_pairs(network, poses, auds, bc_img, expr, latent_code, torso_pose):
    """The per-frame body of the head + torso clip loop: once per clip the smoothed audio features, then
    pairs(j) -> (rgb of the head pair at poses[j], last_weight and rgb_fg of the torso pair at torso_pose), on the device.
    expr: one vector for the whole clip, a track [F, E] whose row j goes to frame j of the clip (ValueError here, before
    anything is rendered, where F is not the clip's length), or None for a head pair without expression columns."""
    device = next(network.parameters()).device
    f32 = lambda t: torch.as_tensor(t).to(device=device, dtype=torch.float32)
    poses_host = torch.as_tensor(poses).detach().to(device="cpu", dtype=torch.float32)   # the camera travels as kernel arguments
    poses_dev, torso_host = f32(poses), torch.as_tensor(torso_pose).detach().to(device="cpu", dtype=torch.float32)
    bc_img, latent_code = f32(bc_img), f32(latent_code)
    expr = None if expr is None else f32(expr)
    per_frame = expr is not None and expr.dim() == 2
    if per_frame and expr.shape[0] != poses_host.shape[0]:
        raise ValueError(f"expr holds {expr.shape[0]} rows, the clip has {poses_host.shape[0]} frames: pass one row per frame "
                         "of the clip, or one vector for all of them")
    H, W = int(bc_img.shape[0]), int(bc_img.shape[1])
    with torch.no_grad():
        aud_smo = clip_audio_features(network.aud_net, network.aud_att_net, f32(auds), network.args.smo_size)
    kw = dict(H=H, W=W, focal=network.focal, chunk=network.args.chunk, near=network.near, far=network.far, bc_rgb=bc_img)
    head = {"coarse": network.face_nerf_coarse, "fine": network.face_nerf_fine}
    torso = {"coarse": network.torso_coarse_nerf, "fine": network.torso_fine_nerf}

    def pairs(j):
        signal = network.torso_signal(aud_smo[j], poses_dev[j])
        rgb, _, _, _, _, _ = network.render_pair(expr=expr[j] if per_frame else expr, latent_code=latent_code,
                                                 aud_para=aud_smo[j], render_poses=poses_host[j][:3, :4], network_nerf=head, **kw)
        _, _, _, last_w, rgb_fg, _ = network.render_pair(expr=None, latent_code=None, aud_para=signal,
                                                         render_poses=torso_host[:3, :4], network_nerf=torso, **kw)
        return rgb, last_w, rgb_fg

    return pairs


def render_torso_clip(network, poses, auds, bc_img, path, *, expr, latent_code, torso_pose, aud_ids=None, frames=None,
                      seed=None, fps=25, codec="MJPG", swap_rb=False, still_every=0, still_path=None, group=None, cull=None):
    """The head + torso clip loop for a ``train_torso.Network``.  poses [F, >=3, 4], auds [F, 16, 29] (the clip's
    DeepSpeech windows), bc_img [H, W, 3] in [0, 1], torso_pose [>=3, 4] (the fixed camera of the torso pair).  expr: one
    expression vector for the whole clip, or a track [F, E] -- row j goes to frame j of the clip, whatever ``frames`` selects
    (another first dimension than F raises ValueError before anything is rendered) --, or None for a head pair built with
    ``dim_expr_head=0``.

    Once per clip (on every rank: it is small, and the ranks stay independent): the smoothed audio feature of
    every frame (``clip_audio_features``, test_torso.py:478-498).  Per frame j: the torso signal
    ``[aud_smo[j][:dim_aud_body] | PE_3(euler) | PE_3(translation)]`` of ``poses[j]`` (:503-507), the head pair at
    ``poses[j]`` with ``aud_smo[j]``, the torso pair at ``torso_pose`` with the signal, and
    ``to8b(rgb * last_weight_torso[..., None] + rgb_fg_torso)`` as one kernel (``ops.compose_to8b``).  This is the
    reference's clip flow; ``Network.forward`` is its training step (unsmoothed audio, one pose for both pairs).

    ``still_path`` is a directory here: with ``still_every=10`` it receives ``{aud_id}.jpg`` and
    ``{aud_id}_torso.jpg`` of every 10th frame (:526-531; aud_ids defaults to the frame numbers).  The reference
    writes ``rgb8[:, :, ::-1]`` to its cv2 writer, which is ``swap_rb=True`` here.  Returns as render_head_clip.
    ``cull`` as there: one grid per pair, each from the whole clip's conditioning; the torso pair's camera is the one
    ``torso_pose``, so its pixels are classified once per clip."""
    device = next(network.parameters()).device
    n_clip = int(poses.shape[0])
    frames = list(range(n_clip) if frames is None else frames)
    aud_ids = list(range(n_clip) if aud_ids is None else aud_ids)
    pairs = _torso_pairs(network, poses, auds, bc_img, expr, latent_code, torso_pose)

    def render_one(pos, j):
        rgb, last_w, rgb_fg = pairs(j)
        flag = torch.zeros(1, dtype=torch.int32, device=device)
        still = bool(still_every) and pos % still_every == 0
        out = ops.compose_to8b(rgb, last_w, rgb_fg, swap_rb, flag, want_fg=still)
        if still:   # the torso-only still is written by the rank that rendered it; the composite's by rank 0's sink
            out, fg = out
            with open(os.path.join(still_path, f"{aud_ids[j]}_torso.jpg"), "wb") as f:
                f.write(encode_jpeg(fg.cpu().numpy()))
        return out, flag

    names = os.path.join(still_path, "{i}.jpg") if still_every and still_path else None
    with _culled(network, cull, lambda o: _torso_grids(network, poses, auds, bc_img, expr, latent_code, torso_pose, frames, o)) as grids:
        done = _run(frames, render_one, network, path, group, seed, fps, codec, swap_rb, still_every, names,
                    [aud_ids[j] for j in frames])
    return _with_cull_summary(done, grids)


def summarise_clip(table):
    """Score table [n, 5, 4] (``ops.frame_scores`` rows, one per frame) -> dict(per_frame, mean, pooled):
    per_frame  ``ops.summarise_scores(table)``: mse / psnr / ssim, [n, 5] each (groups: ops.SCORE_GROUPS);
    mean       per group the mean over frames of psnr and of ssim, taken over the frames where the value is finite, with
               ``n_excluded`` = how many frames that leaves out (a group absent from a frame, a perfect or a non-finite frame):
               reported, never silently dropped;
    pooled     mse / psnr / ssim of the table summed over frames (every pixel and window of the clip weighs the same)."""
    import numpy as np
    t = np.asarray(table.detach().cpu() if isinstance(table, torch.Tensor) else table, dtype=np.float64).reshape(-1, 5, 4)
    per_frame = ops.summarise_scores(t)
    mean = dict(n_excluded={})
    for key in ("psnr", "ssim"):
        ok = np.isfinite(per_frame[key])
        kept = ok.sum(0)
        with np.errstate(invalid="ignore"):
            mean[key] = np.where(kept > 0, np.where(ok, per_frame[key], 0.0).sum(0) / np.maximum(kept, 1), np.nan)
        mean["n_excluded"][key] = (t.shape[0] - kept).astype(np.int64)
    return dict(per_frame=per_frame, mean=mean, pooled=ops.summarise_scores(t.sum(0)))


def _score(frames, score_one, network, path, group, seed, fps, codec, swap_rb, device):
    """What both scoring flows share around ``_run``: this rank's rows of the device table, the loop, the one gather, the
    result.  score_one(frame, out_row, want_bytes) renders frame `frame`, scores it into out_row (float64 [5, 4], device) and
    returns (u8 or None, flag or None)."""
    rank, world = _ranks(group)
    n = len(frames)
    table = torch.zeros((len(frames_of(rank, world, n)), 5, 4), dtype=torch.float64, device=device)
    write = path is not None
    t0 = time.perf_counter()
    done = _run(frames, lambda pos, frame: score_one(frame, table[pos // world], write), network, path, group, seed, fps, codec,
                swap_rb, 0, None, None, write=write)
    rows = gather_frame_rows(table, n, group)
    if rows is None:
        return None
    rows = rows.cpu()             # the one device-to-host copy: 160 bytes per frame
    seconds = time.perf_counter() - t0
    bad = sorted(set(done["nonfinite_frames"]) | {int(i) for i in torch.nonzero(~torch.isfinite(rows[:, 0, 1])).reshape(-1)})
    return dict(summarise_clip(rows), frames=list(frames), table=rows, n_frames=n, nonfinite_frames=bad, seconds=seconds,
                frames_per_s=n / seconds if n else 0.0, world=world)


def score_head_clip(network, frames, global_step, *, latent_code, frame_ids=None, path=None, seed=None, group=None, fps=25,
                    codec="MJPG", swap_rb=False, model="head", cull=None):
    """``render_head_clip`` with the ground truth beside it.  ``frames`` is a val-mode ``dataset.ResidentFrames``: frame j of
    ``frame_ids`` (default: all of them) comes from ``frames.frame(j)`` -- no file read, no host meshgrid -- goes through
    ``network([data, global_step, frames.data_size])`` in eval mode under no_grad (the caller's mode is restored), and the float
    render is scored on the device against ``frames.imgs[j]`` per region of ``frames.maps[j]`` (``ops.frame_scores``).  No
    float frame leaves the device.  Frame-parallel like the render loops (``parallel.frames_of``; ``seed`` as there), with one
    collective at the end of the clip (``parallel.gather_frame_rows``).

    ``model="baseline"``: a ``head_baseline.Network`` on a val-mode ``dataset.ResidentBaselineFrames`` (``latent_code`` is not
    read; the torso group of its byte map is empty, so that row stays nan).

    ``path=None``: nothing is converted to bytes and nothing is written.  With ``path`` the clip is also written, through the
    same conversion, assembler and sink as ``render_head_clip``: the same file.

    Returns on rank 0 (None on the other ranks) ``dict(frames, table, per_frame, mean, pooled, n_frames, nonfinite_frames,
    seconds, frames_per_s, world)``: ``table`` float64 [n, 5, 4] on the host (rows ops.SCORE_GROUPS, columns
    ops.SCORE_COLUMNS), per_frame / mean / pooled as ``summarise_clip``; nonfinite_frames: POSITIONS in the clip whose render
    holds a NaN/Inf (their sums are not finite, so ``mean`` counts them in n_excluded); seconds: first render to the table
    on the host.  ``cull`` as ``render_head_clip``."""
    device = next(network.parameters()).device
    ids = list(range(frames.data_size) if frame_ids is None else frame_ids)
    ws = torch.empty(ops.frame_scores_workspace_doubles(frames.H, frames.W), dtype=torch.float64, device=device)

    def score_one(j, row, want_bytes):
        data = frames.frame(j)
        rgb = network([_forward_tuple(data, latent_code, model), global_step, frames.data_size])[0]
        ops.frame_scores(rgb, frames.imgs[j], frames.maps[j], out=row, workspace=ws)
        if not want_bytes:
            return None, None
        flag = torch.zeros(1, dtype=torch.int32, device=device)
        return ops.to8b(rgb, swap_rb, flag), flag

    items = lambda: (frames.frame(j) for j in ids)
    with _culled(network, cull, lambda o: _head_grid(network, items(), global_step, frames.data_size, latent_code, model, o)) as grids:
        done = _score(ids, score_one, network, path, group, seed, fps, codec, swap_rb, device)
    return _with_cull_summary(done, grids)


def score_torso_clip(network, poses, auds, bc_img, truth, *, regions=None, expr, latent_code, torso_pose, frames=None,
                     path=None, seed=None, group=None, fps=25, codec="MJPG", swap_rb=False, cull=None):
    """``render_torso_clip`` with the ground truth beside it: truth uint8 [F, H, W, 3] and (optionally) regions uint8 [F, H, W]
    (``dataset.region_byte_map``) on the device, indexed like poses; expr as there (one vector, or a track [F, E] indexed by
    the clip's frame number).  Per frame the same two render pairs; what is scored is
    the FLOAT composite ``rgb * last_weight[..., None] + rgb_fg`` -- a torch expression with one frame-sized temporary, since
    the fused tail (``ops.compose_to8b``) keeps the composite in registers and hands out bytes only; with ``path`` the clip's
    bytes still come from that fused tail, so the file is ``render_torso_clip``'s.  Everything else, and the return value, as
    ``score_head_clip``; ``cull`` as ``render_torso_clip``."""
    device = next(network.parameters()).device
    ids = list(range(int(poses.shape[0])) if frames is None else frames)
    pairs = _torso_pairs(network, poses, auds, bc_img, expr, latent_code, torso_pose)
    ws = torch.empty(ops.frame_scores_workspace_doubles(truth.shape[1], truth.shape[2]), dtype=torch.float64, device=device)

    def score_one(j, row, want_bytes):
        rgb, last_w, rgb_fg = pairs(j)
        ops.frame_scores(rgb * last_w[..., None] + rgb_fg, truth[j], None if regions is None else regions[j], out=row, workspace=ws)
        if not want_bytes:
            return None, None
        flag = torch.zeros(1, dtype=torch.int32, device=device)
        return ops.compose_to8b(rgb, last_w, rgb_fg, swap_rb, flag), flag

    with _culled(network, cull, lambda o: _torso_grids(network, poses, auds, bc_img, expr, latent_code, torso_pose, ids, o)) as grids:
        done = _score(ids, score_one, network, path, group, seed, fps, codec, swap_rb, device)
    return _with_cull_summary(done, grids)
