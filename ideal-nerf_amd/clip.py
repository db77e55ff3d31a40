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
from .parallel import ClipAssembler, frames_of


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


def _run(frames, render_one, network, path, group, seed, fps, codec, swap_rb, still_every, still_path, still_ids):
    """The loop both flows share.  render_one(position, frame) -> (u8 [H, W, 3], int32 flag), both on the device."""
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
                if assembler is None:   # rank 0 holds frame 0: its size is the clip's
                    sink = None
                    if rank == 0:
                        sink = FrameSink(path, u8.shape[1], u8.shape[0], fps=fps, swap_rb=swap_rb, device=device, codec=codec,
                                         still_every=still_every, still_path=still_path, still_ids=still_ids)
                    assembler = ClipAssembler(sink, n, group)
                assembler.push(u8, flag if u8 is not None else False)
        done = assembler.close() if assembler is not None else (dict(n_frames=0, nonfinite_frames=[]) if rank == 0 else None)
    finally:
        network.train(was_training)
    if done is None:
        return None
    seconds = time.perf_counter() - t0
    return dict(done, seconds=seconds, frames_per_s=n / seconds if n else 0.0, world=world)


def render_head_clip(network, dataset, path, global_step, *, latent_code, frames=None, seed=None, fps=25, codec="MJPG",
                     swap_rb=False, still_every=0, still_path=None, group=None):
    """The head-only eval loop: every frame of ``frames`` (default: the whole ``dataset``, a ``dataset.GetData`` in
    val mode) through ``network([data, global_step, dataset.data_size])`` in eval mode under no_grad, converted on
    the device and written to the AVI at ``path`` in order; ``still_path="dir/name_{i}.jpg"`` with
    ``still_every=10`` adds the reference's stills ({i}: position in the clip).  This rank reads only its own frames,
    through a batch-1 in-process loader, so every field is collated as the reference's loader collates it.

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
        rgb = network([(*data[:7], latent_code, data[7]), global_step, dataset.data_size])[0]
        flag = torch.zeros(1, dtype=torch.int32, device=device)
        return ops.to8b(rgb, swap_rb, flag), flag

    return _run(frames, render_one, network, path, group, seed, fps, codec, swap_rb, still_every, still_path, None)


def render_torso_clip(network, poses, auds, bc_img, path, *, expr, latent_code, torso_pose, aud_ids=None, frames=None,
                      seed=None, fps=25, codec="MJPG", swap_rb=False, still_every=0, still_path=None, group=None):
    """The head + torso clip loop for a ``train_torso.Network``.  poses [F, >=3, 4], auds [F, 16, 29] (the clip's
    DeepSpeech windows), bc_img [H, W, 3] in [0, 1], torso_pose [>=3, 4] (the fixed camera of the torso pair).

    Once per clip (on every rank: it is small, and the ranks stay independent): the smoothed audio feature of
    every frame (``clip_audio_features``, test_torso.py:478-498).  Per frame j: the torso signal
    ``[aud_smo[j][:dim_aud_body] | PE_3(euler) | PE_3(translation)]`` of ``poses[j]`` (:503-507), the head pair at
    ``poses[j]`` with ``aud_smo[j]``, the torso pair at ``torso_pose`` with the signal, and
    ``to8b(rgb * last_weight_torso[..., None] + rgb_fg_torso)`` as one kernel (``ops.compose_to8b``).  This is the
    reference's clip flow; ``Network.forward`` is its training step (unsmoothed audio, one pose for both pairs).

    ``still_path`` is a directory here: with ``still_every=10`` it receives ``{aud_id}.jpg`` and
    ``{aud_id}_torso.jpg`` of every 10th frame (:526-531; aud_ids defaults to the frame numbers).  The reference
    writes ``rgb8[:, :, ::-1]`` to its cv2 writer, which is ``swap_rb=True`` here.  Returns as render_head_clip."""
    device = next(network.parameters()).device
    n_clip = int(poses.shape[0])
    frames = list(range(n_clip) if frames is None else frames)
    aud_ids = list(range(n_clip) if aud_ids is None else aud_ids)
    f32 = lambda t: torch.as_tensor(t).to(device=device, dtype=torch.float32)
    poses_host = torch.as_tensor(poses).detach().to(device="cpu", dtype=torch.float32)   # the camera travels as kernel arguments
    poses_dev, torso_host = f32(poses), torch.as_tensor(torso_pose).detach().to(device="cpu", dtype=torch.float32)
    bc_img, expr, latent_code = f32(bc_img), f32(expr), f32(latent_code)
    H, W = int(bc_img.shape[0]), int(bc_img.shape[1])
    with torch.no_grad():
        aud_smo = clip_audio_features(network.aud_net, network.aud_att_net, f32(auds), network.args.smo_size)
    kw = dict(H=H, W=W, focal=network.focal, chunk=network.args.chunk, near=network.near, far=network.far, bc_rgb=bc_img)
    head = {"coarse": network.face_nerf_coarse, "fine": network.face_nerf_fine}
    torso = {"coarse": network.torso_coarse_nerf, "fine": network.torso_fine_nerf}

    def render_one(pos, j):
        signal = network.torso_signal(aud_smo[j], poses_dev[j])
        rgb, _, _, _, _, _ = network.render_pair(expr=expr, latent_code=latent_code, aud_para=aud_smo[j],
                                                 render_poses=poses_host[j][:3, :4], network_nerf=head, **kw)
        _, _, _, last_w, rgb_fg, _ = network.render_pair(expr=None, latent_code=None, aud_para=signal,
                                                         render_poses=torso_host[:3, :4], network_nerf=torso, **kw)
        flag = torch.zeros(1, dtype=torch.int32, device=device)
        still = bool(still_every) and pos % still_every == 0
        out = ops.compose_to8b(rgb, last_w, rgb_fg, swap_rb, flag, want_fg=still)
        if still:   # the torso-only still is written by the rank that rendered it; the composite's by rank 0's sink
            out, fg = out
            with open(os.path.join(still_path, f"{aud_ids[j]}_torso.jpg"), "wb") as f:
                f.write(encode_jpeg(fg.cpu().numpy()))
        return out, flag

    names = os.path.join(still_path, "{i}.jpg") if still_every and still_path else None
    return _run(frames, render_one, network, path, group, seed, fps, codec, swap_rb, still_every, names,
                [aud_ids[j] for j in frames])
