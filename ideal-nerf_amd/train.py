"""The reference's training-loop body (NeRFs/HeadNeRF/train/audio_exp_nerf.py:529-558) as
a function (``train_step``): render the sampled rays with gradients, MSE(fine) + MSE(coarse) +
10 * lc_weight * ||latent||, Adam step, exponential learning-rate decay, PSNR -- and the loop around it
(``train``, audio_exp_nerf.py:451-593): datasets, Xavier init, per-frame latent codes, resume, epochs, the validation
frame, ``head.tar``.
"""
import logging
import os

import torch

from .helper import img2mse, mse2psnr


def make_optimizer(network, latent_codes, lrate=8e-4):
    """Adam over the network and the per-frame latent codes (audio_exp_nerf.py:493).  torch's default (foreach) form, as
    upstream: `fused=True` was measured in round 4 -- the same 14.3 ms step (the update is 0.09 ms of it either way), and on
    this ROCm build its steps did not track the CPU oracle's Adam (test_train_loop_adam_steps_match_oracle: 2 % off after
    three steps; 300 steps diverged) -- so it is not used."""
    return torch.optim.Adam(list(network.parameters()) + [latent_codes], lr=lrate, betas=(0.9, 0.999))


def decayed_lr(lrate, lrate_decay, global_step, decay_rate=0.1):
    """new_lrate = lrate * 0.1 ** (global_step / (lrate_decay * 1500))  (audio_exp_nerf.py:554-556)."""
    return lrate * (decay_rate ** (global_step / (lrate_decay * 1500)))


def _ssim_term(ssim, rgb, target):
    """``ssim`` = (weight, rows, k, p) of a step (``train(ssim_weight=, patches=)``) -> (weight * ssim_patch_loss on the FINE
    image's patch rows, the unweighted loss detached)."""
    from .ssim_loss import ssim_patch_loss
    weight, rows, k, p = ssim
    term = ssim_patch_loss(rgb[rows], target[rows], k, p)
    return weight * term, term.detach()


def train_step(network, optimizer, data, latent_codes, global_step, dataset_size, lrate=8e-4, lrate_decay=500, ssim=None):
    """One iteration of the loop at audio_exp_nerf.py:530-558.  ``data`` is the reference's
    8-tuple (batch_rays, target_s, bg_img, auds, raw_img, pose, expr, index).  ssim = (weight, rows, k, p) (no counterpart
    upstream; None: the step is what it was): ``weight * ssim_patch_loss`` of the fine image on the batch's patch rows
    (``ResidentFrames.patch_rows``) joins the loss, and the returned dict gains ``ssim_loss``, the unweighted term."""
    batch_rays, target_s, bg_img, auds, raw_img, pose, expr, index = data
    latent_code = latent_codes[int(index)]
    rgb, _, _, _, extras = network([(batch_rays, target_s, bg_img, auds, raw_img, pose, expr, latent_code, index),
                                    global_step, dataset_size])
    target = target_s.reshape(-1, 3).to(rgb.device, torch.float32)
    optimizer.zero_grad()
    img_loss = img2mse(rgb, target)
    loss = img_loss
    psnr = mse2psnr(img_loss.detach())
    if 'rgb0' in extras:
        loss = loss + img2mse(extras['rgb0'], target)
    latent_code_loss = torch.norm(latent_code) * network.args.lc_weight
    loss = loss + latent_code_loss * 10
    if ssim is not None:
        term, ssim_loss = _ssim_term(ssim, rgb, target)
        loss = loss + term
    new_lrate = _backward_and_update(loss, optimizer, global_step, lrate, lrate_decay)
    info = dict(loss=loss.detach(), psnr=psnr, latent_code_loss=latent_code_loss.detach(), lr=new_lrate)
    if ssim is not None:
        info["ssim_loss"] = ssim_loss
    return info


def baseline_train_step(network, optimizer, data, global_step, dataset_size, lrate=5e-4, lrate_decay=500, ssim=None):
    """One iteration of the AD-NeRF baseline's loop (NeRFs/HeadNeRF/train/head_baseline.py:466-491) on ``head_baseline.Network``:
    ``data`` is the baseline loader's 7-tuple (batch_rays, target_s, bg_img, auds, raw_img, pose, index); the loss is
    mse(rgb, target) + mse(rgb0, target) (:475-481) -- there is no latent code and so no latent term.  ssim: as ``train_step``."""
    target_s = data[1]
    rgb, _, _, _, extras = network([data, global_step, dataset_size])
    target = target_s.reshape(-1, 3).to(rgb.device, torch.float32)
    optimizer.zero_grad()
    img_loss = img2mse(rgb, target)
    loss = img_loss
    psnr = mse2psnr(img_loss.detach())
    if 'rgb0' in extras:
        loss = loss + img2mse(extras['rgb0'], target)
    if ssim is not None:
        term, ssim_loss = _ssim_term(ssim, rgb, target)
        loss = loss + term
    new_lrate = _backward_and_update(loss, optimizer, global_step, lrate, lrate_decay)
    info = dict(loss=loss.detach(), psnr=psnr, lr=new_lrate)
    if ssim is not None:
        info["ssim_loss"] = ssim_loss
    return info


def _backward_and_update(loss, optimizer, global_step, lrate, lrate_decay):
    """The tail both stages' steps share: backward, the gradient all-reduce inside a process group, the Adam step and the
    decayed learning rate for the next one -> that rate."""
    loss.backward()
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        from .parallel import average_gradients   # one bucketed all-reduce; a no-op for a single rank
        average_gradients([p for g in optimizer.param_groups for p in g['params']])
    optimizer.step()
    new_lrate = decayed_lr(lrate, lrate_decay, global_step)
    for group in optimizer.param_groups:
        # (a group with a rate of its own -- the pose deltas -- follows the same schedule at its own scale)
        group['lr'] = new_lrate * group['lr_scale'] if 'lr_scale' in group else new_lrate
    return new_lrate


def torso_train_step(network, optimizer, data, latent_codes, global_step, dataset_size, lrate=5e-4, lrate_decay=500):
    """One iteration of the torso stage's loop (NeRFs/TorsoNeRF/train_torso.py:516-541) on ``train_torso.Network``: ``data`` is
    the torso loader's 9-tuple (batch_rays, batch_rays_torso, target_s, bg_img, auds, raw_img, pose, expr, index); the loss is
    mse(rgb_com, target) + mse(rgb_com0, target), with no latent term.  ``optimizer`` holds what the stage trains (the torso
    pair and the audio nets); a head pair whose parameters do not require gradients runs the conditioning-only backward."""
    batch_rays, batch_rays_torso, target_s, bg_img, auds, raw_img, pose, expr, index = data
    latent_code = latent_codes[int(index)]
    rgb, rgb0 = network([(batch_rays, batch_rays_torso, target_s, bg_img, auds, raw_img, pose, expr, latent_code, index),
                         global_step, dataset_size])
    target = target_s.reshape(-1, 3).to(rgb.device, torch.float32)
    optimizer.zero_grad()
    img_loss = img2mse(rgb, target)
    psnr = mse2psnr(img_loss.detach())
    loss = img_loss + img2mse(rgb0, target)
    new_lrate = _backward_and_update(loss, optimizer, global_step, lrate, lrate_decay)
    return dict(loss=loss.detach(), psnr=psnr, lr=new_lrate)


logger = logging.getLogger("adnerf")


def draw_index(global_step, rank=0, world=1):
    """The sampler draw a replica uses at a step: rank r of N takes draw `global_step * N + r`, so the replicas of one step
    sample different rays and no draw is used twice.  A function of the step alone: a resumed run continues the sequence."""
    if not (0 <= rank < world) or global_step < 0:
        raise ValueError(f"rank {rank} of {world}, step {global_step}")
    return int(global_step) * int(world) + int(rank)


def _as_loader_item(item, with_expr=True):
    """What the reference's DataLoader makes of a GetData item (either stage's: the tuples end in raw_img, pose, expr, index; the
    baseline's, with_expr=False, in raw_img, pose, index), as far as Network.forward reads it: the pose as a tensor."""
    if not with_expr:
        *head, pose, index = item
        return (*head, torch.as_tensor(pose, dtype=torch.float32), index)
    *head, pose, expr, index = item
    return (*head, torch.as_tensor(pose, dtype=torch.float32), expr, index)


def _summary_writer(logdir):
    try:   # a TensorBoard writer if and only if it imports
        from torch.utils.tensorboard import SummaryWriter
    except Exception:
        return None
    return SummaryWriter(logdir)


def train(args, *, loader="resident", sample_seed=0, device="cuda", steps=None, on_log=None, on_step=None, max_bytes=8 << 30,
          val="reference", refine_poses=False, pose_lrate=None, refine_expr=False, expr_lrate=None, learn_background=False,
          bg_lrate=None, ssim_weight=0.0, patches=None, patch_region="rect"):
    """The reference's ``train()`` (audio_exp_nerf.py:451-593) on the flags ``args`` (``helper.config_parser().parse_args()``):
    write_config, the train and validation datasets, ``Network`` + ``init_weights``, ``latent_codes = ones[n_frames, 32]``, Adam,
    warm start from ``ft_path`` or resume from the newest ``*.tar`` of ``basedir/expname``, then epochs over the frames in
    order (one frame per step, as upstream's forward takes them) with a log line every ``i_print`` steps, one validation frame
    every ``100 * i_print`` and ``head.tar`` every ``i_weights``.

    loader = "resident": ``dataset.ResidentFrames`` -- the clip on the device, pixels drawn there, draw number
             ``draw_index(global_step, rank, world)``;
    loader = "reference": ``dataset.GetData`` -- upstream's host-side loader and its numpy draw sequence.

    val = "reference": the validation frame comes from ``dataset.GetData(val)`` (``validation_frame``);
    val = "resident":  the validation clip is resident too (``dataset.ResidentFrames(mode="val")``): the same frame index from
             the same generator, rendered from ``ResidentFrames.frame`` without a file read, and scored on the device
             (``ops.frame_scores``) -- ``val/psnr`` and ``val/ssim`` are logged and ``on_log("val_scores", ...)`` is called beside
             the image.  The scores are read at the validation moment only: one host sync every ``100 * i_print`` steps.

    Two departures from upstream, both so that a run resumed from ``head.tar`` continues exactly as the uninterrupted run
    would (with perturb = 0 and the resident loader: bit for bit): ``head.tar`` is written at upstream's moments but records
    the number of COMPLETED steps (upstream records the index of the step just done and so repeats that step after a resume),
    and a resumed run enters its first epoch at frame ``global_step % n_frames`` (upstream restarts the epoch at frame 0 while
    keeping ``global_step``).  ``steps``: stop after that many steps of THIS call (None: run ``N_iters + 1`` epochs).

    ``on_log(kind, global_step, payload)`` receives ("train", step, {loss, psnr, learning_rate, latent_code_loss}) and
    ("val", step, image [3, 2 H, W] RGB: prediction over ground truth) and, with val = "resident", ("val_scores", step,
    {frame, groups, mse, psnr, ssim: one value per ops.SCORE_GROUPS}); ``on_step(global_step, info)`` runs after every step.
    Inside a process group every rank trains (``train_step`` all-reduces the gradients); rank 0 alone logs and saves.

    refine_poses (no counterpart upstream; off: nothing below exists and the run is what it was): the training cameras are
    refined jointly with the model (``pose_refine.PoseRefiner``: one (omega, tau) per training frame, zero at the start).  Each
    step's ray batch goes through the frame's correction before the network sees it, and the render backward returns the
    gradient of the rays.  The deltas are a third parameter set of the same Adam, in a group of their own whose rate is
    ``pose_lrate`` (default 0.1 * lrate: a starting point nobody has tuned) and decays by the same schedule; inside a process
    group the gradient all-reduce covers them.  The checkpoint gains ``pose_deltas`` and a resumed run restores them.  Validation
    frames are rendered from their own poses.

    refine_expr / learn_background (no counterpart upstream either; off: nothing below exists, and the file's keys, the
    optimizer's groups and every launch of the step are what they were): two more inputs of the offline pipeline train with the
    model (``cond_refine``).  refine_expr: one additive correction per training frame on the tracker's expression row
    (``ExprRefiner``, zero at the start), applied to the step's expression before the network sees it; the render backward
    returns d expr.  learn_background: the background image is a parameter (``Background``, initialised from ``bc.jpg`` as
    uint8 / 255, not clamped); the step renders over its pixels at the batch's pixel indices -- which only the resident loader
    hands over (``ResidentFrames.selection``): with loader = "reference" it raises ValueError -- and the render backward
    returns d bc.  Each is a parameter group of the same Adam with a rate of its own that decays by the same schedule and is
    covered by the gradient all-reduce: ``expr_lrate`` (default 0.1 * lrate) and ``bg_lrate`` (default lrate) -- both starting
    points nobody has tuned.  The checkpoint gains ``expr_deltas`` / ``background`` and a resumed run restores them (it
    continues bit for bit under the conditions above as long as no pixel is drawn more than twice in a batch: two addends
    commute).  Validation frames keep their own expressions and are rendered over the learned background.  A model without an
    expression (the AD-NeRF baseline) raises ValueError for refine_expr.  The torso stage has neither option.

    ssim_weight / patches / patch_region (no counterpart upstream, whose image-level terms need external weights; off -- the
    defaults --: the draw, every launch, the checkpoint's keys and every byte of the run are what they were): SSIM, the
    structural score ``val/ssim`` reports, as a training term.  patches = (k, p): every batch carries k contiguous p x p patches
    in its last k p^2 rows (``ResidentFrames(patches=, patch_region=)``: the batch keeps N_rand rows, the patch rays come out of
    the rect region's share; patch_region "rect" or "frame" is where their corners are drawn) -- which only the resident loader
    can do: with loader = "reference" it raises ValueError.  Upstream's terms run over all N_rand rows as before, and the step
    adds ``ssim_weight * ssim_patch_loss(rgb[patch rows], target[patch rows])`` on the FINE image alone (``ssim_loss.py``:
    1 - mean SSIM over the patches, the scorer's index, on the device in fp64).  ssim_weight > 0 needs patches (ValueError);
    patches with ssim_weight = 0 only changes the draw.  ``ssim_weight`` has no tuned default: nobody has measured what it does
    to a trained model.  ``info`` of ``on_step`` and the "train" payload of ``on_log`` gain ``ssim_loss`` (the unweighted term).
    The option composes with the three above, adds no parameter and no checkpoint key, and a resumed run reproduces the patch
    positions: they are a function of (sample_seed, frame, draw index) alone.  The torso stage does not have it.
    -> dict(network, optimizer, latent_codes, global_step, data_size[, pose_refiner][, expr_refiner][, background])."""
    from . import dataset
    return _train_head_model(args, "head", dataset.ResidentFrames, dataset.GetData, lambda epoch: 'head.tar', True, loader=loader,
                             sample_seed=sample_seed, device=device, steps=steps, on_log=on_log, on_step=on_step,
                             max_bytes=max_bytes, val=val, refine_poses=refine_poses, pose_lrate=pose_lrate,
                             refine_expr=refine_expr, expr_lrate=expr_lrate, learn_background=learn_background, bg_lrate=bg_lrate,
                             ssim_weight=ssim_weight, patches=patches, patch_region=patch_region)


def _train_head_model(args, model, resident_cls, reference_cls, checkpoint_name, flip, *, loader, sample_seed, device, steps,
                      on_log, on_step, max_bytes, val, with_codes=True, refine_poses=False, pose_lrate=None, refine_expr=False,
                      expr_lrate=None, learn_background=False, bg_lrate=None, ssim_weight=0.0, patches=None, patch_region="rect"):
    """The body of ``train`` for a head-stage model (``agg_aud_exp_nerf.HEAD_MODELS``): its two loader classes, its checkpoint
    name per epoch, and whether the validation image is channel-flipped (the loader reads BGR).  with_codes=False (the AD-NeRF
    baseline): no per-frame latent codes exist -- Adam runs over the network alone, the step is ``baseline_train_step`` on the
    loaders' 7-tuples, ``ft_path`` is read in full (``checkpoint.load_adnerf``) and the run file is
    ``checkpoint.save_baseline_checkpoint``'s; the returned ``latent_codes`` is None.  refine_poses / pose_lrate, refine_expr / expr_lrate,
    learn_background / bg_lrate, ssim_weight / patches / patch_region: as ``train``."""
    import numpy as np
    from . import checkpoint
    from .agg_aud_exp_nerf import build_head_network
    from .audio_exp_nerf import init_weights
    from .helper import write_config

    if loader not in ("resident", "reference"):
        raise ValueError(f"loader must be 'resident' or 'reference', got {loader!r}")
    if val not in ("reference", "resident"):
        raise ValueError(f"val must be 'reference' or 'resident', got {val!r}")
    # the expression's width: the agg pair's is its own constant (79), the head pair's the flag; the baseline has none
    if model == "agg":
        from .agg_aud_exp_nerf import DIM_EXPR as dim_expr
    else:
        dim_expr = getattr(args, "dim_expr", 0) if with_codes else 0
    if refine_expr and not dim_expr:
        raise ValueError(f"refine_expr: the {model} model takes no expression")
    if learn_background and loader != "resident":
        raise ValueError("learn_background needs the step's pixel indices, which the resident loader alone hands over "
                         "(loader='resident')")
    ssim_weight = float(ssim_weight)
    if ssim_weight < 0:
        raise ValueError(f"ssim_weight must not be negative, got {ssim_weight}")
    if patches is not None:
        from .ssim_loss import PATCH_REGIONS, check_patches
        if loader != "resident":
            raise ValueError("patches are put into the batch by the resident loader alone (loader='resident')")
        patches = check_patches(patches)
        if patch_region not in PATCH_REGIONS:
            raise ValueError(f"patch_region must be one of {PATCH_REGIONS}, got {patch_region!r}")
    elif ssim_weight > 0:
        raise ValueError("ssim_weight > 0 needs patches=(k, p): SSIM is a statistic of 11 x 11 windows, which scattered pixels "
                         "cannot carry")
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
    rank, world = (torch.distributed.get_rank(), torch.distributed.get_world_size()) if dist_on else (0, 1)
    basedir, expname = args.basedir, args.expname
    run_dir = os.path.join(basedir, expname)

    if loader == "resident":
        patch_kw = {} if patches is None else dict(patches=patches, patch_region=patch_region)
        dataset_train = resident_cls(args.datadir, args.aud_file, "train", args, device=device, max_bytes=max_bytes,
                                     seed=sample_seed, **patch_kw)
    else:
        dataset_train = reference_cls(args.datadir, args.aud_file, mode="train", args=args, device=device)
    dataset_val = reference_cls(args.datadir, args.aud_file, mode="val", args=args, skip=args.testskip, device=device)
    logger.info(f'dataset_val length: {dataset_val.data_size}')
    frames_val = None
    if val == "resident" and rank == 0:
        frames_val = resident_cls(args.datadir, args.aud_file, "val", args, skip=args.testskip, device=device,
                                  max_bytes=max_bytes, seed=sample_seed)
    data_size = dataset_train.data_size
    H, W, focal = dataset_val.H, dataset_val.W, dataset_val.focal
    intrinsic = np.array([[focal, 0., W / 2], [0, focal, H / 2], [0, 0, 1.]])
    if rank == 0:
        write_config(args)

    network = build_head_network(args, H, W, focal, model, intrinsic).to(device)
    latent_codes = torch.ones(data_size, 32, dtype=torch.float32, device=device) if with_codes else None
    network.apply(init_weights)
    if with_codes:
        latent_codes.requires_grad = True
        optimizer = make_optimizer(network, latent_codes, args.lrate)
    else:   # head_baseline.py:460
        optimizer = torch.optim.Adam(list(network.parameters()), lr=args.lrate, betas=(0.9, 0.999))
    refiner = None
    if refine_poses:
        from .pose_refine import PoseRefiner
        refiner = PoseRefiner(data_size).to(device)
        pose_lrate = 0.1 * args.lrate if pose_lrate is None else float(pose_lrate)
        optimizer.add_param_group({'params': [refiner.deltas], 'lr': pose_lrate, 'lr_scale': pose_lrate / args.lrate})

    expr_refiner = background = None
    if refine_expr:
        from .cond_refine import ExprRefiner
        expr_refiner = ExprRefiner(data_size, dim_expr).to(device)
        expr_lrate = 0.1 * args.lrate if expr_lrate is None else float(expr_lrate)
        optimizer.add_param_group({'params': [expr_refiner.deltas], 'lr': expr_lrate, 'lr_scale': expr_lrate / args.lrate})
    if learn_background:
        from .cond_refine import Background
        background = Background(dataset_train.background).to(device)
        bg_lrate = args.lrate if bg_lrate is None else float(bg_lrate)
        optimizer.add_param_group({'params': [background.image], 'lr': bg_lrate, 'lr_scale': bg_lrate / args.lrate})

    global_step = 0
    if args.ft_path is not None and args.ft_path != 'None':
        logger.info(f'Found ckpts:{[args.ft_path]}')
        (checkpoint.load_adnerf_finetune if with_codes else checkpoint.load_adnerf)(args.ft_path, network, map_location=device)
    else:
        ckpt_path = checkpoint.latest_checkpoint(run_dir)
        if ckpt_path is not None:
            logger.info(f'Found ckpts:{ckpt_path}')
            if with_codes:
                global_step, saved_codes = checkpoint.load_checkpoint(ckpt_path, network, optimizer, map_location=device)
                latent_codes.data = saved_codes.to(device)
            else:
                global_step = checkpoint.load_baseline_checkpoint(ckpt_path, network, optimizer, map_location=device)
            if refiner is not None:
                refiner.deltas.data.copy_(checkpoint.load_pose_deltas(ckpt_path, map_location=device))
            if expr_refiner is not None:
                expr_refiner.deltas.data.copy_(checkpoint.load_expr_deltas(ckpt_path, map_location=device))
            if background is not None:
                background.image.data.copy_(checkpoint.load_background(ckpt_path, map_location=device))

    network.train()

    def validate(step):
        bg = None if background is None else background().detach()   # a validation frame stands before the learned background
        if frames_val is None:
            return validation_frame(network, dataset_val, latent_codes, step, sample_seed, flip=flip, background=bg), None
        return resident_validation_frame(network, frames_val, latent_codes, step, sample_seed, flip=flip, background=bg)

    # the SSIM term of a step: its weight and where the loader has put the patches (off: the steps are called as they were)
    ssim_kw = {} if not ssim_weight > 0 else dict(ssim=(ssim_weight, dataset_train.patch_rows(), *patches))
    if with_codes:
        step_fn = lambda data, step: train_step(network, optimizer, data, latent_codes, step, data_size, lrate=args.lrate,
                                                lrate_decay=args.lrate_decay, **ssim_kw)
        scalars_of = lambda info: dict(loss=info["loss"].item(), psnr=info["psnr"].item(), learning_rate=info["lr"],
                                       latent_code_loss=info["latent_code_loss"].item())
        log_line = lambda sc: f"LatentLoss: {sc['latent_code_loss']}  PSNR: {sc['psnr']} LR: {sc['learning_rate']}"
        save = checkpoint.save_checkpoint
    else:
        step_fn = lambda data, step: baseline_train_step(network, optimizer, data, step, data_size, lrate=args.lrate,
                                                         lrate_decay=args.lrate_decay, **ssim_kw)
        scalars_of = lambda info: dict(loss=info["loss"].item(), psnr=info["psnr"].item(), learning_rate=info["lr"])
        log_line = lambda sc: f"Loss: {sc['loss']}  PSNR: {sc['psnr']} LR: {sc['learning_rate']}"
        save = lambda path, net, opt, codes, step: checkpoint.save_baseline_checkpoint(path, net, opt, step)
    if ssim_kw:
        plain_scalars, plain_line = scalars_of, log_line
        scalars_of = lambda info: dict(plain_scalars(info), ssim_loss=info["ssim_loss"].item())
        log_line = lambda sc: f"{plain_line(sc)} SSIMLoss: {sc['ssim_loss']}"
    if refiner is not None:
        # the frame's correction on the step's ray batch (the tuples begin with batch_rays and end with the frame index), and
        # the deltas beside everything else in the checkpoint
        plain_step = step_fn
        step_fn = lambda data, step: plain_step((refiner(int(data[-1]), data[0]), *data[1:]), step)
    if expr_refiner is not None:   # (the tuples with an expression end in expr, index)
        pose_step = step_fn
        step_fn = lambda data, step: pose_step((*data[:-2], expr_refiner(int(data[-1]), data[-2]), data[-1]), step)
    if background is not None:
        # bc_rgb is the third field of every head-stage tuple: the parameter's pixels at the indices the loader has just drawn
        # (its buffer holds them until the next draw: past this step's backward) in place of the rows it gathered from bc.jpg
        expr_step = step_fn
        step_fn = lambda data, step: expr_step((*data[:2], background.rows(dataset_train.selection()), *data[3:]), step)
    if refiner is not None or expr_refiner is not None or background is not None:
        extras = dict(pose_deltas=None if refiner is None else refiner.deltas)
        if background is not None:
            extras["background"] = background.image
        if with_codes:
            if expr_refiner is not None:
                extras["expr_deltas"] = expr_refiner.deltas
            save = lambda path, net, opt, codes, step: checkpoint.save_checkpoint(path, net, opt, codes, step, **extras)
        else:
            save = lambda path, net, opt, codes, step: checkpoint.save_baseline_checkpoint(path, net, opt, step, **extras)
    global_step = _run_epochs(
        args, network, optimizer, latent_codes, data_size, global_step, steps, rank, on_log, on_step,
        batch=lambda it, step: (dataset_train.batch(it, draw_index(step, rank, world)) if loader == "resident"
                                else _as_loader_item(dataset_train[it], with_codes)),
        step_fn=step_fn, scalars_of=scalars_of, log_line=log_line, validate=validate, checkpoint_name=checkpoint_name, save=save)
    out = dict(network=network, optimizer=optimizer, latent_codes=latent_codes, global_step=global_step, data_size=data_size)
    if refiner is not None:
        out["pose_refiner"] = refiner
    if expr_refiner is not None:
        out["expr_refiner"] = expr_refiner
    if background is not None:
        out["background"] = background
    return out


def _run_epochs(args, network, optimizer, latent_codes, data_size, global_step, steps, rank, on_log, on_step, *, batch, step_fn,
                scalars_of, log_line, validate, checkpoint_name, save=None):
    """The skeleton both stages' ``train`` share (audio_exp_nerf.py:527-593, train_torso.py:509-574): epochs over the frames
    in order from ``global_step`` on, and per step ``step_fn(batch(it, global_step), global_step)``, the log line every
    ``i_print`` steps, ``validate(global_step) -> (image, scores or None)`` every ``100 * i_print`` and the checkpoint
    ``checkpoint_name(epoch)`` every ``i_weights`` -- recording the COMPLETED steps (through ``save(path, network, optimizer,
    latent_codes, steps)``, default ``checkpoint.save_checkpoint``); a resumed run enters its first epoch at
    frame ``global_step % data_size``.  Rank 0 alone logs, validates and saves.  -> the global step reached."""
    from . import checkpoint
    run_dir = os.path.join(args.basedir, args.expname)
    N_iters = args.N_iters + 1
    writer = _summary_writer(run_dir) if rank == 0 else None
    start = int(global_step / data_size)
    logger.info(f"start: {start}, global_step:{global_step}")
    done = 0
    try:
        for epoch in range(start, N_iters):
            for it in range(global_step % data_size if epoch == start else 0, data_size):
                if steps is not None and done >= steps:
                    break
                info = step_fn(batch(it, global_step), global_step)

                if global_step % args.i_print == 0 and rank == 0:
                    scalars = scalars_of(info)
                    logger.info(f"[TRAIN] epoch: {epoch} Iter: {it} {log_line(scalars)}")
                    for k, v in scalars.items():
                        if writer is not None:
                            writer.add_scalar('train/' + k, v, global_step=global_step)
                    if on_log is not None:
                        on_log("train", global_step, scalars)

                if global_step % (100 * args.i_print) == 0 and rank == 0:
                    image, scores = validate(global_step)
                    if writer is not None:
                        writer.add_image("val/rgb_fine", image, global_step=global_step)
                        if scores is not None:
                            writer.add_scalar("val/psnr", scores["psnr"][0], global_step=global_step)
                            writer.add_scalar("val/ssim", scores["ssim"][0], global_step=global_step)
                    if on_log is not None:
                        on_log("val", global_step, image)
                        if scores is not None:
                            on_log("val_scores", global_step, scores)
                    logger.info('Saved test set and turn back to trainning mode')

                if global_step % args.i_weights == 0 and rank == 0:
                    path = os.path.join(run_dir, checkpoint_name(epoch))
                    (save or checkpoint.save_checkpoint)(path, network, optimizer, latent_codes, global_step + 1)
                    logger.info(f'Saved checkpoints at {path} and start to test with network')
                global_step += 1
                done += 1
                if on_step is not None:
                    on_step(global_step, info)
            if steps is not None and done >= steps:
                break
    finally:
        if writer is not None:
            writer.close()
    return global_step


def _validation_index(n, global_step, sample_seed):
    gen = torch.Generator().manual_seed((int(sample_seed) * 1000003 + int(global_step)) & (2 ** 63 - 1))
    return int(torch.randint(n, (1,), generator=gen))


def validation_frame(network, dataset_val, latent_codes, global_step, sample_seed=0, flip=True, background=None):
    """audio_exp_nerf.py:568-581: one randomly chosen validation frame rendered in eval mode under no_grad with
    ``latent_codes[0]``, stacked over its ground truth, channels flipped to RGB -> [3, 2 H, W] on the host; the network
    goes back to train mode.  The frame is chosen by a generator of its own seeded from (sample_seed, global_step) --
    upstream shuffles its validation loader -- so a validation neither depends on nor disturbs the training draws.
    Either stage's loader and network: the item ends in (raw_img, pose, expr, index) and the forward's first output is the
    frame; flip=False for the torso stage, whose images are RGB already (train_torso.py:558-560)."""
    val_i = _validation_index(len(dataset_val), global_step, sample_seed)
    network.eval()
    try:
        item = _over_background(_as_loader_item(dataset_val[val_i], latent_codes is not None), background)
        with torch.no_grad():
            rgb = network([_eval_tuple(item, latent_codes), global_step, dataset_val.data_size])[0]
    finally:
        network.train()
    return _pred_over_label(rgb, _raw_img(item, latent_codes), flip)


def _over_background(item, background):
    """A head-stage loader's eval item with ``background`` [H, W, 3] (a learned one: ``train(learn_background=True)``) in its
    bg_img field, the third; None: the item as it is."""
    return item if background is None else (*item[:2], background, *item[3:])


def _eval_tuple(item, latent_codes):
    """A loader's item as the eval forward takes it: latent code row 0 before the index (audio_exp_nerf.py:571) -- or the item
    as it is for a model without latent codes (latent_codes None: the baseline's 7-tuple)."""
    return item if latent_codes is None else (*item[:-1], latent_codes[0], item[-1])


def _raw_img(item, latent_codes):
    return item[-3] if latent_codes is None else item[-4]


def _pred_over_label(rgb, raw_img, flip):
    pred_with_label = torch.cat((rgb.cpu().permute(2, 0, 1), raw_img.cpu().permute(2, 0, 1) / 255.0), dim=1)
    return pred_with_label[[2, 1, 0], :, :] if flip else pred_with_label


def resident_validation_frame(network, frames_val, latent_codes, global_step, sample_seed=0, flip=True, background=None):
    """``validation_frame`` from a resident validation clip (``dataset.ResidentFrames(mode="val")``, or the torso stage's): the
    same frame index from the same generator, the frame's inputs from ``frames_val.frame`` (no file read, no host meshgrid), and
    the render scored on the device against the frame's ground truth, whole frame and per sampling region
    (``ops.frame_scores``) -> (image as ``validation_frame``, dict(frame, groups, mse, psnr, ssim) with one float per
    ``ops.SCORE_GROUPS``; nan where a group has no pixel or window).  The scores are read back here, together with the image:
    the validation moment's one host sync."""
    from . import ops
    val_i = _validation_index(len(frames_val), global_step, sample_seed)
    network.eval()
    try:
        data = _over_background(frames_val.frame(val_i), background)
        with torch.no_grad():
            rgb = network([_eval_tuple(data, latent_codes), global_step, frames_val.data_size])[0]
            table = ops.frame_scores(rgb, frames_val.imgs[val_i], frames_val.maps[val_i])
    finally:
        network.train()
    scores = {k: [float(x) for x in v] for k, v in ops.summarise_scores(table).items()}
    return _pred_over_label(rgb, _raw_img(data, latent_codes), flip), dict(scores, frame=val_i, groups=list(ops.SCORE_GROUPS))
