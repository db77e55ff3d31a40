"""The AD-NeRF baseline's trainer: ``train()`` of NeRFs/HeadNeRF/train/head_baseline.py (:410-522) on this project's loop
(``train._run_epochs``) and step (``train.baseline_train_step``: mse(rgb) + mse(rgb0), :475-481).
"""
from . import train as T


def checkpoint_name(epoch):
    """head_baseline.py:516."""
    return '{:06d}_head.tar'.format(epoch)


def train(args, *, loader="resident", sample_seed=0, device="cuda", steps=None, on_log=None, on_step=None, max_bytes=8 << 30,
          val="reference", refine_poses=False, pose_lrate=None, refine_expr=False, expr_lrate=None, learn_background=False,
          bg_lrate=None, ssim_weight=0.0, patches=None, patch_region="rect"):
    """The reference's baseline ``train()`` on the flags ``args`` (``helper.config_parser().parse_args()``): write_config, the
    datasets, ``head_baseline.Network`` + ``init_weights``, Adam over ``network.parameters()`` alone -- there are no latent
    codes --, the whole AD-NeRF checkpoint of ``ft_path`` (``checkpoint.load_adnerf``: all four dicts, strict) or a resume from
    the newest ``*.tar`` of ``basedir/expname``, then ``train.train``'s loop with ``{epoch:06d}_head.tar`` =
    {global_step, model_state_dict, optimizer} every ``i_weights`` (``checkpoint.save_baseline_checkpoint``: upstream's
    ``module.``-prefixed keys) and a validation image that is NOT channel-flipped: this trainer's loader reads RGB (:88), so
    prediction over ground truth is RGB over RGB.  The learning rate is ``train.decayed_lr``'s (:487-489).

    loader = "resident": ``dataset.ResidentBaselineFrames``; "reference": ``dataset.BaselineGetData`` (upstream's numpy draw
    sequence).  val, steps, sample_seed, on_log (its "train" payload is {loss, psnr, learning_rate}), on_step, max_bytes, the
    process-group behaviour and the two departures from upstream (the checkpoint records COMPLETED steps; a resumed run enters
    its epoch at ``global_step % n_frames``): as ``train.train``; so are
    refine_poses / pose_lrate (joint refinement of the training cameras) and learn_background / bg_lrate (the background as
    a parameter).  refine_expr raises ValueError: this model has no expression.
    ssim_weight / patches / patch_region (an SSIM term on patches that ride in the batch): as ``train.train``.
    -> dict(network, optimizer, latent_codes=None, global_step, data_size)."""
    from . import dataset
    return T._train_head_model(args, "baseline", dataset.ResidentBaselineFrames, dataset.BaselineGetData, checkpoint_name, False,
                               loader=loader, sample_seed=sample_seed, device=device, steps=steps, on_log=on_log, on_step=on_step,
                               max_bytes=max_bytes, val=val, with_codes=False, refine_poses=refine_poses,
                               pose_lrate=pose_lrate, refine_expr=refine_expr, expr_lrate=expr_lrate,
                               learn_background=learn_background, bg_lrate=bg_lrate, ssim_weight=ssim_weight,
                               patches=patches, patch_region=patch_region)
