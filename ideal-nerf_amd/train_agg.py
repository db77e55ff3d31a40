"""The feature-aggregation trainer: ``train()`` of NeRFs/HeadNeRF/train/agg_aud_exp_nerf.py (:415-554) on this project's loop
(``train._run_epochs``) and step (``train.train_step``: the loss is the head stage's, :507-518).
"""
from . import train as T


def checkpoint_name(epoch):
    """agg_aud_exp_nerf.py:548."""
    return '{:06d}_head.tar'.format(epoch)


def train(args, *, loader="resident", sample_seed=0, device="cuda", steps=None, on_log=None, on_step=None, max_bytes=8 << 30,
          val="reference", refine_poses=False, pose_lrate=None, refine_expr=False, expr_lrate=None, learn_background=False,
          bg_lrate=None, ssim_weight=0.0, patches=None, patch_region="rect"):
    """The reference's agg ``train()`` on the flags ``args`` (``helper.config_parser().parse_args()``; the loaders also read
    ``use_highlight``): write_config, the datasets, ``agg_aud_exp_nerf.Network`` + ``init_weights``,
    ``latent_codes = ones[n_frames, 32]``, Adam over the network (both ``agg_linears`` and the audio nets included) and the
    latent codes, warm start from ``ft_path`` or resume from the newest ``*.tar`` of ``basedir/expname``, then ``train.train``'s
    loop with ``{epoch:06d}_head.tar`` every ``i_weights`` and a validation image that is NOT channel-flipped: this trainer's
    loader reads RGB (:90), so prediction over ground truth is RGB over RGB.

    loader = "resident": ``dataset.ResidentAggFrames``; "reference": ``dataset.AggGetData`` (upstream's numpy draw sequence).
    val, steps, sample_seed, on_log, on_step, max_bytes, the process-group behaviour and the two departures from upstream (the
    checkpoint records COMPLETED steps; a resumed run enters its epoch at ``global_step % n_frames``): as ``train.train``; so are
    refine_poses / pose_lrate (joint refinement of the training cameras) and refine_expr / expr_lrate, learn_background /
    bg_lrate (the expressions and the background as parameters; the expression's gradient reaches its deltas through
    ``agg_linears`` in torch: the kernels of this model see no expression).
    ssim_weight / patches / patch_region (an SSIM term on patches that ride in the batch): as ``train.train``.
    -> dict(network, optimizer, latent_codes, global_step, data_size)."""
    from . import dataset
    return T._train_head_model(args, "agg", dataset.ResidentAggFrames, dataset.AggGetData, checkpoint_name, False, loader=loader,
                               sample_seed=sample_seed, device=device, steps=steps, on_log=on_log, on_step=on_step,
                               max_bytes=max_bytes, val=val, refine_poses=refine_poses,
                               pose_lrate=pose_lrate, refine_expr=refine_expr, expr_lrate=expr_lrate,
                               learn_background=learn_background, bg_lrate=bg_lrate, ssim_weight=ssim_weight,
                               patches=patches, patch_region=patch_region)
