"""Drop-in for the head + torso renderer ``NeRFs/TorsoNeRF/train_torso.py::Network``
(:198-271; BASELINE config 5): two pairs of FaceNeRFs rendered on their own ray sets and
composited as ``rgb_com = rgb_head * last_weight_torso + rgb_fg_torso`` (:269-270).

The head pair is conditioned on (audio, expression, latent); the torso pair on
``[aud[:dim_aud_body] | PE_3(euler) | PE_3(translation)]`` of the head pose (:238-240) with
no expression / latent code.  Both pairs run the same HIP kernels: the conditioning
widths only enter the folded biases.
"""
import torch
import torch.nn as nn

from .audio_exp_nerf import Network as HeadNetwork
from .helper import RenderConfig, get_embedder, input_channels
from .models.audio_net import AudioAttNet, AudioNet
from .models.face_nerf import FaceNeRF


def config_parser():
    """NeRFs/TorsoNeRF/run_nerf_helpers.py:231-365 (`from run_nerf_helpers import *` puts it into train_torso's namespace)."""
    from .config import ConfigParser
    return ConfigParser("torso")


def pose_to_euler_trans(poses):
    """[b, >=3, 4] -> [b, 6] (euler angles, translation)  (run_nerf_helpers.py:26-47)."""
    R = poses[:, :3, :3]
    e = torch.stack([torch.atan2(R[:, 2, 2], R[:, 1, 2]), torch.asin(-R[:, 0, 2]),
                     torch.atan2(R[:, 0, 0], -R[:, 0, 1])], dim=1)
    return torch.cat((e, poses[:, :3, 3]), dim=1)


class Network(HeadNetwork):
    def __init__(self, H, W, focal, near, far, chunk, N_samlpes, N_importance, args: RenderConfig = None,
                 dim_aud_body=None, dim_expr_head=79):
        """The reference's positional arguments (train_torso.py:185: no `intrinsic`, unlike the head-only Network).
        Without `args=` the flags are the process's TorsoNeRF flags (run_nerf_helpers.py:231-365: `dim_aud`,
        `dim_aud_body`, ...), as upstream's class reads them from its `args` global (train_torso.py:200-221)."""
        nn.Module.__init__(self)
        from . import config
        if args is None:
            args = config.default_render_config("torso")
            args.dim_expr = dim_expr_head
            ns = config.current_args("torso")
            if dim_aud_body is None and ns is not None:
                dim_aud_body = ns.dim_aud_body
        else:
            config.check_against_current(args, "torso")
        dim_aud_body = 64 if dim_aud_body is None else dim_aud_body
        self.args = args
        self.H, self.W, self.focal, self.near, self.far = H, W, focal, near, far
        self.chunk, self.intrinsic = chunk, None
        self.N_samples, self.N_importance = N_samlpes, N_importance
        self.output_ch, self.skips = 4, [4]
        self.dim_aud_body = dim_aud_body
        self.embed_torso_aud_fn, ch = get_embedder(3, 0)  # 21 per 3-vector (:38)
        input_ch, input_ch_views = input_channels(args)   # all four networks: train_torso.py:36-37,200-221
        head = lambda: FaceNeRF(D=args.netdepth, W=args.netwidth, input_ch=input_ch, dim_aud=args.dim_aud, skips=self.skips,
                                dim_latent=32, dim_expr=dim_expr_head, input_ch_views=input_ch_views)
        torso = lambda: FaceNeRF(D=args.netdepth, W=args.netwidth, input_ch=input_ch, dim_aud=dim_aud_body + 2 * ch,
                                 skips=self.skips, input_ch_views=input_ch_views)
        self.face_nerf_coarse, self.face_nerf_fine = head(), head()
        self.aud_net = AudioNet(args.dim_aud, args.win_size)
        self.aud_att_net = AudioAttNet()
        self.torso_coarse_nerf, self.torso_fine_nerf = torso(), torso()

    def torso_signal(self, aud_feature, pose):
        et = pose_to_euler_trans(pose.unsqueeze(0))
        emb = torch.cat((self.embed_torso_aud_fn(et[:, :3]), self.embed_torso_aud_fn(et[:, 3:])), dim=1)
        return torch.cat((aud_feature[..., :self.dim_aud_body], torch.squeeze(emb)), dim=-1)

    def forward(self, inputs):
        """-> (rgb_com, rgb_com0)   (train_torso.py:223-271)."""
        x, global_step, dataset_size = inputs
        batch_rays, batch_rays_torso, target_s, bg_img, auds, raw_img, pose, expr, latent_code, index = x
        dev = self.face_nerf_coarse.alpha_linear.weight.device
        sq = lambda t: torch.squeeze(t).to(device=dev, dtype=torch.float32)
        batch_rays, batch_rays_torso, bg_img, auds, pose, expr = (sq(batch_rays), sq(batch_rays_torso), sq(bg_img),
                                                                    sq(auds), sq(pose), sq(expr))
        latent_code = torch.squeeze(latent_code).to(dev)
        aud_window = auds[int(index)]
        aud_feature = self.aud_net(aud_window.unsqueeze(0) if aud_window.dim() == 2 else aud_window)
        aud_torso = self.torso_signal(aud_feature, pose)
        render_poses = None if self.training is True else pose[:3, :4]
        kw = dict(H=self.H, W=self.W, focal=self.focal, render_poses=render_poses, chunk=self.args.chunk,
                  near=self.near, far=self.far, bc_rgb=bg_img)
        rgb, _, _, last_w, rgb_fg, extras = self.render_pair(
            expr=expr, latent_code=latent_code, rays=batch_rays, aud_para=aud_feature,
            network_nerf={'coarse': self.face_nerf_coarse, 'fine': self.face_nerf_fine}, **kw)
        _, _, _, last_w_t, rgb_fg_t, extras_t = self.render_pair(
            expr=None, latent_code=None, rays=batch_rays_torso, aud_para=aud_torso,
            network_nerf={'coarse': self.torso_coarse_nerf, 'fine': self.torso_fine_nerf}, **kw)
        rgb_com = rgb * last_w_t[..., None] + rgb_fg_t
        rgb_com0 = extras['rgb0'] * extras_t['last_weight0'][..., None] + extras_t['rgb_map_fg0']
        return rgb_com, rgb_com0

    def render_pair(self, H, W, focal, expr, latent_code, render_poses=None, chunk=1024 * 32, near=0., far=1.,
                    rays=None, bc_rgb=None, aud_para=None, network_nerf=None, rows=None):
        """train_torso.py::render_dynamic_face (:381-426): [rgb_map, disp_map, acc_map, last_weight,
        rgb_map_fg, {rest}] for one coarse/fine pair."""
        coarse, fine = network_nerf['coarse'], network_nerf['fine']
        rec, frame, bc, sh = self._ray_inputs(H, W, focal, near, far, render_poses, rays, bc_rgb, rows)
        all_ret = self._batchify(rec, bc, aud_para, latent_code, expr, coarse, fine, True, chunk, frame=frame)
        for k in all_ret:
            all_ret[k] = torch.reshape(all_ret[k], list(sh[:-1]) + list(all_ret[k].shape[1:]))
        k_extract = ['rgb_map', 'disp_map', 'acc_map', 'last_weight', 'rgb_map_fg']
        return [all_ret[k] for k in k_extract] + [{k: v for k, v in all_ret.items() if k not in k_extract}]


def load_stage_checkpoints(run_dir, network, optimizer=None, device=None):
    """How the torso stage finds its weights (train_torso.py:489-499): the newest ``*head.tar*`` of ``run_dir`` with
    strict=False (the head pair and the audio nets), then the newest ``*torso.tar*`` strictly, with the optimiser state where
    an ``optimizer`` is given.  -> (the torso checkpoint's step, else 0; the latent codes of the last file loaded, else None).
    What ``train`` resumes from and what ``drive.drive_torso`` renders with."""
    import logging
    from . import checkpoint
    log = logging.getLogger("adnerf")
    global_step, codes = 0, None
    head_path = checkpoint.latest_checkpoint(run_dir, contains="head.tar")
    if head_path is not None:
        log.info(f'Found ckpts:{head_path}')
        _, codes = checkpoint.load_checkpoint(head_path, network, map_location=device, strict=False)
    torso_path = checkpoint.latest_checkpoint(run_dir, contains="torso.tar")
    if torso_path is not None:
        log.info(f'Found ckpts:{torso_path}')
        global_step, codes = checkpoint.load_checkpoint(torso_path, network, optimizer, map_location=device)
    return global_step, codes


def train(args, *, loader="resident", sample_seed=0, device="cuda", steps=None, on_log=None, on_step=None, max_bytes=8 << 30,
          val="reference"):
    """The reference's torso-stage ``train()`` (NeRFs/TorsoNeRF/train_torso.py:443-574) on the flags ``args``
    (``config_parser().parse_args()``): write_config, the datasets, ``Network`` + ``init_weights`` (the head pair's expression
    width is the length of the clip's ``exp`` vectors: upstream's literal 79 on upstream's data), ``latent_codes = ones[n, 32]``
    (saved, not optimised), Adam over the torso pair and the two audio nets only, the newest ``*head.tar*`` of
    ``basedir/expname`` with strict=False (and its latent codes), then the newest ``*torso.tar*`` strictly (latent codes, step,
    optimiser state), and ``train.train``'s loop: a log line every ``i_print`` steps, one validation frame every
    ``100 * i_print`` (rendered by ``Network.forward`` in eval mode -- the torso pair at the frame's own pose, as upstream --
    and stacked over its truth without a channel flip: the torso loader's images are RGB) and ``{epoch:06d}_torso.tar`` every
    ``i_weights``.

    The head pair is in eval mode and its parameters do not require gradients: its backward is the conditioning-only plan
    (``autograd.RenderRaysFn.backward``), and its weights leave training bit for bit as they entered.

    loader / val / steps / sample_seed / on_log / on_step / max_bytes and the two departures from upstream (the checkpoint
    records COMPLETED steps; a resumed run enters its epoch at ``global_step % n_frames``): as ``train.train`` -- with
    ``dataset.ResidentTorsoFrames`` and ``dataset.TorsoGetData`` as the two loaders.  ``on_log("train", ...)`` carries
    {loss, psnr, learning_rate}.  -> dict(network, optimizer, latent_codes, global_step, data_size)."""
    import os
    from . import dataset, train as T
    from .audio_exp_nerf import init_weights
    from .config import to_render_config
    from .helper import write_config

    if loader not in ("resident", "reference"):
        raise ValueError(f"loader must be 'resident' or 'reference', got {loader!r}")
    if val not in ("reference", "resident"):
        raise ValueError(f"val must be 'reference' or 'resident', got {val!r}")
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
    rank, world = (torch.distributed.get_rank(), torch.distributed.get_world_size()) if dist_on else (0, 1)
    run_dir = os.path.join(args.basedir, args.expname)

    if loader == "resident":
        dataset_train = dataset.ResidentTorsoFrames(args.datadir, args.aud_file, "train", args, device=device, max_bytes=max_bytes,
                                                    seed=sample_seed)
    else:
        dataset_train = dataset.TorsoGetData(args.datadir, args.aud_file, mode="train", args=args, device=device)
    dataset_val = dataset.TorsoGetData(args.datadir, args.aud_file, mode="val", args=args, skip=args.testskip, device=device)
    T.logger.info(f'dataset_val length: {dataset_val.data_size}')
    frames_val = None
    if val == "resident" and rank == 0:
        frames_val = dataset.ResidentTorsoFrames(args.datadir, args.aud_file, "val", args, skip=args.testskip, device=device,
                                                 max_bytes=max_bytes, seed=sample_seed)
    data_size = dataset_train.data_size
    if rank == 0:
        write_config(args)

    cfg = to_render_config(args)
    cfg.dim_expr = len(dataset_val.all_exprs[0])
    network = Network(dataset_val.H, dataset_val.W, dataset_val.focal, near=args.near, far=args.far, chunk=args.chunk,
                      N_samlpes=args.N_samples, N_importance=args.N_importance, args=cfg, dim_aud_body=args.dim_aud_body,
                      dim_expr_head=cfg.dim_expr).to(device)
    latent_codes = torch.ones(data_size, 32, dtype=torch.float32, device=device)
    network.apply(init_weights)
    trained = [p for m in (network.torso_coarse_nerf, network.torso_fine_nerf, network.aud_net, network.aud_att_net)
               for p in m.parameters()]
    optimizer = torch.optim.Adam(params=trained, lr=args.lrate, betas=(0.9, 0.999))

    global_step = 0
    if args.ft_path is None or args.ft_path == 'None':
        global_step, saved_codes = load_stage_checkpoints(run_dir, network, optimizer, device)
        if saved_codes is not None:
            latent_codes.data = saved_codes.to(device)

    network.train()
    for m in (network.face_nerf_coarse, network.face_nerf_fine):   # frozen in this stage (train_torso.py:476-479, 512-513)
        m.requires_grad_(False)
        m.eval()                                                   # (as upstream, until the first validation's network.train())

    def validate(step):
        if frames_val is None:
            return T.validation_frame(network, dataset_val, latent_codes, step, sample_seed, flip=False), None
        return T.resident_validation_frame(network, frames_val, latent_codes, step, sample_seed, flip=False)

    global_step = T._run_epochs(
        args, network, optimizer, latent_codes, data_size, global_step, steps, rank, on_log, on_step,
        batch=lambda it, step: (dataset_train.batch(it, T.draw_index(step, rank, world)) if loader == "resident"
                                else T._as_loader_item(dataset_train[it])),
        step_fn=lambda data, step: T.torso_train_step(network, optimizer, data, latent_codes, step, data_size, lrate=args.lrate,
                                                      lrate_decay=args.lrate_decay),
        scalars_of=lambda info: dict(loss=info["loss"].item(), psnr=info["psnr"].item(), learning_rate=info["lr"]),
        log_line=lambda sc: f" PSNR: {sc['psnr']} LR: {sc['learning_rate']}",
        validate=validate, checkpoint_name=lambda epoch: '{:06d}_torso.tar'.format(epoch))
    return dict(network=network, optimizer=optimizer, latent_codes=latent_codes, global_step=global_step, data_size=data_size)
