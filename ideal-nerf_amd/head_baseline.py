"""Drop-in for the AD-NeRF baseline renderer ``NeRFs/HeadNeRF/train/head_baseline.py::Network`` (:171-398; the tester
``test/test_nerf.py`` imports the same class).

The head ``Network`` conditioned on the audio alone: the pair is ``FaceNeRF(dim_aud, dim_latent=0, dim_expr=0)`` (:186-194,
C = 63 + 64 = 127), the submodules are ``face_nerf_coarse``, ``face_nerf_fine``, ``aud_net`` and ``aud_att_net`` -- no
DeepSpeech squeeze, so a state dict carries upstream's keys and nothing else --, the audio branch is the smoothed window from
``nosmo_iters`` on and ``aud_net(auds[index])`` before it with no ``dim_aud`` condition (:211-235), and ``forward`` takes
upstream's 7-tuple (batch_rays, target_s, bg_img, auds, raw_img, pose, index).  The render methods have upstream's
signatures of THIS class, which name neither an expression nor a latent code; each delegates to the head renderer's body with
``expr = latent_code = None``: eval is one C call per frame, the precision handling and the packed-weight cache are
inherited, and training goes through ``autograd.RenderRaysFn`` unchanged (no latent gradient is ever asked for).
"""
import torch

from .audio_exp_nerf import Network as HeadNetwork, init_weights  # noqa: F401  (init_weights: the trainer applies it)
from .helper import input_channels
from .models.face_nerf import FaceNeRF


def config_parser():
    """The head stage's parser: head_baseline.py:26 takes ``helper.config_parser()``."""
    from .config import ConfigParser
    return ConfigParser("head")


class Network(HeadNetwork):
    config_kind = "head"
    deepspeech_net = False

    def make_nerf(self):
        args = self.args
        input_ch, input_ch_views = input_channels(args)   # head_baseline.py:37-38
        return FaceNeRF(D=args.netdepth, W=args.netwidth, input_ch=input_ch, dim_aud=args.dim_aud, dim_latent=0, dim_expr=0,
                        output_ch=4, skips=self.skips, input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs)

    def audio_feature(self, auds, index, global_step, dataset_size):
        if global_step >= self.args.nosmo_iters:
            return self.smoothed_audio_feature(auds, index, dataset_size)
        return self.aud_net(auds[index].unsqueeze(0) if auds[index].dim() == 2 else auds[index])

    def expr_feature(self, expr):
        return None

    # ---- forward: head_baseline.py:198-242 ------------------------------------------
    def forward(self, inputs):
        args = self.args
        x, global_step, dataset_size = inputs
        batch_rays, target_s, bg_img, auds, raw_img, pose, index = x
        dev = self.face_nerf_coarse.alpha_linear.weight.device
        sq = lambda t: torch.squeeze(t).to(device=dev, dtype=torch.float32)
        # the camera of a full-frame render travels as kernel arguments: keep the loader's host copy (audio_exp_nerf.Network.forward)
        pose_host = None if self.training is True else torch.squeeze(pose).detach().to(device="cpu", dtype=torch.float32)
        batch_rays, bg_img, auds, pose = sq(batch_rays), sq(bg_img), sq(auds), sq(pose)
        aud_feature = self.audio_feature(auds, int(index), global_step, dataset_size)
        render_poses = None if pose_host is None else pose_host[:3, :4]
        raw_img = torch.squeeze(raw_img)
        return self.render_dynamic_face(raw_img.shape[0], raw_img.shape[1], self.focal, poses=pose, intrinsic=self.intrinsic,
                                        render_poses=render_poses, chunk=args.chunk, near=self.near, far=self.far, rays=batch_rays,
                                        bc_rgb=bg_img, aud_para=aud_feature, ndc=False)

    # ---- the render methods under upstream's signatures of this class (:244, :259, :336, :357) ----
    def batchify_rays(self, rays, bc_rgb, aud_para, poses=None, intrinsic=None, images_features=None, chunk=1024 * 32):
        return HeadNetwork.batchify_rays(self, rays, bc_rgb, aud_para, poses, None, None, chunk=chunk)

    def render_rays(self, rays, bc_rgb, aud_para, retraw=False, lindisp=False, perturb=None, white_bkgd=False, raw_noise_std=0.,
                    attention_embed_ln=0, pytest=False, taps=False):
        return HeadNetwork.render_rays(self, rays, bc_rgb, aud_para, None, None, None, retraw=retraw, lindisp=lindisp,
                                       perturb=perturb, white_bkgd=white_bkgd, raw_noise_std=raw_noise_std,
                                       attention_embed_ln=attention_embed_ln, pytest=pytest, taps=taps)

    def run_network(self, inputs, viewdirs, aud_para, nerf_model, netchunk=1024 * 64):
        return HeadNetwork.run_network(self, inputs, None, viewdirs, aud_para, nerf_model, None, netchunk=netchunk)

    def render_dynamic_face(self, H, W, focal, poses, intrinsic, render_poses=None, chunk=1024 * 32, near=0., far=1., rays=None,
                            bc_rgb=None, aud_para=None, ndc=False, use_viewdirs=True, rows=None):
        return HeadNetwork.render_dynamic_face(self, H, W, focal, None, poses, None, render_poses=render_poses, chunk=chunk,
                                               near=near, far=far, rays=rays, bc_rgb=bc_rgb, aud_para=aud_para, ndc=ndc,
                                               use_viewdirs=use_viewdirs, rows=rows)
