"""Drop-in for the feature-aggregation renderer ``NeRFs/HeadNeRF/train/agg_aud_exp_nerf.py::Network`` (:175-247 and the
render methods behind it, which are the head renderer's).

The head ``Network`` with three differences, all upstream's: the pair is ``FaceNeRFAgg(dim_aud, dim_expr=79, dim_agg=64,
dim_latent=32)`` (:190-199, literals included), the audio branch is the smoothed window from ``nosmo_iters`` on and
``aud_net(auds[index])`` before it -- no ``dim_aud > 29`` condition and no DeepSpeech net (:216-240) --, and the expression is
always passed (:245).  Everything else -- constructor arguments, ``forward([data, global_step, dataset_size])`` and its return
values, ``render_rays`` / ``render_dynamic_face`` / ``batchify_rays``, the precision handling, one C call per frame in eval
mode, the packed-weight cache -- is inherited.

Training: ``render_rays`` under autograd hands each network's fused feature ``g = agg_linears(cat(aud, expr / 3))`` to
``autograd.RenderRaysFn`` as that network's conditioning vector.  For the kernels the network is a FaceNeRF with
``dim_aud = 64``, ``dim_expr = 0``: ``aud := g``, ``views_linears.0.weight := W0[:, :283]``,
``views_linears.0.bias := b0 + W0[:, 283:] @ g``.  ``FaceNeRFAgg.forward`` itself stays an inference
entry and raises under autograd.
"""
from .audio_exp_nerf import Network as HeadNetwork, init_weights  # noqa: F401  (init_weights: the trainer applies it)
from .helper import input_channels
from .models.face_nerf_agg import FaceNeRFAgg

DIM_EXPR, DIM_AGG, DIM_LATENT = 79, 64, 32   # agg_aud_exp_nerf.py:190-199


def config_parser():
    """The head stage's parser plus the ``use_highlight`` switch this trainer reads (config.AGG_FLAGS)."""
    from .config import ConfigParser
    return ConfigParser("agg")


class Network(HeadNetwork):
    config_kind = "agg"
    deepspeech_net = False

    def make_nerf(self):
        args = self.args
        input_ch, input_ch_views = input_channels(args)   # agg_aud_exp_nerf.py:33-34
        return FaceNeRFAgg(D=args.netdepth, W=args.netwidth, input_ch=input_ch, dim_aud=args.dim_aud, dim_latent=DIM_LATENT,
                           dim_expr=DIM_EXPR, dim_agg=DIM_AGG, output_ch=4, skips=self.skips, input_ch_views=input_ch_views,
                           use_viewdirs=args.use_viewdirs)

    def audio_feature(self, auds, index, global_step, dataset_size):
        if global_step >= self.args.nosmo_iters:
            return self.smoothed_audio_feature(auds, index, dataset_size)
        return self.aud_net(auds[index].unsqueeze(0) if auds[index].dim() == 2 else auds[index])

    def expr_feature(self, expr):
        return expr


HEAD_MODELS = ("head", "agg", "baseline")


def head_network_class(model="head"):
    """The renderer class of a head-stage model: "head" (audio_exp_nerf.Network), "agg" (this module's) or "baseline"
    (head_baseline.Network: audio only, no expression and no latent code anywhere in its tuples)."""
    if model not in HEAD_MODELS:
        raise ValueError(f"model must be one of {HEAD_MODELS}, got {model!r}")
    if model == "baseline":
        from .head_baseline import Network as BaselineNetwork
        return BaselineNetwork
    return HeadNetwork if model == "head" else Network


def build_head_network(args, H, W, focal, model="head", intrinsic=None):
    """The head-stage network of the flags ``args`` as the trainers and the clip tools build it (on the CPU, uninitialised).
    The agg pair's expression width is upstream's literal 79 whatever ``args.dim_expr`` says."""
    from .config import to_render_config
    return head_network_class(model)(H, W, focal, near=args.near, far=args.far, chunk=args.chunk, intrinsic=intrinsic,
                                     N_samlpes=args.N_samples, N_importance=args.N_importance, args=to_render_config(args))
