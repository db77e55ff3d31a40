"""Training path: ``Network.render_rays`` with gradients
(NeRFs/HeadNeRF/train/audio_exp_nerf.py:534-552).

One ``torch.autograd.Function`` per render: forward runs the HIP stages with the
activation-saving MLP variant, backward is two C calls (fine pass, coarse pass), each
compositing-backward + 11 layers of MFMA GEMMs + the conditioning fold.  Gradients reach
every FaceNeRF parameter of both networks, ``aud_para`` (and through it the audio nets,
which stay ordinary autograd modules), ``latent_code`` and -- only when ``rays`` require one (pose refinement,
pose_refine.py) -- the ray records: origins, directions and view directions, summed over the two passes.  ``expr`` and ``bc_rgb``
get theirs on the same condition (cond_refine.py): d expr from the conditioning fold of both passes (``idealnerf_pass_bwd_ex``),
d bc = g_rgb_map * last_weight of each pass, the exact derivative of the fp32 forward (rgb_map is linear in the background).
Sampled depths are detached exactly as upstream (:345).  A FaceNeRFAgg pair (agg_aud_exp_nerf.Network) goes through the same function:
each network's fused feature is its conditioning vector, its columns of ``views_linears.0`` are a bias term
(``_pass_bwd``), and torch carries the feature's gradient into ``agg_linears`` and the audio nets.

``FaceNeRFFn`` is the same machinery for ``FaceNeRF.forward`` on pre-embedded rows (models/face_nerf.py:40-80): the
activation-saving forward in the rows' mode, and a backward seeded by dL/d out that also returns d x and d expr.
"""
import os

import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops
from .helper import linspace01

PARAM_KEYS = ([f"pts_linears.{i}.{k}" for i in range(8) for k in ("weight", "bias")] +
              [f"views_linears.{i}.{k}" for i in range(3) for k in ("weight", "bias")] +
              ["alpha_linear.weight", "alpha_linear.bias", "rgb_linear.weight", "rgb_linear.bias"])

# Arithmetic of the training forward: "bf16x6" (six bf16 piece products per fp32 product, weights and activations as
# three bf16 pieces: fp32-grade, 1.6x the fp32 pipe) or "f32" (fp32 MFMA).  The backward's pipes are a property of the
# library build.
TRAIN_PRECISION = os.environ.get("IDN_TRAIN_PRECISION", "bf16x6")


def _train_code():
    if TRAIN_PRECISION not in ("f32", "bf16x6"):
        raise _lib.IdealNerfError(f"IDN_TRAIN_PRECISION must be f32 or bf16x6 (got {TRAIN_PRECISION!r})")
    return TRAIN_PRECISION, (_lib.IDN_PREC_F32 if TRAIN_PRECISION == "f32" else _lib.IDN_PREC_BF16X6)


def _train_query(net, folded, rays, z):
    prec_name, code = _train_code()
    return ops.query_rays_train_fwd(net.packed_weights(prec_name), folded, rays, z, code, net.input_xyz_ch, net.input_views_ch)


def _pass_bwd(net, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent, frozen=False,
              d_rays=None, d_expr=None):
    """One pass's backward -> its 24 parameter gradients by PARAM_KEYS.  frozen = (need_aud, need_latent) for a network none of
    whose parameters needs a gradient: the conditioning-only plan -- d_aud / d_latent alone, each only if needed (neither: no
    launch at all), and None for every parameter.

    A network whose ``bias_columns()`` is a block E of ``views_linears.0.weight`` (FaceNeRFAgg: E @ aud is part of that layer's
    bias) gets, from the layer's bias gradient b: dE = outer(b, aud) appended to the kernels' weight gradient, and
    d_aud += E^T b (frozen: b alone, from the conditioning-only plan's deltas).

    d_rays [n, 11] (pose refinement): OVERWRITTEN with the pass's gradient of the ray records, by the entry that also runs
    the input-row gradient and its per-ray reduction (ops.pass_bwd_rays); None: that entry is never reached.  The frozen
    plan has no ray gradient.

    d_expr [dim_expr] (expression refinement): ACCUMULATED, in either plan, through ops.pass_bwd_ex; None: the calls above,
    unchanged.  In the frozen plan it counts as a wanted output beside d_aud / d_latent."""
    ext = net.bias_columns()
    if frozen and d_rays is not None:
        raise _lib.IdealNerfError("rays require a gradient but the network is frozen: the conditioning-only backward "
                                  "(idealnerf_pass_bwd_cond) returns no ray gradient")
    if frozen:
        d_aud, d_latent = (d if want else None for d, want in zip((d_aud, d_latent), frozen))
        if d_expr is not None:
            ops.pass_bwd_ex(net.kernel_params(), None, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud,
                            d_latent, d_expr=d_expr)
        elif d_aud is not None or d_latent is not None:
            args = (net.kernel_params(), aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent)
            if ext is not None and d_aud is not None:
                b = torch.empty(ext.shape[0], dtype=torch.float32, device=ext.device)
                ops.pass_bwd_cond(*args, b)
                d_aud.addmv_(ext.detach().t(), b)
            else:
                ops.pass_bwd_cond(*args)
        return dict.fromkeys(PARAM_KEYS)
    sd = net.kernel_tensors()
    # (no column stays uninitialised: the fold kernel writes all conditioning columns, the GEMM reductions all others)
    grads = {k: torch.empty_like(sd[k]) for k in PARAM_KEYS}
    args = (net.kernel_params(), grads, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent)
    if d_expr is not None:
        ops.pass_bwd_ex(*args, d_expr=d_expr, d_rays=d_rays)
    elif d_rays is None:
        ops.pass_bwd(*args)
    else:
        ops.pass_bwd_rays(*args, d_rays)
    if ext is not None:
        b = grads["views_linears.0.bias"]
        if d_aud is not None:
            d_aud.addmv_(ext.detach().t(), b)
        grads["views_linears.0.weight"] = torch.cat((grads["views_linears.0.weight"], torch.outer(b, aud)), dim=1)
    return grads


class RenderRaysFn(torch.autograd.Function):
    """outputs: rgb_map, disp_map, acc_map [, rgb0, disp0, acc0, z_std, last_weight]
    [, rgb_fg [, rgb_fg0, last_weight0]]  (middle group when N_importance > 0, last group for the
    torso variant).  disp / z_std carry no gradient.

    ``aud`` is the coarse network's conditioning vector and, with ``aud_fine`` None, the fine network's too (a FaceNeRF pair:
    one audio feature, one gradient buffer both passes accumulate into).  ``aud_fine``: the fine network's own vector (a
    FaceNeRFAgg pair: each network fuses its feature with its own ``agg_linears``), with a gradient of its own."""

    N_FIXED = 14  # non-parameter arguments of forward

    @staticmethod
    def forward(ctx, coarse, fine, S, Ni, with_fg, rays, bc, expr, t_rand, u, aud, aud_fine, latent, lindisp, *params):
        dev = rays.device
        f32 = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
        aud_d, expr_d, lat_d = f32(aud), f32(expr), f32(latent)
        aud_fd = aud_d if aud_fine is None else f32(aud_fine)
        fc = coarse.cond_folded_bias(aud_d, expr_d, lat_d)
        z_c = ops.coarse_depths(rays, linspace01(S, dev), t_rand, lindisp=lindisp)
        raw_c, acts_c = _train_query(coarse, fc, rays, z_c)
        if Ni > 0:   # coarse compositing + importance sampling + merge: one kernel, the weights stay on chip
            comp_c = smp = ops.march_fwd(raw_c, z_c, rays, bc, u, Ni, with_fg=with_fg)
        else:
            comp_c = ops.composite_fwd(raw_c, z_c, rays, bc, with_fg=with_fg, with_weights=False)
        # outputs the loss does not touch (acc_map, last_weight, ... in the reference's loop) come back as None, not as
        # zero tensors autograd would have to allocate and fill (a fill launch each): the C backward takes NULL for them
        ctx.set_materialize_grads(False)
        ctx.nets, ctx.Ni, ctx.with_fg = (coarse, fine), Ni, with_fg
        ctx.cond = (aud_d, aud_fd, expr_d, lat_d)
        need_aud = aud is not None and aud.requires_grad
        # (need d aud of the coarse pass, of the fine pass -- one and the same where the vector is shared --, need d latent)
        ctx.needs = (need_aud, need_aud if aud_fine is None else aud_fine.requires_grad, latent is not None and latent.requires_grad)
        ctx.shared_aud = aud_fine is None
        need_bc = ctx.needs_input_grad[6]   # (only then are the two [n] coefficient vectors kept for the backward)
        if ctx.needs_input_grad[5]:   # rays (pose refinement): both passes run the full backward, or none can return d rays
            n_keys = len(PARAM_KEYS)
            trained = [any(t.requires_grad for t in params[i * n_keys:(i + 1) * n_keys]) for i in range(2 if Ni > 0 else 1)]
            if not all(trained):
                raise _lib.IdealNerfError("rays require a gradient but a network of the pair is frozen (none of its parameters "
                                          "requires one): the conditioning-only backward returns no ray gradient")
        if Ni == 0:
            ctx.saved = (rays, bc, raw_c, z_c, acts_c)
            ctx.bc_weights = (comp_c["last_weight"],) if need_bc else None
            outs = [comp_c["rgb_map"], comp_c["disp_map"], comp_c["acc_map"]]
            if with_fg:
                outs.append(comp_c["rgb_fg"])
            ctx.mark_non_differentiable(outs[1])
            return tuple(outs)
        ff = fine.cond_folded_bias(aud_fd, expr_d, lat_d)
        z_f = smp["z_fine"]
        raw_f, acts_f = _train_query(fine, ff, rays, z_f)
        comp_f = ops.composite_fwd(raw_f, z_f, rays, bc, with_fg=with_fg, with_weights=False)
        ctx.saved = (rays, bc, raw_c, z_c, acts_c, raw_f, z_f, acts_f)
        ctx.bc_weights = (comp_c["last_weight"], comp_f["last_weight"]) if need_bc else None
        outs = [comp_f["rgb_map"], comp_f["disp_map"], comp_f["acc_map"], comp_c["rgb_map"], comp_c["disp_map"],
                comp_c["acc_map"], smp["z_std"], comp_f["last_weight"]]
        if with_fg:
            outs += [comp_f["rgb_fg"], comp_c["rgb_fg"], comp_c["last_weight"]]
        ctx.mark_non_differentiable(outs[1], outs[4], outs[6])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g):
        coarse, fine = ctx.nets
        Ni, with_fg = ctx.Ni, ctx.with_fg
        aud, aud_f, expr, lat = ctx.cond
        need_aud, need_aud_f, need_lat = ctx.needs
        # the plan of each network, from what autograd asks for: a network none of whose 24 parameters needs a gradient runs the
        # conditioning-only backward (and nothing at all if neither aud nor latent needs one either)
        need_p = ctx.needs_input_grad[RenderRaysFn.N_FIXED:]
        frozen_c, frozen_f = not any(need_p[:len(PARAM_KEYS)]), not any(need_p[len(PARAM_KEYS):])
        both_frozen = frozen_c and (frozen_f or Ni == 0)
        d_lat = torch.zeros_like(lat) if lat is not None and (need_lat or not both_frozen) else None
        if ctx.shared_aud:
            d_aud = d_aud_f = torch.zeros_like(aud) if aud is not None and (need_aud or not both_frozen) else None
        else:
            d_aud = torch.zeros_like(aud) if need_aud or not frozen_c else None
            d_aud_f = torch.zeros_like(aud_f) if Ni > 0 and (need_aud_f or not frozen_f) else None
        c = lambda t: None if t is None else t.contiguous()
        # d rays: one buffer per pass (each entry overwrites its own), only when rays require a gradient -- otherwise nothing
        # new is allocated or launched and the step is what it was
        need_rays = ctx.needs_input_grad[5]
        new_d_rays = lambda: torch.empty_like(ctx.saved[0]) if need_rays else None
        # d expr: one buffer both passes accumulate into, as for the latent code; d bc: no kernel -- rgb_map (rgb0) is linear in the
        # background with the pass's last_weight as coefficient, and rgb_fg has no background term.  Each only if asked for.
        d_expr = torch.zeros_like(expr) if ctx.needs_input_grad[7] and expr is not None else None
        d_bc = None
        if Ni == 0:
            rays, bc, raw_c, z_c, acts_c = ctx.saved
            d_rays = new_d_rays()
            gc = _pass_bwd(coarse, aud, expr, lat, acts_c, raw_c, z_c, rays, bc, c(g[0]), c(g[3]) if with_fg else None,
                           None, c(g[2]), d_aud, d_lat, frozen=frozen_c and (need_aud, need_lat), d_rays=d_rays, d_expr=d_expr)
            gf = {k: None for k in PARAM_KEYS}
            if ctx.bc_weights is not None:
                d_bc = torch.zeros_like(bc) if g[0] is None else g[0] * ctx.bc_weights[0][:, None]
        else:
            rays, bc, raw_c, z_c, acts_c, raw_f, z_f, acts_f = ctx.saved
            d_rays_f, d_rays = new_d_rays(), new_d_rays()
            gf = _pass_bwd(fine, aud_f, expr, lat, acts_f, raw_f, z_f, rays, bc, c(g[0]), c(g[8]) if with_fg else None,
                           c(g[7]), c(g[2]), d_aud_f, d_lat, frozen=frozen_f and (need_aud_f, need_lat), d_rays=d_rays_f,
                           d_expr=d_expr)
            gc = _pass_bwd(coarse, aud, expr, lat, acts_c, raw_c, z_c, rays, bc, c(g[3]), c(g[9]) if with_fg else None,
                           c(g[10]) if with_fg else None, c(g[5]), d_aud, d_lat, frozen=frozen_c and (need_aud, need_lat),
                           d_rays=d_rays, d_expr=d_expr)
            if need_rays:
                d_rays += d_rays_f   # coarse + fine, one fp32 addition per element
            if ctx.bc_weights is not None:
                lw_c, lw_f = ctx.bc_weights
                d_bc = torch.zeros_like(bc) if g[0] is None else g[0] * lw_f[:, None]
                if g[3] is not None:
                    d_bc = d_bc + g[3] * lw_c[:, None]
        ctx.saved = ctx.bc_weights = None
        param_grads = [gc[k] for k in PARAM_KEYS] + [gf[k] for k in PARAM_KEYS]
        fixed = [None] * RenderRaysFn.N_FIXED
        fixed[5] = d_rays
        fixed[6] = d_bc
        fixed[7] = d_expr
        fixed[10] = d_aud if need_aud else None
        fixed[11] = d_aud_f if need_aud_f and not ctx.shared_aud else None
        fixed[12] = d_lat if need_lat else None
        return (*fixed, *param_grads)


def render_rays_apply(network, coarse, fine, rays, bc_rgb, aud_para, latent_code, expr, perturb, pytest, with_fg=False,
                      lindisp=False):
    args = network.args
    if not rays.requires_grad:   # rays that require a gradient (pose refinement) keep their graph edge
        rays = rays.detach()
    rays = rays.to(torch.float32).contiguous()
    if not bc_rgb.requires_grad:   # a background that requires a gradient (cond_refine.Background) keeps its graph edge
        bc_rgb = bc_rgb.detach()
    bc = bc_rgb.to(torch.float32).contiguous()
    n, dev = rays.shape[0], rays.device
    S, Ni = args.N_samples, args.N_importance
    t_rand, u = network.draw_randoms(n, S, Ni, perturb, pytest, dev)
    pc, pf = dict(coarse.named_parameters()), dict(fine.named_parameters())
    params = [pc[k] for k in PARAM_KEYS] + [pf[k] for k in PARAM_KEYS]
    # each network's conditioning vector (FaceNeRF: the audio feature itself, one for both; FaceNeRFAgg: its fused feature,
    # computed here with autograd on, so that torch carries its gradient into agg_linears and the audio nets)
    cond, expr_k = coarse.conditioning(aud_para, expr)
    cond_fine = fine.conditioning(aud_para, expr)[0] if Ni > 0 else None
    if cond_fine is cond:
        cond_fine = None
    if expr_k is not None and expr_k.requires_grad:   # (its gradient comes back as fp32, the kernels' type)
        expr_k = expr_k.to(torch.float32)
    outs = RenderRaysFn.apply(coarse, fine, S, Ni, with_fg, rays, bc, expr_k, t_rand, u, cond, cond_fine, latent_code,
                              bool(lindisp), *params)
    ret = {'rgb_map': outs[0], 'disp_map': outs[1], 'acc_map': outs[2]}
    if Ni > 0:
        ret.update(rgb0=outs[3], disp0=outs[4], acc0=outs[5], z_std=outs[6], last_weight=outs[7])
        if with_fg:
            ret.update(rgb_map_fg=outs[8], rgb_map_fg0=outs[9], last_weight0=outs[10])
    elif with_fg:
        ret['rgb_map_fg'] = outs[3]
    return ret


class FaceNeRFFn(torch.autograd.Function):
    """FaceNeRF.forward (models/face_nerf.py:40-80) with gradients: one activation-saving forward launch, one C call
    backward (the render pass's delta chain and weight-gradient products, seeded by dL/d out).  Gradients reach the 24
    parameters idn_facenerf_params names (feature_linear is never applied upstream and gets none), x, aud, expr and
    latent_code -- each only if it requires grad.  The forward runs TRAIN_PRECISION (as render training does).

    Memory: the saved activation slab holds 2648 floats per row (10.6 KB; rows rounded up to 128), kept until the
    backward: 40 000 rows hold about 0.42 GB, 2^19 rows 5.6 GB.  Once differentiable (create_graph=True raises)."""

    @staticmethod
    def forward(ctx, module, x, aud, expr, latent, *params):
        prec_name, code = _train_code()
        f32 = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
        aud_d, expr_d, lat_d = f32(aud), f32(expr), f32(latent)
        folded = module.folded_bias(aud_d, expr_d, lat_d)
        out, acts = ops.facenerf_train_fwd(module.packed_weights(prec_name), folded, f32(x), code, module.input_xyz_ch,
                                           module.input_views_ch)
        ctx.module, ctx.acts, ctx.cond = module, acts, (aud_d, expr_d, lat_d)
        ctx.like = [None if t is None else (t.dtype, t.shape) for t in (x, aud, expr, latent)]   # gradients come back alike
        return out

    @staticmethod
    def backward(ctx, g_out):
        if torch.is_grad_enabled():
            raise _lib.IdealNerfError("FaceNeRF.forward is once differentiable: create_graph=True (double backward) is not built")
        return _facenerf_backward(ctx, g_out)


@once_differentiable
def _facenerf_backward(ctx, g_out):
    module, acts = ctx.module, ctx.acts
    aud, expr, lat = ctx.cond
    need = ctx.needs_input_grad        # (module, x, aud, expr, latent, *params)
    sd = dict(module.named_parameters())
    dev = acts.device
    n = g_out.shape[0]
    zeros = lambda t, want: torch.zeros(t.shape, dtype=torch.float32, device=dev) if want and t is not None else None
    d_aud, d_expr, d_lat = zeros(aud, need[2]), zeros(expr, need[3]), zeros(lat, need[4])
    d_x = torch.empty((n, module.input_xyz_ch + module.input_views_ch), dtype=torch.float32, device=dev) if need[1] else None
    grads = {k: (torch.empty_like if n else torch.zeros_like)(sd[k]) for k in PARAM_KEYS}
    if n:
        ops.facenerf_bwd(module.kernel_params(), grads, aud, expr, lat, acts, g_out.detach().to(torch.float32).contiguous(),
                         d_x=d_x, d_aud=d_aud, d_expr=d_expr, d_latent=d_lat)
    elif d_x is not None:
        d_x.zero_()
    ctx.acts = None
    cast = lambda d, like: None if d is None else d.to(like[0]).view(like[1])
    fixed = (None, *[cast(d, like) for d, like in zip((d_x, d_aud, d_expr, d_lat), ctx.like)])
    return (*fixed, *[grads[k] if need[5 + i] else None for i, k in enumerate(PARAM_KEYS)])


def facenerf_apply(module, x, aud, expr, latent_code):
    sd = dict(module.named_parameters())
    return FaceNeRFFn.apply(module, x, aud, expr, latent_code, *[sd[k] for k in PARAM_KEYS])
