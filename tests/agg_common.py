"""What tests/test_agg_cpu.py and tests/test_agg_gpu.py share (not collected by pytest): the reduction of a FaceNeRFAgg to the
FaceNeRF the kernels and the oracle see, as torch expressions of fp32 leaves, and the 32 x 32 training scene with an agg pair.

The reduction, for one network with fused feature g = agg_linears(cat(aud, expr / 3)):

    aud := g,   views_linears.0.weight := W0[:, :283],   views_linears.0.bias := b0 + W0[:, 283:] @ g

``oracle.render_rays`` takes ONE conditioning vector for both networks of a pair, and the two networks of an agg pair fuse
their own.  ``reduced_pair`` therefore hands it ``aud = cat(g_coarse, g_fine)`` and gives each network's ``pts_linears.0`` /
``.5`` zero columns where the other network's feature sits: every product with a zero column is an exact zero, so each
network computes exactly the reduction above on its own g.
"""
import numpy as np
import torch

import oracle

NEAR, FAR = 0.5772005200386048, 1.1772005200386046
N_H = 256 + 27
DIM_AGG, DIM_EXPR, DIM_LATENT = 64, 79, 32
RECT64, MOUTH64 = [2, 2, 40, 40], (30, 34)   # a 64 x 64 clip geometry the highlight recipe can draw from (test_agg_cpu.clip)


def leaves(module):
    """fp32 leaf copies of a module's parameters on the CPU, by state_dict key."""
    return {k: v.detach().cpu().clone().requires_grad_(True) for k, v in module.state_dict().items()}


def agg_feature(p, aud, expr):
    h = torch.cat([aud, expr * 1 / 3], dim=-1)
    for i in (0, 1):
        h = torch.nn.functional.linear(h, p[f"agg_linears.{i}.weight"], p[f"agg_linears.{i}.bias"])
    return h


def reduced(p, aud, expr):
    """-> (the reduced FaceNeRF parameter dictionary of the agg parameters p, g): torch expressions of p, aud, expr."""
    g = agg_feature(p, aud, expr)
    out = {k: v for k, v in p.items() if not k.startswith("agg_linears")}
    W0 = p["views_linears.0.weight"]
    out["views_linears.0.weight"] = W0[:, :N_H]
    out["views_linears.0.bias"] = p["views_linears.0.bias"] + W0[:, N_H:] @ g
    return out, g


def reduced_dims(dim_aud=DIM_AGG):
    return oracle.facenerf_dims(dim_aud=dim_aud, dim_expr=0, dim_latent=DIM_LATENT)


def reduced_pair(pc, pf, aud, expr):
    """-> (coarse dict, fine dict, aud vector, dims) for ONE oracle.render_rays call on an agg pair (module docstring)."""
    rc, g_c = reduced(pc, aud, expr)
    rf, g_f = reduced(pf, aud, expr)
    zeros = torch.zeros(256, DIM_AGG)
    for p, mine_first in ((rc, True), (rf, False)):
        for layer in (0, 5):
            W = p[f"pts_linears.{layer}.weight"]
            own = W[:, 63:63 + DIM_AGG]
            p[f"pts_linears.{layer}.weight"] = torch.cat([W[:, :63], *((own, zeros) if mine_first else (zeros, own)),
                                                          W[:, 63 + DIM_AGG:]], dim=1)
    return rc, rf, torch.cat([g_c, g_f]), reduced_dims(2 * DIM_AGG)


def scene(dim_expr=DIM_EXPR):
    """test_hip_parity._train_net's 32 x 32 synthetic scene, with an expression as wide as the agg pair takes."""
    return oracle.synthetic_frame(32, 32, seed=0, dims=oracle.facenerf_dims(dim_aud=64, dim_expr=dim_expr, dim_latent=DIM_LATENT))


def agg_train_net(dev, n_importance=128, seeds=(6, 7)):
    """_train_net with an agg pair: weights by _agg_state's recipe (Xavier-uniform from numpy RandomState(seed) in state_dict
    order, bias 0.01 -- synthetic.xavier_state_dict is that recipe for any module) and scale_sigma's density (gain 300,
    bias 0.3).  Seeds 6 / 7: 16 % of the coarse and 56 % of the fine samples of this scene have a positive density, so both
    passes carry gradients (with 2 / 3 the fine network's volume is empty and its gradients are exact zeros).
    -> (network in train mode on dev, scene)."""
    from idealnerf_amd import synthetic
    from idealnerf_amd.agg_aud_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    torch.manual_seed(1234)   # the audio nets are torch-initialised
    syn = scene()
    cfg = RenderConfig(perturb=0.0, chunk=512, near=NEAR, far=FAR, N_importance=n_importance)
    net = Network(32, 32, syn["focal"], NEAR, FAR, 512, None, 64, n_importance, args=cfg)
    synthetic.xavier_state_dict(net.face_nerf_coarse, seeds[0], 300.0, 0.3)
    synthetic.xavier_state_dict(net.face_nerf_fine, seeds[1], 300.0, 0.3)
    net = net.to(dev)
    net.train()
    return net, syn


def pick_rays(syn, n_rays, seed):
    """n_rays ray records of the scene, their background colours and a random target, as
    test_train_step_matches_oracle_autograd_ragged draws them."""
    rs = np.random.RandomState(seed)
    ro, rd = oracle.camera_rays(32, 32, syn["focal"], syn["c2w"])
    rays_all = oracle.ray_records(ro, rd, NEAR, FAR)
    sel = torch.from_numpy(rs.choice(1024, size=n_rays, replace=False))
    tgt = torch.from_numpy(rs.uniform(0, 1, size=(n_rays, 3)).astype(np.float32))
    return rays_all[sel].contiguous(), syn["bc"].reshape(-1, 3)[sel].contiguous(), tgt
