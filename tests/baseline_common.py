"""What tests/test_baseline_cpu.py and tests/test_baseline_gpu.py share (not collected by pytest): the 32 x 32 training scene
with an AD-NeRF baseline pair (audio only: dim_expr = dim_latent = 0, C = 127), weights by the fixtures' recipe
(tests/golden/make_golden_baseline.py), and an AD-NeRF four-dict checkpoint built from seeds."""
import numpy as np
import torch

import oracle

NEAR, FAR = 0.5772005200386048, 1.1772005200386046
DIMS = oracle.facenerf_dims(dim_aud=64, dim_expr=0, dim_latent=0)
SEEDS = (1, 2)   # make_golden_baseline.pick_seeds: the first pair (s, s + 1) that leaves both volumes occupied


def scene():
    """The 32 x 32 synthetic scene as the baseline fixtures draw it: no expression, no latent code."""
    return oracle.synthetic_frame(32, 32, seed=0, dims=DIMS)


def baseline_state(seed, gain=300.0, bias=0.3):
    """The fixtures' recipe for one network of the pair -> its state dict on the CPU: Xavier-uniform from numpy
    RandomState(seed) in state_dict order, bias 0.01, the density head scaled by `gain` with bias `bias`."""
    import idealnerf_amd
    from idealnerf_amd import synthetic
    m = idealnerf_amd.FaceNeRF(dim_aud=64, dim_latent=0, dim_expr=0)
    synthetic.xavier_state_dict(m, seed, gain, bias)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def render_config(n_importance=128, **over):
    from idealnerf_amd.helper import RenderConfig
    return RenderConfig(**{**dict(perturb=0.0, chunk=512, near=NEAR, far=FAR, N_importance=n_importance, dim_aud=64, dim_expr=0,
                                  dim_latent=0), **over})


def baseline_network(dev, n_importance=128, seeds=SEEDS, size=32, focal=None):
    """A head_baseline.Network with the recipe's pair (seeds 1 / 2: 92 % of the coarse and 74 % of the fine samples of the
    fixture's rays have a positive density, so both passes carry gradients) -> (network in train mode on dev, scene)."""
    from idealnerf_amd.head_baseline import Network
    torch.manual_seed(1234)   # the audio nets are torch-initialised
    syn = scene()
    net = Network(size, size, syn["focal"] if focal is None else focal, NEAR, FAR, 512, None, 64, n_importance,
                  args=render_config(n_importance))
    net.face_nerf_coarse.load_state_dict(baseline_state(seeds[0]))
    net.face_nerf_fine.load_state_dict(baseline_state(seeds[1]))
    net = net.to(dev)
    net.train()
    return net, syn


def pick_rays(syn, n_rays, seed):
    """n_rays ray records of the scene, their background colours and a random target (agg_common.pick_rays)."""
    rs = np.random.RandomState(seed)
    ro, rd = oracle.camera_rays(32, 32, syn["focal"], syn["c2w"])
    rays_all = oracle.ray_records(ro, rd, NEAR, FAR)
    sel = torch.from_numpy(rs.choice(1024, size=n_rays, replace=False))
    tgt = torch.from_numpy(rs.uniform(0, 1, size=(n_rays, 3)).astype(np.float32))
    return rays_all[sel].contiguous(), syn["bc"].reshape(-1, 3)[sel].contiguous(), tgt


def adnerf_checkpoint(seeds=(11, 12), aud_seed=5, global_step=400000):
    """An AD-NeRF checkpoint as its tooling writes it: the coarse / fine FaceNeRF (C = 127) and the two audio nets under
    network_fn / network_fine / network_audnet / network_audattnet _state_dict, all built from seeds (density gain 200)."""
    from idealnerf_amd.models.audio_net import AudioAttNet, AudioNet
    torch.manual_seed(aud_seed)
    return {"network_fn_state_dict": baseline_state(seeds[0], 200.0), "network_fine_state_dict": baseline_state(seeds[1], 200.0),
            "network_audnet_state_dict": AudioNet(64, 16).state_dict(), "network_audattnet_state_dict": AudioAttNet().state_dict(),
            "global_step": global_step}


def forward_data(g, index):
    """The 7-tuple of tests/golden/baseline_forward.npz for frame `index`, collated as a batch-1 loader collates it."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return (torch.zeros(1, 2, 1, 3), torch.zeros(1, 3), T(g["bg"])[None], T(g["auds"])[None], torch.zeros(1, 32, 32, 3),
            T(g["pose"])[None], torch.tensor([int(index)]))
