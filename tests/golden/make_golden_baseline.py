#!/usr/bin/env python3
"""Golden fixtures of the AD-NeRF baseline model, from the REFERENCE itself on the CPU (build container only, like
make_golden.py, whose stand-ins for the optional imports this script uses):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_baseline.py

The reference module (NeRFs/HeadNeRF/train/head_baseline.py) makes CUDA tensors the default at import (:36);
``torch.set_default_tensor_type`` is a no-op while it is imported here.

``baseline_train_step.npz``   one training step of the reference's baseline ``Network``: 64 rays of the 32 x 32 scene (the
                              ``sel`` of train_step.npz), perturb 0 -- loss = mse(rgb) + mse(rgb0), the rgb maps, ``g_aud`` and
                              agg_train_step.npz's selection of parameter gradients (without the ``agg_linears``) at the same row
                              step.  Weights are not stored: ``make_golden_agg.recipe`` (Xavier-uniform from numpy
                              RandomState(seed) in state_dict order, bias 0.01, the density head scaled by 300 with bias 0.3), as
                              the tests rebuild them; the seeds are in the file.  Also the network's state-dict keys and shapes.
                              The seeds are chosen here, from the reference's own forward and nothing else: the first pair
                              (s, s + 1), s = 1, 2, ..., that leaves both volumes occupied -- at least MIN_OCCUPANCY of the
                              coarse and of the fine samples of the fixture's 64 rays with a positive density
                              (agg_train_step.npz's pair has 0.16 / 0.56).  A pair below that (6 / 7 here: 0.06 coarse, some
                              rays without any coarse weight) makes the importance sampling's cdf a quotient of last-ulp noise
                              and the fixture a test of that noise.
``baseline_forward.npz``      the reference's eval ``forward`` on the 32 x 32 frame of a 10-frame clip, built the way
                              smoother.npz was: one case before ``nosmo_iters`` (``aud_net(auds[index])``) and two at it (the
                              smoothed window at both ends of the clip: four zero-padded slots on the left, three on the right).
                              Stored: the inputs, the two audio nets' weights, and per case the audio feature handed to the
                              renderer, rgb and rgb0.
``baseline_sample_rays.npz``  the reference's ``GetData.sample_rays`` on a 96 x 96 frame: TWO consecutive calls from one seeded
                              generator (the second call's pixels depend on the zero-size third draw of the first).  Stored
                              per call: pixel rows (recovered from a rerun whose target image holds each pixel's coordinates),
                              rays, targets, background rows.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import NEAR, FAR, REF, REPO, install_shims  # noqa: E402
from make_golden_agg import GRAD_KEYS, ROW_STEP, recipe  # noqa: E402

SEEDS = (1, 2)          # what pick_seeds() finds; main() checks it
MIN_OCCUPANCY = 0.15
BASELINE_GRAD_KEYS = tuple(k for k in GRAD_KEYS if not k.startswith("agg_linears"))


def import_baseline():
    import importlib
    real = torch.set_default_tensor_type
    torch.set_default_tensor_type = lambda *a, **k: None
    try:
        return importlib.import_module("NeRFs.HeadNeRF.train.head_baseline")
    finally:
        torch.set_default_tensor_type = real


def occupancy(net, rays, bc, aud):
    """Share of the samples with a positive density, per network (the recipe's seeds must leave both volumes occupied)."""
    out = []
    real = net.raw2outputs

    def tap(raw, *a, **k):
        out.append(float((raw[..., 3] > 0).float().mean()))
        return real(raw, *a, **k)
    net.raw2outputs = tap
    with torch.no_grad():
        net.render_rays(rays, bc, aud)
    net.raw2outputs = real
    return out


def pick_seeds(hb, limit=12):
    """The first pair (s, s + 1) whose coarse and fine volumes are both occupied on the fixture's rays (module docstring)."""
    import oracle
    syn = oracle.synthetic_frame(32, 32, seed=0, dims=oracle.facenerf_dims(dim_aud=64, dim_expr=0, dim_latent=0))
    net = hb.Network(32, 32, syn["focal"], NEAR, FAR, 512, None, 64, 128)
    rays = torch.from_numpy(np.load(os.path.join(HERE, "frame32.npz"))["rays"])
    sel = torch.from_numpy(np.load(os.path.join(HERE, "train_step.npz"))["sel"])
    for s in range(1, limit):
        recipe(net.face_nerf_coarse, s, 300.0, 0.3)
        recipe(net.face_nerf_fine, s + 1, 300.0, 0.3)
        occ = occupancy(net, rays[sel], syn["bc"].reshape(-1, 3)[sel], syn["aud"])
        print(f"seeds {s} / {s + 1}: occupancy coarse {occ[0]:.3f} fine {occ[1]:.3f}")
        if min(occ) >= MIN_OCCUPANCY:
            return s, s + 1
    raise SystemExit("no seed pair leaves both volumes occupied")


def train_step(hb, helper):
    import oracle
    dims = oracle.facenerf_dims(dim_aud=64, dim_expr=0, dim_latent=0)
    syn = oracle.synthetic_frame(32, 32, seed=0, dims=dims)
    torch.manual_seed(1234)
    net = hb.Network(32, 32, syn["focal"], NEAR, FAR, 512, None, 64, 128)
    recipe(net.face_nerf_coarse, SEEDS[0], 300.0, 0.3)
    recipe(net.face_nerf_fine, SEEDS[1], 300.0, 0.3)
    net.train()
    rays = torch.from_numpy(np.load(os.path.join(HERE, "frame32.npz"))["rays"])
    sel = torch.from_numpy(np.load(os.path.join(HERE, "train_step.npz"))["sel"])
    rs = np.random.RandomState(79)
    tgt = torch.from_numpy(rs.uniform(0, 1, size=(sel.numel(), 3)).astype(np.float32))
    bc = syn["bc"].reshape(-1, 3)[sel]
    occ = occupancy(net, rays[sel], bc, syn["aud"])
    print("share of samples with a positive density (coarse, fine):", occ)
    assert min(occ) >= MIN_OCCUPANCY, occ
    aud = syn["aud"].clone().requires_grad_(True)
    ret = net.render_rays(rays[sel], bc, aud)
    img_loss = helper.img2mse(ret["rgb_map"], tgt)
    loss = img_loss + helper.img2mse(ret["rgb0"], tgt)
    loss.backward()
    sd = net.state_dict()
    shapes = np.zeros((len(sd), 3), dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = list(v.shape)
    fx = dict(sel=sel.numpy(), target=tgt.numpy(), loss=loss.detach().numpy(), img_loss=img_loss.detach().numpy(),
              rgb_map=ret["rgb_map"].detach().numpy(), rgb0=ret["rgb0"].detach().numpy(), g_aud=aud.grad.numpy(),
              seed_coarse=np.int64(SEEDS[0]), seed_fine=np.int64(SEEDS[1]), occupancy=np.array(occ),
              state_keys=np.array(list(sd)), state_shapes=shapes, state_ndim=np.array([v.dim() for v in sd.values()]))
    for tag, m in (("c", net.face_nerf_coarse), ("f", net.face_nerf_fine)):
        named = dict(m.named_parameters())
        for k in BASELINE_GRAD_KEYS:
            grad = named[k].grad.numpy()
            fx[f"g_{tag}_{k}"] = grad[::ROW_STEP] if grad.ndim == 2 and grad.shape[0] >= 128 else grad
        assert named["feature_linear.weight"].grad is None
    fx["row_step"] = np.int64(ROW_STEP)
    path = os.path.join(HERE, "baseline_train_step.npz")
    np.savez_compressed(path, **fx)
    print("baseline_train_step.npz", os.path.getsize(path) // 1024, "KiB")


def forward(hb):
    import oracle
    dims = oracle.facenerf_dims(dim_aud=64, dim_expr=0, dim_latent=0)
    H = W = 32
    F_ = 10
    syn = oracle.synthetic_frame(H, W, seed=0, dims=dims)
    torch.manual_seed(0)
    net = hb.Network(H, W, syn["focal"], NEAR, FAR, 512, None, 64, 128)
    net.apply(hb.init_weights)
    recipe(net.face_nerf_coarse, SEEDS[0], 300.0, 0.3)
    recipe(net.face_nerf_fine, SEEDS[1], 300.0, 0.3)
    net.eval()
    rs = np.random.RandomState(77)
    auds = torch.from_numpy(rs.standard_normal((F_, 16, 29)).astype(np.float32))
    pose = torch.cat([syn["c2w"], torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
    nosmo = int(hb.args.nosmo_iters)
    cases = [(nosmo - 1, F_ - 1), (nosmo, 0), (nosmo, F_ - 1)]
    fx = dict(auds=auds.numpy(), pose=pose.numpy(), bg=syn["bc"].numpy(), focal=np.float64(syn["focal"]), nosmo_iters=np.int64(nosmo),
              smo_size=np.int64(hb.args.smo_size), cases=np.array(cases, dtype=np.int64), seed_coarse=np.int64(SEEDS[0]),
              seed_fine=np.int64(SEEDS[1]))
    for k, v in net.aud_net.state_dict().items():
        fx["audnet." + k] = v.numpy()
    for k, v in net.aud_att_net.state_dict().items():
        fx["attnet." + k] = v.numpy()
    real_rdf = net.render_dynamic_face
    for c, (step, idx) in enumerate(cases):
        seen = {}

        def spy(*a, **k):
            seen["aud"] = k["aud_para"].detach().clone()
            return real_rdf(*a, **k)

        net.render_dynamic_face = spy
        data = (torch.zeros(1, 2, 1, 3), torch.zeros(1, 3), syn["bc"][None], auds[None], torch.zeros(1, H, W, 3), pose[None],
                torch.tensor([idx]))
        with torch.no_grad():
            rgb, disp, acc, last_w, extras = net([data, step, F_])
        fx[f"aud_feature_{c}"] = seen["aud"].numpy()
        fx[f"rgb_{c}"] = rgb.numpy()
        fx[f"rgb0_{c}"] = extras["rgb0"].numpy()
    net.render_dynamic_face = real_rdf
    assert fx["aud_feature_0"].shape == (64,) and not np.allclose(fx["aud_feature_0"], fx["aud_feature_2"])
    vis = float(np.abs(fx["rgb_1"] - syn["bc"].numpy()).mean())
    path = os.path.join(HERE, "baseline_forward.npz")
    np.savez_compressed(path, **fx)
    print(f"baseline_forward.npz: cases (step, index) {cases} of a {F_}-frame clip, {H}x{W}, visibility {vis:.3f},",
          os.path.getsize(path) // 1024, "KiB")


def sample_rays(hb):
    import oracle
    Hs = Ws = 96
    syn = oracle.synthetic_frame(32, 32, seed=0)
    ds = object.__new__(hb.GetData)
    ds.H, ds.W, ds.focal, ds.cx, ds.cy = Hs, Ws, 256.0, 48.0, 48.0
    ds.args = types.SimpleNamespace(N_rand=96, sample_rate=0.95)
    rs = np.random.RandomState(21)
    pose = syn["c2w"].numpy().astype(np.float64)
    rect = np.array([10, 8, 70, 80], dtype=np.int32)
    lms = rs.uniform(8, 88, size=(68, 2))
    lms[48:] = rs.uniform(42, 54, size=(20, 2))
    target = torch.from_numpy(rs.uniform(0, 1, size=(Hs, Ws, 3)).astype(np.float32))
    bcimg = torch.from_numpy(rs.uniform(0, 1, size=(Hs, Ws, 3)))   # float64 like imread() / 255.0
    rows, cols = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    where = torch.from_numpy(np.stack([rows, cols, rows * Ws + cols], -1).astype(np.float32))
    fx = dict(pose=pose[:3, :4], rect=rect, landmark=lms, target=target.numpy(), bc=bcimg.numpy(), focal=256.0, cx=48.0, cy=48.0,
              N_rand=96, sample_rate=0.95, seed=7)
    np.random.seed(7)
    with torch.no_grad():
        for call in (0, 1):
            brays, tgt_s, bc_s = ds.sample_rays(pose[:3, :4], rect, target, bcimg, lms)
            fx[f"batch_rays_{call}"], fx[f"target_s_{call}"], fx[f"bc_s_{call}"] = brays.numpy(), tgt_s.numpy(), bc_s.numpy()
    np.random.seed(7)
    with torch.no_grad():
        for call in (0, 1):
            _, px, _ = ds.sample_rays(pose[:3, :4], rect, where, bcimg, lms)
            fx[f"pixels_{call}"] = px[:, :2].numpy().astype(np.int64)
            assert np.array_equal(target.numpy()[fx[f"pixels_{call}"][:, 0], fx[f"pixels_{call}"][:, 1]], fx[f"target_s_{call}"])
    assert not np.array_equal(fx["pixels_0"], fx["pixels_1"])
    path = os.path.join(HERE, "baseline_sample_rays.npz")
    np.savez_compressed(path, **fx)
    print("baseline_sample_rays.npz", os.path.getsize(path) // 1024, "KiB")


def main():
    install_shims()
    sys.argv = [sys.argv[0], "--perturb", "0", "--dim_aud", "64", "--N_samples", "64", "--N_importance", "128",
                "--near", str(NEAR), "--far", str(FAR), "--vis_path", "/tmp/idealnerf_golden_vis", "--chunk", "512"]
    sys.path.insert(0, REF)
    sys.path.insert(0, REPO)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import importlib
    hb = import_baseline()
    helper = importlib.import_module("NeRFs.HeadNeRF.helper")
    assert pick_seeds(hb) == SEEDS
    train_step(hb, helper)
    forward(hb)
    sample_rays(hb)


if __name__ == "__main__":
    main()
