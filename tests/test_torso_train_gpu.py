"""The torso stage's training loop on the GPU (run with ``-m gpu``): the conditioning-only backward of a frozen network against
fp64, the plan ``RenderRaysFn.backward`` picks, ``gather_ray_pairs``, ``ResidentTorsoFrames`` against ``TorsoGetData``, three
Adam steps of ``torso_train_step`` against the CPU oracle, and ``train_torso.train``: resume, checkpoint, validation, hand loop."""
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle
import test_hip_parity as hp
from idealnerf_amd.synthetic import write_clip_directory
from train_loop_common import sampler_reference, train_flags

pytestmark = pytest.mark.gpu

NEAR, FAR = hp.NEAR, hp.FAR


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()
    return idealnerf_amd


# ------------------------------------------------------------------------------------------------ T1: pass_bwd_cond vs fp64
def _fp64_d_cond(module, C, acts, raw, z, rec, bc, g_rgb, g_lw, dev):
    """d cond [C] of one pass by an fp64 torch delta chain on the SAME saved activations (hence the same ReLU masks): the
    construction of test_backward_kernels_vs_fp64_on_saved_activations, without the weight gradients."""
    n, S = z.shape
    Pn = n * S
    Pp = (Pn + 127) // 128 * 128
    mat = lambda o, w: acts[o * Pp:(o + w) * Pp].view(Pp, w)[:Pn].double()
    a = [mat(128 + 256 * i, 256) for i in range(8)]
    v = [mat(128 + 2048 + 128 * i, 128) for i in range(3)]
    raw64 = raw.double().cpu().requires_grad_(True)
    comp = oracle.composite(raw64, z.double().cpu(), rec[:, 3:6].double().cpu(), bc.double().cpu())
    ((comp[0] * g_rgb.double().cpu()).sum() + (comp[3][:, -1] * g_lw.double().cpu()).sum()).backward()
    d_raw = raw64.grad.to(dev).view(Pn, 4)
    sd = {k: p.detach().double() for k, p in module.named_parameters()}
    d_rgb, d_sig = d_raw[:, :3], d_raw[:, 3:4]
    dl = (d_rgb @ sd["rgb_linear.weight"]) * (v[2] > 0)
    for i in (2, 1):
        dl = (dl @ sd[f"views_linears.{i}.weight"]) * (v[i - 1] > 0)
    dh = (dl @ sd["views_linears.0.weight"][:, :256] + d_sig @ sd["alpha_linear.weight"]) * (a[7] > 0)
    d_cond = torch.zeros(C, dtype=torch.float64, device=dev)
    for l in range(7, 0, -1):
        W = sd[f"pts_linears.{l}.weight"]
        if l == 5:
            d_cond += (dh @ W[:, 63:63 + C]).sum(0)
            W = W[:, 63 + C:]
        dh = (dh @ W) * (a[l - 1] > 0)
    return d_cond + (dh @ sd["pts_linears.0.weight"][:, 63:]).sum(0)


@pytest.mark.parametrize("n,sample_counts", [(48, (64, 192)), (5, (64, 192)), (1, (64, 192)), (700, (64,))])
def test_pass_bwd_cond_vs_fp64(idn, dev, n, sample_counts):
    """``ops.pass_bwd_cond`` -- d aud and d latent of a frozen pass -- against fp64 under the bound of
    test_backward_kernels_vs_fp64_on_saved_activations (rel_err < 5e-6), head pair (C = 64 + 79 + 32) and torso pair (C = 106,
    no expression, no latent), coarse S = 64 and fine S = 192.  48 rays: 3072 / 9216 rows; 5: 320 rows padded to 384; 1: the
    smallest slab; 700 x 64 = 44 800 rows: several row blocks per column sum.  The entry accumulates (a non-zero initial d_aud
    comes back as initial + result, exactly) and two calls on the same inputs give the same bits."""
    from idealnerf_amd import autograd as ag
    from idealnerf_amd.helper import linspace01
    ops = idn.ops
    net, syn, P, dims, d = hp._torso_setup(idn, dev, n)
    with torch.no_grad():
        aud_h = net.aud_net(d["auds"][1:2].to(dev)).contiguous()
        aud_t = net.torso_signal(aud_h, d["pose"].to(dev)).contiguous()
    expr, lat = d["expr"].to(dev), d["latent"].to(dev)
    bc = d["bg"].to(dev).contiguous()
    pairs = {"head": ((net.face_nerf_coarse, net.face_nerf_fine), d["batch_rays"], aud_h, expr, lat),
             "torso": ((net.torso_coarse_nerf, net.torso_fine_nerf), d["batch_rays_torso"], aud_t, None, None)}
    for tag, (modules, rays, aud, ex, la) in pairs.items():
        rec = oracle.ray_records(rays[0], rays[1], NEAR, FAR).to(dev)
        C = aud.numel() + (0 if ex is None else ex.numel() + la.numel())
        for module, S in zip(modules, (64, 192)):
            if S not in sample_counts:
                continue
            z = ops.coarse_depths(rec, linspace01(S, dev))
            raw, acts = ag._train_query(module, module.folded_bias(aud, ex, la), rec, z)
            rs = np.random.RandomState(S)
            g_rgb = hp.T(rs.standard_normal((n, 3)).astype(np.float32) * 0.01).to(dev)
            g_lw = hp.T(rs.standard_normal(n).astype(np.float32) * 0.01).to(dev)
            want = _fp64_d_cond(module, C, acts, raw, z, rec, bc, g_rgb, g_lw, dev)

            def run(d_aud, d_lat):
                ops.pass_bwd_cond(module.kernel_params(), aud, ex, la, acts, raw, z, rec, bc, g_rgb, None, g_lw, None, d_aud, d_lat)
                return d_aud, d_lat
            zl = lambda: None if la is None else torch.zeros_like(la)
            d_aud, d_lat = run(torch.zeros_like(aud), zl())
            e_aud = hp.rel_err(d_aud, want[:aud.numel()])
            e_lat = None if la is None else hp.rel_err(d_lat, want[aud.numel() + ex.numel():])
            print(f"{tag} S={S} n={n}: rel_err d_aud {e_aud:.2e} d_latent {e_lat if e_lat is None else format(e_lat, '.2e')}")
            assert e_aud < 5e-6, (tag, S, n)
            assert e_lat is None or e_lat < 5e-6, (tag, S, n)
            again = run(torch.zeros_like(aud), zl())
            assert torch.equal(again[0], d_aud) and (la is None or torch.equal(again[1], d_lat)), (tag, S)
            start = hp.T(rs.standard_normal(aud.numel()).astype(np.float32)).to(dev)
            summed, _ = run(start.clone(), zl())
            assert torch.equal(summed, start + d_aud), (tag, S)          # d_aud[c] += (float) sum: one fp32 addition
            only_lat = run(None, zl()) if la is not None else None        # either pointer may be NULL
            assert only_lat is None or torch.equal(only_lat[1], d_lat)


# ------------------------------------------------------------------------------------------------ T2: plan selection
def _torso_backward(net, d, dev):
    for p in net.parameters():
        p.grad = None
    x = (d["batch_rays"][None], d["batch_rays_torso"][None], d["target"], d["bg"], d["auds"][None], None, d["pose"],
         d["expr"][None], d["latent"], torch.tensor([1]))
    rgb_com, rgb_com0 = net([x, 0, 4])
    tgt = d["target"].to(dev)
    (((rgb_com - tgt) ** 2).mean() + ((rgb_com0 - tgt) ** 2).mean()).backward()


def test_backward_plan_follows_requires_grad(idn, dev, monkeypatch):
    """``RenderRaysFn.backward`` picks each network's plan from what requires a gradient: calls of ops.pass_bwd /
    ops.pass_bwd_cond are counted by the network's audio width (64: head pair, 106: torso pair)."""
    ops = idn.ops
    net, syn, P, dims, d = hp._torso_setup(idn, dev)
    net.train()
    calls = []
    real_full, real_cond = ops.pass_bwd, ops.pass_bwd_cond
    monkeypatch.setattr(ops, "pass_bwd", lambda p, *a: (calls.append(("full", p.dim_aud)), real_full(p, *a))[1])
    monkeypatch.setattr(ops, "pass_bwd_cond", lambda p, *a: (calls.append(("cond", p.dim_aud)), real_cond(p, *a))[1])
    head = list(net.face_nerf_coarse.parameters()) + list(net.face_nerf_fine.parameters())
    torso = {k: p for m in ("torso_coarse_nerf", "torso_fine_nerf") for k, p in getattr(net, m).named_parameters(prefix=m)}

    _torso_backward(net, d, dev)                                          # nothing frozen: today's plan everywhere
    assert sorted(calls) == [("full", 64)] * 2 + [("full", 106)] * 2
    base = {k: p.grad.clone() for k, p in torso.items() if p.grad is not None}
    from idealnerf_amd.autograd import PARAM_KEYS
    assert len(base) == 2 * len(PARAM_KEYS)

    calls.clear()
    for p in head:
        p.requires_grad_(False)
    _torso_backward(net, d, dev)                                          # head pair frozen, aud (the audio net) trained
    assert sorted(calls) == [("cond", 64)] * 2 + [("full", 106)] * 2
    assert all(p.grad is None for p in head)
    for k, g in base.items():
        assert torch.equal(torso[k].grad, g), k
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.aud_net.parameters())

    calls.clear()
    one = dict(net.face_nerf_fine.named_parameters())["rgb_linear.bias"]
    one.requires_grad_(True)
    _torso_backward(net, d, dev)                                          # one parameter of the fine head network unfrozen
    assert sorted(calls) == [("cond", 64), ("full", 64)] + [("full", 106)] * 2
    assert one.grad is not None and all(p.grad is None for p in head if p is not one)
    one.requires_grad_(False)

    calls.clear()
    for p in net.aud_net.parameters():
        p.requires_grad_(False)
    _torso_backward(net, d, dev)                                          # nothing on the head pair needs a gradient: no call
    assert sorted(calls) == [("full", 106)] * 2
    for k, g in base.items():
        assert torch.equal(torso[k].grad, g), k


# ------------------------------------------------------------------------------------------------ T3: gather_ray_pairs
@pytest.mark.parametrize("cxcy", [None, (30.25, 41.5)])
def test_gather_ray_pairs_equals_two_gathers(idn, dev, cxcy):
    from idealnerf_amd import synthetic
    ops = idn.ops
    H, W, focal = 48, 80, 173.5
    rs = np.random.RandomState(2)
    pose, pose0 = synthetic.frame(H, W, seed=4)["c2w"][:3, :4], synthetic.frame(H, W, seed=9)["c2w"][:3, :4]
    img = torch.from_numpy(((np.arange(H * W * 3) * 37 + 11) % 256).astype(np.uint8).reshape(H, W, 3)).to(dev)
    bg = torch.from_numpy(((np.arange(H * W * 3) * 101 + 5) % 256).astype(np.uint8).reshape(H, W, 3)).to(dev)
    cx, cy = (None, None) if cxcy is None else cxcy
    for n in (1, 64, 300):
        flat = torch.from_numpy(rs.randint(0, H * W, n).astype(np.int64)).to(dev)
        rays, rays0, tgt, bc = ops.gather_ray_pairs(flat, pose, pose0, H, W, focal, img, bg, cx, cy)
        r1, t1, b1 = ops.gather_rays(flat, pose, H, W, focal, img, bg, cx, cy)
        r0, _, _ = ops.gather_rays(flat, pose0, H, W, focal, img, bg, cx, cy)
        for got, want in ((rays, r1), (rays0, r0), (tgt, t1), (bc, b1)):
            np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
        assert rays0.shape == (2, n, 3) and not torch.equal(rays, rays0)
    bad = torch.tensor([-1, H * W, 5], dtype=torch.int64, device=dev)
    rays, rays0, tgt, bc = ops.gather_ray_pairs(bad, pose, pose0, H, W, focal, img, bg, cx, cy)
    for t in (rays[:, :2], rays0[:, :2], tgt[:2], bc[:2]):
        assert float(t.abs().max()) == 0.0
    assert float(rays0[1, 2].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ T4: the loaders
@pytest.fixture(scope="module")
def clip128(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("clip128"))
    flags, meta = write_clip_directory(d, 128, 3, seed=1, N_rand=64, dim_expr=79, face_rect=[8, 8, 60, 60], mouth_range=(30, 38))
    flags.use_highlight = True
    return d, flags, meta


def test_resident_torso_frames_against_torso_getdata(idn, dev, clip128, monkeypatch, golden):
    from idealnerf_amd import dataset
    d, flags, meta = clip128
    ds = dataset.TorsoGetData(d, "aud.npy", "train", flags, device=dev)
    fr = dataset.ResidentTorsoFrames(d, "aud.npy", "train", flags, device=dev, seed=5)
    assert len(fr) == len(ds) == 3 and fr.counts == (45, 3, 16, 0)
    for i in (0, 2):
        sel = fr.select(i, 3 + i)
        m = fr.maps[i].cpu().numpy()
        assert torch.equal(sel, torch.from_numpy(sampler_reference(m, fr.counts, 5, 3 + i)).to(dev))
        flat = sel.cpu().numpy()
        monkeypatch.setattr(dataset, "torso_select_pixels", lambda *a, **k: np.stack([flat // fr.W, flat % fr.W], 1))
        g_rays, g_rays0, g_tgt, g_bc, g_auds, g_raw, g_pose, g_expr, g_index = ds[i]
        r_rays, r_rays0, r_tgt, r_bc, r_auds, r_raw, r_pose, r_expr, r_index = fr.batch(i, 3 + i)
        assert torch.equal(r_rays, g_rays) and torch.equal(r_rays0, g_rays0)
        assert torch.equal(r_tgt, g_tgt) and torch.equal(r_bc, g_bc.to(torch.float32))
        assert r_rays.shape == (2, 64, 3) and (i == 0) == torch.equal(r_rays, r_rays0)     # frame 0's pose IS the torso pose
        assert torch.equal(r_auds.cpu(), g_auds) and r_index == g_index == i and torch.equal(r_expr.cpu(), g_expr)
        assert torch.equal(r_pose.cpu(), torch.as_tensor(g_pose, dtype=torch.float32)) and torch.equal(r_raw.cpu(), g_raw)
        assert all(t.is_cuda for t in (r_rays, r_rays0, r_tgt, r_bc, r_auds, r_raw, r_pose, r_expr))
    ev = fr.frame(1)
    assert len(ev) == 9 and not ev[6].is_cuda and ev[6].dtype == torch.float64 and ev[3].dtype == torch.float64
    monkeypatch.undo()

    # the reference's own sample_rays: the host path under its numpy seed, and the pair gather on its coordinates, at the
    # bound of test_dataset_sample_rays_golden
    g = golden("torso_sample_rays")
    H, W = g["image"].shape[:2]
    image, background = torch.from_numpy(g["image"]).to(dev), torch.from_numpy(g["background"]).to(dev)
    target = (torch.from_numpy(g["image"]).float() / 255.0).to(dev)       # the reference ran on the CPU: its division, not the device's
    table = idn.ops.byte_tables(dev)[0]
    for case in ("off", "on"):
        np.random.seed(int(g["seed"]))
        out = dataset.torso_sample_rays(g["pose"], g["pose_torso"], g["rect"], target, torch.tensor(g["background"] / 255.0).to(dev),
                                        g["landmark"], H, W, float(g["focal"]), float(g["cx"]), float(g["cy"]), int(g["N_rand"]),
                                        case == "on", float(g["sample_rate"]), dev)
        rc = g[f"coords_{case}"]
        pair = idn.ops.gather_ray_pairs(torch.from_numpy(rc[:, 0] * W + rc[:, 1]).to(dev), g["pose"], g["pose_torso"], H, W,
                                        float(g["focal"]), image, background, float(g["cx"]), float(g["cy"]))
        for rays, rays0, tgt, bc in (out, pair):
            assert hp.rel_err(rays, g[f"batch_rays_{case}"]) < 1e-6 and hp.rel_err(rays0, g[f"batch_rays_torso_{case}"]) < 1e-6
            np.testing.assert_array_equal(bc.cpu().numpy(), g[f"bc_s_{case}"].astype(bc.cpu().numpy().dtype))
        np.testing.assert_array_equal(out[2].cpu().numpy(), g[f"target_s_{case}"])
        # the kernel's targets are the DEVICE's `uint8 -> float / 255.0` of the reference's pixels (ops.byte_tables): the
        # loader's own values on this device, which the first half of this test holds bit for bit
        assert torch.equal(pair[2], table[image[rc[:, 0], rc[:, 1]].long()])
        assert hp.rel_err(pair[2], g[f"target_s_{case}"]) < 1e-6


def test_torso_batch_is_reproducible_and_does_not_synchronise(idn, dev, clip128):
    from idealnerf_amd import dataset
    d, flags, _ = clip128
    fr = dataset.ResidentTorsoFrames(d, "aud.npy", "train", flags, device=dev, seed=9)
    a, b, c = fr.batch(1, 70), fr.batch(1, 70), fr.batch(1, 71)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[2], c[2])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = fr.batch(2, 5)            # raises here if anything inside waits for the device
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out[1], fr.batch(2, 5)[1])


# ------------------------------------------------------------------------------------------------ T5: Adam steps vs the oracle
def test_torso_adam_steps_match_oracle(idn, dev):
    """Three iterations of the torso stage's loop body (train_torso.py:516-541) through ``torso_train_step``: loss trajectory,
    PSNR, learning rate and the updated torso / audio-net weights against the CPU oracle's head + torso render driven by the
    same torch Adam over the same parameter set, under the tolerances of test_train_loop_adam_steps_match_oracle; the head
    pair's weights and the latent codes end bit for bit as they began."""
    from idealnerf_amd import train as T_
    LR = 8e-4
    net, syn, P, (dh, dt), d = hp._torso_setup(idn, dev)      # 48 rays, 64 + 128 samples, perturb = 0
    net.train()
    for m in (net.face_nerf_coarse, net.face_nerf_fine):
        m.requires_grad_(False)
        m.eval()
    head0 = {k: v.detach().clone() for k, v in net.state_dict().items() if k.startswith("face_nerf_")}
    latent_codes = torch.ones(4, 32, device=dev)
    trained = [p for m in (net.torso_coarse_nerf, net.torso_fine_nerf, net.aud_net, net.aud_att_net) for p in m.parameters()]
    opt = torch.optim.Adam(params=trained, lr=LR, betas=(0.9, 0.999))
    # oracle twin on the CPU
    for tag in ("tc", "tf"):
        for v in P[tag].values():
            v.requires_grad_(True)
    aud_net_o = type(net.aud_net)(64, 16)
    aud_net_o.load_state_dict({k: v.detach().cpu() for k, v in net.aud_net.state_dict().items()})
    live = lambda p: [v for k, v in p.items() if not k.startswith("feature_linear")]
    opt_o = torch.optim.Adam(live(P["tc"]) + live(P["tf"]) + list(aud_net_o.parameters()), lr=LR, betas=(0.9, 0.999))
    rec = lambda r: oracle.ray_records(r[0], r[1], NEAR, FAR)
    data = (d["batch_rays"][None], d["batch_rays_torso"][None], d["target"], d["bg"], d["auds"][None], torch.zeros(1, 32, 32, 3),
            d["pose"], d["expr"][None], torch.tensor([1]))
    for step in range(3):
        info = T_.torso_train_step(net, opt, data, latent_codes, step, 4, lrate=LR, lrate_decay=500)
        opt_o.zero_grad()
        aud_f = aud_net_o(d["auds"][1:2])
        head = oracle.render_rays(rec(d["batch_rays"]), d["bg"], P["hc"], P["hf"], aud_f, d["expr"], d["latent"], dims=dh, with_fg=True)
        torso = oracle.render_rays(rec(d["batch_rays_torso"]), d["bg"], P["tc"], P["tf"], oracle.torso_signal(aud_f, d["pose"]), None,
                                   None, dims=dt, with_fg=True)
        com, com0 = oracle.head_torso_composite(head, torso)
        img_o = ((com - d["target"]) ** 2).mean()
        loss_o = img_o + ((com0 - d["target"]) ** 2).mean()
        loss_o.backward()
        opt_o.step()
        lr_o = LR * (0.1 ** (step / (500 * 1500)))
        for gq in opt_o.param_groups:
            gq["lr"] = lr_o
        print(f"step {step}: loss {float(info['loss']):.8f} oracle {float(loss_o):.8f}")
        assert abs(float(info["loss"]) - float(loss_o)) < 2e-4 * abs(float(loss_o)), step
        assert abs(float(info["psnr"]) - float(oracle.mse_to_psnr(img_o.detach()))) < 1e-2
        assert info["lr"] == pytest.approx(lr_o)
        assert set(info) == {"loss", "psnr", "lr"}

    def close(got, want, name):
        # Adam's first steps move every weight by ~lr * sign(g): entries whose gradient is rounding noise around zero can
        # land 2*lr apart, everything else must agree
        diff = (got.detach().cpu() - want.detach()).abs()
        assert float((diff > 1e-4).float().mean()) < 0.02, name
        assert float(diff.median()) < 1e-5, name
        assert float(diff.max()) < 3 * 2 * LR + 1e-6, name
    for name in ("pts_linears.0.weight", "pts_linears.5.weight", "views_linears.0.weight", "alpha_linear.weight", "rgb_linear.bias"):
        close(dict(net.torso_fine_nerf.named_parameters())[name], P["tf"][name], "torso fine " + name)
        close(dict(net.torso_coarse_nerf.named_parameters())[name], P["tc"][name], "torso coarse " + name)
    for (name, prm), (_, ref_p) in zip(net.aud_net.named_parameters(), aud_net_o.named_parameters()):
        close(prm, ref_p, "aud_net " + name)
    for k, v in net.state_dict().items():
        if k.startswith("face_nerf_"):
            assert torch.equal(v, head0[k]), k
    assert torch.equal(latent_codes, torch.ones(4, 32, device=dev))
    assert all(p.grad is None for m in (net.face_nerf_coarse, net.face_nerf_fine) for p in m.parameters())


# ------------------------------------------------------------------------------------------------ T6: the loop
K = 4


def _torso_flags(datadir, basedir, expname, loader_flags, **over):
    from idealnerf_amd import config
    ns = config.load_config(kind="torso", argv=["--datadir", str(datadir), "--basedir", str(basedir), "--expname", expname])
    for k, v in {**vars(loader_flags), **over}.items():
        setattr(ns, k, v)
    return ns


@pytest.fixture(scope="module")
def torso_runs(idn, dev, tmp_path_factory):
    """A 64 x 64 directory (expression width 79, 3 frames, N_rand 64, use_highlight off), a head.tar from two steps of
    train.train on it, and ``mk(name, datadir=, flags=)``: the torso flags of a run directory that already holds that head.tar."""
    from idealnerf_amd import train as T_
    tmp = tmp_path_factory.mktemp("torso_loop")
    d = str(tmp / "clip")
    os.makedirs(d)
    flags, _ = write_clip_directory(d, 64, 3, seed=2, dim_expr=79)
    torch.manual_seed(5)
    T_.train(train_flags(d, tmp / "logs", "head", flags, perturb=0.0, i_print=2, i_weights=1, N_iters=10, chunk=8192, dim_expr=79),
             loader="resident", sample_seed=3, device=dev, steps=2)
    head_tar = str(tmp / "logs" / "head" / "head.tar")
    tflags = SimpleNamespace(gt_dirs=flags.gt_dirs, testskip=1, N_rand=64, sample_rate=0.95, use_highlight=False)

    def mk(name, datadir=d, flags=tflags):
        os.makedirs(str(tmp / "logs" / name), exist_ok=True)
        if not os.path.exists(str(tmp / "logs" / name / "head.tar")):
            shutil.copy(head_tar, str(tmp / "logs" / name / "head.tar"))
        return _torso_flags(datadir, tmp / "logs", name, flags, perturb=0.0, i_print=2, i_weights=K - 1, N_iters=10, chunk=8192)
    return tmp, d, head_tar, mk


def test_torso_train_resume_checkpoint_validation_and_hand_loop(idn, dev, torso_runs):
    from idealnerf_amd import checkpoint, dataset, train as T_, train_torso as TT
    from idealnerf_amd.audio_exp_nerf import init_weights
    from idealnerf_amd.config import to_render_config
    from test_train_loop_gpu import _assert_same_state, _state
    tmp, d, head_tar, mk = torso_runs
    events = []
    torch.manual_seed(11)
    whole = TT.train(mk("whole"), loader="resident", sample_seed=3, device=dev, steps=2 * K,
                     on_log=lambda kind, step, payload: events.append((kind, step, payload)))
    assert whole["global_step"] == 2 * K and whole["data_size"] == 3
    assert [s for k, s, _ in events if k == "train"] == [0, 2, 4, 6]
    assert [s for k, s, _ in events if k == "val"] == [0]
    assert all(set(p) == {"loss", "psnr", "learning_rate"} and np.isfinite(list(p.values())).all() for k, _, p in events if k == "train")
    val = [p for k, _, p in events if k == "val"][0]
    assert val.shape == (3, 128, 64) and torch.isfinite(val).all() and not val.is_cuda
    run_dir = str(tmp / "logs" / "whole")
    assert sorted(f for f in os.listdir(run_dir) if "torso.tar" in f) == ["000000_torso.tar", "000001_torso.tar", "000002_torso.tar"]
    ck = torch.load(os.path.join(run_dir, "000002_torso.tar"), weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer", "latent_codes"} and ck["global_step"] == 7
    head_sd = torch.load(head_tar, weights_only=False)
    n_head = 0
    for k, v in head_sd["model_state_dict"].items():
        if k.startswith("face_nerf_"):
            n_head += 1
            assert torch.equal(ck["model_state_dict"][k].cpu(), v.cpu()), k        # the frozen pair: bit for bit head.tar's
            assert torch.equal(whole["network"].state_dict()[k].cpu(), v.cpu()), k
    assert n_head == sum(k.startswith("face_nerf_") for k in whole["network"].state_dict()) > 0
    assert torch.equal(ck["latent_codes"].cpu(), head_sd["latent_codes"].cpu())
    assert not any(p.requires_grad for m in ("face_nerf_coarse", "face_nerf_fine") for p in getattr(whole["network"], m).parameters())
    assert os.path.exists(os.path.join(run_dir, "args.txt"))

    torch.manual_seed(11)
    first = TT.train(mk("parts"), loader="resident", sample_seed=3, device=dev, steps=K)
    assert first["global_step"] == K
    assert checkpoint.latest_checkpoint(str(tmp / "logs" / "parts"), contains="torso.tar").endswith("000001_torso.tar")
    del first
    torch.manual_seed(999)                       # nothing of the second half may come from anywhere but the two checkpoints
    events2 = []
    second = TT.train(mk("parts"), loader="resident", sample_seed=3, device=dev, steps=K,
                      on_log=lambda kind, step, payload: events2.append((kind, step)))
    assert second["global_step"] == 2 * K and events2 == [("train", 4), ("train", 6)]
    _assert_same_state(_state(whole), _state(second))

    # the same 2 K steps written by hand
    args = mk("hand")
    torch.manual_seed(11)
    frames = dataset.ResidentTorsoFrames(d, "aud.npy", "train", args, device=dev, seed=3)
    cfg = to_render_config(args)
    assert cfg.dim_expr == 79 == frames.exprs.shape[1]
    net = TT.Network(64, 64, frames.focal, near=args.near, far=args.far, chunk=args.chunk, N_samlpes=args.N_samples,
                     N_importance=args.N_importance, args=cfg, dim_aud_body=args.dim_aud_body, dim_expr_head=79).to(dev)
    lat = torch.ones(len(frames), 32, dtype=torch.float32, device=dev)
    net.apply(init_weights)
    opt = torch.optim.Adam([p for m in (net.torso_coarse_nerf, net.torso_fine_nerf, net.aud_net, net.aud_att_net) for p in m.parameters()],
                           lr=args.lrate, betas=(0.9, 0.999))
    _, codes = checkpoint.load_checkpoint(head_tar, net, map_location=dev, strict=False)
    lat.data = codes.to(dev)
    net.train()
    for m in (net.face_nerf_coarse, net.face_nerf_fine):
        m.requires_grad_(False)
    for step in range(2 * K):
        T_.torso_train_step(net, opt, frames.batch(step % len(frames), step), lat, step, len(frames), lrate=args.lrate,
                            lrate_decay=args.lrate_decay)
    _assert_same_state(_state(whole), _state(dict(network=net, optimizer=opt, latent_codes=lat)))


def test_torso_train_loaders_and_validation_variants(idn, dev, torso_runs):
    from idealnerf_amd import train_torso as TT
    tmp, d, head_tar, mk = torso_runs
    events = []
    torch.manual_seed(11)
    run = TT.train(mk("resval"), loader="resident", sample_seed=3, device=dev, steps=1, val="resident",
                   on_log=lambda kind, step, payload: events.append((kind, step, payload)))
    assert run["global_step"] == 1 and [k for k, _, _ in events] == ["train", "val", "val_scores"]
    scores = events[2][2]
    assert np.isfinite(scores["psnr"][0]) and np.isfinite(scores["ssim"][0]) and scores["groups"][0] == "frame"
    assert events[1][2].shape == (3, 128, 64)
    np.random.seed(0)
    torch.manual_seed(11)
    assert TT.train(mk("ref"), loader="reference", device=dev, steps=2)["global_step"] == 2
    # 128 x 128, use_highlight on: the mouth block (a quarter of the batch) with both loaders
    d2 = str(tmp / "clip128")
    if not os.path.isdir(d2):
        os.makedirs(d2)
        write_clip_directory(d2, 128, 3, seed=4, dim_expr=79, face_rect=[8, 8, 60, 60], mouth_range=(30, 38))
    hl = SimpleNamespace(gt_dirs="head_imgs", testskip=1, N_rand=64, sample_rate=0.95, use_highlight=True)
    for loader in ("resident", "reference"):
        np.random.seed(0)
        torch.manual_seed(11)
        run = TT.train(mk("hl_" + loader, datadir=d2, flags=hl), loader=loader, device=dev, steps=2)
        assert run["global_step"] == 2 and all(torch.isfinite(p).all() for p in run["network"].parameters())
    with pytest.raises(ValueError):
        TT.train(mk("ref"), loader="nope", device=dev, steps=1)
