"""The feature-aggregation model (FaceNeRFAgg) on the GPU: gradients through ``Network.render_rays`` against the oracle's
autograd on the reduced parameters (agg_common) and against one training step of the reference itself, the host-side terms of
the backward, the eval plumbing, the frozen plan, Adam steps, the training loop and whole clips."""
import json
import os

import numpy as np
import pytest
import torch

import oracle
import agg_common as ac
import test_hip_parity as hp
from idealnerf_amd.synthetic import write_clip_directory
from train_loop_common import sampler_reference, train_flags

pytestmark = pytest.mark.gpu

NEAR, FAR = ac.NEAR, ac.FAR
PAIR = ("face_nerf_coarse", "face_nerf_fine")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()
    return idealnerf_amd


def _split(module):
    named = list(module.named_parameters())
    return ([(k, p) for k, p in named if not k.startswith("agg_linears")], [(k, p) for k, p in named if k.startswith("agg_linears")])


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("n_rays,ni", [(37, 128), (50, 0)])
def test_agg_render_step_gradients_match_oracle_autograd(idn, dev, n_rays, ni):
    """test_train_step_matches_oracle_autograd_ragged for the agg pair: 37 rays with 64 + 128 samples and 50 rays with
    N_importance = 0, against oracle.render_rays' autograd on the reduced parameters.  That test's bounds: loss 1e-5 relative;
    GRAD_L2_COARSE / GRAD_L2_FINE / GRAD_MAX for the 24 trunk tensors of each network (views_linears.0.weight at its full
    width, feature columns included); GRAD_L2_FINE for d aud, d latent and the agg_linears tensors; feature_linear gets none.

    In the same backward the host-side terms are exact: views_linears.0.weight.grad[:, 283:] == outer(views_linears.0.bias.grad,
    g), both sides in fp64 from the fp32 values, within 1e-6 of the largest entry (each side is one fp32 rounding of the same
    product)."""
    from idealnerf_amd.helper import img2mse
    net, syn = ac.agg_train_net(dev, ni)
    rays, bc, tgt = ac.pick_rays(syn, n_rays, n_rays)
    # oracle autograd on fp32 leaves of the agg parameters
    pc, pf = ac.leaves(net.face_nerf_coarse), ac.leaves(net.face_nerf_fine)
    aud_o, lat_o = syn["aud"].clone().requires_grad_(True), syn["latent"].clone().requires_grad_(True)
    if ni:
        rc, rf, cond, dims = ac.reduced_pair(pc, pf, aud_o, syn["expr"])
    else:
        (rc, cond), rf, dims = ac.reduced(pc, aud_o, syn["expr"]), None, ac.reduced_dims()
    out_o = oracle.render_rays(rays, bc, rc, rf, cond, None, lat_o, n_importance=ni, dims=dims)
    loss_o, _ = oracle.train_loss(out_o, tgt, lat_o)
    loss_o.backward()
    # HIP
    aud, lat = syn["aud"].to(dev).requires_grad_(True), syn["latent"].to(dev).requires_grad_(True)
    expr = syn["expr"].to(dev)
    ret = net.render_rays(rays.to(dev), bc.to(dev), aud, syn["c2w"], lat, expr)
    loss = img2mse(ret["rgb_map"], tgt.to(dev))
    if ni:
        loss = loss + img2mse(ret["rgb0"], tgt.to(dev))
    loss = loss + 10 * (torch.norm(lat) * 0.0005)
    loss.backward()
    e_loss = abs(float(loss) - float(loss_o)) / abs(float(loss_o))
    e_aud, e_lat = hp.l2_err(aud.grad, aud_o.grad), hp.l2_err(lat.grad, lat_o.grad)
    print(f"\nn_rays {n_rays} Ni {ni}: loss {e_loss:.2e}  d aud {e_aud:.2e}  d latent {e_lat:.2e}")
    assert e_loss < 1e-5
    assert e_aud < hp.GRAD_L2_FINE and e_lat < hp.GRAD_L2_FINE
    for module, ref, fine in ((net.face_nerf_coarse, pc, False), (net.face_nerf_fine, pf, True)):
        trunk, agg = _split(module)
        if fine and not ni:
            assert all(p.grad is None for _, p in trunk + agg)
            continue
        assert dict(trunk)["views_linears.0.weight"].grad.shape == (128, ac.N_H + 64)
        hp.check_grads(trunk, ref, fine, n_rays)
        for k, p in agg:
            e = hp.l2_err(p.grad, ref[k].grad)
            print(f"   {'fine' if fine else 'coarse'} {k}: {e:.2e}")
            assert e < hp.GRAD_L2_FINE, (n_rays, k)
        assert dict(trunk)["feature_linear.weight"].grad is None and dict(trunk)["feature_linear.bias"].grad is None
        # exactness of the host terms
        with torch.no_grad():
            g = module.agg_feature(aud.detach(), expr)
        got = dict(trunk)["views_linears.0.weight"].grad[:, ac.N_H:].double()
        want = torch.outer(dict(trunk)["views_linears.0.bias"].grad.double(), g.double())
        e = float((got - want).abs().max() / want.abs().max())
        print(f"   {'fine' if fine else 'coarse'} feature columns vs outer(b', g): {e:.2e}")
        assert e < 1e-6, (n_rays, fine)


def test_agg_train_step_gradients_golden(idn, dev, golden):
    """One training step of the reference's own agg Network (tests/golden/agg_train_step.npz, make_golden_agg.py) at
    test_train_step_gradients_golden's bounds: RGB 1e-4, loss 1e-5 relative, gradients 2e-3 of each tensor's largest entry --
    train_step.npz's tensor selection plus the four agg_linears gradients of each network (every second row of the weight
    gradients with 128 rows or more, which is what fits a committed fixture)."""
    from idealnerf_amd.helper import img2mse
    g, f = golden("agg_train_step"), golden("frame32")
    net, syn = ac.agg_train_net(dev, seeds=(int(g["seed_coarse"]), int(g["seed_fine"])))
    sel = hp.T(g["sel"])
    rays = hp.T(f["rays"])[sel].contiguous().to(dev)
    bc = syn["bc"].reshape(-1, 3)[sel].contiguous().to(dev)
    aud, lat = syn["aud"].to(dev).requires_grad_(True), syn["latent"].to(dev).requires_grad_(True)
    tgt = hp.T(g["target"]).to(dev)
    ret = net.render_rays(rays, bc, aud, syn["c2w"], lat, syn["expr"].to(dev))
    e_rgb, e_rgb0 = hp.rel_err(ret["rgb_map"], g["rgb_map"]), hp.rel_err(ret["rgb0"], g["rgb0"])
    loss = img2mse(ret["rgb_map"], tgt) + img2mse(ret["rgb0"], tgt) + 10 * (torch.norm(lat) * 0.0005)
    loss.backward()
    e_loss = abs(float(loss) - float(g["loss"])) / abs(float(g["loss"]))
    errs = {"aud": hp.rel_err(aud.grad, g["g_aud"]), "latent": hp.rel_err(lat.grad, g["g_latent"])}
    for tag, m in (("c", net.face_nerf_coarse), ("f", net.face_nerf_fine)):
        named = dict(m.named_parameters())
        for key in g:
            if key.startswith(f"g_{tag}_"):
                grad = named[key[4:]].grad
                rows = grad[::int(g["row_step"])] if grad.dim() == 2 and grad.shape[0] >= 128 else grad   # as the fixture stores them
                errs[f"{tag}.{key[4:]}"] = hp.rel_err(rows, g[key])
        assert named["feature_linear.weight"].grad is None
    assert sum(k.split(".", 1)[1].startswith("agg_linears") for k in errs if "." in k) == 8
    print(f"\nrgb {e_rgb:.1e} rgb0 {e_rgb0:.1e} loss {e_loss:.1e}; gradient errors (max abs / max |ref|):",
          {k: f"{v:.1e}" for k, v in errs.items()})
    assert e_rgb < hp.RGB_TOL and e_rgb0 < hp.RGB_TOL and e_loss < 1e-5
    bad = {k: v for k, v in errs.items() if not v < 2e-3}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ plumbing
def test_agg_eval_forward_equals_a_head_network_on_the_reduced_parameters(idn, dev):
    """Eval-mode ``Network.forward`` of the agg network on a 32 x 32 frame, bit for bit against an ``audio_exp_nerf.Network``
    that carries the reduced FaceNeRF parameters and is handed g computed the same way (on the device, by the same
    expressions).  One head Network takes one audio vector for both of its networks, so it is built with dim_aud = 128 and
    given cat(g_coarse, g_fine), each network with zero columns under the other's feature: the fold adds exact zeros in the
    same lane order.  And inside the project's fixed RGB budget (1e-4) of oracle.render_rays on the reduced parameters: rgb0
    plainly, rgb_map by parity_proof.prove_render (see below).  Measured on this scene: rgb0 8.1e-7; rgb_map end to end 7.0e-4 on
    the worst of the 1024 rays."""
    from idealnerf_amd.audio_exp_nerf import Network as HeadNetwork
    from idealnerf_amd.helper import RenderConfig
    net, syn = ac.agg_train_net(dev)
    net.eval()
    rs = np.random.RandomState(5)
    auds = hp.T(rs.standard_normal((4, 16, 29)).astype(np.float32))
    pose = torch.cat([syn["c2w"], torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
    bg = syn["bc"]
    index, lat = 2, syn["latent"]
    x = (torch.empty(0), torch.empty(0), bg[None], auds[None], torch.zeros(1, 32, 32, 3), pose[None], syn["expr"][None], lat, torch.tensor([index]))
    with torch.no_grad():
        rgb, disp, acc, last_w, extras = net([x, 0, 4])
        assert rgb.shape == (32, 32, 3)
        # the same conditioning, by the same expressions on the device
        expr = syn["expr"].to(dev)
        aud_feature = net.aud_net(auds[index].to(dev).unsqueeze(0))
        cfg = RenderConfig(perturb=0.0, chunk=512, near=NEAR, far=FAR, dim_aud=128, dim_expr=0)
        head = HeadNetwork(32, 32, syn["focal"], NEAR, FAR, 512, None, 64, 128, args=cfg).to(dev).eval()
        feats = []
        for k, (src, dst) in enumerate(zip((net.face_nerf_coarse, net.face_nerf_fine), (head.face_nerf_coarse, head.face_nerf_fine))):
            g = src.agg_feature(aud_feature, expr)
            feats.append(g)
            sd = {key: v.clone() for key, v in src.state_dict().items() if not key.startswith("agg_linears")}
            v0 = src.views_linears[0]
            sd["views_linears.0.weight"] = v0.weight[:, :ac.N_H].contiguous()
            sd["views_linears.0.bias"] = (v0.bias + v0.weight[:, ac.N_H:] @ g).contiguous()
            zeros = torch.zeros(256, 64, device=dev)
            for layer in (0, 5):
                W = sd[f"pts_linears.{layer}.weight"]
                own = W[:, 63:127]
                sd[f"pts_linears.{layer}.weight"] = torch.cat([W[:, :63], *((own, zeros) if k == 0 else (zeros, own)), W[:, 127:]], 1)
            dst.load_state_dict(sd)
        h_rgb, h_disp, h_acc, h_last, h_extras = head.render_dynamic_face(
            H=32, W=32, focal=head.focal, expr=None, poses=pose.to(dev), latent_code=lat.to(dev), render_poses=pose[:3, :4], chunk=512,
            near=NEAR, far=FAR, rays=None, bc_rgb=bg.to(dev), aud_para=torch.cat(feats))
    assert torch.equal(rgb, h_rgb) and torch.equal(disp, h_disp) and torch.equal(acc, h_acc) and torch.equal(last_w, h_last)
    assert extras.keys() == h_extras.keys() and all(torch.equal(extras[k], h_extras[k]) for k in extras)
    # the oracle on the reduced parameters, conditioning from the CPU copy of the audio net's output.  The scene is sharp (both
    # volumes are occupied), so rgb_map is judged the way every run-time oracle comparison on a sharp scene is
    # (tests/parity_proof.py): the fixed 1e-4 for the fine pass on given sample positions -- the oracle's and this render's --
    # and for every ray whose positions equal the oracle's, the sampling stage bit-exact on this render's coarse weights, no
    # ray beyond E2E_CAP.  The taps come from render_rays on the frame's ray records, which must be the frame itself.
    with torch.no_grad():
        rec = idn.ops.frame_rays(syn["c2w"], 32, 32, syn["focal"], NEAR, FAR, device=dev)
        bc_dev = bg.reshape(-1, 3).to(dev)
        taps = net.render_rays(rec, bc_dev, aud_feature, pose.to(dev), lat.to(dev), expr, taps=True)
        assert torch.equal(taps["rgb_map"], rgb.reshape(-1, 3)) and torch.equal(taps["rgb0"], extras["rgb0"].reshape(-1, 3))
        pc = {k: v.detach().cpu() for k, v in net.face_nerf_coarse.state_dict().items()}
        pf = {k: v.detach().cpu() for k, v in net.face_nerf_fine.state_dict().items()}
        rc, rf, cond, dims = ac.reduced_pair(pc, pf, aud_feature.cpu(), syn["expr"])
        ref = oracle.render_rays(rec.cpu(), bg.reshape(-1, 3), rc, rf, cond, None, lat, dims=dims, taps=True)
        fine = net.face_nerf_fine
        hp.prove_render(idn, "agg eval frame", taps, ref, fine.packed_weights(), fine.folded_bias(aud_feature, expr, lat.to(dev)), rec,
                        bc_dev, lambda z: hp.oracle_fine_pass(rf, dims, rec, bc_dev, cond, None, lat, z), hp.FLIP_TOL_SHARP,
                        precision_fine=fine.prec_code)
    e0 = hp.rel_err(extras["rgb0"].reshape(-1, 3), ref["rgb0"])
    print(f"agg eval frame vs oracle on the reduced parameters: rgb0 {e0:.2e}")
    assert e0 < hp.RGB_TOL                                          # the coarse composite has no sampling before it


# ------------------------------------------------------------------------------------------------ frozen plan
def _fp64_frozen_d_aud(module, acts, raw, z, rec, bc, g_rgb, aud, expr, dev):
    """d aud of one frozen agg pass in fp64 on the SAME saved activations (the construction of
    test_torso_train_gpu._fp64_d_cond): the delta chain on the reduced weights -> d g through pts_linears.0 / .5 and, from the
    column sums of views_linears.0's deltas, through the feature columns of views_linears.0 -> d aud through agg_linears."""
    n, S = z.shape
    Pn = n * S
    Pp = (Pn + 127) // 128 * 128
    mat = lambda o, w: acts[o * Pp:(o + w) * Pp].view(Pp, w)[:Pn].double()
    a = [mat(128 + 256 * i, 256) for i in range(8)]
    v = [mat(128 + 2048 + 128 * i, 128) for i in range(3)]
    raw64 = raw.double().cpu().requires_grad_(True)
    comp = oracle.composite(raw64, z.double().cpu(), rec[:, 3:6].double().cpu(), bc.double().cpu())
    (comp[0] * g_rgb.double().cpu()).sum().backward()
    d_raw = raw64.grad.to(dev).view(Pn, 4)
    sd = {k: p.detach().double() for k, p in module.named_parameters()}
    dl = (d_raw[:, :3] @ sd["rgb_linear.weight"]) * (v[2] > 0)
    for i in (2, 1):
        dl = (dl @ sd[f"views_linears.{i}.weight"]) * (v[i - 1] > 0)
    W0 = sd["views_linears.0.weight"]
    d_g = W0[:, ac.N_H:].t() @ dl.sum(0)
    dh = (dl @ W0[:, :256] + d_raw[:, 3:4] @ sd["alpha_linear.weight"]) * (a[7] > 0)
    for l in range(7, 0, -1):
        W = sd[f"pts_linears.{l}.weight"]
        if l == 5:
            d_g = d_g + (dh @ W[:, 63:127]).sum(0)
            W = W[:, 63 + 96:]
        dh = (dh @ W) * (a[l - 1] > 0)
    d_g = d_g + (dh @ sd["pts_linears.0.weight"][:, 63:127]).sum(0)
    return (sd["agg_linears.1.weight"] @ sd["agg_linears.0.weight"][:, :aud.numel()]).t() @ d_g


def _frozen_backward(idn, dev, monkeypatch):
    """The agg pair frozen (agg_linears included), aud requiring a gradient: one render + backward on 48 rays with the calls
    of ops.pass_bwd / ops.pass_bwd_cond counted and each pass's saved activations kept.  -> (calls, d aud, fp64 d aud)."""
    from idealnerf_amd import autograd as ag
    from idealnerf_amd.helper import img2mse
    ops = idn.ops
    net, syn = ac.agg_train_net(dev)
    for m in PAIR:
        getattr(net, m).requires_grad_(False)
    rays, bc, tgt = ac.pick_rays(syn, 48, 48)
    rays, bc, tgt = rays.to(dev), bc.to(dev), tgt.to(dev)
    calls, saved = [], []
    real_full, real_cond, real_query = ops.pass_bwd, ops.pass_bwd_cond, ag._train_query
    monkeypatch.setattr(ops, "pass_bwd", lambda p, *a: (calls.append("full"), real_full(p, *a))[1])
    monkeypatch.setattr(ops, "pass_bwd_cond", lambda p, *a: (calls.append("cond"), real_cond(p, *a))[1])

    def query(module, folded, r, z):
        out = real_query(module, folded, r, z)
        saved.append((module, z, *out))
        return out
    monkeypatch.setattr(ag, "_train_query", query)
    aud = syn["aud"].to(dev).requires_grad_(True)
    expr, lat = syn["expr"].to(dev), syn["latent"].to(dev)
    ret = net.render_rays(rays, bc, aud, syn["c2w"], lat, expr)
    (img2mse(ret["rgb_map"], tgt) + img2mse(ret["rgb0"], tgt)).backward()
    assert all(p.grad is None for m in PAIR for p in getattr(net, m).parameters())
    want = torch.zeros(64, dtype=torch.float64, device=dev)
    for (module, z, raw, acts), rgb in zip(saved, (ret["rgb0"], ret["rgb_map"])):
        g_rgb = (2.0 * (rgb.detach().double() - tgt.double()) / rgb.numel())
        want += _fp64_frozen_d_aud(module, acts, raw, z, rays, bc, g_rgb, aud, expr, dev)
    return calls, aud.grad, want


def test_agg_frozen_pair_d_aud_vs_fp64(idn, dev, monkeypatch):
    """With the agg pair's parameters not requiring gradients and aud requiring one, d aud against the fp64 chain on the same
    saved activations, under test_pass_bwd_cond_vs_fp64's bound (rel_err < 5e-6)."""
    calls, d_aud, want = _frozen_backward(idn, dev, monkeypatch)
    e = hp.rel_err(d_aud, want)
    print(f"\nfrozen agg pair: d aud vs fp64 {e:.2e}; backward calls {calls}")
    assert e < 5e-6


def test_agg_frozen_pair_launches_no_weight_gradient_product(idn, dev, monkeypatch):
    """The same backward launches no weight-gradient product: both passes run the conditioning-only plan.  (d g has a share
    through the feature columns of views_linears.0, W0[:, 283:]^T b'; b' comes from the deltas that plan leaves behind,
    ops.pass_bwd_cond(d_views0_bias=).)"""
    calls, _, _ = _frozen_backward(idn, dev, monkeypatch)
    assert calls == ["cond", "cond"], calls


def test_agg_frozen_pair_without_conditioning_gradients_launches_nothing(idn, dev, monkeypatch):
    """Nothing of the pair and neither aud nor latent needs a gradient: no backward call at all; latent alone: the
    conditioning-only plan (the latent code does not reach the colour branch)."""
    from idealnerf_amd.helper import img2mse
    ops = idn.ops
    net, syn = ac.agg_train_net(dev)
    for m in PAIR:
        getattr(net, m).requires_grad_(False)
    calls = []
    real_full, real_cond = ops.pass_bwd, ops.pass_bwd_cond
    monkeypatch.setattr(ops, "pass_bwd", lambda p, *a: (calls.append("full"), real_full(p, *a))[1])
    monkeypatch.setattr(ops, "pass_bwd_cond", lambda p, *a: (calls.append("cond"), real_cond(p, *a))[1])
    rays, bc, tgt = (t.to(dev) for t in ac.pick_rays(syn, 48, 48))
    lat = syn["latent"].to(dev).requires_grad_(True)
    ret = net.render_rays(rays, bc, syn["aud"].to(dev), syn["c2w"], lat, syn["expr"].to(dev))
    (img2mse(ret["rgb_map"], tgt) + img2mse(ret["rgb0"], tgt)).backward()
    assert calls == ["cond", "cond"] and torch.isfinite(lat.grad).all() and float(lat.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ Adam
def test_agg_adam_steps_match_oracle(idn, dev):
    """Three iterations of the loop body through ``train.train_step`` on the agg network against the CPU oracle on the reduced
    parameters driven by the same torch Adam, under test_torso_adam_steps_match_oracle's tolerances; agg_linears included."""
    from idealnerf_amd import train as T_
    LR = 8e-4
    net, syn = ac.agg_train_net(dev)
    rs = np.random.RandomState(3)
    n = 96
    ro, rd = oracle.camera_rays(32, 32, syn["focal"], syn["c2w"])
    sel = hp.T(rs.choice(1024, size=n, replace=False))
    batch_rays = torch.stack([ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]], 0)
    bg = syn["bc"].reshape(-1, 3)[sel].contiguous()
    tgt = hp.T(rs.uniform(0, 1, size=(n, 3)).astype(np.float32))
    auds = hp.T(rs.standard_normal((4, 16, 29)).astype(np.float32))
    pose = torch.cat([syn["c2w"], torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
    latent_codes = torch.ones(4, 32, device=dev, requires_grad=True)
    pc, pf = ac.leaves(net.face_nerf_coarse), ac.leaves(net.face_nerf_fine)
    aud_net_o = type(net.aud_net)(64, 16)
    aud_net_o.load_state_dict({k: v.detach().cpu() for k, v in net.aud_net.state_dict().items()})
    lat_o = torch.ones(4, 32, requires_grad=True)
    live = lambda p: [v for k, v in p.items() if not k.startswith("feature_linear")]
    opt_o = torch.optim.Adam(live(pc) + live(pf) + list(aud_net_o.parameters()) + [lat_o], lr=LR, betas=(0.9, 0.999))
    opt = T_.make_optimizer(net, latent_codes, lrate=LR)
    rays_rec = oracle.ray_records(batch_rays[0], batch_rays[1], NEAR, FAR)
    data = (batch_rays[None], tgt, bg, auds[None], torch.zeros(1, 32, 32, 3), pose, syn["expr"][None], torch.tensor([2]))
    for step in range(3):
        info = T_.train_step(net, opt, data, latent_codes, step, 4, lrate=LR, lrate_decay=500)
        opt_o.zero_grad()
        rc, rf, cond, dims = ac.reduced_pair(pc, pf, aud_net_o(auds[2:3]), syn["expr"])
        out = oracle.render_rays(rays_rec, bg, rc, rf, cond, None, lat_o[2], dims=dims)
        loss_o, img_o = oracle.train_loss(out, tgt, lat_o[2])
        loss_o.backward()
        opt_o.step()
        lr_o = LR * (0.1 ** (step / (500 * 1500)))
        for gq in opt_o.param_groups:
            gq["lr"] = lr_o
        print(f"step {step}: loss {float(info['loss']):.8f} oracle {float(loss_o):.8f}")
        assert abs(float(info["loss"]) - float(loss_o)) < 2e-4 * abs(float(loss_o)), step
        assert abs(float(info["psnr"]) - float(oracle.mse_to_psnr(img_o.detach()))) < 1e-2
        assert info["lr"] == pytest.approx(lr_o)

    def close(got, want, name):
        diff = (got.detach().cpu() - want.detach()).abs()
        assert float((diff > 1e-4).float().mean()) < 0.02, name
        assert float(diff.median()) < 1e-5, name
        assert float(diff.max()) < 3 * 2 * LR + 1e-6, name
    for name in ("pts_linears.0.weight", "pts_linears.5.weight", "views_linears.0.weight", "alpha_linear.weight", "rgb_linear.bias",
                 "agg_linears.0.weight", "agg_linears.0.bias", "agg_linears.1.weight", "agg_linears.1.bias"):
        close(dict(net.face_nerf_fine.named_parameters())[name], pf[name], "fine " + name)
        close(dict(net.face_nerf_coarse.named_parameters())[name], pc[name], "coarse " + name)
    for (name, prm), (_, ref_p) in zip(net.aud_net.named_parameters(), aud_net_o.named_parameters()):
        close(prm, ref_p, "aud_net " + name)
    assert hp.abs_err(latent_codes[2], lat_o[2]) < 2e-4
    assert torch.equal(latent_codes[0].detach().cpu(), torch.ones(32))
    assert dict(net.face_nerf_fine.named_parameters())["feature_linear.weight"].grad is None


# ------------------------------------------------------------------------------------------------ the loop
K = 4


def _agg_flags(datadir, basedir, expname, loader_flags, **over):
    ns = train_flags(datadir, basedir, expname, loader_flags, **over)
    ns.use_highlight = getattr(loader_flags, "use_highlight", True)
    return ns


@pytest.fixture(scope="module")
def flat_clip(tmp_path_factory):
    """The flat two-colour 64 x 64 clip the head loop's learning test uses (5 frames, seed 6, N_rand 256; three frames train,
    two are held out), with 79-wide expressions and the geometry the highlight recipe can draw from (agg_common.RECT64)."""
    tmp = tmp_path_factory.mktemp("agg_loop")
    d = str(tmp / "flat")
    os.makedirs(d)
    flags, meta = write_clip_directory(d, 64, 5, seed=6, flat=True, N_rand=256, dim_expr=79, face_rect=ac.RECT64,
                                       mouth_range=ac.MOUTH64)
    flags.use_highlight = True
    json.dump(dict(meta, frames=meta["frames"][:3]), open(os.path.join(d, "transforms_exp_train.json"), "w"))
    json.dump(dict(meta, frames=meta["frames"][3:]), open(os.path.join(d, "transforms_exp_val.json"), "w"))
    return tmp, d, flags, meta


def test_resident_agg_frames_against_agg_getdata(idn, dev, flat_clip, monkeypatch):
    """The resident loader's batches against AggGetData on one directory: its draw is the sampler's definition on the torso
    recipe's byte map (the populations torso_select_pixels draws from, counts rect / outside / mouth = 182 / 10 / 64), and
    AggGetData fed those very pixels returns the same 8-tuple bit for bit; frame() is the eval 8-tuple."""
    from idealnerf_amd import dataset
    tmp, d, flags, meta = flat_clip
    ds = dataset.AggGetData(d, "aud.npy", "train", flags, device=dev)
    fr = dataset.ResidentAggFrames(d, "aud.npy", "train", flags, device=dev, seed=5)
    assert len(fr) == len(ds) == 3 and fr.counts == (182, 10, 64, 0)
    for i in (0, 2):
        lm = np.loadtxt(ds.all_landmarks[i])
        m = dataset.torso_region_byte_map(64, 64, ds.all_face_rects[i], lm)
        assert np.array_equal(fr.maps[i].cpu().numpy(), m)
        coords, mouth_w, rect_w, drawn, M = dataset.torso_region_masks(64, 64, ds.all_face_rects[i], lm)
        assert fr.populations[i].tolist() == [int((rect_w & ~mouth_w).sum()), int((~rect_w).sum()), min(M, int((~rect_w).sum())), 0]
        sel = fr.select(i, 3 + i)
        assert torch.equal(sel, torch.from_numpy(sampler_reference(m, fr.counts, 5, 3 + i)).to(dev))
        flat = sel.cpu().numpy()
        monkeypatch.setattr(dataset, "torso_select_pixels", lambda *a, **k: np.stack([flat // fr.W, flat % fr.W], 1))
        g_item, r_item = ds[i], fr.batch(i, 3 + i)
        assert len(g_item) == len(r_item) == 8
        g_rays, g_tgt, g_bc, g_auds, g_raw, g_pose, g_expr, g_index = g_item
        r_rays, r_tgt, r_bc, r_auds, r_raw, r_pose, r_expr, r_index = r_item
        assert r_rays.shape == (2, 256, 3) and torch.equal(r_rays, g_rays)
        assert torch.equal(r_tgt, g_tgt) and torch.equal(r_bc, g_bc.to(torch.float32))
        assert torch.equal(r_auds.cpu(), g_auds) and r_index == g_index == i and torch.equal(r_expr.cpu(), g_expr)
        assert torch.equal(r_pose.cpu(), torch.as_tensor(g_pose, dtype=torch.float32)) and torch.equal(r_raw.cpu(), g_raw)   # RGB bytes
        assert all(t.is_cuda for t in (r_rays, r_tgt, r_bc, r_auds, r_raw, r_pose, r_expr))
    ev = fr.frame(1)
    assert len(ev) == 8 and ev[0].numel() == 0 and not ev[5].is_cuda and ev[5].dtype == torch.float64 and ev[2].dtype == torch.float64


def test_agg_train_resume_validation_and_learning(idn, dev, flat_clip):
    """train_agg.train on the flat clip, perturb 0, resident loader.  2 K steps == K steps, then new objects under another
    torch seed and K steps resumed from {epoch:06d}_head.tar, bit for bit (weights, latent codes, optimizer state); the
    checkpoints carry the reference's four keys and the completed step count; the validation image is RGB over RGB: its lower
    half is the held-out frame's bytes / 255 unflipped.  Then 240 steps at N_rand 256 (the head loop's learning run): the mean
    loss of the last ten steps is below that of the first ten."""
    from PIL import Image
    from idealnerf_amd import checkpoint, train_agg
    from idealnerf_amd.agg_aud_exp_nerf import Network
    from test_train_loop_gpu import _assert_same_state, _state
    tmp, d, flags, meta = flat_clip
    small = type(flags)(**{**vars(flags), "N_rand": 64})
    mk = lambda name, fl=small, **over: _agg_flags(d, tmp / "logs", name, fl, **{**dict(perturb=0.0, i_print=2, i_weights=K - 1, N_iters=10,
                                                                                          chunk=8192, dim_expr=79), **over})
    events = []
    torch.manual_seed(11)
    whole = train_agg.train(mk("whole"), loader="resident", sample_seed=3, device=dev, steps=2 * K,
                            on_log=lambda kind, step, payload: events.append((kind, step, payload)))
    assert isinstance(whole["network"], Network) and whole["global_step"] == 2 * K and whole["data_size"] == 3
    assert [s for k, s, _ in events if k == "train"] == [0, 2, 4, 6] and [s for k, s, _ in events if k == "val"] == [0]
    run_dir = str(tmp / "logs" / "whole")
    assert sorted(f for f in os.listdir(run_dir) if f.endswith(".tar")) == ["000000_head.tar", "000001_head.tar", "000002_head.tar"]
    ck = torch.load(os.path.join(run_dir, "000002_head.tar"), weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer", "latent_codes"} and ck["global_step"] == 7
    assert any(k.startswith("face_nerf_coarse.agg_linears.") for k in ck["model_state_dict"])
    assert not any(k.startswith("ds_aud_net.") for k in ck["model_state_dict"])
    val = [p for k, _, p in events if k == "val"][0]
    assert val.shape == (3, 128, 64) and torch.isfinite(val).all() and not val.is_cuda
    held = [torch.from_numpy(np.asarray(Image.open(os.path.join(d, "head_imgs", f"{f['img_id']}.jpg"))).copy()).permute(2, 0, 1) / 255.0
            for f in meta["frames"][3:]]
    assert any(torch.equal(val[:, 64:], h) for h in held)                       # RGB over RGB: no channel flip
    assert not any(torch.equal(val[:, 64:], h[[2, 1, 0]]) for h in held)

    torch.manual_seed(11)
    first = train_agg.train(mk("parts"), loader="resident", sample_seed=3, device=dev, steps=K)
    assert first["global_step"] == K
    assert checkpoint.latest_checkpoint(str(tmp / "logs" / "parts")).endswith("000001_head.tar")
    del first
    torch.manual_seed(999)                       # nothing of the second half may come from anywhere but the checkpoint
    second = train_agg.train(mk("parts"), loader="resident", sample_seed=3, device=dev, steps=K)
    assert second["global_step"] == 2 * K
    _assert_same_state(_state(whole), _state(second))

    # the reference loader drives the same loop (upstream's numpy draw sequence), with the resident validation clip
    np.random.seed(0)
    torch.manual_seed(11)
    ev2 = []
    ref = train_agg.train(mk("ref"), loader="reference", device=dev, steps=2, val="resident",
                          on_log=lambda kind, step, payload: ev2.append(kind))
    assert ref["global_step"] == 2 and ev2 == ["train", "val", "val_scores"]

    losses = []
    torch.manual_seed(0)
    train_agg.train(mk("learn", fl=flags, i_print=10 ** 6, i_weights=10 ** 6, N_iters=10 ** 4), loader="resident", sample_seed=0,
                    device=dev, steps=240, on_step=lambda step, info: losses.append(info["loss"]))
    losses = torch.stack(losses).cpu()
    first10, last10 = float(losses[:10].mean()), float(losses[-10:].mean())
    print(f"\nagg loop, 240 steps: mean loss of the first ten steps {first10:.5f}, of the last ten {last10:.5f}")
    assert torch.isfinite(losses).all() and last10 < first10


# ------------------------------------------------------------------------------------------------ clips
def test_agg_clips_render_and_score(idn, dev, tmp_path):
    """A 3-frame 40 x 40 clip (tests/drive_common.py's shape and sample counts): clip.render_head_clip with the agg network
    equals frame-by-frame ``forward`` byte for byte, clip.score_head_clip returns finite scores for it, and
    drive.drive_head(model="agg") renders the newest checkpoint of a run directory.  (The mouth landmarks sit in a corner, so
    that the face rect keeps pixels outside the mouth box for the loader's draw.)"""
    import drive_common as dc
    from idealnerf_amd import clip, dataset, synthetic
    from idealnerf_amd.agg_aud_exp_nerf import Network, init_weights
    from idealnerf_amd.helper import RenderConfig
    d = str(tmp_path / "clip")
    os.makedirs(d)
    flags, meta = write_clip_directory(d, dc.SIZE, 3, seed=dc.SEED, dim_expr=79, face_rect=[1, 1, 24, 24], mouth_range=(36, 39))
    flags.use_highlight, flags.N_rand = False, 16
    cfg = RenderConfig(perturb=0.0, chunk=8192, near=synthetic.NEAR, far=synthetic.FAR, dim_aud=64, dim_expr=79,
                       N_samples=dc.N_SAMPLES, N_importance=dc.N_IMPORTANCE)
    torch.manual_seed(5)
    net = Network(dc.SIZE, dc.SIZE, meta["focal_len"], cfg.near, cfg.far, cfg.chunk, None, dc.N_SAMPLES, dc.N_IMPORTANCE, args=cfg)
    net.apply(init_weights)
    synthetic.xavier_state_dict(net.face_nerf_coarse, 2, 300.0, 0.3)
    synthetic.xavier_state_dict(net.face_nerf_fine, 3, 300.0, 0.3)
    net = net.to(dev).eval()
    latent = torch.from_numpy(np.random.RandomState(7).standard_normal(32).astype(np.float32))
    val = dataset.AggGetData(d, "aud.npy", "val", flags, skip=1, device=dev)
    out = str(tmp_path / "agg.avi")
    res = clip.render_head_clip(net, val, out, 0, latent_code=latent, codec="raw")
    assert res["n_frames"] == 3 and res["nonfinite_frames"] == []
    info, frames = dc.decode_raw(out)
    assert len(frames) == 3
    with torch.no_grad():
        for j in range(3):
            item = val[j]
            x = (*(t[None] if torch.is_tensor(t) else torch.as_tensor(t)[None] for t in item[:7]), latent, torch.tensor([item[7]]))
            rgb = net([x, 0, val.data_size])[0]
            assert np.array_equal(idn.ops.to8b(rgb).cpu().numpy(), frames[j]), j
    fr = dataset.ResidentAggFrames(d, "aud.npy", "val", flags, device=dev)
    scores = clip.score_head_clip(net, fr, 0, latent_code=latent, frame_ids=range(3))
    assert np.isfinite(np.asarray(scores["mean"]["psnr"])[0]) and np.isfinite(np.asarray(scores["mean"]["ssim"])[0])
    assert np.isfinite(np.asarray(scores["per_frame"]["psnr"])[:, 0]).all()

    # drive.drive_head(model="agg"): the newest {epoch:06d}_head.tar of the run directory on the driving loader's track (the
    # clip's own val file as the expression track), byte for byte the network's forward on that loader
    from idealnerf_amd import checkpoint, config, drive
    run = tmp_path / "logs" / "run"
    codes = torch.from_numpy(np.random.RandomState(8).standard_normal((3, 32)).astype(np.float32))
    for epoch, scale in ((2, 0.5), (10, 1.0)):       # 000010 is the newest in natural order; 000002 holds other latent codes
        checkpoint.save_checkpoint(str(run / f"{epoch:06d}_head.tar"), net, None, codes * scale, 7)
    ns = config.load_config(kind="agg", argv=[
        "--datadir", d, "--basedir", str(tmp_path / "logs"), "--expname", "run", "--save_path", str(tmp_path / "out"), "--evalExpr_path",
        os.path.join(d, "transforms_exp_val.json"), "--testskip", "1", "--N_samples", str(dc.N_SAMPLES), "--N_importance",
        str(dc.N_IMPORTANCE), "--perturb", "0", "--chunk", "8192", "--near", repr(synthetic.NEAR), "--far", repr(synthetic.FAR),
        "--dim_aud", "64", "--aud_file", "aud.npy"])
    driven = str(tmp_path / "driven.avi")
    res = drive.drive_head(ns, out=driven, device=dev, codec="raw", still_every=0, model="agg")
    assert res["n_frames"] == 3 and res["nonfinite_frames"] == [] and res["path"] == driven
    track = dataset.DrivingFrames(d, "aud.npy", "val", ns, skip=1, device=dev)
    _, driven_frames = dc.decode_raw(driven)
    with torch.no_grad():
        for j in range(3):
            item = track[j]
            x = (*(t[None] if torch.is_tensor(t) else torch.as_tensor(t)[None] for t in item[:7]), codes[0], torch.tensor([item[7]]))
            assert np.array_equal(idn.ops.to8b(net([x, 0, track.data_size])[0]).cpu().numpy(), driven_frames[j]), j
    with pytest.raises(ValueError, match="dim_expr is 0"):
        drive.drive_head(ns, out=driven, device=dev, codec="raw", still_every=0, model="head")   # the head network of these flags takes no expression
