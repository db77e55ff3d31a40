"""Networks whose encoding widths are not 10 / 4 octaves (``--multires``, ``--multires_views``, ``--i_embed``), on the GPU
(run with ``-m gpu``).  The width pairs and the oracle's width-aware query: tests/multires_common.py.

1  exact zero-column equivalence: a narrow network and the 10 / 4 network that holds its weights with zeros in the added
   columns give the same bits -- in every precision, through the kernel sequence, the fused march and pts mode.  No tolerance:
   it pins the packers, the fold and every column offset.
2  x mode against the reference's own FaceNeRF outputs (tests/golden/multires.npz), in each precision at the tolerance
   tests/test_hip_parity.py holds that precision to at 10 / 4.
3  the reference's shipped ablation config by name against the oracle (tests/parity_proof.py) and against the reference's own
   16-ray render.
4  FaceNeRF.forward gradients, 5  a train step through render_rays, 6  ray gradients: against the fp64 oracle, at the bounds
   the 10 / 4 tests state.
7  the loops: train / resume, the torso and the agg trainer, drive_head from the narrow checkpoint.

$IDN_MULTIRES_RECORD names a JSON file the measured figures are merged into (profiles/multires.json)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle
import multires_common as mc
import ray_grad_common as rg
from parity_proof import RGB_TOL, W_TOL, flipped_rows, oracle_fine_pass, prove_render
from test_facenerf_autograd_gpu import GRAD_FLOOR_MULT, _check, _hip_grads, _off_kinks, _oracle_grads
from test_ray_grad_gpu import FACTOR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREC = {"f32": 0, "bf16x3": 1, "bf16": 2, "fp16x3": 3, "bf16x6": 4}
COND = dict(dim_aud=64, dim_expr=76, dim_latent=32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()
    return idealnerf_amd


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_err(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def abs_err(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return np.abs(a - b).max()


def scale_sigma(p, gain=300.0, bias=0.3):
    p = {k: v.clone() for k, v in p.items()}
    p["alpha_linear.weight"] = p["alpha_linear.weight"] * gain
    p["alpha_linear.bias"] = torch.full_like(p["alpha_linear.bias"], bias)
    return p


def _record(key, value):
    path = os.environ.get("IDN_MULTIRES_RECORD")
    if not path:
        return
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(old, open(path, "w"), indent=1, sort_keys=True)


def device_net(idn, params, dims, dev):
    """(pack(precision) -> weight stream, fold(aud, expr, latent) -> bias block) of oracle-style params at ``dims``' widths."""
    sd = {k: v.to(dev).contiguous() for k, v in params.items()}
    ps = idn.ops.params_struct(sd, dims["dim_aud"], dims["dim_expr"], dims["dim_latent"], pts_ch=dims["input_ch"],
                               views_ch=dims["input_ch_views"])
    g = lambda t: None if t is None else t.to(dev).contiguous()
    pack = lambda precision=0: idn.ops.pack_weights(ps, dev, precision)
    fold = lambda aud, expr, latent: idn.ops.fold_conditioning(ps, g(aud), g(expr), g(latent), dev)
    fold.keep = sd
    return pack, fold


def _head_network(dev, pair, S=64, Ni=128, train=False, **cfg_over):
    from idealnerf_amd.audio_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    torch.manual_seed(77)   # the audio nets are torch-initialised (and unused here)
    cfg = RenderConfig(perturb=0.0, chunk=512, near=rg.NEAR, far=rg.FAR, N_samples=S, N_importance=Ni, multires=pair[0],
                       multires_views=pair[1], **cfg_over)
    net = Network(32, 32, 50.0, rg.NEAR, rg.FAR, 512, None, S, Ni, args=cfg).to(dev)
    return net.train() if train else net.eval()


# ------------------------------------------------------------------------------------------------ 1: zero-column equivalence
@pytest.mark.parametrize("pair", mc.PAIRS)
def test_narrow_network_equals_the_zero_padded_10_4_network_bit_for_bit(idn, dev, pair):
    """3 rays at 64 + 128, perturb 0: kernel sequence in all five precisions, both fused arrangements (fp32), and 130 points
    through run_network -- the narrow network against the 10 / 4 network with zeros in the columns the narrow one lacks."""
    sc = rg.scene("3x64+128")
    dims_n, dims_w = mc.dims_of(pair, **COND), oracle.facenerf_dims(**COND)
    nets = {}
    for tag, seed in (("c", 40), ("f", 41)):
        p = oracle.xavier_facenerf_params(seed, dims_n)
        p["alpha_linear.weight"] = p["alpha_linear.weight"] * rg.GAIN
        nets[tag] = (device_net(idn, p, dims_n, dev), device_net(idn, mc.widen(p, pair, dims_n), dims_w, dev), p)
    cond = (sc["aud"], sc["expr"], sc["latent"])
    rays, bc = sc["rays"].to(dev), sc["bc"].to(dev)
    t, u = torch.linspace(0.0, 1.0, 64).to(dev), torch.linspace(0.0, 1.0, 128).to(dev)

    def render(which, precision, fused):
        (pack_c, fold_c), (pack_f, fold_f) = nets["c"][which], nets["f"][which]
        return idn.ops.render_rays_fwd(rays, bc, pack_c(precision), fold_c(*cond), pack_f(precision), fold_f(*cond), t, u, 128,
                                       taps=True, precision=precision, fused=fused)

    runs = [(name, code, False) for name, code in PREC.items()] + [("f32", 0, 1), ("f32", 0, "split")]
    for name, code, fused in runs:
        narrow, wide = render(0, code, fused), render(1, code, fused)
        assert narrow.keys() == wide.keys() and "tap_raw_fine" in narrow
        for k in narrow:
            assert torch.equal(narrow[k], wide[k]), (pair, name, fused, k)
        assert torch.isfinite(narrow["rgb_map"]).all() and float(narrow["tap_raw_fine"].abs().max()) > 0
    # the folded bias blocks and the weight streams themselves: the same bytes
    for tag in ("c", "f"):
        (pack_n, fold_n), (pack_w, fold_w), _ = nets[tag]
        assert torch.equal(fold_n(*cond), fold_w(*cond)), (pair, tag)
        for name, code in PREC.items():
            assert torch.equal(pack_n(code), pack_w(code)), (pair, tag, name)

    # pts mode: 130 points (26 rays x 5) through Network.run_network, narrow Network against 10 / 4 Network
    pts = (torch.rand(26, 5, 3, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    dirs = torch.nn.functional.normalize(torch.randn(26, 3, generator=torch.Generator().manual_seed(4)), dim=-1).to(dev)
    net_n, net_w = _head_network(dev, pair), _head_network(dev, (10, 4))
    net_n.face_nerf_coarse.load_state_dict(nets["c"][2])
    net_w.face_nerf_coarse.load_state_dict(mc.widen(nets["c"][2], pair, dims_n))
    g = lambda x: x.to(dev)
    for name in PREC:
        net_n.face_nerf_coarse.precision = net_w.face_nerf_coarse.precision = name
        with torch.no_grad():
            raw_n = net_n.run_network(pts, g(sc["expr"]), dirs, g(sc["aud"]), net_n.face_nerf_coarse, g(sc["latent"]))
            raw_w = net_w.run_network(pts, g(sc["expr"]), dirs, g(sc["aud"]), net_w.face_nerf_coarse, g(sc["latent"]))
        assert raw_n.shape == (26, 5, 4) and torch.equal(raw_n, raw_w), (pair, name)


# ------------------------------------------------------------------------------------------------ 2: x mode
# The tolerance of each precision on the reference's FaceNeRF golden at 10 / 4, tests/test_hip_parity.py:
#   f32 1e-5 (:113, test_facenerf_fwd_golden), bf16x3 5e-5 (:1243), fp16x3 5e-6 (:2024), bf16x6 5e-6 (:2103);
#   plain bf16 is held to its rounding model there (:1307-1309, BF16_MODEL_*: median, share beyond 1e-4, worst point).
X_TOL = {"f32": 1e-5, "bf16x3": 5e-5, "fp16x3": 5e-6, "bf16x6": 5e-6}


@pytest.mark.parametrize("tag,pair", [("m52", (5, 2)), ("id", (0, 0))])
def test_x_mode_forward_matches_the_reference_golden(idn, dev, golden, tag, pair):
    from test_hip_parity import BF16_MODEL_FLIPPED, BF16_MODEL_TYPICAL, BF16_MODEL_WORST
    g = golden("multires")
    dims = mc.dims_of(pair, **COND)
    params = oracle.xavier_facenerf_params(11, dims)
    x = torch.cat([T(g[tag + "_pe"]), T(g[tag + "_ped"])], -1)
    assert x.shape == (130, mc.channels(pair[0]) + mc.channels(pair[1]))
    if pair == (0, 0):
        assert np.array_equal(g["id_pe"], g["x130"]) and np.array_equal(g["id_ped"], g["d130"])       # the identity embedder
    else:   # the reference's embedder is the oracle's (and the kernels' prefix of gamma_10)
        assert rel_err(mc.embed(T(g["x130"]), pair[0]), g[tag + "_pe"]) < 1e-6
    aud, expr, lat = (T(g[f"{tag}_{k}"]) for k in ("aud", "expr", "latent"))
    with torch.no_grad():
        assert rel_err(oracle.facenerf_forward(params, x, aud, expr, lat, dims), g[tag + "_out"]) < 1e-5   # oracle == reference
    net = idn.FaceNeRF(input_ch=dims["input_ch"], input_ch_views=dims["input_ch_views"], dim_aud=64, dim_latent=32, dim_expr=76)
    net.load_state_dict(params, strict=True)
    net = net.to(dev)
    args = [t.to(dev) for t in (x, aud, expr, lat)]
    for name, tol in X_TOL.items():
        net.precision = name
        with torch.no_grad():
            out = net(*args)
        err = rel_err(out, g[tag + "_out"])
        print(f"\nx mode {pair} {name}: max rel err vs the reference = {err:.2e} (bound {tol:.0e})")
        assert out.shape == (130, 4) and err < tol, (pair, name, err)
    net.precision = "bf16"
    with torch.no_grad():
        out = net(*args).cpu().double()
        emu = oracle.facenerf_forward_bf16_emulated(params, x, aud, expr, lat, dims).double()
    e = ((out - emu).abs().max(1)[0] / float(emu.abs().max())).numpy()
    assert np.median(e) < BF16_MODEL_TYPICAL and (e > 1e-4).mean() < BF16_MODEL_FLIPPED and e.max() < BF16_MODEL_WORST, \
        (pair, np.median(e), (e > 1e-4).mean(), e.max())
    # rows of the default width into a narrow network: refused by name, before any launch
    with torch.no_grad(), pytest.raises(idn._lib.IdealNerfError, match=rf"\[\*, {x.shape[1]}\]"):
        net(torch.zeros(130, 90, device=dev), *args[1:])


# ------------------------------------------------------------------------------------------------ 3: the shipped config
def test_positional_encoding_config_renders_by_name(idn, dev, golden, monkeypatch):
    """configs/audio_expr_nerf/may/ablation/positional_encoding.txt, set up as test_obama_configs_render_by_name: 24 x 24,
    rows 8..14 against the CPU oracle with parity_proof's constants; then the reference's own 16 rays of that band."""
    from idealnerf_amd import config
    from idealnerf_amd.audio_exp_nerf import Network
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "configs_parsed.json")))[mc.CONFIG]
    ns = config.load_config(text="\n".join(gold["lines"]))
    cfg = config.to_render_config(ns)
    cfg.perturb = 0.0
    pair = (cfg.multires, cfg.multires_views)
    assert pair == (5, 2)
    mc.install(monkeypatch, pair)
    H = W = 24
    dims = mc.dims_of(pair, dim_aud=cfg.dim_aud, dim_expr=cfg.dim_expr, dim_latent=cfg.dim_latent)
    syn = oracle.synthetic_frame(H, W, seed=3, dims=dims)
    net = Network(H, W, syn["focal"], cfg.near, cfg.far, cfg.chunk, None, cfg.N_samples, cfg.N_importance, args=cfg).to(dev).eval()
    assert tuple(net.face_nerf_coarse.pts_linears[0].weight.shape) == (256, 33 + 64 + 79 + 32)
    pc, pf = scale_sigma(oracle.xavier_facenerf_params(31, dims)), scale_sigma(oracle.xavier_facenerf_params(32, dims))
    net.face_nerf_coarse.load_state_dict(pc)
    net.face_nerf_fine.load_state_dict(pf)
    g = lambda t: None if t is None else t.to(dev)
    rows = (8, 14)
    expr = g(syn["expr"])
    with torch.no_grad():
        rgb, disp, acc, last_w, extras = net.render_dynamic_face(
            H, W, syn["focal"], expr=expr, poses=syn["c2w"], latent_code=g(syn["latent"]), render_poses=syn["c2w"][:3, :4],
            chunk=cfg.chunk, near=cfg.near, far=cfg.far, bc_rgb=g(syn["bc"]), aud_para=g(syn["aud"]), rows=rows)
        ref = oracle.render_frame(H, W, syn["focal"], syn["c2w"], cfg.near, cfg.far, syn["bc"], pc, pf, syn["aud"], syn["expr"],
                                  syn["latent"], dims=dims, rows=rows, taps=True)
        rays = idn.ops.frame_rays(syn["c2w"][:3, :4], H, W, syn["focal"], cfg.near, cfg.far, rows[0], rows[1] - rows[0], device=dev)
        bc = g(syn["bc"])[rows[0]:rows[1]].reshape(-1, 3).contiguous()
        tapped = net.render_rays(rays, bc, g(syn["aud"]), syn["c2w"], g(syn["latent"]), expr, taps=True)
        ff = net.face_nerf_fine.folded_bias(g(syn["aud"]), expr, g(syn["latent"]))
    assert rgb.shape == (6, W, 3) and torch.equal(tapped["rgb_map"], rgb.reshape(-1, 3))
    flat = {k: v.reshape((-1,) + tuple(v.shape[2:])) for k, v in ref.items()}
    res = prove_render(idn, "positional_encoding band", tapped, flat, net.face_nerf_fine.packed_weights(), ff, rays, bc,
                       lambda z: oracle_fine_pass(pf, dims, rays, bc, syn["aud"], syn["expr"], syn["latent"], z), 2e-4,
                       precision_fine=net.face_nerf_fine.prec_code)
    fl, _ = flipped_rows(tapped["tap_inds"], flat["tap_inds"])
    keep = torch.from_numpy(~fl)
    assert abs_err(last_w.reshape(-1)[keep.to(dev)], flat["last_weight"][keep]) < RGB_TOL
    assert rel_err(extras["rgb0"], ref["rgb0"]) < RGB_TOL
    _record("config_band_end_to_end", dict(rays=int(rays.shape[0]), **res["rgb_map"]))

    # the reference's own render of 16 of the band's rays (tests/golden/multires.npz: rr_*)
    m = golden("multires")
    sel = T(m["rr_sel"]).long() - rows[0] * W
    assert rel_err(rays[sel.to(dev)], m["rr_rays"]) < 1e-6 and np.array_equal(bc[sel.to(dev)].cpu().numpy(), m["rr_bc"])
    with torch.no_grad():
        out = net.render_rays(T(m["rr_rays"]).to(dev), T(m["rr_bc"]).to(dev), g(syn["aud"]), syn["c2w"], g(syn["latent"]), expr, taps=True)
    np.testing.assert_array_equal(out["tap_z_coarse"].cpu().numpy(), m["rr_tap_z_coarse"])
    assert abs_err(out["tap_weights_coarse"], m["rr_tap_weights_coarse"]) < W_TOL
    assert rel_err(out["rgb0"], m["rr_rgb0"]) < RGB_TOL and rel_err(out["acc0"], m["rr_acc0"]) < RGB_TOL
    for k, gk in (("rgb_map", "rr_rgb"), ("disp_map", "rr_disp"), ("acc_map", "rr_acc")):
        assert rel_err(out[k], m[gk]) < RGB_TOL, k
    assert abs_err(out["last_weight"], m["rr_last_weight"]) < W_TOL
    flips = int((out["tap_inds"].cpu().numpy() != m["rr_tap_inds"].astype(np.int64)).sum())
    _record("config_16_rays_vs_reference", dict(rays=16, rgb=rel_err(out["rgb_map"], m["rr_rgb"]), rgb0=rel_err(out["rgb0"], m["rr_rgb0"]),
                                                flipped_indices=flips))


# ------------------------------------------------------------------------------------------------ 4: FaceNeRF.forward gradients
@pytest.mark.parametrize("pair", mc.PAIRS)
def test_facenerf_forward_gradients_match_the_fp64_oracle(idn, dev, pair, monkeypatch):
    """n in {1, 129}, both training arithmetics: every parameter gradient (of the parameter's own, narrower shape), d x
    [n, pts_ch + views_ch], d aud, d expr, d latent within GRAD_FLOOR_MULT of the fp32 noise floor (test_facenerf_autograd_gpu.py)."""
    from idealnerf_amd import autograd
    dims = mc.dims_of(pair, **COND)
    params = oracle.xavier_facenerf_params(5, dims)
    net = idn.FaceNeRF(input_ch=dims["input_ch"], input_ch_views=dims["input_ch_views"], dim_aud=64, dim_latent=32, dim_expr=76)
    net.load_state_dict(params)
    net = net.to(dev)
    width = dims["input_ch"] + dims["input_ch_views"]
    bad, worst = {}, 0.0
    for n in (1, 129):
        gen = torch.Generator().manual_seed(n)
        x = torch.rand(n, width, generator=gen) * 2 - 1
        cond = [torch.randn(d, generator=gen) * 0.3 for d in (64, 76, 32)]
        w = _off_kinks(params, dims, x, cond, torch.randn(n, 4, generator=gen))
        g64 = _oracle_grads(params, dims, x, cond, w, torch.float64)
        g32 = _oracle_grads(params, dims, x, cond, w, torch.float32)
        for prec in ("bf16x6", "f32"):
            monkeypatch.setattr(autograd, "TRAIN_PRECISION", prec)
            got = _hip_grads(net, dev, x, cond, w)
            assert got["x"].shape == (n, width)
            for k, p in net.named_parameters():
                if not k.startswith("feature_linear"):
                    assert got[k].shape == p.shape == params[k].shape, k
            ctx = f"pair {pair} n {n} {prec}"
            ratios = _check(got, g64, g32, ctx)
            bad.update({(ctx, k): r for k, r in ratios.items()})
            worst = max([worst] + [oracle_ratio(got[k], g64[k], g32[k]) for k in got])
    _record(f"facenerf_gradients/{pair[0]}_{pair[1]}", dict(worst_ratio_to_fp32_floor=worst, bound=GRAD_FLOOR_MULT))
    assert not bad, bad


def oracle_ratio(got, ref64, ref32):
    floor = max(oracle.fp32_noise_floor(ref32, ref64), 2.0 ** -23)
    err = float((got.detach().double().cpu() - ref64.double()).abs().max() / ref64.double().abs().max().clamp_min(1e-30))
    return err / floor


# ------------------------------------------------------------------------------------------------ 5: a train step
def _train_step_scene(pair):
    """Three rays (pixels 200, 250, 300: rows 8..12) of the 24 x 24 synthetic frame of the config test, 64 / 79 / 32 conditioning
    columns, Xavier weights of seeds 31 (coarse) / 33 (fine) with the density head scaled by 30 and bias 0.3, and a fixed random
    linear functional of rgb_map and rgb0 as the loss.  Chosen on the CPU with the oracle alone, at the oracle's own depths:
    both volumes are occupied at both width pairs (every coarse and every fine sample has a positive density; with fine seed 32
    the 0 / 0 fine network is empty and its gradients are 7e-7 against 1.0 -- nothing would be measured, as on scene
    "3x64+128", whose re-drawn coarse volume is empty), and the fp32 oracle's gradients are within 6.5e-5 (0 / 0) and 3.0e-5
    (5 / 2) relative L2 of the fp64 oracle's in every tensor: a thirtieth of the tightest bound below."""
    dims = mc.dims_of(pair, dim_aud=64, dim_expr=79, dim_latent=32)
    syn = oracle.synthetic_frame(24, 24, seed=3, dims=dims)
    ro, rd = oracle.camera_rays(24, 24, syn["focal"], syn["c2w"])
    sel = torch.tensor([200, 250, 300])
    rs = np.random.RandomState(0)
    weights = {k: T(rs.standard_normal((3, 3)).astype(np.float32)) for k in ("rgb_map", "rgb0")}
    return dict(dims=dims, rays=oracle.ray_records(ro, rd, rg.NEAR, rg.FAR)[sel].contiguous(), bc=syn["bc"].reshape(-1, 3)[sel].contiguous(),
                aud=syn["aud"], expr=syn["expr"], latent=syn["latent"], weights=weights,
                coarse=scale_sigma(oracle.xavier_facenerf_params(31, dims), 30.0, 0.3),
                fine=scale_sigma(oracle.xavier_facenerf_params(33, dims), 30.0, 0.3))


@pytest.mark.parametrize("pair", [(5, 2), (0, 0)])
def test_train_step_through_render_rays_matches_the_fp64_oracle(idn, dev, pair, monkeypatch):
    """3 rays at 64 + 128: every parameter gradient of both networks, d aud and d latent against the fp64 oracle's autograd
    AT THE FORWARD'S DEPTHS (so that no importance index can flip between the two sides).  The bound the 10 / 4 train-step
    parity test states (tests/test_hip_parity.py: check_grads with GRAD_L2_COARSE / GRAD_L2_FINE / GRAD_MAX; d aud and
    d latent at GRAD_L2_FINE)."""
    from idealnerf_amd import autograd as ag
    from test_hip_parity import GRAD_L2_FINE, check_grads, l2_err
    mc.install(monkeypatch, pair)
    sc = _train_step_scene(pair)
    net = _head_network(dev, pair, train=True, dim_expr=79)
    net.face_nerf_coarse.load_state_dict(sc["coarse"])
    net.face_nerf_fine.load_state_dict(sc["fine"])
    g = lambda t: t.to(dev)
    zs = []
    real_query = ag._train_query
    monkeypatch.setattr(ag, "_train_query", lambda net_, folded, r, z: (zs.append(z.detach().clone()), real_query(net_, folded, r, z))[1])
    aud, lat = g(sc["aud"]).requires_grad_(True), g(sc["latent"]).requires_grad_(True)
    ret = net.render_rays(g(sc["rays"]), g(sc["bc"]), aud, None, lat, g(sc["expr"]))
    rg.loss_of(ret, sc["weights"]).backward()
    z_c, z_f = zs[0].cpu().double(), zs[1].cpu().double()
    # the fp64 oracle at those depths
    f = oracle.to_f64
    pc = {k: v.double().clone().requires_grad_(True) for k, v in sc["coarse"].items()}
    pf = {k: v.double().clone().requires_grad_(True) for k, v in sc["fine"].items()}
    aud_o, lat_o = f(sc["aud"]).clone().requires_grad_(True), f(sc["latent"]).clone().requires_grad_(True)
    rays = f(sc["rays"])
    out_o = {}
    for params, z, tag in ((pc, z_c, "0"), (pf, z_f, "_map")):
        pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
        raw = oracle.render_oracle._query(params, pts, rays[:, 8:11], aud_o, f(sc["expr"]), lat_o, sc["dims"])
        assert float((raw[..., 3] > 0).double().mean()) > 0.5, "the volume is empty: nothing to measure"
        out_o["rgb" + tag] = oracle.composite(raw, z, rays[:, 3:6], f(sc["bc"]))[0]
    rg.loss_of(out_o, sc["weights"]).backward()
    for k in ("rgb_map", "rgb0"):
        assert rel_err(ret[k], out_o[k]) < RGB_TOL, k
    worst = {}
    for tag, m, ref, fine in (("c", net.face_nerf_coarse, pc, False), ("f", net.face_nerf_fine, pf, True)):
        for k, p in m.named_parameters():
            if not k.startswith("feature_linear"):
                assert p.grad is not None and p.grad.shape == ref[k].shape, k
                worst[f"{tag}.{k}"] = l2_err(p.grad, ref[k].grad)
        check_grads(m.named_parameters(), ref, fine, pair)
    e_aud, e_lat = l2_err(aud.grad, aud_o.grad), l2_err(lat.grad, lat_o.grad)
    _record(f"train_step/{pair[0]}_{pair[1]}", dict(d_aud_l2=e_aud, d_latent_l2=e_lat, worst_param_l2=max(worst.values()),
                                                    worst_param=max(worst, key=worst.get)))
    assert e_aud < GRAD_L2_FINE and e_lat < GRAD_L2_FINE, (e_aud, e_lat)


# ------------------------------------------------------------------------------------------------ 6: ray gradients
# Weight seeds of the ray-gradient scene, as an offset to ray_grad_common's (40 / 41 + 2 x the scene's seed).  At (3, 4) the
# scene's own seeds put unit 174 of the coarse network's pts_linears.7 at 1.2e-7 from its ReLU kink at sample 60 of ray 2
# (fp64 oracle; the coarse depths are the same on every side).  The fp32 kernels and the fp32 oracle land on the fp64 side; the
# six-piece bf16 forward -- fp32-grade, another summation order -- lands on the other, and d rays_o / d rays_d of that ONE ray
# then differ by 8.6e-5 / 1.1e-4 of the block's largest entry (the other two rays: 5e-7; the f32 arithmetic: 7.9e-7 / 1.1e-6).
# With that single ReLU forced to the other side in the fp64 oracle, the bf16x6 gradient is within 5.3e-7 / 6.0e-7 of it: a
# gradient is not defined to 1e-6 at a kink, and the scene, not the kernels, was at fault (measured on an MI355X from the
# forward's depths).  The replacement was chosen on the CPU with the oracle alone, at the oracle's depths, among offsets 100,
# 200, ..., 800 by: both volumes occupied, no pre-activation of either pass within 7e-7 of a kink, the fp32 oracle within 1.1e-6
# of the fp64 oracle in every block.  Offset 200 is the first that meets it (100: empty fine volume, 3.5e-8 from a kink).
SEED_OFFSET = {(3, 4): 200}


def _narrow_scene(name, pair):
    """ray_grad_common's scene with its weights re-drawn at the pair's widths (same seeds but for SEED_OFFSET, same density head)."""
    sc = rg.scene(name)
    dims = mc.dims_of(pair, **COND)
    seed = sc["seed"] + SEED_OFFSET.get(pair, 0) // 2

    def params(s):
        p = oracle.xavier_facenerf_params(s, dims)
        p["alpha_linear.weight"] = p["alpha_linear.weight"] * rg.GAIN
        p["alpha_linear.bias"] = torch.full_like(p["alpha_linear.bias"], rg.BIAS)
        return p
    return dict(sc, name=f"{name}@{pair[0]}/{pair[1]}", dims=dims, coarse=params(40 + 2 * seed), fine=params(41 + 2 * seed))


@pytest.mark.parametrize("pair", mc.PAIRS)
def test_ray_gradients_match_the_fp64_oracle(idn, dev, pair, monkeypatch):
    """Scene "3x64+128" at the narrow widths, both training arithmetics; per block (o, d, viewdirs) within FACTOR times the
    fp32 oracle's own distance from fp64 (test_ray_grad_gpu.py).  With the oracle's depths, on the CPU, that distance is at
    most 3.1e-6 in every block for each of these pairs -- far under the 1e-3 at which a scene counts as too sharp; the test
    re-checks it at the forward's depths."""
    from idealnerf_amd import autograd as ag
    mc.install(monkeypatch, pair)
    sc = _narrow_scene("3x64+128", pair)
    net = _head_network(dev, pair, train=True)
    net.face_nerf_coarse.load_state_dict(sc["coarse"])
    net.face_nerf_fine.load_state_dict(sc["fine"])
    g = lambda t: t.to(dev)
    worst, bad = {}, {}
    for prec in ("bf16x6", "f32"):
        monkeypatch.setattr(ag, "TRAIN_PRECISION", prec)
        zs = []
        real_query = ag._train_query
        with monkeypatch.context() as mp:
            mp.setattr(ag, "_train_query", lambda net_, folded, r, z: (zs.append(z.detach().clone()), real_query(net_, folded, r, z))[1])
            rays = g(sc["rays"]).clone().requires_grad_(True)
            ret = net.render_rays(rays, g(sc["bc"]), g(sc["aud"]), None, g(sc["latent"]), g(sc["expr"]))
            rg.loss_of(ret, sc["weights"]).backward()
        d_rays = rays.grad
        assert d_rays.shape == (3, 11) and torch.isfinite(d_rays).all() and float(d_rays[:, 6:8].abs().max()) == 0.0
        g64 = rg.oracle_d_rays(sc, zs[0], zs[1], torch.float64)
        g32 = rg.oracle_d_rays(sc, zs[0], zs[1], torch.float32)
        e32 = oracle.fp32_noise_floor(g32, g64)
        errs, floor = rg.block_errors(d_rays, g64), rg.block_errors(g32, g64)
        print(f"\nray gradients {pair} [{prec}]: e32 {e32:.2e}; HIP " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
              "; fp32 oracle " + "  ".join(f"{k} {v:.2e}" for k, v in floor.items()))
        assert e32 <= 1e-3, "the scene is too sharp to test a gradient on"
        for k, v in errs.items():                  # per block: FACTOR x the fp32 oracle's own distance from fp64 in that block
            worst[f"{prec}/{k}"] = v / floor[k]
            if not v <= FACTOR * floor[k]:
                bad[(prec, k)] = (v, FACTOR * floor[k])
    _record(f"ray_gradients/{pair[0]}_{pair[1]}", dict(worst_ratio_to_fp32_oracle=max(worst.values()), bound=FACTOR, per_block=worst))
    assert not bad, (pair, bad)


# ------------------------------------------------------------------------------------------------ 7: the loops
def test_loops_train_resume_and_drive_at_5_2(idn, dev, tmp_path):
    """train.train on a generated 64 x 64 clip with multires = 5, multires_views = 2: three steps, save, one resumed step ==
    four uninterrupted steps bit for bit, and the checkpoint holds the narrow shapes; train_torso.train and the agg trainer
    run the same flags; drive.drive_head renders two frames from the head checkpoint."""
    import drive_common as dc
    from idealnerf_amd import config, drive, train as T_, train_agg, train_torso as TT
    from idealnerf_amd.synthetic import write_clip_directory
    from test_train_loop_gpu import _assert_same_state, _state
    from train_loop_common import train_flags
    d = str(tmp_path / "clip")
    os.makedirs(d)
    flags, _ = write_clip_directory(d, 64, 3, seed=2)
    wide = dict(multires=5, multires_views=2)
    # (i_weights = 2: the third step, index 2, is one that saves)
    mk = lambda name, **over: train_flags(d, tmp_path / "logs", name, flags, perturb=0.0, i_print=2, i_weights=2, N_iters=10,
                                          chunk=8192, **wide, **over)
    torch.manual_seed(11)
    whole = T_.train(mk("whole"), loader="resident", sample_seed=3, device=dev, steps=4)
    torch.manual_seed(11)
    first = T_.train(mk("parts"), loader="resident", sample_seed=3, device=dev, steps=3)
    assert first["global_step"] == 3
    head_tar = str(tmp_path / "logs" / "parts" / "head.tar")
    assert torch.load(head_tar, weights_only=False)["global_step"] == 3
    sd = torch.load(head_tar, weights_only=False)["model_state_dict"]
    for tag in ("face_nerf_coarse", "face_nerf_fine"):
        assert tuple(sd[f"{tag}.pts_linears.0.weight"].shape) == (256, 33 + 64 + 76 + 32)
        assert tuple(sd[f"{tag}.pts_linears.5.weight"].shape) == (256, 33 + 64 + 76 + 32 + 256)
        assert tuple(sd[f"{tag}.views_linears.0.weight"].shape) == (128, 15 + 256 + 76)
    del first
    torch.manual_seed(999)
    second = T_.train(mk("parts"), loader="resident", sample_seed=3, device=dev, steps=1)
    assert second["global_step"] == 4
    _assert_same_state(_state(whole), _state(second))
    # a 10 / 4 network refuses that checkpoint by shape, as torch does
    with pytest.raises(RuntimeError, match="size mismatch"):
        _head_network(dev, (10, 4), dim_expr=76).load_state_dict(sd, strict=False)

    # the agg trainer and the torso stage on the same flags (no resume)
    d79 = str(tmp_path / "clip79")
    os.makedirs(d79)
    flags79, _ = write_clip_directory(d79, 64, 3, seed=2, dim_expr=79)
    import agg_common as ac
    dflat = str(tmp_path / "flat")     # the agg loop test's clip: the geometry the highlight recipe can draw from
    os.makedirs(dflat)
    fflags, meta = write_clip_directory(dflat, 64, 5, seed=6, flat=True, N_rand=64, dim_expr=79, face_rect=ac.RECT64, mouth_range=ac.MOUTH64)
    json.dump(dict(meta, frames=meta["frames"][:3]), open(os.path.join(dflat, "transforms_exp_train.json"), "w"))
    json.dump(dict(meta, frames=meta["frames"][3:]), open(os.path.join(dflat, "transforms_exp_val.json"), "w"))
    agg_ns = train_flags(dflat, tmp_path / "logs", "agg", fflags, perturb=0.0, i_print=2, i_weights=3, N_iters=10, chunk=8192,
                         dim_expr=79, **wide)
    agg_ns.use_highlight = True
    agg = train_agg.train(agg_ns, loader="resident", sample_seed=3, device=dev, steps=2)
    assert agg["global_step"] == 2 and agg["network"].face_nerf_coarse.input_xyz_ch == 33
    assert tuple(agg["network"].face_nerf_fine.views_linears[0].weight.shape) == (128, 15 + 256 + 64)
    T_.train(train_flags(d79, tmp_path / "logs", "torso", flags79, perturb=0.0, i_print=2, i_weights=1, N_iters=10, chunk=8192,
                         dim_expr=79, **wide), loader="resident", sample_seed=3, device=dev, steps=2)
    tns = config.load_config(kind="torso", argv=["--datadir", d79, "--basedir", str(tmp_path / "logs"), "--expname", "torso"])
    for k, v in {**vars(SimpleNamespace(gt_dirs=flags79.gt_dirs, testskip=1, N_rand=64, sample_rate=0.95, use_highlight=False)),
                 **dict(perturb=0.0, i_print=2, i_weights=3, N_iters=10, chunk=8192), **wide}.items():
        setattr(tns, k, v)
    torso = TT.train(tns, loader="resident", sample_seed=3, device=dev, steps=2)
    assert torso["global_step"] == 2
    for m in (torso["network"].face_nerf_coarse, torso["network"].torso_fine_nerf):
        assert (m.input_xyz_ch, m.input_views_ch) == (33, 15)

    # drive_head: two frames of the driving track from the narrow head checkpoint
    paths = dc.build_directory(str(tmp_path / "May"))
    args, _ = dc.flags(paths, str(tmp_path / "dlogs"), str(tmp_path / "out"), "head")
    args.multires, args.multires_views, args.ft_path, args.testskip = 5, 2, head_tar, 5
    out = str(tmp_path / "driven.avi")
    res = drive.drive_head(args, out=out, device=dev, codec="raw")
    assert res["n_frames"] == 2 and res["nonfinite_frames"] == []
    info, frames = dc.decode_raw(out)
    assert info["frames"] == 2 and frames[0].shape == (dc.SIZE, dc.SIZE, 3) and not np.array_equal(frames[0], frames[1])
