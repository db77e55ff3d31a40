"""Encoding widths other than 10 / 4 octaves (``--multires``, ``--multires_views``, ``--i_embed``), the part that needs no
GPU: constructor shapes, the config layer, the params struct's encoding and the argument checks of the new entries."""
import ctypes as C
import json
import os
import re

import pytest
import torch

import oracle
from multires_common import CONFIG, PAIRS, channels, dims_of, widen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 4096   # a non-NULL "device address" for entries that must refuse their arguments before any launch


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    return idealnerf_amd


def _shapes(module):
    return {k: tuple(t.shape) for k, t in module.state_dict().items()}


@pytest.mark.parametrize("pair", PAIRS + [(6, 0), (10, 4)])
def test_constructor_shapes_are_the_references(idn, pair):
    for cond in (dict(dim_aud=64, dim_expr=76, dim_latent=32), dict(dim_aud=106, dim_expr=0, dim_latent=0)):
        dims = dims_of(pair, **cond)
        net = idn.FaceNeRF(input_ch=channels(pair[0]), input_ch_views=channels(pair[1]), **cond)
        assert _shapes(net) == oracle.facenerf_param_shapes(dims)
        assert (net.input_xyz_ch, net.input_views_ch) == (channels(pair[0]), channels(pair[1]))
    from idealnerf_amd.models.face_nerf_agg import FaceNeRFAgg
    agg = FaceNeRFAgg(input_ch=channels(pair[0]), input_ch_views=channels(pair[1]), dim_agg=64, dim_aud=64, dim_expr=76, dim_latent=32)
    sh = _shapes(agg)
    assert sh["pts_linears.0.weight"] == (256, channels(pair[0]) + 64 + 32)
    assert sh["pts_linears.5.weight"] == (256, channels(pair[0]) + 64 + 32 + 256)
    assert sh["views_linears.0.weight"] == (128, channels(pair[1]) + 256 + 64)


def test_widths_beyond_the_input_tiles_raise_by_name(idn):
    from idealnerf_amd.models.face_nerf_agg import FaceNeRFAgg
    for cls in (idn.FaceNeRF, FaceNeRFAgg):
        with pytest.raises(NotImplementedError, match=r"input_ch=69.*0\.\.10"):
            cls(input_ch=69)                      # multires 11
        with pytest.raises(NotImplementedError, match=r"input_ch_views=33.*0\.\.4"):
            cls(input_ch_views=33)                # multires_views 5
        with pytest.raises(NotImplementedError, match="input_ch=34"):
            cls(input_ch=34)                      # not 3 + 6 L
    # the existing refusals stay
    with pytest.raises(NotImplementedError):
        idn.FaceNeRF(D=4)
    with pytest.raises(NotImplementedError):
        idn.FaceNeRF(W=128)


def _head_network(idn, ns, kind="head"):
    from idealnerf_amd import config
    cfg = config.to_render_config(ns)
    if kind == "head":
        from idealnerf_amd.audio_exp_nerf import Network
    elif kind == "baseline":
        from idealnerf_amd.head_baseline import Network
    else:
        from idealnerf_amd.agg_aud_exp_nerf import Network
    return Network(16, 16, 20.0, cfg.near, cfg.far, cfg.chunk, None, cfg.N_samples, cfg.N_importance, args=cfg), cfg


def test_the_shipped_ablation_config_builds_the_33_15_network(idn):
    """positional_encoding.txt (multires = 5, multires_views = 2), parsed by the product's config layer."""
    from idealnerf_amd import config
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "configs_parsed.json")))[CONFIG]
    ns = config.load_config(text="\n".join(gold["lines"]))
    assert (ns.multires, ns.multires_views) == (gold["parsed"]["multires"], gold["parsed"]["multires_views"]) == (5, 2)
    net, cfg = _head_network(idn, ns)
    assert (cfg.multires, cfg.multires_views, cfg.i_embed) == (5, 2, 0)
    C_all = cfg.dim_aud + cfg.dim_expr + cfg.dim_latent
    for m in (net.face_nerf_coarse, net.face_nerf_fine):
        assert (m.input_xyz_ch, m.input_views_ch) == (33, 15)
        assert tuple(m.pts_linears[0].weight.shape) == (256, 33 + C_all)
        assert tuple(m.pts_linears[5].weight.shape) == (256, 33 + C_all + 256)
        assert tuple(m.views_linears[0].weight.shape) == (128, 15 + 256 + cfg.dim_expr)
    if (cfg.dim_aud, cfg.dim_expr, cfg.dim_latent) == (64, 79, 32):
        assert tuple(net.face_nerf_coarse.pts_linears[0].weight.shape) == (256, 33 + 64 + 79 + 32)
    for kind in ("baseline", "agg"):
        other, _ = _head_network(idn, ns, kind)
        assert (other.face_nerf_coarse.input_xyz_ch, other.face_nerf_fine.input_views_ch) == (33, 15), kind


def test_i_embed_minus_one_and_flag_limits_in_the_config_layer(idn):
    from idealnerf_amd import config
    from idealnerf_amd.helper import RenderConfig, input_channels
    ns = config.load_config(text="dim_aud = 64\ndim_expr = 76\ni_embed = -1\nmultires = 7")
    net, cfg = _head_network(idn, ns)
    assert cfg.i_embed == -1 and (net.face_nerf_coarse.input_xyz_ch, net.face_nerf_coarse.input_views_ch) == (3, 3)
    zero, _ = _head_network(idn, config.load_config(text="dim_aud = 64\ndim_expr = 76\nmultires = 0\nmultires_views = 0"))
    assert _shapes(zero) == _shapes(net)                       # the identity embedder IS the network of 0 / 0 octaves
    assert input_channels(RenderConfig()) == (63, 27) and input_channels(RenderConfig(multires=10, multires_views=2)) == (63, 15)
    with pytest.raises(NotImplementedError, match=r"multires=11.*0\.\.10"):
        _head_network(idn, config.load_config(text="dim_aud = 64\nmultires = 11"))
    with pytest.raises(NotImplementedError, match=r"multires_views=5.*0\.\.4"):
        _head_network(idn, config.load_config(text="dim_aud = 64\nmultires_views = 5"))
    # the torso parser carries the same flags, and all four networks of the stage follow them
    from idealnerf_amd.train_torso import Network as TorsoNetwork
    tns = config.load_config(text="multires = 5\nmultires_views = 2", kind="torso")
    tcfg = config.to_render_config(tns)
    tnet = TorsoNetwork(16, 16, 20.0, tcfg.near, tcfg.far, tcfg.chunk, tcfg.N_samples, tcfg.N_importance, args=tcfg)
    for m in (tnet.face_nerf_coarse, tnet.face_nerf_fine, tnet.torso_coarse_nerf, tnet.torso_fine_nerf):
        assert (m.input_xyz_ch, m.input_views_ch) == (33, 15)


def test_checkpoint_of_a_narrow_network_loads_by_shape_only(idn):
    narrow = idn.FaceNeRF(input_ch=33, input_ch_views=15, dim_aud=64, dim_expr=76, dim_latent=32)
    again = idn.FaceNeRF(input_ch=33, input_ch_views=15, dim_aud=64, dim_expr=76, dim_latent=32)
    again.load_state_dict(narrow.state_dict(), strict=True)
    wide = idn.FaceNeRF(dim_aud=64, dim_expr=76, dim_latent=32)
    with pytest.raises(RuntimeError, match="size mismatch"):
        wide.load_state_dict(narrow.state_dict(), strict=True)
    # (multires_common.widen is the explicit way across: same function, zeros in the columns the narrow network lacks)
    wide.load_state_dict(widen(narrow.state_dict(), (5, 2), dims_of((5, 2))), strict=True)


def test_zero_initialised_params_struct_means_10_4(idn):
    lib = idn._lib.load()
    p = idn._lib.FaceNerfParams()
    assert (p.multires_plus1, p.multires_views_plus1) == (0, 0)
    assert (lib.idealnerf_params_pts_ch(C.byref(p)), lib.idealnerf_params_views_ch(C.byref(p))) == (63, 27) == idn.ops.widths(p)
    for pair in PAIRS:
        p.multires_plus1, p.multires_views_plus1 = pair[0] + 1, pair[1] + 1
        want = (channels(pair[0]), channels(pair[1]))
        assert (lib.idealnerf_params_pts_ch(C.byref(p)), lib.idealnerf_params_views_ch(C.byref(p))) == want == idn.ops.widths(p)
    p.multires_plus1 = 12
    assert lib.idealnerf_params_pts_ch(C.byref(p)) == -1 and lib.idealnerf_params_pts_ch(None) == -1
    # the trailing fields sit behind the three conditioning widths: every older caller's struct is a prefix of this one
    hdr = open(os.path.join(ROOT, "include", "idealnerf.h")).read()
    body = re.search(r"typedef struct idn_facenerf_params \{(.*?)\} idn_facenerf_params;", hdr, re.S).group(1)
    assert body.index("dim_latent") < body.index("multires_plus1")
    assert [n for n, _ in idn._lib.FaceNerfParams._fields_][-5:] == ["dim_aud", "dim_expr", "dim_latent", "multires_plus1", "multires_views_plus1"]


def test_params_struct_follows_the_modules_widths(idn):
    sd = dict(idn.FaceNeRF(input_ch=33, input_ch_views=15, dim_aud=8, dim_expr=0, dim_latent=0).named_parameters())
    fake = {k: torch.empty(v.shape, device="meta") for k, v in sd.items()}   # shapes only; the pointers are never read here
    with pytest.raises(idn._lib.IdealNerfError, match="33 point and 15 direction"):
        idn.ops.params_struct({**fake, "pts_linears.0.weight": torch.empty(256, 63 + 8)}, 8, 0, 0, pts_ch=33, views_ch=15)
    with pytest.raises(NotImplementedError, match="input_ch=69"):
        idn.ops.params_struct(fake, 8, 0, 0, pts_ch=69)


def test_new_entries_are_declared_and_refuse_bad_widths_without_a_gpu(idn):
    lib = idn._lib.load()
    hdr = open(os.path.join(ROOT, "include", "idealnerf.h")).read()
    for name in ("idealnerf_facenerf_fwd_ch", "idealnerf_facenerf_train_fwd_ch", "idealnerf_params_pts_ch", "idealnerf_params_views_ch"):
        assert re.search(r"\b" + name + r"\(", hdr) and hasattr(lib, name) and name in idn._lib.PROTOTYPES
    f32, x6 = idn._lib.IDN_PREC_F32, idn._lib.IDN_PREC_BF16X6
    for pts_ch, views_ch, word in ((69, 27, b"pts_ch 69"), (63, 33, b"views_ch 33"), (34, 27, b"pts_ch 34"), (0, 27, b"pts_ch 0"),
                                   (63, 0, b"views_ch 0"), (27, 63, b"views_ch 63")):
        assert lib.idealnerf_facenerf_fwd_ch(F, F, f32, F, pts_ch, views_ch, 8, F, None) == -1     # IDN_EINVAL, before any launch
        assert word in lib.idealnerf_last_error()
        assert lib.idealnerf_facenerf_train_fwd_ch(F, F, x6, F, pts_ch, views_ch, 8, F, F, None) == -1
        assert word in lib.idealnerf_last_error()
    # in range: the checks of the old entries, in their order
    assert lib.idealnerf_facenerf_fwd_ch(F, F, 99, F, 33, 15, 8, F, None) == -2
    assert lib.idealnerf_facenerf_fwd_ch(F, F, f32, F, 33, 15, -1, F, None) == -1
    assert lib.idealnerf_facenerf_fwd_ch(None, None, f32, None, 3, 3, 0, None, None) == 0         # nothing to do
    assert lib.idealnerf_facenerf_fwd_ch(None, F, f32, F, 33, 15, 8, F, None) == -1
    assert lib.idealnerf_facenerf_train_fwd_ch(F, F, idn._lib.IDN_PREC_BF16X3, F, 33, 15, 8, F, F, None) == -2
    assert lib.idealnerf_facenerf_train_fwd_ch(F, F, x6, F, 33, 15, 8, F, None, None) == -1      # acts NULL
    # entries that take the struct read the widths from it and refuse a value out of range before anything else happens
    p = idn._lib.FaceNerfParams()
    for field in ("pts_w", "pts_b"):
        for i in range(8):
            getattr(p, field)[i] = F
    for field in ("views_w", "views_b"):
        for i in range(3):
            getattr(p, field)[i] = F
    p.alpha_w = p.alpha_b = p.rgb_w = p.rgb_b = F
    for m, v, word in ((12, 0, b"multires must be in 0..10"), (0, 6, b"multires_views must be in 0..4"), (-1, 0, b"multires")):
        p.multires_plus1, p.multires_views_plus1 = m, v
        assert lib.idealnerf_pack_weights(C.byref(p), f32, F, None) == -1 and word in lib.idealnerf_last_error()
        assert lib.idealnerf_fold_conditioning(C.byref(p), None, None, None, F, None) == -1 and word in lib.idealnerf_last_error()
        g = idn._lib.FaceNerfGrads()
        assert lib.idealnerf_facenerf_bwd(C.byref(p), C.byref(g), None, None, None, F, 8, F, None, None, None, None, None, 0, None) == -1
        assert word in lib.idealnerf_last_error()
        assert lib.idealnerf_pass_bwd_cond(C.byref(p), None, None, None, F, F, F, F, F, 2, 8, None, None, None, None, None, None, None, 0, None) == -1
        assert word in lib.idealnerf_last_error()


def test_row_width_mismatch_raises_before_the_c_call(idn):
    """[n, 90] rows into a 33 / 15 network: refused by name by the tensor layer (CPU tensors: no launch is ever reached)."""
    lib = idn._lib.load()
    packed, folded = torch.zeros(lib.idealnerf_packed_weight_floats(0)), torch.zeros(lib.idealnerf_folded_bias_floats())
    with pytest.raises(idn._lib.IdealNerfError, match=r"x must be \[\*, 48\], got \[4, 90\]"):
        idn.ops.facenerf_fwd(packed, folded, torch.zeros(4, 90), 0, 33, 15)
    with pytest.raises(idn._lib.IdealNerfError, match=r"x must be \[\*, 48\]"):
        idn.ops.facenerf_train_fwd(packed, folded, torch.zeros(4, 90), idn._lib.IDN_PREC_F32, 33, 15)


def test_width_aware_oracle_reproduces_the_reference_golden(golden, monkeypatch):
    """tests/golden/multires.npz (the reference itself at 5 / 2 and at i_embed = -1) against the oracle with
    multires_common's query installed: the yardstick of the GPU tests is the reference's arithmetic."""
    import numpy as np
    from multires_common import embed, install
    g = golden("multires")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    cond = dict(dim_aud=64, dim_expr=76, dim_latent=32)
    for tag, pair in (("m52", (5, 2)), ("id", (0, 0))):
        dims = dims_of(pair, **cond)
        x = torch.cat([embed(T(g["x130"]), pair[0]), embed(T(g["d130"]), pair[1])], -1)
        assert x.shape == (130, channels(pair[0]) + channels(pair[1]))
        assert np.abs(x.numpy() - np.concatenate([g[tag + "_pe"], g[tag + "_ped"]], -1)).max() < 1e-6
        with torch.no_grad():
            out = oracle.facenerf_forward(oracle.xavier_facenerf_params(11, dims), x, T(g[tag + "_aud"]), T(g[tag + "_expr"]),
                                          T(g[tag + "_latent"]), dims)
        assert np.abs(out.numpy() - g[tag + "_out"]).max() / np.abs(g[tag + "_out"]).max() < 1e-5, tag
    # the 16 rays of the reference's Network at --multires 5 --multires_views 2
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "configs_parsed.json")))[CONFIG]["parsed"]
    install(monkeypatch, (5, 2))
    dims = dims_of((5, 2), dim_aud=gold["dim_aud"], dim_expr=gold["dim_expr"], dim_latent=32)
    syn = oracle.synthetic_frame(24, 24, seed=3, dims=dims)

    def sharp(seed):
        p = oracle.xavier_facenerf_params(seed, dims)
        p["alpha_linear.weight"] = p["alpha_linear.weight"] * 300.0
        p["alpha_linear.bias"] = torch.full_like(p["alpha_linear.bias"], 0.3)
        return p
    with torch.no_grad():
        ref = oracle.render_rays(T(g["rr_rays"]), T(g["rr_bc"]), sharp(31), sharp(32), syn["aud"], syn["expr"], syn["latent"],
                                 dims=dims, taps=True)
    assert np.array_equal(ref["tap_z_coarse"].numpy(), g["rr_tap_z_coarse"])
    assert np.abs(ref["tap_weights_coarse"].numpy() - g["rr_tap_weights_coarse"]).max() < 1e-5
    same = (ref["tap_inds"].numpy() == g["rr_tap_inds"].astype(np.int64)).all(1)      # rays without a flipped importance index
    assert same.sum() >= 14
    for k, gk in (("rgb_map", "rr_rgb"), ("rgb0", "rr_rgb0"), ("acc_map", "rr_acc")):
        err = np.abs(ref[k].numpy()[same] - g[gk][same]).max() / np.abs(g[gk]).max()
        assert err < 1e-4, (k, err)
    assert {"rays", "rgb", "disp", "acc", "last_weight", "rgb0", "disp0", "acc0", "z_std", "tap_z_coarse", "tap_weights_coarse", "tap_cdf",
            "tap_u", "tap_inds", "tap_z_samples", "tap_z_fine", "tap_raw_coarse", "tap_raw_fine", "tap_weights_fine"} <= {k[3:] for k in g if k.startswith("rr_")}
