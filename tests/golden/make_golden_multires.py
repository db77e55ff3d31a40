#!/usr/bin/env python3
"""Golden fixtures for encoding widths other than 10 / 4 octaves, from the REFERENCE itself on the CPU (build container only,
like make_golden.py, whose stand-ins for the optional imports this script uses):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_multires.py

The flags of the reference's shipped ablation config (configs/audio_expr_nerf/may/ablation/positional_encoding.txt:
``multires = 5``, ``multires_views = 2``; its text is part of configs_parsed.json) go through ``sys.argv`` before the import,
with ``--perturb 0``: the reference parses them when its modules are imported and builds its embedders from them
(train/audio_exp_nerf.py:35-36).

``multires.npz``
  x130 / d130          130 points and 130 unit directions (two rows more than a 128-point tile)
  m52_pe / m52_ped     the reference's ``get_embedder(5, 0)`` / ``get_embedder(2, 0)`` outputs on them ([130, 33] / [130, 15])
  id_pe / id_ped       ``get_embedder(10, -1)`` / ``get_embedder(4, -1)``: the identity ([130, 3] each)
  m52_* / id_*         ``aud``, ``expr``, ``latent`` and ``out``: the reference's ``FaceNeRF(input_ch, input_ch_views)`` on
                       [pe | ped] with 64 / 76 / 32 conditioning columns.  Weights are not stored:
                       ``oracle.xavier_facenerf_params(SEED_X, dims)``, as the tests rebuild them.
  rr_*                 a 16-ray ``render_rays`` of the reference's ``Network`` built under those flags, on rays of rows 8..14 of
                       the 24 x 24 synthetic frame (seed 3), weights ``xavier_facenerf_params(31 / 32)`` with the density head
                       scaled by 300 and bias 0.3: every key frame32.npz holds (``rays``, the eight maps, the taps), plus ``sel``
                       (the rays' flat pixel indices) and ``bc``.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REPO, install_shims, load_state, scale_sigma  # noqa: E402

CONFIG = "NeRFs/HeadNeRF/configs/audio_expr_nerf/may/ablation/positional_encoding.txt"
SEED_X = 11            # FaceNeRF weights of the row fixtures
SEEDS_RR = (31, 32)    # coarse / fine weights of the render fixture
N_ROWS, N_RAYS = 130, 16
H = W = 24
ROWS = (8, 14)


def main():
    install_shims()
    flags = json.load(open(os.path.join(HERE, "configs_parsed.json")))[CONFIG]["parsed"]
    assert (flags["multires"], flags["multires_views"]) == (5, 2)
    sys.argv = [sys.argv[0], "--perturb", "0", "--vis_path", "/tmp/idealnerf_golden_vis", "--chunk", "512"]
    for k in ("dim_aud", "dim_expr", "N_samples", "N_importance", "near", "far", "multires", "multires_views"):
        sys.argv += ["--" + k, str(flags[k])]
    sys.path.insert(0, REF)
    sys.path.insert(0, REPO)
    torch.manual_seed(0)
    torch.set_num_threads(8)

    import oracle  # weight construction and synthetic inputs only (no oracle output is stored)
    from models.face_nerf import FaceNeRF
    import NeRFs.HeadNeRF.helper as helper
    from NeRFs.HeadNeRF.train import audio_exp_nerf as aen

    assert (aen.input_ch, aen.input_ch_views) == (33, 15)   # the module's embedders follow the flags
    rs = np.random.RandomState(4321)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    fx = {}

    # ---- rows: the embedders and FaceNeRF at 5 / 2 and at i_embed = -1 ---------------------------------------------------
    pts = f32(rs.uniform(-1.0, 1.0, size=(N_ROWS, 3)))
    dirs = f32(rs.standard_normal((N_ROWS, 3)))
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    fx.update(x130=pts.numpy(), d130=dirs.numpy())
    cond = dict(dim_aud=64, dim_expr=76, dim_latent=32)
    for tag, (m, mv, i_embed) in (("m52", (5, 2, 0)), ("id", (10, 4, -1))):
        e, ch = helper.get_embedder(m, i_embed)
        ev, chv = helper.get_embedder(mv, i_embed)
        assert (ch, chv) == ((33, 15) if tag == "m52" else (3, 3))
        xin = torch.cat([e(pts), ev(dirs)], -1)
        dims = oracle.facenerf_dims(input_ch=ch, input_ch_views=chv, **cond)
        net = FaceNeRF(D=8, W=256, input_ch=ch, input_ch_views=chv, dim_aud=64, dim_latent=32, dim_expr=76, skips=[4])
        assert {k: tuple(t.shape) for k, t in net.state_dict().items()} == oracle.facenerf_param_shapes(dims)
        load_state(net, oracle.xavier_facenerf_params(SEED_X, dims))
        aud, expr, lat = (f32(rs.standard_normal(n)) for n in (64, 76, 32))
        with torch.no_grad():
            y = net(xin, aud, expr, lat)
        fx.update({f"{tag}_pe": e(pts).numpy(), f"{tag}_ped": ev(dirs).numpy(), f"{tag}_aud": aud.numpy(),
                   f"{tag}_expr": expr.numpy(), f"{tag}_latent": lat.numpy(), f"{tag}_out": y.numpy()})

    # ---- 16 rays through the reference's Network.render_rays at 5 / 2 ---------------------------------------------------
    near, far = flags["near"], flags["far"]
    dims = oracle.facenerf_dims(dim_aud=flags["dim_aud"], dim_expr=flags["dim_expr"], dim_latent=32, input_ch=33, input_ch_views=15)
    syn = oracle.synthetic_frame(H, W, seed=3, dims=dims)
    net = aen.Network(H, W, syn["focal"], near, far, 512, None, flags["N_samples"], flags["N_importance"])
    load_state(net.face_nerf_coarse, scale_sigma(oracle.xavier_facenerf_params(SEEDS_RR[0], dims), 300.0, 0.3))
    load_state(net.face_nerf_fine, scale_sigma(oracle.xavier_facenerf_params(SEEDS_RR[1], dims), 300.0, 0.3))
    net.eval()
    ro, rd = helper.get_rays(H, W, syn["focal"], syn["c2w"])
    viewdirs = rd / torch.norm(rd, dim=-1, keepdim=True)
    rays = torch.cat([ro.reshape(-1, 3), rd.reshape(-1, 3), near * torch.ones(H * W, 1), far * torch.ones(H * W, 1),
                      viewdirs.reshape(-1, 3)], -1).float()
    sel = torch.from_numpy(np.sort(ROWS[0] * W + rs.choice((ROWS[1] - ROWS[0]) * W, size=N_RAYS, replace=False)))
    bc = syn["bc"].reshape(-1, 3)[sel]

    taps, captured = {}, {}
    real_r2o, real_sp, real_ss = aen.raw2outputs, aen.sample_pdf, torch.searchsorted

    def spy(cdf, u, **kw):
        r = real_ss(cdf, u, **kw)
        captured["cdf"], captured["u"], captured["inds"] = cdf.clone(), u.clone(), r.clone()
        return r

    def tap_r2o(raw, z_vals, rays_d, bc_rgb, *a, **k):
        r = real_r2o(raw, z_vals, rays_d, bc_rgb, *a, **k)
        tag = "coarse" if raw.shape[1] == flags["N_samples"] else "fine"
        taps["raw_" + tag], taps["z_" + tag], taps["weights_" + tag] = raw.detach().clone(), z_vals.detach().clone(), r[3].detach().clone()
        return r

    def tap_sp(bins, weights, N, det=False, pytest=False):
        torch.searchsorted = spy
        try:
            r = real_sp(bins, weights, N, det=det, pytest=pytest)
        finally:
            torch.searchsorted = real_ss
        taps.update(cdf=captured["cdf"], u=captured["u"], inds=captured["inds"], z_samples=r.detach().clone())
        return r

    aen.raw2outputs, aen.sample_pdf = tap_r2o, tap_sp
    try:
        with torch.no_grad():
            ret = net.render_rays(rays[sel], bc, syn["aud"], syn["c2w"], syn["latent"], syn["expr"])
    finally:
        aen.raw2outputs, aen.sample_pdf = real_r2o, real_sp
    n = lambda t: t.detach().numpy()
    fx.update(rr_sel=sel.numpy(), rr_bc=bc.numpy(), rr_rays=rays[sel].numpy(),
              # frame32.npz's names for the eight maps
              rr_rgb=n(ret["rgb_map"]), rr_disp=n(ret["disp_map"]), rr_acc=n(ret["acc_map"]), rr_last_weight=n(ret["last_weight"]),
              rr_rgb0=n(ret["rgb0"]), rr_disp0=n(ret["disp0"]), rr_acc0=n(ret["acc0"]), rr_z_std=n(ret["z_std"]),
              rr_tap_z_coarse=n(taps["z_coarse"]), rr_tap_weights_coarse=n(taps["weights_coarse"]), rr_tap_cdf=n(taps["cdf"]),
              rr_tap_u=n(taps["u"])[:1], rr_tap_inds=n(taps["inds"]).astype(np.int16), rr_tap_z_samples=n(taps["z_samples"]),
              rr_tap_z_fine=n(taps["z_fine"]), rr_tap_raw_coarse=n(taps["raw_coarse"]), rr_tap_raw_fine=n(taps["raw_fine"]),
              rr_tap_weights_fine=n(taps["weights_fine"]))
    frame32 = set(np.load(os.path.join(HERE, "frame32.npz")).files)
    assert frame32 <= {k[3:] for k in fx if k.startswith("rr_")}, frame32 - {k[3:] for k in fx if k.startswith("rr_")}
    out = os.path.join(HERE, "multires.npz")
    np.savez_compressed(out, **fx)
    print(out, os.path.getsize(out), "bytes;", "occupied samples coarse / fine:",
          float((taps["raw_coarse"][..., 3] > 0).float().mean()), float((taps["raw_fine"][..., 3] > 0).float().mean()))


if __name__ == "__main__":
    main()
