"""The ray cull on the device (csrc/cull.hip, cull.py): the grid kernels against numpy word for word, the classification
against the fp64 model of its march, the gathered rays against the frame's own, and the culled frame against the unculled
one bit for bit on the analytic box scene (tests/cull_common.py) -- S = 64, Ni = 128, G = 32, fp32 unless a case says else.

The march model: a pixel's ray is sampled at z_k = near + k dz and at far, in fp64, exactly where the kernel samples it in
fp32; "inside / near an occupied cell" is asked of those points with a margin of cell / 1000 (fp32 rounding of coordinates
of size 1 is 1e-7, a cell is 0.02)."""
import numpy as np
import pytest
import torch

import cull_common as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()
    return idealnerf_amd


@pytest.fixture(scope="module")
def syn(dev):
    from idealnerf_amd import synthetic
    s = synthetic.frame(cc.SIZE, cc.SIZE, seed=0)
    s["focal"] = cc.FOCAL
    return {k: (v.to(dev) if torch.is_tensor(v) and k != "c2w" else v) for k, v in s.items()}


def _frame(idn, syn, H=cc.SIZE, W=cc.SIZE, row0=0, nrows=None):
    return idn.ops.make_frame(syn["c2w"], H, W, cc.FOCAL, syn["near"], syn["far"], row0, nrows)


def _grid(net, syn, conds=None, G=cc.G, dilate=1, pair="head", H=cc.SIZE, W=cc.SIZE, camera=None):
    from idealnerf_amd import cull
    nets = (net.face_nerf_coarse, net.face_nerf_fine) if pair == "head" else (net.torso_coarse_nerf, net.torso_fine_nerf)
    conds = [(syn["aud"], syn["expr"], syn["latent"])] if conds is None else conds
    return cull.build_grid(nets, conds, [syn["c2w"] if camera is None else camera], H, W, cc.FOCAL, syn["near"], syn["far"], G=G, dilate=dilate)


def _render(net, syn, frame, aud=None, with_fg=True, taps=False, **kw):
    bc = syn["bc"].reshape(-1, 3)[frame.row0 * frame.W:(frame.row0 + frame.nrows) * frame.W]
    return net._render(None, bc, syn["aud"] if aud is None else aud, syn["latent"], syn["expr"], net.face_nerf_coarse, net.face_nerf_fine,
                       with_fg, taps=taps, frame=frame, **kw)


def _culled_mask(grid, frame):
    sel, n = grid.live(frame)
    live = torch.zeros(frame.nrows * frame.W, dtype=torch.bool, device=sel.device)
    live[sel[:n]] = True
    return ~live


@pytest.fixture(scope="module")
def net32(dev, idn):
    return cc.box_network(dev, "f32")


@pytest.fixture(scope="module")
def unculled32(idn, net32, syn):
    """The reference of the fp32 cases, computed once: the frame-mode render with taps, no grid installed."""
    net32.set_cull()
    return _render(net32, syn, _frame(idn, syn), taps=True)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_mark_and_cells_equal_numpy(idn, dev, dilate):
    rs = np.random.RandomState(dilate)
    n = 33 ** 3
    raw = rs.standard_normal((n, 4)).astype(np.float32)
    raw[:, 3] -= 2.4                                   # ~ 1 % of the corners above 0: blobs, not noise
    raw[rs.randint(0, n, 50), 3] = 0.0                 # exactly sigma_min: not marked
    raw[rs.randint(0, n, 20), 3] = np.nan
    before = (rs.rand(n) < 0.002).astype(np.uint8)     # marks of an earlier frame stay
    corners = torch.from_numpy(before.copy()).to(dev)
    half = n // 2 + 7                                  # two chunks, the second from an odd offset
    idn.ops.cull_mark(torch.from_numpy(raw[:half]).to(dev), 0.0, corners[:half])
    idn.ops.cull_mark(torch.from_numpy(raw[half:]).to(dev), 0.0, corners[half:])
    want = cc.np_mark(raw, 0.0, before)
    assert 0 < want.sum() < n // 20
    np.testing.assert_array_equal(corners.cpu().numpy(), want)
    bits = idn.ops.cull_cells(corners, 32, dilate)
    occ, words = cc.np_cells(want, 32, dilate)
    assert bits.dtype == torch.int32 and bits.shape == (32 ** 3 // 32,)
    np.testing.assert_array_equal(bits.cpu().numpy().view(np.uint32), words)
    np.testing.assert_array_equal(cc.unpack(bits, 32), occ)
    assert 0 < occ.mean() < 1


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_grid_of_the_box_scene(idn, net32, syn):
    g = _grid(net32, syn)
    occ = cc.unpack(g.bits, cc.G)
    lo, cell = np.array(g.lo), g.cell
    idx = np.stack(np.meshgrid(*[np.arange(cc.G)] * 3, indexing="ij"), -1)[..., ::-1]     # [z, y, x] -> (x, y, z) per cell
    c_lo, c_hi = lo + idx * cell, lo + (idx + 1) * cell
    box_lo, box_hi = np.array(cc.CENTRE) - cc.HALF, np.array(cc.CENTRE) + cc.HALF
    gap = np.maximum(np.maximum(box_lo - c_hi, c_lo - box_hi), 0.0)                       # per axis distance cell <-> box
    meets = (gap == 0).all(-1)
    far_away = gap.max(-1) > 1.0 / cc.SLOPE + (g.dilate + 1) * cell * (1 + 1e-5)          # one cell of marking, `dilate` of dilation
    assert meets.sum() > 100 and far_away.sum() > cc.G ** 3 // 2
    assert occ[meets].all() and not occ[far_away].any()
    assert g.occupied_share == pytest.approx(occ.mean(), abs=1e-12)
    # the raw set (no dilation): nothing farther than 1 / slope + one cell
    occ0 = cc.unpack(idn.ops.cull_cells(g.corners, cc.G, 0), cc.G)
    assert occ0[meets].all() and not occ0[gap.max(-1) > 1.0 / cc.SLOPE + cell * (1 + 1e-5)].any()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,row0,nrows", [(48, 48, 0, 48), (50, 37, 5, 20)])
def test_classify_against_the_fp64_march(idn, net32, syn, H, W, row0, nrows):
    g = _grid(net32, syn, H=H, W=W)
    frame = _frame(idn, syn, H, W, row0, nrows)
    dz, K = g.steps(frame)
    sel, n_dev = idn.ops.cull_classify(g.bits, g.G, g.lo, g.cell, frame, dz, K)
    n = int(n_dev.item())
    live = sel[:n].cpu().numpy()
    assert n == len(live) and (np.diff(live) > 0).all() and (n == 0 or (live[0] >= 0 and live[-1] < nrows * W))
    o, d = cc.rays64(syn["c2w"].numpy(), H, W, cc.FOCAL, row0, nrows)
    assert dz * np.sqrt((d * d).sum(1)).max() <= g.cell / 2
    must, may = cc.march_model(cc.unpack(g.bits, g.G), g.G, g.lo, g.cell, o, d, syn["near"], syn["far"], dz, K, 1e-3)
    got = np.zeros(nrows * W, dtype=bool)
    got[live] = True
    free = may & ~must
    print(f"classify {H}x{W} rows {row0}+{nrows}: K = {K}, live {n} / {nrows * W}, must {must.sum()}, free {free.sum()}")
    assert free.sum() < 0.02 * nrows * W                       # (the model's own property, checked before the kernel's)
    assert got[must].all(), "a pixel whose march enters an occupied cell was culled"
    assert not got[~may].any(), "a pixel whose march stays clear of every occupied cell is live"
    assert 0 < n < nrows * W
    # the same bytes on a second run, and through the grid's cache
    sel2, n2 = idn.ops.cull_classify(g.bits, g.G, g.lo, g.cell, frame, dz, K)
    assert int(n2.item()) == n and torch.equal(sel2[:n], sel[:n])
    sel3, n3 = g.live(frame)
    assert n3 == n and torch.equal(sel3[:n], sel[:n])


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,row0,nrows", [(48, 48, 0, 48), (50, 37, 5, 20)])
def test_gather_rows_are_the_frames_rays(idn, dev, syn, H, W, row0, nrows):
    frame = _frame(idn, syn, H, W, row0, nrows)
    rays = idn.ops.frame_rays(syn["c2w"], H, W, cc.FOCAL, syn["near"], syn["far"], row0, nrows, device=dev)
    rs = np.random.RandomState(3)
    npix = nrows * W
    for sel in (np.arange(npix), np.sort(rs.choice(npix, 301, replace=False)), np.array([0]), np.array([npix - 1])):
        sel = torch.from_numpy(sel.astype(np.int64)).to(dev)
        bc = torch.rand(npix, 3, device=dev)
        got, bc_live = idn.ops.cull_gather(sel, frame, bc)
        assert torch.equal(got, rays[sel]) and torch.equal(bc_live, bc[sel])
    # the scatter puts them back: live rows over the fill
    sel = torch.from_numpy(np.sort(rs.choice(npix, 100, replace=False)).astype(np.int64)).to(dev)
    v3, v1 = torch.rand(100, 3, device=dev), torch.rand(100, device=dev)
    out = idn.ops.cull_scatter(sel, 100, bc, dict(a=(v3, 3, "bc"), b=(v1, 1, 0.25), c=(v3, 3, 0.0)))
    want_a, want_b, want_c = bc.clone(), torch.full((npix,), 0.25, device=dev), torch.zeros(npix, 3, device=dev)
    want_a[sel], want_b[sel], want_c[sel] = v3, v1, v3
    assert torch.equal(out["a"], want_a) and torch.equal(out["b"], want_b) and torch.equal(out["c"], want_c)
    out = idn.ops.cull_scatter(None, 0, bc, dict(a=(None, 3, "bc"), b=(None, 1, 0.25)))
    assert torch.equal(out["a"], bc) and torch.equal(out["b"], torch.full((npix,), 0.25, device=dev))


# ---- 5, 6 ---------------------------------------------------------------------------------------------------------------------
def _assert_culled_frame(idn, net, syn, grid, ref, frame, aud=None, must_cull=None, some_culled=True):
    """The assertions of case 5 for one frame: every output of the guarantee torch.equal, z_std equal on live pixels and 0 on
    culled ones, every culled pixel's coarse and fine sigma_raw <= 0 in the unculled taps, `must_cull` pixels culled."""
    net.set_cull(head=grid)
    try:
        out = _render(net, syn, frame, aud=aud)
    finally:
        net.set_cull()
    culled = _culled_mask(grid, frame)
    for k in cc.OUTPUTS:
        assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), k
    assert torch.equal(out["z_std"][~culled], ref["z_std"][~culled]) and not out["z_std"][culled].any()
    assert (ref["tap_raw_coarse"][culled][..., 3] <= 0).all() and (ref["tap_raw_fine"][culled][..., 3] <= 0).all()
    assert torch.equal(out["rgb_map"][culled], syn["bc"].reshape(-1, 3)[culled])
    assert int(culled.sum()) < culled.numel() and (int(culled.sum()) > 0 or not some_culled)
    if must_cull is not None:
        assert culled[torch.from_numpy(must_cull).to(culled.device)].all()
    return culled


def _misses_inflated_box(syn, cell, half=cc.HALF):
    o, d = cc.rays64(syn["c2w"].numpy(), cc.SIZE, cc.SIZE, cc.FOCAL)
    return ~cc.ray_hits_box(o, d, float(np.float32(syn["near"])), float(np.float32(syn["far"])), cc.CENTRE,
                            half + 1.0 / cc.SLOPE + 3 * cell)


@pytest.mark.parametrize("precision", ["f32", "bf16x6"])
def test_culled_frame_equals_unculled_frame(idn, dev, syn, net32, unculled32, precision):
    frame = _frame(idn, syn)
    if precision == "f32":
        net, ref = net32, unculled32
    else:
        net = cc.box_network(dev, precision)
        ref = _render(net, syn, frame, taps=True)
    grid = _grid(net, syn)
    culled = _assert_culled_frame(idn, net, syn, grid, ref, frame, must_cull=_misses_inflated_box(syn, grid.cell))
    # at G = 32 three cells are 0.06: the inflated box fills the frame and the statement above is empty; at G = 64 it is not
    fine_grid = _grid(net, syn, G=64)
    far_off = _misses_inflated_box(syn, fine_grid.cell)
    assert far_off.sum() > 0.2 * far_off.size
    culled64 = _assert_culled_frame(idn, net, syn, fine_grid, ref, frame, must_cull=far_off)
    print(f"{precision}: culled {int(culled.sum())} (G = 32) / {int(culled64.sum())} (G = 64) of {culled.numel()} pixels")
    assert culled64.sum() > culled.sum()


def test_union_over_conditioning(idn, dev, syn):
    net = cc.box_network(dev, "f32", aud_gain=0.05)
    frame = _frame(idn, syn)
    auds = [syn["aud"].clone(), syn["aud"].clone()]
    auds[0][0], auds[1][0] = 0.0, 1.0
    conds = [(a, syn["expr"], syn["latent"]) for a in auds]
    refs = [_render(net, syn, frame, aud=a, taps=True) for a in auds]
    both = _grid(net, syn, conds)
    for a, ref in zip(auds, refs):
        # (frame 1's box, half 0.13, plus the grid's margin covers this 48 x 48 frame: the union may leave nothing to cull)
        culled = _assert_culled_frame(idn, net, syn, both, ref, frame, aud=a, some_culled=False)
        print(f"union grid: culled {int(culled.sum())} of {culled.numel()}")
    # the grid of frame 0 alone does not know the box frame 1's audio grows: it culls pixels frame 1 renders
    first = _grid(net, syn, conds[:1])
    culled = _culled_mask(first, frame)
    bc = syn["bc"].reshape(-1, 3)
    wrong = culled & (refs[1]["rgb_map"] != bc).any(-1)
    print(f"grid of frame 0 alone on frame 1: culled {int(culled.sum())}, of them rendered differently {int(wrong.sum())}")
    assert int(wrong.sum()) >= 1
    assert not (_culled_mask(both, frame) & (refs[1]["rgb_map"] != bc).any(-1)).any()
    assert float(both.occupied_share) > float(first.occupied_share)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_nothing_occupied_launches_no_network(idn, dev, syn):
    net = cc.box_network(dev, "f32", sigma_bias=-1.0)
    frame = _frame(idn, syn)
    grid = _grid(net, syn)
    assert grid.occupied_share == 0.0
    ref = _render(net, syn, frame)
    net.set_cull(head=grid)
    idn.ops.profile_begin()
    out = _render(net, syn, frame)
    _, launches, points = idn.ops.profile_end()
    assert launches == 0 and points == 0
    assert grid.live(frame)[1] == 0
    bc = syn["bc"].reshape(-1, 3)
    assert torch.equal(out["rgb_map"], bc) and torch.equal(out["rgb0"], bc)
    for k in cc.OUTPUTS:
        assert torch.equal(out[k], ref[k]), k
    assert not out["z_std"].any()
    idn.ops.profile_begin()                         # (the counter does count: the unculled frame launches both networks)
    net.set_cull()
    _render(net, syn, frame)
    assert idn.ops.profile_end()[1] >= 2


def test_everything_live_equals_the_frame_mode_render(idn, syn, net32, unculled32):
    frame = _frame(idn, syn)
    grid = _grid(net32, syn, dilate=cc.G)
    assert grid.occupied_share == 1.0
    net32.set_cull(head=grid)
    try:
        out = _render(net32, syn, frame)
    finally:
        net32.set_cull()
    assert grid.live(frame)[1] == cc.SIZE * cc.SIZE
    for k in cc.OUTPUTS + ("z_std",):
        assert torch.equal(out[k], unculled32[k]), k


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_torso_clip_bytes_and_one_torso_classification(idn, dev, syn, tmp_path, monkeypatch):
    from idealnerf_amd import clip, cull, synthetic
    net = cc.box_network(dev, "f32", aud_gain=0.0, model="torso")
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]])
    poses = torch.stack([torch.cat([synthetic.frame(cc.SIZE, cc.SIZE, seed=10 + j)["c2w"], bottom], 0) for j in range(8)])
    auds = torch.from_numpy(np.random.RandomState(11).standard_normal((8, 16, 29)).astype(np.float32))
    kw = dict(expr=syn["expr"], latent_code=syn["latent"], torso_pose=torch.cat([syn["c2w"], bottom], 0), frames=range(3), codec="raw")
    plain, culled = str(tmp_path / "plain.avi"), str(tmp_path / "culled.avi")
    res0 = clip.render_torso_clip(net, poses, auds, syn["bc"], plain, **kw)
    built = {}
    real = cull.build_grid
    monkeypatch.setattr(cull, "build_grid", lambda nets, *a, **k: built.setdefault(id(nets[0]), real(nets, *a, **k)))
    res1 = clip.render_torso_clip(net, poses, auds, syn["bc"], culled, cull=dict(G=cc.G), **kw)
    assert open(plain, "rb").read() == open(culled, "rb").read()
    assert "cull" not in res0 and res1["n_frames"] == 3 and res1["nonfinite_frames"] == []
    head, torso = built[id(net.face_nerf_coarse)], built[id(net.torso_coarse_nerf)]
    assert torso.classify_calls == 1 and head.classify_calls == 3
    assert 0 < res1["cull"]["live_share"]["torso"] < 1 and 0 < res1["cull"]["live_share"]["head"] < 1
    assert res1["cull"]["live_share"]["torso"] == pytest.approx(torso.live_share)
    assert 0 < res1["cull"]["occupied_share"]["head"] < 0.2 and res1["cull"]["build_seconds"] > 0
    assert not getattr(net, "_cull")                                    # removed at the end of the clip


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_kernel", [False, True])
def test_perturb_with_a_seed(idn, dev, syn, in_kernel):
    net = cc.box_network(dev, "f32", perturb=1.0)
    net.in_kernel_draws = in_kernel
    frame = _frame(idn, syn)
    grid = _grid(net, syn)
    culled = _culled_mask(grid, frame)
    n_live = grid.live(frame)[1]
    net.set_cull(head=grid)
    outs = []
    for _ in range(2):
        torch.manual_seed(5)
        outs.append(_render(net, syn, frame))
    out = outs[0]
    bc = syn["bc"].reshape(-1, 3)
    assert torch.equal(out["rgb_map"][culled], bc[culled]) and torch.equal(out["rgb0"][culled], bc[culled])
    assert all(torch.isfinite(v).all() for v in out.values())
    assert grid.live(frame)[1] == n_live == int((~culled).sum()) and grid.classify_calls == 1
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in out)            # the seed governs the draws
    assert (out["rgb_map"][~culled] != bc[~culled]).any()


# ---- 10 -----------------------------------------------------------------------------------------------------------------------
def test_baseline_frame_equals_its_unculled_frame(idn, dev, syn):
    net = cc.box_network(dev, "f32", model="baseline")
    frame = _frame(idn, syn)
    bc = syn["bc"].reshape(-1, 3)
    call = lambda: net._render(None, bc, syn["aud"], None, None, net.face_nerf_coarse, net.face_nerf_fine, False, frame=frame)
    ref = call()
    from idealnerf_amd import cull
    grid = cull.build_grid((net.face_nerf_coarse, net.face_nerf_fine), [(syn["aud"], None, None)], [syn["c2w"]], cc.SIZE, cc.SIZE,
                           cc.FOCAL, syn["near"], syn["far"], G=cc.G)
    net.set_cull(head=grid)
    out = call()
    assert 0 < grid.live(frame)[1] < cc.SIZE * cc.SIZE
    for k in ref:
        if k != "z_std":
            assert torch.equal(out[k], ref[k]), k


def test_agg_frame_equals_its_unculled_frame(idn, dev, syn):
    """The feature-aggregation pair on the box scene: its trunk has FaceNeRF's layout (the fused feature takes the audio
    columns' place, aud_gain 0), so the analytic density loads as it is."""
    from idealnerf_amd import cull, synthetic
    from idealnerf_amd.agg_aud_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    import idealnerf_amd
    torch.manual_seed(0)
    net = Network(cc.SIZE, cc.SIZE, cc.FOCAL, syn["near"], syn["far"], 32768, None, cc.S, cc.NI,
                  args=RenderConfig(perturb=0.0, chunk=32768, near=syn["near"], far=syn["far"], dim_expr=79))
    synthetic.box_density_state_dict(net.face_nerf_coarse, 2, cc.CENTRE, cc.HALF, cc.SLOPE)
    synthetic.box_density_state_dict(net.face_nerf_fine, 3, cc.CENTRE, cc.HALF, cc.SLOPE)
    net = net.to(dev).eval()
    idealnerf_amd.set_render_precision(net, "f32")
    expr = torch.from_numpy(np.random.RandomState(4).standard_normal(79).astype(np.float32)).to(dev)
    frame = _frame(idn, syn)
    bc = syn["bc"].reshape(-1, 3)
    call = lambda **kw: net._render(None, bc, syn["aud"], syn["latent"], expr, net.face_nerf_coarse, net.face_nerf_fine, False, frame=frame, **kw)
    ref = call(taps=True)
    grid = cull.build_grid((net.face_nerf_coarse, net.face_nerf_fine), [(syn["aud"], expr, syn["latent"])], [syn["c2w"]], cc.SIZE,
                           cc.SIZE, cc.FOCAL, syn["near"], syn["far"], G=cc.G)
    net.set_cull(head=grid)
    out = call()
    culled = _culled_mask(grid, frame)
    print(f"agg: culled {int(culled.sum())} of {culled.numel()}")
    assert 0 < int(culled.sum()) < culled.numel()
    assert (ref["tap_raw_coarse"][culled][..., 3] <= 0).all() and (ref["tap_raw_fine"][culled][..., 3] <= 0).all()
    for k in ("rgb_map", "rgb0", "acc_map", "acc0", "last_weight", "disp_map", "disp0"):
        assert torch.equal(out[k], ref[k]), k
    assert torch.equal(out["z_std"][~culled], ref["z_std"][~culled]) and not out["z_std"][culled].any()
