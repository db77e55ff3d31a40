"""The sample cull on the device (csrc/cull.hip: cull_sample_*; ops.render_rays_sparse_fwd; cull.py's ``samples``): the
classification against its numpy fp32 restatement exactly (tests/cull_samples_common.py), gather and scatter bit for bit, and
the sample-culled frame against the ray-culled and the unculled frame with torch.equal, on the analytic box scene of
tests/cull_common.py -- 48 x 48 at focal 128, S = 64, Ni = 128, G = 32, and the ragged band (50, 37, 5, 20)."""
import numpy as np
import pytest
import torch

import cull_common as cc
import cull_samples_common as sc

pytestmark = pytest.mark.gpu

SHAPES = [(48, 48, 0, 48), (50, 37, 5, 20)]


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


@pytest.fixture(scope="module")
def net32(dev, idn):
    return cc.box_network(dev, "f32")


def _frame(idn, syn, H=cc.SIZE, W=cc.SIZE, row0=0, nrows=None):
    return idn.ops.make_frame(syn["c2w"], H, W, cc.FOCAL, syn["near"], syn["far"], row0, nrows)


def _grid(net, syn, H=cc.SIZE, W=cc.SIZE, samples=True, dilate=1):
    from idealnerf_amd import cull
    return cull.build_grid((net.face_nerf_coarse, net.face_nerf_fine), [(syn["aud"], syn["expr"], syn["latent"])], [syn["c2w"]], H, W,
                           cc.FOCAL, syn["near"], syn["far"], G=cc.G, dilate=dilate, samples=samples)


def _render(net, syn, frame, with_fg=True, taps=False):
    bc = syn["bc"].reshape(-1, 3)[frame.row0 * frame.W:(frame.row0 + frame.nrows) * frame.W]
    return net._render(None, bc, syn["aud"], syn["latent"], syn["expr"], net.face_nerf_coarse, net.face_nerf_fine, with_fg, taps=taps,
                       frame=frame)


def _three_frames(net, grid, render):
    """(unculled, ray-culled, sample-culled) of one render call; the grid's counters cover the sample-culled one alone."""
    net.set_cull()
    plain = render()
    try:
        grid.samples = False
        net.set_cull(head=grid)
        by_ray = render()
        grid.samples = True
        grid.points_seen = grid.points_evaluated = 0
        by_sample = render()
    finally:
        net.set_cull()
    return plain, by_ray, by_sample


def _record_passes(idn, monkeypatch):
    """Every sample classification of the renders that follow: a list of (rays, z, n_live) on the host."""
    seen, real = [], idn.ops.cull_sample_classify

    def wrapper(bits, G, lo, cell, rays, z, *a, **k):
        sel, n = real(bits, G, lo, cell, rays, z, *a, **k)
        seen.append((rays.cpu().numpy(), z.cpu().numpy(), int(n.item())))
        return sel, n

    monkeypatch.setattr(idn.ops, "cull_sample_classify", wrapper)
    return seen


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,row0,nrows", SHAPES)
def test_classification_equals_the_restatement(idn, dev, net32, syn, H, W, row0, nrows):
    from idealnerf_amd.helper import linspace01
    ops = idn.ops
    assert float(ops._lib.load().idealnerf_colour_gate_max_dist()) == float(sc.MAX_DIST)
    g = _grid(net32, syn, H, W)
    occ = cc.unpack(g.bits, g.G)
    rays = ops.frame_rays(syn["c2w"], H, W, cc.FOCAL, syn["near"], syn["far"], row0, nrows, device=dev)
    n = rays.shape[0]
    bc = syn["bc"].reshape(-1, 3)[:n].contiguous()
    coarse = net32.face_nerf_coarse
    z_c = ops.coarse_depths(rays, linspace01(cc.S, dev))
    raw = ops.query_rays_fwd(coarse.packed_weights(), coarse.folded_bias(syn["aud"], syn["expr"], syn["latent"]), rays, z_c, coarse.prec_code)
    z_f = ops.march_fwd(raw, z_c, rays, bc, linspace01(cc.NI, dev), cc.NI)["z_fine"]
    assert z_f.shape == (n, cc.S + cc.NI) and bool((z_f[:, 1:] >= z_f[:, :-1]).all())
    # by hand: sample 5 pulled back towards sample 4, so the gap to sample 6 is 0.0185 |d| > 0.0125 -- in front of the box,
    # where every cell is clear
    z_h = z_c.clone()
    z_h[:, 5] -= 0.009
    total = ambiguous = 0
    cases = [("coarse", rays, z_c), ("fine", rays, z_f), ("hand", rays, z_h)]
    if n % 4 == 0 and row0:
        # S is a multiple of 64, so the band's 740 rays still fill whole workgroups of 256 points: without its last ray the
        # coarse and the fine array both end inside a workgroup (and inside a wave)
        cases += [("coarse, 739 rays", rays[:-1].contiguous(), z_c[:-1].contiguous()), ("fine, 739 rays", rays[:-1].contiguous(), z_f[:-1].contiguous())]
        assert ((n - 1) * cc.S) % 256 and ((n - 1) * (cc.S + cc.NI)) % 256
    for name, rays, z in cases:
        want = sc.np_sample_live(occ, g.G, g.lo, g.cell, rays.cpu().numpy(), z.cpu().numpy())
        live64, amb = sc.model64(occ, g.G, g.lo, g.cell, rays.cpu().numpy(), z.cpu().numpy())
        sel, n_dev = ops.cull_sample_classify(g.bits, g.G, g.lo, g.cell, rays, z)
        m = int(n_dev.item())
        got = sel[:m].cpu().numpy()
        print(f"{H}x{W} rows {row0}+{nrows} {name}: live {m} of {want.size} ({m / want.size:.4f}), fp64 model differs at "
              f"{int((want != live64).sum())}, ambiguous {amb.mean():.5f}")
        assert sel.dtype == torch.int64 and sel.shape == (want.size,)
        assert m == int(want.sum())
        np.testing.assert_array_equal(got, np.nonzero(want.reshape(-1))[0])
        assert (np.diff(got) > 0).all()
        assert not ((want != live64) & ~amb).any(), "restatement and fp64 model differ away from a cell face and the threshold"
        assert 0 < m < want.size
        total, ambiguous = total + amb.size, ambiguous + int(amb.sum())
        sel2, n2 = ops.cull_sample_classify(g.bits, g.G, g.lo, g.cell, rays, z)
        assert int(n2.item()) == m and torch.equal(sel2[:m], sel[:m])
        if name == "hand":
            p5 = sc.np_points(rays.cpu().numpy(), z.cpu().numpy())[:, 5]
            assert not sc.np_occupied(occ, g.G, g.lo, g.cell, p5).any() and want[:, 5].all() and not want[:, 4].any()
    assert ambiguous / total <= sc.AMBIGUOUS_CAP


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16x6", "bf16"])
def test_gather_and_scatter(idn, dev, syn, precision):
    from idealnerf_amd.helper import linspace01
    ops = idn.ops
    H, W, row0, nrows = SHAPES[1]
    net = cc.box_network(dev, precision)
    g = _grid(net, syn, H, W)
    rays = ops.frame_rays(syn["c2w"], H, W, cc.FOCAL, syn["near"], syn["far"], row0, nrows, device=dev)
    n = rays.shape[0]
    z = ops.coarse_depths(rays, linspace01(cc.S, dev))
    sel, n_dev = ops.cull_sample_classify(g.bits, g.G, g.lo, g.cell, rays, z)
    m = int(n_dev.item())
    assert 0 < m < n * cc.S
    pts, dirs = ops.cull_sample_gather(sel[:m], rays, z)
    idx = sel[:m].cpu().numpy()
    want_p = sc.np_points(rays.cpu().numpy(), z.cpu().numpy()).reshape(-1, 3)[idx]
    np.testing.assert_array_equal(pts.cpu().numpy().view(np.uint32), want_p.view(np.uint32))
    np.testing.assert_array_equal(dirs.cpu().numpy().view(np.uint32), rays.cpu().numpy()[idx // cc.S, 8:11].view(np.uint32))
    fine = net.face_nerf_fine
    packed, folded = fine.packed_weights(), fine.folded_bias(syn["aud"], syn["expr"], syn["latent"])
    raw_live = ops.query_points_fwd(packed, folded, pts.view(m, 1, 3), dirs, fine.prec_code).view(m, 4)
    raw = ops.cull_sample_scatter(sel, m, raw_live, n, cc.S)
    full = ops.query_rays_fwd(packed, folded, rays, z, fine.prec_code)
    live = torch.zeros(n * cc.S, dtype=torch.bool, device=dev)
    live[sel[:m]] = True
    assert raw.shape == (n, cc.S, 4)
    assert torch.equal(raw.view(-1, 4)[live], full.view(-1, 4)[live])
    assert not _bits(raw.view(-1, 4)[~live]).any(), "a skipped sample is +0.0 in all four channels"
    assert (full.view(-1, 4)[~live][:, 3] <= 0).all()                   # the contract on this scene: nothing skipped has density
    assert torch.equal(_bits(ops.cull_sample_scatter(sel, m, raw_live, n, cc.S)), _bits(raw))
    empty = ops.cull_sample_scatter(None, 0, None, n, cc.S, device=dev)
    assert empty.shape == (n, cc.S, 4) and not _bits(empty).any()


# ---- 3, 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16x6"])
def test_sample_culled_frame_equals_ray_culled_and_unculled(idn, dev, syn, net32, precision, monkeypatch):
    net = net32 if precision == "f32" else cc.box_network(dev, precision)
    frame = _frame(idn, syn)
    grid = _grid(net, syn)
    assert grid.samples is True
    occ = cc.unpack(grid.bits, grid.G)
    passes = _record_passes(idn, monkeypatch)
    plain, by_ray, by_sample = _three_frames(net, grid, lambda: _render(net, syn, frame))
    for k in cc.OUTPUTS:
        assert torch.equal(by_sample[k], plain[k]) and torch.equal(by_sample[k], by_ray[k]), k
    assert torch.equal(by_sample["z_std"], by_ray["z_std"])
    assert set(by_sample) == set(by_ray)
    # the share the grid reports is the restatement's, and the cull does cull
    n_live = grid.live(frame)[1]
    assert [z.shape for _, z, _ in passes] == [(n_live, cc.S), (n_live, cc.S + cc.NI)]
    want = [int(sc.np_sample_live(occ, grid.G, grid.lo, grid.cell, r, z).sum()) for r, z, _ in passes]
    assert [m for _, _, m in passes] == want
    assert grid.points_seen == n_live * (2 * cc.S + cc.NI) and grid.points_evaluated == sum(want)
    assert grid.evaluated_share == sum(want) / grid.points_seen and 0 < grid.evaluated_share < 1
    print(f"{precision}: live rays {n_live} of {frame.nrows * frame.W}, evaluated share {grid.evaluated_share:.4f} "
          f"(coarse {want[0] / (n_live * cc.S):.4f}, fine {want[1] / (n_live * (cc.S + cc.NI)):.4f})")
    from idealnerf_amd import cull
    assert cull.summary(dict(head=grid, torso=None))["evaluated_share"] == dict(head=grid.evaluated_share)
    grid.samples = False
    assert "evaluated_share" not in cull.summary(dict(head=grid))


def test_everything_marked_evaluates_everything(idn, dev, syn):
    net = cc.box_network(dev, "f32", sigma_bias=1000.0)
    frame = _frame(idn, syn)
    grid = _grid(net, syn)
    assert grid.occupied_share == 1.0
    plain, by_ray, by_sample = _three_frames(net, grid, lambda: _render(net, syn, frame))
    assert grid.points_seen == cc.SIZE * cc.SIZE * (2 * cc.S + cc.NI) and grid.evaluated_share == 1.0
    for k in cc.OUTPUTS + ("z_std",):
        assert torch.equal(by_sample[k], plain[k]) and torch.equal(by_sample[k], by_ray[k]), k


def test_nothing_occupied_launches_no_network(idn, dev, syn):
    from idealnerf_amd.helper import linspace01
    net = cc.box_network(dev, "f32", sigma_bias=-1.0)
    frame = _frame(idn, syn)
    grid = _grid(net, syn)
    assert grid.occupied_share == 0.0 and grid.samples
    ref = _render(net, syn, frame)
    net.set_cull(head=grid)
    idn.ops.profile_begin()
    out = _render(net, syn, frame)
    _, launches, points = idn.ops.profile_end()
    net.set_cull()
    assert launches == 0 and points == 0 and grid.points_seen == 0
    for k in cc.OUTPUTS:
        assert torch.equal(out[k], ref[k]), k
    # the sparse render itself, on every ray of the frame: both passes find nothing to evaluate
    rays = idn.ops.frame_rays(syn["c2w"], cc.SIZE, cc.SIZE, cc.FOCAL, syn["near"], syn["far"], device=dev)
    bc = syn["bc"].reshape(-1, 3)
    c, f = net.face_nerf_coarse, net.face_nerf_fine
    cond = (syn["aud"], syn["expr"], syn["latent"])
    args = (rays, bc, c.packed_weights(), c.folded_bias(*cond), f.packed_weights(), f.folded_bias(*cond), linspace01(cc.S, dev),
            linspace01(cc.NI, dev), cc.NI)
    idn.ops.profile_begin()
    sparse = idn.ops.render_rays_sparse_fwd(grid, *args, with_fg=True, precision=c.prec_code, precision_fine=f.prec_code)
    _, launches, points = idn.ops.profile_end()
    assert launches == 0 and points == 0
    assert grid.points_seen == rays.shape[0] * (2 * cc.S + cc.NI) and grid.points_evaluated == 0
    dense = idn.ops.render_rays_fwd(*args, with_fg=True, precision=c.prec_code, precision_fine=f.prec_code)
    assert set(sparse) == set(dense)
    for k in dense:
        assert torch.equal(sparse[k], dense[k]), k
    assert torch.equal(sparse["rgb_map"], bc)
    idn.ops.profile_begin()                         # (the counter does count: the dense render launches both networks)
    idn.ops.render_rays_fwd(*args, with_fg=True, precision=c.prec_code, precision_fine=f.prec_code)
    assert idn.ops.profile_end()[1] >= 2


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_kernel", [False, True])
def test_perturb_with_a_seed(idn, dev, syn, in_kernel, monkeypatch):
    net = cc.box_network(dev, "f32", perturb=1.0)
    net.in_kernel_draws = in_kernel
    frame = _frame(idn, syn)
    grid = _grid(net, syn)
    occ = cc.unpack(grid.bits, grid.G)
    passes = _record_passes(idn, monkeypatch)

    def render():
        torch.manual_seed(5)
        return _render(net, syn, frame)

    _, by_ray, by_sample = _three_frames(net, grid, render)
    assert set(by_sample) == set(by_ray)
    for k in by_ray:
        assert torch.equal(by_sample[k], by_ray[k]), k
    bc = syn["bc"].reshape(-1, 3)
    assert (by_sample["rgb_map"] != bc).any() and all(torch.isfinite(v).all() for v in by_sample.values())
    # jittered gaps above the threshold in clear cells were there, and were evaluated
    wide = 0
    for rays, z, m in passes:
        with np.errstate(invalid="ignore"):
            far_apart = np.abs(sc.np_dist(rays, z)) > sc.MAX_DIST
        clear = ~sc.np_occupied(occ, grid.G, grid.lo, grid.cell, sc.np_points(rays, z))[:, :-1]
        live = sc.np_sample_live(occ, grid.G, grid.lo, grid.cell, rays, z)
        assert m == int(live.sum()) and live[:, :-1][far_apart].all()
        wide += int((far_apart & clear).sum())
    print(f"in_kernel = {in_kernel}: {wide} samples in clear cells with a gap above the threshold")
    assert len(passes) == 2 and wide >= 1
    assert 0 < grid.evaluated_share < 1


def test_chunks_do_not_change_the_result(idn, dev, syn, net32):
    """The sparse render in chunks of 1000 rays (the last one of 304) against the dense render of all rays at once: per-ray
    tensor draws are sliced per chunk, in-kernel draws continue at row ray0 + the chunk's first ray."""
    from idealnerf_amd.helper import linspace01
    ops = idn.ops
    grid = _grid(net32, syn)
    rays = ops.frame_rays(syn["c2w"], cc.SIZE, cc.SIZE, cc.FOCAL, syn["near"], syn["far"], device=dev)
    n = rays.shape[0]
    bc = syn["bc"].reshape(-1, 3)
    c, f = net32.face_nerf_coarse, net32.face_nerf_fine
    cond = (syn["aud"], syn["expr"], syn["latent"])
    nets = (c.packed_weights(), c.folded_bias(*cond), f.packed_weights(), f.folded_bias(*cond), linspace01(cc.S, dev))
    kw = dict(with_fg=True, precision=c.prec_code, precision_fine=f.prec_code)
    g = torch.Generator(device=dev).manual_seed(3)
    t_rand, u = torch.rand((n, cc.S), device=dev, generator=g), torch.rand((n, cc.NI), device=dev, generator=g)
    for draws in (dict(u=u, t_rand=t_rand), dict(u=None, draws=(1234567, 7)), dict(u=linspace01(cc.NI, dev))):
        u_arg = draws.pop("u")
        dense = ops.render_rays_fwd(rays, bc, *nets, u_arg, cc.NI, **draws, **kw)
        sparse = ops.render_rays_sparse_fwd(grid, rays, bc, *nets, u_arg, cc.NI, chunk=1000, **draws, **kw)
        assert set(sparse) == set(dense)
        for k in dense:
            assert sparse[k].shape == dense[k].shape and torch.equal(sparse[k], dense[k]), (sorted(draws), k)
    assert grid.points_seen == 3 * n * (2 * cc.S + cc.NI) and 0 < grid.evaluated_share < 1
    none = ops.render_rays_sparse_fwd(grid, rays[:0], bc[:0], *nets, linspace01(cc.NI, dev), cc.NI, **kw)
    assert {k: tuple(v.shape) for k, v in none.items()} == {k: (0,) + tuple(v.shape[1:]) for k, v in dense.items()}


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_head_pair_without_fg_and_without_importance_samples(idn, dev, syn, net32):
    frame = _frame(idn, syn)
    grid = _grid(net32, syn)
    plain, by_ray, by_sample = _three_frames(net32, grid, lambda: _render(net32, syn, frame, with_fg=False))
    assert set(by_sample) == set(by_ray) and "rgb_map_fg" not in by_sample
    for k in by_ray:
        assert torch.equal(by_sample[k], by_ray[k]), k
        assert k == "z_std" or torch.equal(by_sample[k], plain[k]), k
    # n_importance = 0: the coarse pass and the compositing alone
    net = cc.box_network(dev, "f32")
    net.args.N_importance = 0
    from idealnerf_amd import cull
    grid = cull.build_grid((net.face_nerf_coarse,), [(syn["aud"], syn["expr"], syn["latent"])], [syn["c2w"]], cc.SIZE, cc.SIZE, cc.FOCAL,
                           syn["near"], syn["far"], G=cc.G, samples=True)
    for with_fg in (False, True):
        plain, by_ray, by_sample = _three_frames(net, grid, lambda: _render(net, syn, frame, with_fg=with_fg))
        assert set(by_sample) == set(by_ray) and "rgb0" not in by_sample
        for k in by_ray:
            assert torch.equal(by_sample[k], by_ray[k]) and torch.equal(by_sample[k], plain[k]), k
        assert grid.points_seen == grid.live(frame)[1] * cc.S and 0 < grid.evaluated_share < 1


def test_torso_pair_equals_its_ray_culled_frame(idn, dev, syn):
    from idealnerf_amd import cull
    net = cc.box_network(dev, "f32", model="torso")
    frame = _frame(idn, syn)
    bc = syn["bc"].reshape(-1, 3)
    aud = torch.from_numpy(np.random.RandomState(6).standard_normal(net.torso_coarse_nerf.dim_aud).astype(np.float32)).to(dev)
    pair = (net.torso_coarse_nerf, net.torso_fine_nerf)
    grid = cull.build_grid(pair, [(aud, None, None)], [syn["c2w"]], cc.SIZE, cc.SIZE, cc.FOCAL, syn["near"], syn["far"], G=cc.G, samples=True)
    render = lambda: net._render(None, bc, aud, None, None, *pair, True, frame=frame)
    ref = render()
    try:
        grid.samples = False
        net.set_cull(torso=grid)
        by_ray = render()
        grid.samples = True
        by_sample = render()
    finally:
        net.set_cull()
    assert 0 < grid.live(frame)[1] < cc.SIZE * cc.SIZE and 0 < grid.evaluated_share < 1
    assert set(by_sample) == set(by_ray)
    for k in by_ray:
        assert torch.equal(by_sample[k], by_ray[k]), k
        assert k == "z_std" or torch.equal(by_sample[k], ref[k]), k


def test_baseline_and_agg_pairs_equal_their_ray_culled_frames(idn, dev, syn):
    import idealnerf_amd
    from idealnerf_amd import cull, synthetic
    from idealnerf_amd.agg_aud_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    frame = _frame(idn, syn)
    bc = syn["bc"].reshape(-1, 3)
    base = cc.box_network(dev, "f32", model="baseline")
    torch.manual_seed(0)
    agg = Network(cc.SIZE, cc.SIZE, cc.FOCAL, syn["near"], syn["far"], 32768, None, cc.S, cc.NI,
                  args=RenderConfig(perturb=0.0, chunk=32768, near=syn["near"], far=syn["far"], dim_expr=79))
    synthetic.box_density_state_dict(agg.face_nerf_coarse, 2, cc.CENTRE, cc.HALF, cc.SLOPE)
    synthetic.box_density_state_dict(agg.face_nerf_fine, 3, cc.CENTRE, cc.HALF, cc.SLOPE)
    agg = agg.to(dev).eval()
    idealnerf_amd.set_render_precision(agg, "f32")
    expr = torch.from_numpy(np.random.RandomState(4).standard_normal(79).astype(np.float32)).to(dev)
    for name, net, cond in (("baseline", base, (syn["aud"], None, None)), ("agg", agg, (syn["aud"], expr, syn["latent"]))):
        pair = (net.face_nerf_coarse, net.face_nerf_fine)
        grid = cull.build_grid(pair, [cond], [syn["c2w"]], cc.SIZE, cc.SIZE, cc.FOCAL, syn["near"], syn["far"], G=cc.G, samples=True)
        plain, by_ray, by_sample = _three_frames(net, grid, lambda: net._render(None, bc, cond[0], cond[2], cond[1], *pair, False, frame=frame))
        assert set(by_sample) == set(by_ray), name
        for k in by_ray:
            assert torch.equal(by_sample[k], by_ray[k]), (name, k)
            assert k == "z_std" or torch.equal(by_sample[k], plain[k]), (name, k)
        assert 0 < grid.evaluated_share < 1, name


def test_torso_clip_bytes_with_and_without_samples(idn, dev, syn, tmp_path):
    from idealnerf_amd import clip, synthetic
    net = cc.box_network(dev, "f32", aud_gain=0.0, model="torso")
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]])
    poses = torch.stack([torch.cat([synthetic.frame(cc.SIZE, cc.SIZE, seed=10 + j)["c2w"], bottom], 0) for j in range(8)])
    auds = torch.from_numpy(np.random.RandomState(11).standard_normal((8, 16, 29)).astype(np.float32))
    kw = dict(expr=syn["expr"], latent_code=syn["latent"], torso_pose=torch.cat([syn["c2w"], bottom], 0), frames=range(2), codec="raw")
    by_ray, by_sample = str(tmp_path / "rays.avi"), str(tmp_path / "samples.avi")
    res0 = clip.render_torso_clip(net, poses, auds, syn["bc"], by_ray, cull=dict(G=cc.G), **kw)
    res1 = clip.render_torso_clip(net, poses, auds, syn["bc"], by_sample, cull=dict(G=cc.G, samples=True), **kw)
    assert open(by_ray, "rb").read() == open(by_sample, "rb").read()
    assert "evaluated_share" not in res0["cull"] and res1["nonfinite_frames"] == []
    share = res1["cull"]["evaluated_share"]
    assert set(share) == {"head", "torso"} and 0 < share["head"] < 1 and 0 < share["torso"] < 1
    assert res1["cull"]["live_share"] == res0["cull"]["live_share"]
    assert not getattr(net, "_cull")
