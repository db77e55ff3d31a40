"""The ray cull without a GPU: the grid's box and the march step on the host, the refusals before any C call, the analytic
box scene in torch's own arithmetic, and ``cull=None`` leaving the clip flows' calls as they are."""
import ctypes as C

import numpy as np
import pytest
import torch

import cull_common as cc


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()
    return idealnerf_amd


def _cameras(n, seed0=0):
    from idealnerf_amd import synthetic
    return [synthetic.frame(cc.SIZE, cc.SIZE, seed=seed0 + j)["c2w"] for j in range(n)]


@pytest.mark.parametrize("H,W,focal,G", [(48, 48, 128.0, 32), (50, 37, 100.0, 64), (450, 450, 1200.0, 128)])
def test_frustum_box_contains_every_sample_point(idn, H, W, focal, G):
    """Every o + d z, z in [near, far], of random pixels of every camera lies in the box, by at least one cell (fp64)."""
    from idealnerf_amd import cull, synthetic
    cams = _cameras(4)
    lo, cell = cull.frustum_box(cams, H, W, focal, synthetic.NEAR, synthetic.FAR, G)
    rs = np.random.RandomState(0)
    for c in cams:
        o, d = cc.rays64(c.numpy(), H, W, focal)
        pick = np.concatenate([rs.randint(0, H * W, 512), [0, W - 1, (H - 1) * W, H * W - 1]])
        z = np.concatenate([rs.uniform(np.float32(synthetic.NEAR), np.float32(synthetic.FAR), 64),
                            [np.float32(synthetic.NEAR), np.float32(synthetic.FAR)]])
        p = o + d[pick][:, None, :] * z[None, :, None]
        assert (p >= lo + cell * (1 - 1e-9)).all() and (p <= lo + (G - 1) * cell * (1 + 1e-9)).all()
    assert cell > 0


@pytest.mark.parametrize("row0,nrows", [(0, None), (5, 20), (47, 1)])
def test_march_step_obeys_half_a_cell(idn, row0, nrows):
    """dz |d|_max <= cell / 2 for the fp32 dz the kernel receives, with |d|_max over EVERY pixel of the band (fp64), and the
    march is not finer than it has to be: one step fewer would break the bound."""
    from idealnerf_amd import cull, synthetic
    for seed in range(3):
        c2w = synthetic.frame(cc.SIZE, cc.SIZE, seed=seed)["c2w"]
        lo, cell = cull.frustum_box([c2w], cc.SIZE, cc.SIZE, cc.FOCAL, synthetic.NEAR, synthetic.FAR, cc.G)
        _, d = cc.rays64(c2w.numpy(), cc.SIZE, cc.SIZE, cc.FOCAL, row0, nrows)
        d_max = np.sqrt((d * d).sum(1)).max()
        corner = cull.corner_dirs(c2w, cc.SIZE, cc.SIZE, cc.FOCAL, None, None, row0, nrows)
        assert np.sqrt((corner * corner).sum(1)).max() == pytest.approx(d_max, rel=1e-12)   # the maximum sits at a corner pixel
        dz, K = cull.march_steps(cell, d_max, synthetic.NEAR, synthetic.FAR)
        assert dz == float(np.float32(dz)) and dz * d_max <= 0.5 * cell
        span = float(np.float32(synthetic.FAR)) - float(np.float32(synthetic.NEAR))
        assert (K - 1) * dz < span <= K * dz * (1 + 1e-6)            # z_K = far is the last, possibly shorter, step
        assert K == 1 or span / (K - 1) * d_max > 0.5 * cell * (1 - 2e-6)


def _frame(idn, c2w=None, **kw):
    from idealnerf_amd import synthetic
    syn = synthetic.frame(cc.SIZE, cc.SIZE, seed=0)
    return idn.ops.make_frame(syn["c2w"] if c2w is None else c2w, cc.SIZE, cc.SIZE, cc.FOCAL, syn["near"], syn["far"], **kw), syn


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"C call {name} after an argument that must be refused before it")


def test_refusals_come_before_any_c_call(idn, monkeypatch):
    """taps / retraw / white_bkgd / raw_noise_std / a fused arrangement with a grid installed, and a grid whose box does not
    hold the frame's frustum: IdealNerfError, named, with the library unreachable."""
    from idealnerf_amd import cull, synthetic
    from idealnerf_amd.audio_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    E = idn._lib.IdealNerfError
    net = Network(cc.SIZE, cc.SIZE, cc.FOCAL, synthetic.NEAR, synthetic.FAR, 8192, None, cc.S, cc.NI,
                  args=RenderConfig(perturb=0.0, near=synthetic.NEAR, far=synthetic.FAR)).eval()
    frame, syn = _frame(idn)
    lo, cell = cull.frustum_box([syn["c2w"]], cc.SIZE, cc.SIZE, cc.FOCAL, syn["near"], syn["far"], cc.G)
    grid = cull.CullGrid(None, None, cc.G, lo, cell, 1, 0.0)
    net.set_cull(head=grid)
    monkeypatch.setattr(idn._lib, "load", lambda: _NoLibrary())
    bc = syn["bc"].reshape(-1, 3)
    call = lambda **kw: net._render(None, bc, syn["aud"], syn["latent"], syn["expr"], net.face_nerf_coarse, net.face_nerf_fine, False,
                                    frame=frame, **kw)
    for kw, word in ((dict(taps=True), "taps"), (dict(retraw=True), "retraw"), (dict(white_bkgd=True), "white_bkgd"),
                     (dict(raw_noise_std=0.5), "raw_noise_std"), (dict(lindisp=True), "lindisp")):
        with pytest.raises(E, match=word):
            call(**kw)
    monkeypatch.setattr(idn.ops, "FUSED_MARCH_DEFAULT", 1)
    with pytest.raises(E, match="fused"):
        call()
    monkeypatch.setattr(idn.ops, "FUSED_MARCH_DEFAULT", 0)
    # another camera position, a wider frame, a farther far plane: the frustum leaves the box
    moved = syn["c2w"].clone()
    moved[0, 3] += 0.2
    for other in (idn.ops.make_frame(moved, cc.SIZE, cc.SIZE, cc.FOCAL, syn["near"], syn["far"]),
                  idn.ops.make_frame(syn["c2w"], cc.SIZE, cc.SIZE, cc.FOCAL / 2, syn["near"], syn["far"]),
                  idn.ops.make_frame(syn["c2w"], cc.SIZE, cc.SIZE, cc.FOCAL, syn["near"], syn["far"] + 0.1)):
        with pytest.raises(E, match="does not contain"):
            net._render(None, bc, syn["aud"], syn["latent"], syn["expr"], net.face_nerf_coarse, net.face_nerf_fine, False, frame=other)
    # a row band of the grid's own frame is inside
    grid.check_contains(idn.ops.make_frame(syn["c2w"], cc.SIZE, cc.SIZE, cc.FOCAL, syn["near"], syn["far"], 5, 20))
    # removing the grid restores the ordinary route (which refuses the host tensors of this test, as it always has)
    net.set_cull(head=None)
    with pytest.raises(E, match="GPU"):
        call()
    # wrappers: sizes and options are checked before the call too
    with pytest.raises(E, match="multiple of 32"):
        idn.ops.cull_cells(torch.zeros(41 ** 3, dtype=torch.uint8), 40, 1)
    with pytest.raises(E, match="dilate"):
        idn.ops.cull_cells(torch.zeros(33 ** 3, dtype=torch.uint8), 32, -1)
    with pytest.raises(E, match="corners"):
        idn.ops.cull_cells(torch.zeros(33 ** 3 - 1, dtype=torch.uint8), 32, 1)
    with pytest.raises(E, match="cull= takes"):
        cull.options(dict(grid=32))
    assert cull.options(None) is None and cull.options(dict(G=64))["dilate"] == 1


def test_c_entries_refuse_bad_arguments_without_a_gpu(idn):
    lib, L = idn._lib.load(), idn._lib
    assert lib.idealnerf_cull_mark(None, 4, 0.0, None, None) == -1 and b"NULL" in lib.idealnerf_last_error()
    assert lib.idealnerf_cull_mark(None, 0, 0.0, None, None) == 0
    assert lib.idealnerf_cull_cells(1, 40, 1, 1, None) == -1 and b"multiple of 32" in lib.idealnerf_last_error()
    assert lib.idealnerf_cull_cells(1, 32, -1, 1, None) == -1 and b"dilate" in lib.idealnerf_last_error()
    frame, _ = _frame(idn)
    g = L.CullGridStruct()
    g.bits, g.G, g.cell = 1, 32, 0.02
    n = cc.SIZE * cc.SIZE
    need = lib.idealnerf_cull_classify_workspace_bytes(n)
    assert need == (n // 256) * (4 * 8 + 2 * 4) and lib.idealnerf_cull_classify_workspace_bytes(0) == 0
    assert lib.idealnerf_cull_classify(C.byref(g), C.byref(frame), 0.01, 0, 1, 1, 1, need, None) == -1 and b"march" in lib.idealnerf_last_error()
    assert lib.idealnerf_cull_classify(C.byref(g), C.byref(frame), 0.01, 60, 1, 1, 1, need - 1, None) == -4
    g.G = 48
    assert lib.idealnerf_cull_classify(C.byref(g), C.byref(frame), 0.01, 60, 1, 1, 1, need, None) == -1
    assert lib.idealnerf_cull_gather(1, n + 1, C.byref(frame), 1, 1, 1, None) == -1 and lib.idealnerf_cull_gather(None, 0, C.byref(frame), None, None, None, None) == 0
    o = (L.CullOutput * 1)()
    o[0].dense, o[0].channels = 1, 2
    assert lib.idealnerf_cull_scatter(None, 0, n, 1, o, 1, None) == -1 and b"channels" in lib.idealnerf_last_error()
    o[0].channels, o[0].fill_background = 1, 1
    assert lib.idealnerf_cull_scatter(None, 0, n, 1, o, 1, None) == -1 and b"background" in lib.idealnerf_last_error()
    assert lib.idealnerf_cull_scatter(None, 0, n, 1, o, L.CULL_MAX_OUTPUTS + 1, None) == -1
    assert lib.idealnerf_cull_scatter(None, n + 1, n, 1, o, 1, None) == -1


def _trunk_sigma(module, pts, aud):
    """sigma_raw of FaceNeRF's trunk in torch's own arithmetic (models/face_nerf.py:40-66 upstream): the encoded point with
    the conditioning appended, eight layers with the skip after layer 4, alpha_linear."""
    from idealnerf_amd.helper import get_embedder
    embed, ch = get_embedder((module.input_xyz_ch - 3) // 6, 0)
    cond = torch.cat([aud, torch.zeros(module.dim_expr), torch.ones(module.dim_latent)])
    x = torch.cat([embed(pts), cond.expand(pts.shape[0], -1)], -1)
    h = x
    for i, lin in enumerate(module.pts_linears):
        h = torch.relu(lin(h))
        if i in module.skips:
            h = torch.cat([x, h], -1)
    return module.alpha_linear(h)[:, 0]


@pytest.mark.parametrize("aud0,aud_gain", [(0.0, 0.0), (1.0, 0.05), (-0.5, 0.05)])
def test_box_density_has_the_stated_sign(idn, aud0, aud_gain):
    """sigma_raw == 1 at points at least 2 / slope inside the box, < 0 at points at least 2 / slope (L-infinity) outside it."""
    from idealnerf_amd import synthetic
    from idealnerf_amd.models.face_nerf import FaceNeRF
    m = synthetic.box_density_state_dict(FaceNeRF(dim_aud=64, dim_expr=76, dim_latent=32), 7, (0.01, -0.02, 0.03), cc.HALF, cc.SLOPE, aud_gain)
    centre, half = np.array([0.01, -0.02, 0.03]), cc.HALF + aud_gain * aud0
    rs = np.random.RandomState(1)
    aud = torch.from_numpy(rs.standard_normal(64).astype(np.float32))
    aud[0] = aud0
    inside = centre + rs.uniform(-(half - 2 / cc.SLOPE), half - 2 / cc.SLOPE, (2000, 3))
    outside = centre + rs.uniform(-0.5, 0.5, (8000, 3))
    outside = outside[np.abs(outside - centre).max(1) >= half + 2 / cc.SLOPE]
    with torch.no_grad():
        s_in = _trunk_sigma(m, torch.from_numpy(inside.astype(np.float32)), aud)
        s_out = _trunk_sigma(m, torch.from_numpy(outside.astype(np.float32)), aud)
    assert len(outside) > 1000
    assert torch.equal(s_in, torch.ones_like(s_in))
    assert float(s_out.max()) <= -1.0 + 1e-3          # 1 - slope * excess, excess >= 2 / slope (fp32 rounding of the excess)
    # the colour branch is the seeded Xavier one
    ref = synthetic.xavier_state_dict(FaceNeRF(dim_aud=64, dim_expr=76, dim_latent=32), 7)
    for k in ("views_linears.0.weight", "views_linears.2.weight", "rgb_linear.weight", "rgb_linear.bias"):
        assert torch.equal(m.state_dict()[k], ref.state_dict()[k])


class _StubNetwork(torch.nn.Module):
    """Records every attribute the flows touch beyond parameters / eval / train / the forward call."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def set_cull(self, **kw):
        self.calls.append(("set_cull", kw))

    def forward(self, inputs):
        self.calls.append(("forward", int(inputs[0][-1])))
        raise _Stop()


class _Stop(Exception):
    pass


def test_cull_none_leaves_the_clip_calls_as_they_are(idn, monkeypatch):
    """cull=None: the flows never import cull.py's builder, never call set_cull, and reach the network's forward as before."""
    from idealnerf_amd import clip, cull

    class Frames:
        data_size, H, W = 2, 4, 4

        def frame(self, j):
            return tuple(torch.zeros(1) for _ in range(7)) + (torch.tensor(j),)

    monkeypatch.setattr(cull, "build_grid", lambda *a, **k: pytest.fail("build_grid with cull=None"))
    monkeypatch.setattr(idn.ops, "frame_scores_workspace_doubles", lambda H, W: 1)
    net = _StubNetwork()
    with pytest.raises(_Stop):
        clip.score_head_clip(net, Frames(), 0, latent_code=torch.zeros(1), cull=None)
    assert net.calls == [("forward", 0)]
    # with cull set the grid is built first, installed, and removed although the body raised
    net.calls.clear()
    monkeypatch.setattr(clip, "_head_grid", lambda *a: dict(head="GRID"))
    with pytest.raises(_Stop):
        clip.score_head_clip(net, Frames(), 0, latent_code=torch.zeros(1), cull=dict(G=32))
    assert net.calls == [("set_cull", dict(head="GRID")), ("forward", 0), ("set_cull", dict(head=None, torso=None))]
