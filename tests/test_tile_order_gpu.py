"""The skewed tile order of the colour-gated fp32 kernel (csrc/tile_order.h) on the device: which CU
renders a tile changes no output bit, every tile is rendered once at every round boundary, and on the shape the order was
made for -- a 512-wide frame, whose row is a whole number of rounds -- the gate still skips exactly the all-dead tiles."""
import pytest
import torch

pytestmark = pytest.mark.gpu

S, NI = 64, 128
BAND_W, BAND_ROWS, BAND_ROW0 = 512, 4, 254


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    return idealnerf_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nets(dev, syn, H, W):
    """The benchmark's pair of networks (seeds 2 / 3, sigma gain 300, bias 0.3), fp32 packing -> (packed_c, folded_c, packed_f, folded_f)"""
    from idealnerf_amd import synthetic
    from idealnerf_amd.audio_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    cfg = RenderConfig(perturb=0.0, chunk=H * W, near=syn["near"], far=syn["far"])
    net = Network(H, W, syn["focal"], syn["near"], syn["far"], 128, None, S, NI, args=cfg).to(dev).eval()
    out = []
    for m, seed in ((net.face_nerf_coarse, 2), (net.face_nerf_fine, 3)):
        synthetic.xavier_state_dict(m, seed, 300.0, 0.3)
        out += [m.packed_weights("f32"), m.folded_bias(syn["aud"].to(dev), syn["expr"].to(dev), syn["latent"].to(dev))]
    return tuple(out)


def _scene(dev, H, W):
    from idealnerf_amd import synthetic
    syn = synthetic.frame(H, W, seed=0)
    return dict(syn=syn, H=H, W=W, bc=syn["bc"].reshape(-1, 3).contiguous().to(dev), t=torch.linspace(0.0, 1.0, S).to(dev),
                u=torch.linspace(0.0, 1.0, NI).to(dev), nets=_nets(dev, syn, H, W))


def _render(idn, scene, gate, dev, rays=None, bc=None, frame=None, fused=0, **kw):
    """-> (outputs, counters [2, 2] on the host: (coarse, fine) x (tiles, skipped))"""
    counters = torch.zeros((2, 2), dtype=torch.int64, device=dev)
    out = idn.ops.render_rays_fwd(rays, bc, *scene["nets"], scene["t"], scene["u"], NI, with_fg=True, fused=fused, frame=frame,
                                  colour_gate=gate, gate_counters=counters, **kw)
    torch.cuda.synchronize()
    return out, counters.cpu()


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: {what} (max diff {(a[k].double() - b[k].double()).abs().max().item():.3e})"


def _tiles(points):
    return (points + 127) // 128


# ---- (a) round boundaries: ray-record renders around one and two rounds of the device's own grid ----

@pytest.fixture(scope="module")
def small(idn, dev):
    scene = _scene(dev, 64, 64)
    syn = scene["syn"]
    scene["rays"] = idn.ops.frame_rays(syn["c2w"][:3, :4], 64, 64, syn["focal"], syn["near"], syn["far"], device=dev)
    scene["G"] = torch.cuda.get_device_properties(dev).multi_processor_count
    return scene


# coarse tiles (64 n / 128 = n / 2) = G - 1, G, G + 1, 2G - 1, 2G + 1; with 256 CUs: n = 510, 512, 514, 1022, 1026 rays
@pytest.mark.parametrize("case", ["G-1", "G", "G+1", "2G-1", "2G+1", "n=1", "n=3"])
def test_round_boundaries(idn, dev, small, case):
    G = small["G"]
    n = {"G-1": 2 * (G - 1), "G": 2 * G, "G+1": 2 * (G + 1), "2G-1": 2 * (2 * G - 1), "2G+1": 2 * (2 * G + 1), "n=1": 1, "n=3": 3}[case]
    assert n <= small["rays"].shape[0]
    rays, bc = small["rays"][:n].contiguous(), small["bc"][:n].contiguous()
    gated, cnt = _render(idn, small, True, dev, rays=rays, bc=bc)
    plain, cnt_plain = _render(idn, small, False, dev, rays=rays, bc=bc)
    print(f"{case}: G = {G}, n = {n}, counters (coarse, fine) x (tiles, skipped): {cnt.tolist()}")
    assert cnt_plain.sum().item() == 0
    assert cnt[:, 0].tolist() == [_tiles(n * S), _tiles(n * (S + NI))]
    if n > 3:
        assert cnt[0, 0].item() == {"G-1": G - 1, "G": G, "G+1": G + 1, "2G-1": 2 * G - 1, "2G+1": 2 * G + 1}[case]
    _same(gated, plain, "gated != ungated")


# ---- (b), (c) the resonant shape: a band of a 512-wide frame, 256 coarse tiles per row ----

@pytest.fixture(scope="module")
def band(idn, dev):
    scene = _scene(dev, BAND_W, BAND_W)
    syn = scene["syn"]
    scene["frame"] = lambda: idn.ops.make_frame(syn["c2w"][:3, :4], BAND_W, BAND_W, syn["focal"], syn["near"], syn["far"],
                                                row0=BAND_ROW0, nrows=BAND_ROWS)
    scene["bc_band"] = scene["bc"][BAND_ROW0 * BAND_W:(BAND_ROW0 + BAND_ROWS) * BAND_W].contiguous()
    scene["gated"] = _render(idn, scene, True, dev, bc=scene["bc_band"], frame=scene["frame"]())
    return scene


def _dead_tiles(raw, z, rays, kmax):
    """All-dead 128-point tiles of one pass, by the gate's predicate (mlp_common.h: gate_point_dead) in fp32 on the host:
    a ray's last sample, or sigma <= 0 across a spacing |(z[s+1] - z[s]) * |d|| <= kmax.  raw [n, s, 4], z [n, s], rays [n, 11]."""
    raw, z, d = raw.cpu(), z.cpu(), rays.cpu()[:, 3:6]
    dn = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    dist = (z[:, 1:] - z[:, :-1]) * dn[:, None]
    dead = torch.ones(z.shape, dtype=torch.bool)
    dead[:, :-1] = (raw[:, :-1, 3] <= 0.0) & (dist.abs() <= kmax)
    dead = dead.reshape(-1)
    assert dead.numel() % 128 == 0
    return int(dead.reshape(-1, 128).all(1).sum())


def test_resonant_band(idn, dev, band):
    n = BAND_ROWS * BAND_W
    gated, cnt = band["gated"]
    plain, _ = _render(idn, band, False, dev, bc=band["bc_band"], frame=band["frame"]())
    _same(gated, plain, "gated != ungated")
    # the independent count: a raw tap turns the gate off, so these raw outputs come from the ungated instruction stream
    tapped, cnt_tapped = _render(idn, band, False, dev, bc=band["bc_band"], frame=band["frame"](), taps=True)
    assert cnt_tapped.sum().item() == 0
    kmax = float(idn._lib.load().idealnerf_colour_gate_max_dist())
    want_c = _dead_tiles(tapped["tap_raw_coarse"], tapped["tap_z_coarse"], tapped["tap_rays"], kmax)
    want_f = _dead_tiles(tapped["tap_raw_fine"], tapped["tap_z_fine"], tapped["tap_rays"], kmax)
    print(f"band rows {BAND_ROW0}..{BAND_ROW0 + BAND_ROWS - 1}: counters (coarse, fine) x (tiles, skipped): {cnt.tolist()}; "
          f"all-dead tiles recomputed: coarse {want_c}, fine {want_f}")
    assert cnt[:, 0].tolist() == [_tiles(n * S), _tiles(n * (S + NI))] == [4 * 256, 4 * 768]
    assert cnt[:, 1].tolist() == [want_c, want_f]
    for k in gated:
        assert torch.equal(gated[k], tapped[k]), k


@pytest.mark.parametrize("fused", [1, "split"])
def test_fused_arrangements_equal_the_gated_sequence(idn, dev, band, fused):
    out, _ = _render(idn, band, True, dev, bc=band["bc_band"], frame=band["frame"](), fused=fused)
    _same(out, band["gated"][0], f"fused={fused!r} != gated sequence")
