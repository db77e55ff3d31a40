"""The sample cull without a GPU: the numpy restatement of its predicate (tests/cull_samples_common.py) on hand-built cases,
its agreement with the fp64 model on the shapes the GPU tests use, the ``samples`` option, and the refusals of
``ops.render_rays_sparse_fwd`` before any C call."""
import numpy as np
import pytest
import torch

import cull_common as cc
import cull_samples_common as sc


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()
    return idealnerf_amd


# a grid of 32^3 cells of edge 0.1 over [0, 3.2]^3 with one occupied cell, (x, y, z) = (5, 6, 7)
G, LO, CELL = 32, (0.0, 0.0, 0.0), 0.1


def _occ():
    occ = np.zeros((G, G, G), dtype=bool)
    occ[7, 6, 5] = True
    return occ


def _ray(o, d):
    d = np.asarray(d, dtype=np.float32)
    return np.concatenate([np.asarray(o, dtype=np.float32), d, [0.0, 1.0], d / np.sqrt((d * d).sum())]).astype(np.float32)[None]


def test_restatement_on_hand_built_cases():
    occ = _occ()
    live = lambda rays, z: sc.np_sample_live(occ, G, LO, CELL, rays, np.asarray(z, dtype=np.float32)[None])[0]
    # a ray along +x through the clear cells (y, z) = (1, 1): spacing 0.01 <= 0.0125, nothing is live
    clear = _ray((0.05, 0.15, 0.15), (1.0, 0.0, 0.0))
    assert not live(clear, [0.10, 0.11, 0.12, 0.13]).any()
    # the same spacing along +x through the row of the occupied cell: live exactly while x is in [0.5, 0.6)
    through = _ray((0.0, 0.65, 0.75), (1.0, 0.0, 0.0))
    np.testing.assert_array_equal(live(through, [0.485, 0.495, 0.505, 0.515, 0.595, 0.605, 0.615]), [0, 0, 1, 1, 1, 0, 0])
    # a point outside the box is live: below 0, at or beyond G cell = 3.2, on any axis
    np.testing.assert_array_equal(live(_ray((-0.005, 0.15, 0.15), (1.0, 0.0, 0.0)), [0.0, 0.01, 0.02]), [1, 0, 0])
    np.testing.assert_array_equal(live(_ray((3.185, 0.15, 0.15), (1.0, 0.0, 0.0)), [0.0, 0.01, 0.02]), [0, 0, 1])
    np.testing.assert_array_equal(live(_ray((0.15, 0.15, 3.25), (1.0, 0.0, 0.0)), [0.0, 0.01]), [1, 1])
    # a last sample in a clear cell is skipped whatever lies before it; in the occupied cell it is live
    np.testing.assert_array_equal(live(clear, [0.1, 0.5, 0.9]), [1, 1, 0])
    np.testing.assert_array_equal(live(through, [0.1, 0.55]), [1, 1])
    assert not live(clear, [0.5]).any()
    # a gap just above and just below 0.0125 / dn, for a direction that is not a unit vector
    d = np.array([1.5, 0.25, -0.5], dtype=np.float32)
    ray = _ray((0.05, 1.05, 2.05), d)
    dn = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    gap = float(sc.MAX_DIST) / float(dn)
    for scale, want in ((1.0 - 1e-5, 0), (1.0 + 1e-5, 1)):
        z = np.array([0.1, 0.1 + gap * scale, 0.1 + gap * scale + 0.001], dtype=np.float32)
        dist = sc.np_dist(ray, z[None])[0]
        assert (abs(dist[0]) <= sc.MAX_DIST) == (not want)              # (the case is on the side it is meant to be)
        np.testing.assert_array_equal(live(ray, z), [want, 0, 0])
    # depths that run backwards by more than the threshold: |dist| decides
    np.testing.assert_array_equal(live(clear, [0.12, 0.10, 0.11]), [1, 0, 0])
    # a NaN depth: its own point is live (the position is NaN), and so is the sample before it (its spacing is NaN)
    np.testing.assert_array_equal(live(clear, [0.10, 0.11, np.nan, 0.13, 0.14]), [0, 1, 1, 0, 0])
    np.testing.assert_array_equal(live(clear, [0.10, 0.11, np.nan]), [0, 1, 1])
    # a NaN direction: every point of the ray
    assert live(_ray((0.05, 0.15, 0.15), (1.0, np.nan, 0.0)), [0.10, 0.11]).all()


def test_points_are_rounded_twice():
    """o + d z with the product rounded before the sum: not the fused value wherever the two differ."""
    rs = np.random.RandomState(0)
    rays = np.zeros((4096, 11), dtype=np.float32)
    rays[:, 0:6] = rs.standard_normal((4096, 6)).astype(np.float32)
    z = rs.uniform(0.5, 1.2, (4096, 1)).astype(np.float32)
    p = sc.np_points(rays, z)[:, 0]
    r64, z64 = rays.astype(np.float64), z.astype(np.float64)
    twice = (r64[:, 0:3] + (r64[:, 3:6] * z64).astype(np.float32).astype(np.float64)).astype(np.float32)
    fused = (r64[:, 0:3] + r64[:, 3:6] * z64).astype(np.float32)
    assert p.dtype == np.float32 and np.array_equal(p, twice) and (twice != fused).any()


@pytest.mark.parametrize("H,W,row0,nrows", [(48, 48, 0, 48), (50, 37, 5, 20)])
def test_restatement_agrees_with_fp64_off_the_faces(idn, H, W, row0, nrows):
    """On the GPU tests' shapes (coarse depths and a 192-sample depth list of the box scene's kind) the fp32 restatement and
    the fp64 model differ only at samples the model calls ambiguous, and those stay under the cap."""
    from idealnerf_amd import cull, synthetic
    syn = synthetic.frame(cc.SIZE, cc.SIZE, seed=0)
    lo, cell = cull.frustum_box([syn["c2w"]], H, W, cc.FOCAL, syn["near"], syn["far"], cc.G)
    lo, cell = [float(np.float32(v)) for v in lo], float(np.float32(cell))
    occ = sc.box_occupancy(cc.G, lo, cell)
    rays = sc.np_ray_records(syn["c2w"].numpy(), H, W, cc.FOCAL, syn["near"], syn["far"], row0, nrows)
    t = np.linspace(0.0, 1.0, cc.S, dtype=np.float32)
    z_c = (np.float32(syn["near"]) * (np.float32(1) - t) + np.float32(syn["far"]) * t)[None].repeat(len(rays), 0)
    # fine depths: the coarse ones merged with 128 samples crowded around the box's depth, as importance sampling leaves them
    rs = np.random.RandomState(1)
    z_s = np.clip(0.877 + 0.1 * rs.standard_normal((len(rays), cc.NI)), syn["near"], syn["far"]).astype(np.float32)
    z_f = np.sort(np.concatenate([z_c, z_s], 1), 1)
    for z in (z_c, z_f):
        live = sc.np_sample_live(occ, cc.G, lo, cell, rays, z)
        live64, amb = sc.model64(occ, cc.G, lo, cell, rays, z)
        print(f"{H}x{W} S = {z.shape[1]}: live {live.mean():.4f}, ambiguous {amb.mean():.5f}, differing {(live != live64).sum()}")
        assert amb.mean() <= sc.AMBIGUOUS_CAP
        assert not ((live != live64) & ~amb).any()
        assert 0 < live.mean() < 1


def test_samples_option(idn):
    from idealnerf_amd import cull
    assert cull.DEFAULTS == dict(G=128, dilate=1, sigma_min=0.0, frame_stride=1, samples=False)
    assert cull.options(dict(samples=True)) == dict(G=128, dilate=1, sigma_min=0.0, frame_stride=1, samples=True)
    assert cull.options(dict(G=64)) == dict(G=64, dilate=1, sigma_min=0.0, frame_stride=1, samples=False)
    g = cull.CullGrid(None, None, 32, (0.0, 0.0, 0.0), 0.1, 1, 0.0)
    assert g.samples is False and g.points_seen == 0 and g.points_evaluated == 0 and np.isnan(g.evaluated_share)
    g = cull.CullGrid(None, None, 32, (0.0, 0.0, 0.0), 0.1, 1, 0.0, samples=True)
    g.points_seen, g.points_evaluated = 200, 50
    assert g.samples is True and g.evaluated_share == 0.25
    with pytest.raises(idn._lib.IdealNerfError, match="samples"):
        cull.build_grid((), [1], [1], 4, 4, 1.0, 0.5, 1.0, G=32, samples=1)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"C call {name} after an argument that must be refused before it")


def test_sparse_render_refusals_come_before_any_c_call(idn, monkeypatch):
    from idealnerf_amd import cull
    E = idn._lib.IdealNerfError
    monkeypatch.setattr(idn._lib, "load", lambda: _NoLibrary())
    grid = cull.CullGrid(None, None, 32, (0.0, 0.0, 0.0), 0.1, 1, 0.0, samples=True)
    n = 8
    rays, bc, t_vals, u = torch.zeros(n, 11), torch.zeros(n, 3), torch.linspace(0, 1, cc.S), torch.linspace(0, 1, cc.NI)
    call = lambda **kw: idn.ops.render_rays_sparse_fwd(grid, rays, bc, None, None, None, None, t_vals, u, cc.NI, **kw)
    for kw, word in ((dict(taps=True), "taps"), (dict(white_bkgd=True), "white_bkgd"), (dict(lindisp=True), "lindisp"),
                     (dict(noise_coarse=torch.zeros(n, cc.S)), "density noise"), (dict(noise_fine=torch.zeros(n, cc.S + cc.NI)), "density noise"),
                     (dict(fused=1), "fused"), (dict(fused="split"), "fused")):
        with pytest.raises(E, match=word):
            call(**kw)
    monkeypatch.setattr(idn.ops, "FUSED_MARCH_DEFAULT", 2)
    with pytest.raises(E, match="fused"):
        call()
    monkeypatch.setattr(idn.ops, "FUSED_MARCH_DEFAULT", 0)
    with pytest.raises(E, match="draws"):
        call(draws=(1, 0))
    with pytest.raises(E, match="chunk"):
        call(chunk=0)
    with pytest.raises(E, match="fine network"):
        call()
    assert grid.points_seen == 0


def test_c_entries_refuse_bad_arguments_without_a_gpu(idn):
    import ctypes as C
    lib, L = idn._lib.load(), idn._lib
    g = L.CullGridStruct()
    g.bits, g.G, g.cell = 1, 32, 0.02
    need = lib.idealnerf_cull_classify_workspace_bytes(100 * 64)
    assert lib.idealnerf_cull_sample_classify(C.byref(g), 1, 1, 100, 64, 1, 1, 1, need - 1, None) == -4
    assert lib.idealnerf_cull_sample_classify(C.byref(g), None, 1, 100, 64, 1, 1, 1, need, None) == -1 and b"NULL" in lib.idealnerf_last_error()
    assert lib.idealnerf_cull_sample_classify(C.byref(g), 1, 1, 1 << 26, 64, 1, 1, 1, need, None) != 0 and b"2^31" in lib.idealnerf_last_error()
    assert lib.idealnerf_cull_sample_classify(C.byref(g), 1, 1, 100, 0, 1, 1, 1, need, None) == -1
    g.G = 48
    assert lib.idealnerf_cull_sample_classify(C.byref(g), 1, 1, 100, 64, 1, 1, 1, need, None) == -1 and b"multiple of 32" in lib.idealnerf_last_error()
    assert lib.idealnerf_cull_sample_gather(1, 6401, 1, 1, 100, 64, 1, 1, None) == -1
    assert lib.idealnerf_cull_sample_gather(None, 0, None, None, 100, 64, None, None, None) == 0
    assert lib.idealnerf_cull_sample_gather(None, 5, 1, 1, 100, 64, 1, 1, None) == -1 and b"NULL" in lib.idealnerf_last_error()
    assert lib.idealnerf_cull_sample_scatter(1, 6401, 16, 6400, 16, None) == -1
    assert lib.idealnerf_cull_sample_scatter(None, 0, None, 0, None, None) == 0
    assert lib.idealnerf_cull_sample_scatter(None, 5, None, 6400, 16, None) == -1 and b"NULL" in lib.idealnerf_last_error()
    assert lib.idealnerf_cull_sample_scatter(16, 5, 20, 6400, 16, None) == -1 and b"aligned" in lib.idealnerf_last_error()
