"""The in-kernel positional encoding, feature by feature against fp64, on the GPU (run with ``-m gpu``).  Inputs, truth, bound
and probe networks: tests/pe_common.py; the CPU side (the reference encoder and the header's arithmetic against the same
truth): tests/test_pe_cpu.py.

1  the slab of both training pipes: every trig element of gamma_10(point) and gamma_4(view direction) within the bound, raw and
   padding columns bit for bit, the two pipes' blocks equal bit for bit;
2  rays mode: the point is fp32 o + d z with product and sum rounded separately, bit for bit;
3  probe networks of unit weights read every one of the 90 features back out of every inference kernel, both entries;
4  a 5 / 2 network's slab holds the first columns of the 10 / 4 result and zeros;
5  a NaN or an inf coordinate stays in its own point.

$IDN_PE_RECORD names a JSON file the measured figures are merged into (profiles/pe.json).  No measured figure is an
assertion: the bounds are pe_common's and the number formats'."""
import json
import os

import numpy as np
import pytest
import torch

import oracle
import pe_common as pc

pytestmark = pytest.mark.gpu

PREC = {"f32": 0, "bf16x3": 1, "bf16": 2, "fp16x3": 3, "bf16x6": 4}
TRAIN_PIPES = ("f32", "bf16x6")


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
def V():
    return pc.vectors()


def _record(key, value):
    path = os.environ.get("IDN_PE_RECORD")
    if not path:
        return
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(old, open(path, "w"), indent=1, sort_keys=True)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def device_net(idn, params, dims, dev):
    """(pack(precision code) -> weight stream, the folded bias block at zero conditioning) of oracle-style params."""
    sd = {k: v.to(dev).contiguous() for k, v in params.items()}
    ps = idn.ops.params_struct(sd, dims["dim_aud"], dims["dim_expr"], dims["dim_latent"], pts_ch=dims["input_ch"],
                               views_ch=dims["input_ch_views"])
    zeros = [torch.zeros(dims[k], device=dev) for k in ("dim_aud", "dim_expr", "dim_latent")]
    pack = lambda code: idn.ops.pack_weights(ps, dev, code)
    pack.keep = sd
    return pack, idn.ops.fold_conditioning(ps, *zeros, dev)


def ray_records(o, view, d=None):
    """[n, 11] records (o, d, near 0, far 1, view direction).  d defaults to -0.0 in every axis: with a positive depth the
    product d z is -0.0, and o + -0.0 == o bit for bit for EVERY o (o + +0.0 would turn a -0.0 coordinate into +0.0)."""
    n = o.shape[0]
    r = np.zeros((n, 11), np.float32)
    r[:, 0:3], r[:, 3:6], r[:, 7], r[:, 8:11] = o, (-0.0 if d is None else d), 1.0, view
    return T(r)


def train_slab(idn, pack, folded, rays, z, prec, widths=(63, 27)):
    """(x0, dir) [n_points, 64] each, numpy, of the rays-mode training forward of pipe `prec` (layout: csrc/idn_internal.h)."""
    n = z.numel()
    p_pad = (n + 127) // 128 * 128
    raw, acts = idn.ops.query_rays_train_fwd(pack(PREC[prec]), folded, rays, z, PREC[prec], *widths)
    torch.cuda.synchronize()
    assert raw.shape == tuple(z.shape) + (4,)
    x0 = acts[:p_pad * 64].view(p_pad, 64)[:n].cpu().numpy()
    dr = acts[p_pad * 64:p_pad * 128].view(p_pad, 64)[:n].cpu().numpy()
    return x0, dr


@pytest.fixture(scope="module")
def xavier(idn, dev):
    return device_net(idn, oracle.xavier_facenerf_params(1, pc.DIMS), pc.DIMS, dev)


@pytest.fixture(scope="module")
def slabs(idn, dev, V, xavier):
    """{pipe: (x0, dir)} of the 386 vectors: V as the ray origins (d = -0.0, so the point IS the origin, S = 1) and
    pe_common.directions(V) as the view directions."""
    pack, folded = xavier
    rays, z = ray_records(V, pc.directions(V)).to(dev), torch.ones(V.shape[0], 1, device=dev)
    return {prec: train_slab(idn, pack, folded, rays, z, prec) for prec in TRAIN_PIPES}


# ------------------------------------------------------------------------------------------------ 1: the slab
def _check_block(got, vec, octaves, name):
    """Every element of one encoding block [n, 64]: raw and padding columns bit for bit, trig columns at the bound."""
    ch = pc.channels(octaves)
    assert np.array_equal(pc.bits(got[:, :3]), pc.bits(vec)), f"{name}: raw columns"
    assert not pc.bits(got[:, ch:]).any(), f"{name}: columns {ch}..63 must be +0.0"
    err = np.abs(got[:, :ch].astype(np.float64) - pc.truth(vec, octaves))
    bnd = pc.bound(vec, octaves)
    worst = pc.per_band_worst(got[:, :ch], vec, octaves)
    for fn in ("sin", "cos"):
        print(f"\n{name} {fn}: " + "  ".join(f"b{w['band']} {w['worst_abs_err']:.2e} ({w['worst_share_of_bound']:.2f})" for w in worst[fn]))
    bad = np.argwhere(~(err[:, 3:] <= bnd[:, 3:]))       # (a NaN is not <= the bound)
    detail = [(pc.column_band(int(c) + 3), float(vec[r, (int(c) + 3) % 3]), float(err[r, c + 3]), float(bnd[r, c + 3])) for r, c in bad[:8]]
    assert bad.shape[0] == 0, f"{name}: {bad.shape[0]} elements beyond the bound, first (band, fn, axis), x, err, bound: {detail}"
    return worst


def test_slab_encodings_match_fp64_in_both_training_pipes(V, slabs):
    """386 points (three tiles and a tail of two), both pipes: every element of x0 and dir."""
    Vd = pc.directions(V)
    for prec in TRAIN_PIPES:
        x0, dr = slabs[prec]
        rec = dict(points=_check_block(x0, V, pc.L_PTS, f"{prec} gamma_10(point)"),
                   directions=_check_block(dr, Vd, pc.L_DIR, f"{prec} gamma_4(direction)"))
        _record(f"slab/{prec}", rec)
    for a, b, name in zip(slabs["f32"], slabs["bf16x6"], ("x0", "dir")):
        assert np.array_equal(pc.bits(a), pc.bits(b)), f"{name}: the two pipes run the same pe_slot"


# ------------------------------------------------------------------------------------------------ 2: the point of a ray
def test_rays_mode_point_is_o_plus_d_z_rounded_separately(idn, dev, xavier):
    """65 rays x 2 samples (a tile and two points): x0[:, 0:3] == fl32(o + fl32(d z)) bit for bit, in both pipes."""
    pack, folded = xavier
    rs = np.random.RandomState(5)
    o = rs.uniform(-1, 1, (65, 3)).astype(np.float32)
    d = rs.standard_normal((65, 3)).astype(np.float32)
    z = rs.uniform(0.2, 1.7, (65, 2)).astype(np.float32)
    prod = (d[:, None, :] * z[:, :, None]).astype(np.float32)
    want = (o[:, None, :] + prod).astype(np.float32).reshape(130, 3)
    fused = (o[:, None, :].astype(np.float64) + d[:, None, :].astype(np.float64) * z[:, :, None].astype(np.float64)).astype(np.float32)
    assert (pc.bits(fused.reshape(130, 3)) != pc.bits(want)).any(), "the inputs must tell a fused multiply-add from two roundings"
    view = d / np.linalg.norm(d, axis=1, keepdims=True)
    for prec in TRAIN_PIPES:
        x0, dr = train_slab(idn, pack, folded, ray_records(o, view, d).to(dev), T(z).to(dev), prec)
        assert np.array_equal(pc.bits(x0[:, :3]), pc.bits(want)), prec
        assert np.array_equal(pc.bits(dr[:, :3]), pc.bits(np.repeat(view.astype(np.float32), 2, axis=0))), prec


# ------------------------------------------------------------------------------------------------ 3: probe networks
def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32; finite input."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


TINY = 2.0 ** -126      # below it a 16-bit piece is a denormal (or flushed): a rounding there is absolute, not relative


def _probe_verdict(prec, out, want, scale):
    """(mask of the elements outside what `prec` must return, the figure of every element, the figure's name).

    f32, bf16x6: the feature itself.  Unit weights, one non-zero term per sum; the six-piece arithmetic splits an activation
      into three bf16 pieces (3 x 8 significand bits, each piece the rounded remainder: the third is exact) and multiplies
      every piece by the weight's first piece, 1.0 -- the pieces sum back to the fp32 value.  A -0.0 comes back as +0.0
      (relu(-0.0) - relu(0.0)), so the feature is compared after + 0.0.  bf16x6 below 2^-102: the construction, not the
      kernel, ends there -- a piece under 2^-126 is a bf16 denormal and under 2^-133 not a bf16 number at all (the one such
      value of the vectors, 2^-149, comes back as 0.0; measured on an MI355X); from 2^-102 = 2^-126 2^24 up every non-zero
      piece of a 24-bit value is a normal bf16.  Below it the feature is held to TINY absolute.
    bf16x3: NOT exact, and the construction is at fault, not the kernel: csrc/mlp_bf16x3.hip splits an activation into TWO
      pieces, hi = bf16(x) and lo = bf16(x - hi) (16 significand bits; the header states ~2^-16 per product), so 1.0 * x returns
      hi + lo.  A rounding to nearest at 8 significand bits is off by at most 2^-8 of the value: |x - hi| <= 2^-8 |x| and
      |x - hi - lo| <= 2^-8 |x - hi| <= 2^-16 |x|; hi + lo has at most 16 significant bits, so every later layer returns it
      unchanged.  Bound 2^-16 |x| + TINY.
    bf16: one bf16 rounding of the feature at the first layer, exact from there on: relative 2^-8, + TINY.
    fp16x3: 5e-6 of the largest feature (tests/test_hip_parity.py holds the precision to that)."""
    want = (want + np.float32(0.0)).astype(np.float32)
    w64, o64 = want.astype(np.float64), out.astype(np.float64)
    if prec in ("f32", "bf16x6"):
        exact = pc.bits(out) == pc.bits(want)
        if prec == "bf16x6":
            exact |= (np.abs(w64) < 2.0 ** -102) & (np.abs(o64 - w64) <= TINY)
        return ~exact, np.abs(o64 - w64), "max abs diff (bit for bit but under 2^-102 in bf16x6)"
    if prec == "bf16x3":
        share = np.abs(o64 - w64) / (2.0 ** -16 * np.abs(w64) + TINY)
        return ~(share <= 1), share, "worst share of 2^-16 |x| + 2^-126"
    if prec == "bf16":
        share = np.abs(o64 - w64) / (2.0 ** -8 * np.abs(w64) + TINY)
        return ~(share <= 1), share, "worst share of 2^-8 |x| + 2^-126"
    share = np.abs(o64 - w64) / (5e-6 * scale)
    return ~(share <= 1), share, "worst share of 5e-6 max |feature|"


@pytest.mark.parametrize("prec", list(PREC))
def test_probe_networks_read_every_feature_out_of_every_inference_kernel(idn, dev, V, slabs, prec):
    """23 unit-weight networks x (query_points_fwd, query_rays_fwd): the four outputs are four features, and they are the
    slab's columns (test 1 holds those to the truth).  f32 / bf16x3 / bf16x6 on all 386 vectors, bf16 and fp16x3 on the points
    whose vector and direction have every |axis| <= 4.  What each precision must return: _probe_verdict."""
    rows = np.arange(V.shape[0]) if prec in ("f32", "bf16x3", "bf16x6") else pc.small_rows(V)
    assert rows.size > 256                                 # more than two tiles either way
    Vp, Vd = V[rows], pc.directions(V)[rows]
    x0, dr = (T(a[rows]) for a in slabs["f32"])
    scale = float(max(np.abs(x0.numpy()).max(), np.abs(dr.numpy()).max()))
    pts, dirs = T(Vp).reshape(-1, 1, 3).to(dev), T(Vd).to(dev)
    rays, z = ray_records(Vp, Vd).to(dev), torch.ones(rows.size, 1, device=dev)
    failures, worst, what = [], 0.0, ""
    for sig, rgb in pc.probe_groups():
        pack, folded = device_net(idn, pc.probe_params(sig, rgb), pc.DIMS, dev)
        packed = pack(PREC[prec])
        want = pc.probe_columns(x0, dr, sig, rgb).numpy()
        outs = dict(points=idn.ops.query_points_fwd(packed, folded, pts, dirs, PREC[prec]),
                    rays=idn.ops.query_rays_fwd(packed, folded, rays, z, PREC[prec]))
        for entry, out in outs.items():
            out = out.reshape(-1, 4).cpu().numpy()
            bad, fig, what = _probe_verdict(prec, out, want, scale)
            worst = max(worst, float(fig.max()))
            feats = list(rgb) + [sig]
            for r, c in np.argwhere(bad)[:3]:       # (feature, got, slab, the feature's input vector)
                vec = (Vp if feats[c][0] == "p" else Vd)[r]
                failures.append((entry, feats[c], float(out[r, c]), float(want[r, c]), vec.tolist(), int(bad.sum())))
    print(f"\nprobes {prec} ({rows.size} vectors, 23 networks, 2 entries): {what} = {worst:.3e}; failing elements listed: {len(failures)}")
    _record(f"probes/{prec}", dict(vectors=int(rows.size), figure=what, worst=worst))
    assert not failures, failures[:12]


# ------------------------------------------------------------------------------------------------ 4: narrow widths
def test_narrow_network_slab_holds_the_first_columns_and_zeros(idn, dev, V, slabs):
    """A 5 / 2 network through the rays-mode training forward: columns 0..32 of x0 and 0..14 of dir are the 10 / 4 slab's,
    bit for bit (gamma_L is a prefix of gamma_10); every other column is +0.0."""
    dims = oracle.facenerf_dims(input_ch=pc.channels(5), input_ch_views=pc.channels(2))
    pack, folded = device_net(idn, oracle.xavier_facenerf_params(2, dims), dims, dev)
    rays, z = ray_records(V, pc.directions(V)).to(dev), torch.ones(V.shape[0], 1, device=dev)
    for prec in TRAIN_PIPES:
        x0, dr = train_slab(idn, pack, folded, rays, z, prec, widths=(33, 15))
        for got, wide, ch, name in ((x0, slabs[prec][0], 33, "x0"), (dr, slabs[prec][1], 15, "dir")):
            assert np.array_equal(pc.bits(got[:, :ch]), pc.bits(wide[:, :ch])), (prec, name)
            assert not pc.bits(got[:, ch:]).any(), (prec, name, "columns beyond the network's width")


# ------------------------------------------------------------------------------------------------ 5: non-finite coordinate
# (precision, what the coordinate is) whose point comes back non-finite in all four channels, as the reference's does
NON_FINITE_SURVIVES = {("f32", "nan")}


@pytest.mark.parametrize("prec", list(PREC))
def test_a_non_finite_coordinate_stays_in_its_own_point(idn, dev, xavier, prec):
    """One full tile, Xavier weights: point 37 has a NaN in axis 1, point 90 an inf in axis 2; both entries.

    MUST hold: the other 126 points return the clean run's bits.

    The two points themselves: the reference returns NaN in all four channels (its first layer multiplies the raw coordinate
    into every unit).  The kernels do NOT, but for the fp32 kernel on a NaN -- a known deviation, asserted here as it is
    (DESIGN.md section 4): relu1 (csrc/mlp_common.h) is a signed-integer max of the bit pattern with 0, one instruction on
    the hot path, and it takes a NaN whose sign bit is set, like -inf, to +0.0.  The coordinate's own (positive) NaN passes
    the fp32 MFMAs and every ReLU unchanged; the NaNs the matrix pipe makes itself -- inf - inf in the layer behind an inf
    coordinate, and every product of the 16-bit pipes with a NaN piece -- carry the sign bit (measured on an MI355X: those
    points return the finite outputs of a network whose poisoned layers are all off).  The encoding's trig columns are
    finite either way: the conversion of a NaN phase to fixed point gives 0."""
    pack, folded = xavier
    packed = pack(PREC[prec])
    rs = np.random.RandomState(9)
    p = rs.uniform(-1, 1, (128, 3)).astype(np.float32)
    d = rs.standard_normal((128, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dirty = p.copy()
    dirty[37, 1], dirty[90, 2] = np.nan, np.inf
    others = np.setdiff1d(np.arange(128), [37, 90])

    def run(points):
        a = idn.ops.query_points_fwd(packed, folded, T(points).reshape(128, 1, 3).to(dev), T(d).to(dev), PREC[prec])
        b = idn.ops.query_rays_fwd(packed, folded, ray_records(points, d).to(dev), torch.ones(128, 1, device=dev), PREC[prec])
        return a.reshape(128, 4).cpu().numpy(), b.reshape(128, 4).cpu().numpy()

    with torch.no_grad():
        ref = oracle.facenerf_forward(oracle.xavier_facenerf_params(1, pc.DIMS), torch.cat(
            [oracle.positional_encoding(T(dirty), 10), oracle.positional_encoding(T(d), 4)], -1), torch.zeros(64), torch.zeros(76),
            torch.zeros(32), pc.DIMS).numpy()
    assert np.isnan(ref[[37, 90]]).all() and np.isfinite(ref[others]).all()
    seen = {}
    for entry, clean, got in zip(("points", "rays"), run(p), run(dirty)):
        assert np.isfinite(clean).all(), (prec, entry)
        assert np.array_equal(pc.bits(got[others]), pc.bits(clean[others])), (prec, entry, "a neighbour of the bad point changed")
        for kind, row in (("nan", 37), ("inf", 90)):
            print(f"\nnon-finite {prec} {entry}: {kind} coordinate -> {got[row]}")
            seen[f"{entry}/{kind}"] = "non-finite" if not np.isfinite(got[row]).any() else "finite" if np.isfinite(got[row]).all() else "mixed"
    _record(f"non_finite/{prec}", seen)
    want = {f"{entry}/{kind}": "non-finite" if (prec, kind) in NON_FINITE_SURVIVES else "finite"
            for entry in ("points", "rays") for kind in ("nan", "inf")}
    assert seen == want, (prec, seen)
