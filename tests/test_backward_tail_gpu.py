"""What a training backward runs after the delta chain, each kernel alone and element by element against torch fp64 on the
device: the input-row gradient (csrc/train.hip: dx_kernel, ``ops.input_grad``), the encoding backward with the per-ray
reduction (csrc/ray_grad.hip: ray_grad_kernel, ``ops.ray_grad``), the conditioning fold's backward (fold_bwd_kernel<false / true>,
``ops.fold_bwd``) and the frozen plan's column sums (colsum_rows_kernel / colsum_finish_kernel, ``ops.cond_colsums``).  The
aids run the kernels through the launch functions of a pass; T7 ties them to the pass bit for bit.

Exact operands first (T1, T3, T5, T6): integers (and multiples of 1/64) whose every product and partial sum is exactly
representable, so fp32 MFMA accumulation in any order, the kernels' fp64 sums and torch fp64 agree exactly and the assertions
are equalities.  Everything a kernel must not read is NaN, every output lives between sentinel guards
(tests/test_delta_chain_gpu.py), and no element is exempted from any comparison.  Then rounding against fp64 with derived
bounds (EPS = 2^-24):
    T2  dx_kernel        |err| <= K EPS sum_k |delta_k| |w_k|, K = 512 (point columns) / 128 (direction columns): a chain of K
                         fp32 accumulations with rounded or fused products
    T4  ray_grad_kernel  |err| <= 18 EPS U (+ 3 EPS |d_norm| on d rays_d), U = sum_s (|g_id| + sum_k 2^k (|g_sin| + |g_cos|)),
                         times |z_s| for d rays_d: 4 EPS for sinf / cosf (the 2^-22 tests/pe_common.py holds the forward to),
                         two roundings in the bracket, at most 11 fp32 additions per sample, one final rounding
    T5  fold             d cond within 2 EPS sum |w| |db| (an fp64 sum, one rounding, one fp32 +=), gW within 3 EPS |db cond|
Measured shares of those bounds (profiles/backward_tail_parity.json; $IDN_BACKWARD_TAIL_RECORD names the file they are merged
into), on an MI355X, the same on either backward pipe (these kernels do not depend on it):
    T2  (63, 27): point columns 0.0070, direction columns 0.0199;  (27, 15): 0.0049 / 0.0255
    T4  band by band, worst band at S = 65: 0.015 (63, 27: view band 3), 0.018 (27, 15: view band 0); at S = 512: 0.0036 and
        0.0050 (the errors of a ray's samples add like a random walk, the bound linearly);  all columns Gaussian:
        0.0039 .. 0.0075 at S = 65, 0.0016 .. 0.0024 at S = 512
    T5  d aud / d expr / d latent 0.028 .. 0.051;  gW 0.52 .. 0.54 with an expression, 0.33 without
Needs an MI355X.
"""
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import backward_tail_common as bt
from backward_tail_common import EPS, NAN
from test_delta_chain_gpu import SENTINEL, guarded, guards_intact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()  # fail loudly if the HIP library is missing
    return idealnerf_amd


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ---------------------------------------------------------------------------------------------- T1
_dx_nets = {}


def _dx_net(idn, dev, widths, dims3, kind):
    """(sd, params, the three read blocks) of a network whose dx blocks hold integers in [-8, 8] ("int"), the code
    64 k + c + 1 of their own position ("code") or Gaussians ("gauss"); every other weight is NaN.  Built once, read-only."""
    key = (widths, dims3, kind)
    if key not in _dx_nets:
        pc, vc = widths
        sd = bt.nan_net(pc, vc, dims3, dev)
        blocks = bt.dx_blocks(sd, pc, vc)
        g = bt.gen(11 + 13 * bt.WIDTHS.index(widths) + 7 * bt.DIMS.index(dims3))
        if kind == "code":
            k = torch.arange(512, device=dev)[:, None]
            blocks[0].copy_((64 * k[:256] + torch.arange(pc, device=dev) + 1).float())
            blocks[1].copy_((64 * k[256:] + torch.arange(pc, device=dev) + 1).float())
            blocks[2].copy_((64 * k[:128] + torch.arange(vc, device=dev) + 1).float())
        else:
            for b in blocks:
                b.copy_((bt.ints(tuple(b.shape), -8, 8, g) if kind == "int" else torch.randn(tuple(b.shape), generator=g)).to(dev))
        _dx_nets[key] = (sd, idn.ops.params_struct(sd, *dims3, pts_ch=pc, views_ch=vc), blocks)
    return _dx_nets[key]


def _assert_dx_exact(d_x, ref64, unit, ctx, decode=False):
    assert float(unit.max()) < 2 ** 24, ctx                     # every partial sum, in any order, is an exact integer
    assert bool((ref64 == ref64.round()).all())
    ref = ref64.float()
    if not torch.equal(d_x, ref):
        count, row, col = bt.first_difference(d_x, ref)
        msg = f"{ctx}: d_x differs in {count} of {d_x.numel()} elements, first at row {row} column {col}: got {float(d_x[row, col])}, want {float(ref[row, col])}"
        if decode:
            pair = lambda v: ((int(v) - 1) // 64, (int(v) - 1) % 64)
            msg += f" -- the kernel read (k, c) = {pair(d_x[row, col])}, the element is (k, c) = {pair(ref[row, col])}"
        raise AssertionError(msg)


@pytest.mark.parametrize("dims3", bt.DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("widths", bt.WIDTHS, ids=lambda w: f"{w[0]}+{w[1]}")
def test_input_grad_exact(idn, dev, widths, dims3):
    """T1: integer deltas and weights in [-8, 8] (sum |delta| |w| <= 512 * 64 < 2^24): d_x equals the fp64 product at all five
    (n, p_pad); then one-hot deltas against weights that hold the code of their own position, so that a wrong fragment lane
    names the (k, c) it read.  NaN in every weight column but the three blocks, in columns 128..255 of dV0 and in all three
    matrices' rows n .. p_pad - 1."""
    pc, vc = widths
    for n, p_pad in bt.ROWS:
        g = bt.gen(1000 * p_pad + n)
        ctx = f"widths {widths} dims {dims3} n {n} p_pad {p_pad}"
        _, p, blocks = _dx_net(idn, dev, widths, dims3, "int")
        deltas = bt.dx_deltas(n, p_pad, lambda r, c: bt.ints((r, c), -8, 8, g), dev)
        d_x, blocks_ran = bt.run_dx(idn, p, deltas, n, pc + vc)
        assert blocks_ran == 1, ctx                             # at most 256 rows: one 16-wave workgroup
        _assert_dx_exact(d_x, *bt.dx_reference(deltas, blocks, n), ctx)
        _, p, blocks = _dx_net(idn, dev, widths, dims3, "code")
        rows = torch.arange(n)

        def one_hot(r, c):                                      # dA0 | dA5: channel (7 p) mod 512; dV0: (7 p) mod 128
            m = torch.zeros(r, c)
            k = (7 * rows) % (512 if c == 256 else 128)
            return m, k
        m0, k = one_hot(n, 256)
        m5 = torch.zeros(n, 256)
        m0[rows[k < 256], k[k < 256]] = 1.0
        m5[rows[k >= 256], k[k >= 256] - 256] = 1.0
        mv, kv = one_hot(n, 128)
        mv[rows, kv] = 1.0
        fills = iter((m0, m5, mv))
        deltas = bt.dx_deltas(n, p_pad, lambda r, c: next(fills), dev)
        d_x, _ = bt.run_dx(idn, p, deltas, n, pc + vc)
        ref64, unit = bt.dx_reference(deltas, blocks, n)
        want = torch.cat([64 * k[:, None] + torch.arange(pc) + 1, 64 * kv[:, None] + torch.arange(vc) + 1], 1).double().to(dev)
        assert torch.equal(ref64, want)                         # the reference itself names (k, c)
        _assert_dx_exact(d_x, ref64, unit, ctx + " one-hot", decode=True)


@pytest.mark.parametrize("widths", [(63, 27), (27, 15)], ids=lambda w: f"{w[0]}+{w[1]}")
def test_input_grad_exact_on_a_capped_grid(idn, dev, cus, widths):
    """T1: 1100 rows of 1152 on one workgroup (waves 0..3 walk three tiles, the others two) and on the grid of a pass give the
    fp64 product, and the same bits as each other."""
    pc, vc = widths
    n, p_pad, dims3 = 1100, 1152, bt.DIMS[bt.WIDTHS.index(widths) % 2]
    g = bt.gen(5)
    _, p, blocks = _dx_net(idn, dev, widths, dims3, "int")
    deltas = bt.dx_deltas(n, p_pad, lambda r, c: bt.ints((r, c), -8, 8, g), dev)
    ref64, unit = bt.dx_reference(deltas, blocks, n)
    one, ran = bt.run_dx(idn, p, deltas, n, pc + vc, max_blocks=1)
    assert ran == 1
    _assert_dx_exact(one, ref64, unit, f"widths {widths} one workgroup")
    full, ran = bt.run_dx(idn, p, deltas, n, pc + vc, max_blocks=0)
    assert ran == min(3, cus)
    _assert_dx_exact(full, ref64, unit, f"widths {widths} the grid of a pass")


def test_input_grad_refuses_misaligned_delta_matrices(idn, dev):
    """The delta rows are read as float4: a matrix that starts 4 bytes into a buffer is refused before the call."""
    _, p, _ = _dx_net(idn, dev, (63, 27), bt.DIMS[0], "int")
    good = torch.zeros((128, 256), device=dev)
    odd = torch.zeros(128 * 256 + 1, device=dev)[1:].view(128, 256)
    for i in range(3):
        mats = [good, good, good]
        mats[i] = odd
        with pytest.raises(idn._lib.IdealNerfError, match="16-byte aligned"):
            idn.ops.input_grad(p, *mats, 100)


# ---------------------------------------------------------------------------------------------- T2
@pytest.mark.parametrize("widths", [(63, 27), (27, 15)], ids=lambda w: f"{w[0]}+{w[1]}")
def test_input_grad_rounding_vs_fp64(idn, dev, widths):
    """T2: Gaussian operands at (185, 256); every element within K EPS sum_k |delta_k| |w_k| of fp64, K = 512 for the point
    columns and 128 for the direction columns, graded separately."""
    pc, vc = widths
    n, p_pad = 185, 256
    g = bt.gen(77)
    _, p, blocks = _dx_net(idn, dev, widths, bt.DIMS[0], "gauss")
    deltas = bt.dx_deltas(n, p_pad, lambda r, c: torch.randn((r, c), generator=g), dev)
    d_x, _ = bt.run_dx(idn, p, deltas, n, pc + vc)
    ref64, unit = bt.dx_reference(deltas, blocks, n)
    assert float(unit.min()) > 0
    share = (d_x.double() - ref64).abs() / unit / EPS
    pts, views = float(share[:, :pc].max()) / 512, float(share[:, pc:].max()) / 128
    print(f"\n  dx_kernel {widths}: worst |err| / (K EPS sum |delta| |w|): point columns {pts:.4f}, direction columns {views:.4f}")
    bt.record(f"T2/{pc}+{vc}", dict(point_columns=pts, direction_columns=views))
    assert pts <= 1.0 and views <= 1.0, (widths, pts, views)


# ---------------------------------------------------------------------------------------------- T3
def _exact_rays(n, pc, vc, S, g, zero_dir=None):
    """n rays of the exact test: d_x non-zero (integers in [-64, 64]) in the identity columns alone, z in multiples of 1 / 64
    in [0, 4), rays_d = (0, 0, 2) (the ray `zero_dir`: 0), an integer dL / d |rays_d|."""
    d_x = torch.zeros(n, S, pc + vc)
    d_x[:, :, 0:3] = bt.ints((n, S, 3), -64, 64, g)
    d_x[:, :, pc:pc + 3] = bt.ints((n, S, 3), -64, 64, g)
    z = torch.randint(0, 256, (n, S), generator=g).float() / 64
    rays = torch.zeros(n, 11)
    rays[:, 0:3] = torch.rand((n, 3), generator=g) * 2 - 1
    rays[:, 5] = 2.0
    rays[:, 6], rays[:, 7] = 0.5, 1.5
    rays[:, 8:11] = torch.rand((n, 3), generator=g) * 2 - 1
    if zero_dir is not None:
        rays[zero_dir, 3:6] = 0.0
    return d_x, z, rays, bt.ints((n,), -100, 100, g)


@pytest.mark.parametrize("S", [2, 63, 64, 65, 130, 512])
@pytest.mark.parametrize("widths", [(63, 27), (3, 3), (27, 15)], ids=lambda w: f"{w[0]}+{w[1]}")
def test_ray_grad_exact(idn, dev, widths, S):
    """T3: d o = sum_s g, d d = sum_s z g (+ the planted dL / d |rays_d| on d d[2], |rays_d| being exactly 2), d v = sum_s g_v:
    exact in fp64 and in the final fp32, so equalities.  Columns 6 and 7 are +0.0 afterwards, the other nine were sentinels.  A
    ray of zero direction stays finite and keeps d d = sum z g.  The single ray of the n_rays = 1 run is ray 4 of the five:
    the same bits."""
    pc, vc = widths
    g = bt.gen(31 * S + pc)
    one = _exact_rays(1, pc, vc, S, g)
    four = _exact_rays(4, pc, vc, S, g, zero_dir=3)
    five = tuple(torch.cat([b, a]) for a, b in zip(one, four))
    got = {}
    for n, (d_x, z, rays, d_norm) in ((1, one), (5, five)):
        d_x, z, rays, d_norm = (t.to(dev) for t in (d_x, z, rays, d_norm))
        out = bt.run_ray_grad(idn, d_x.view(n * S, pc + vc).contiguous(), pc, vc, rays, z, d_norm)
        g64, z64 = d_x.double(), z.double()[:, :, None]
        want = torch.zeros((n, 11), dtype=torch.float64, device=dev)
        want[:, 0:3] = g64[:, :, 0:3].sum(1)
        want[:, 3:6] = (z64 * g64[:, :, 0:3]).sum(1)
        want[:, 5] += torch.where(rays[:, 5] != 0, d_norm.double(), torch.zeros_like(d_norm).double())
        want[:, 8:11] = g64[:, :, pc:pc + 3].sum(1)
        assert bool((want.float().double() == want).all())       # exact in fp32 too
        assert torch.equal(out, want.float()), (widths, S, n, (out != want.float()).nonzero()[:4].tolist(), out, want)
        got[n] = out
    assert torch.equal(got[1][0].view(torch.int32), got[5][4].view(torch.int32)), "the same ray behind four others gives other bits"


# ---------------------------------------------------------------------------------------------- T4
def _graded_rays(n, S, g):
    """Rays with points up to |p| = 4: o in [-1, 1], |d| in [0.9, 1.0] by axis sum, z in [0, 3)."""
    rays = torch.zeros(n, 11)
    rays[:, 0:3] = torch.rand((n, 3), generator=g) * 2 - 1
    d = torch.randn((n, 3), generator=g)
    rays[:, 3:6] = d / d.abs().max(1, keepdim=True)[0]          # the largest component is +-1: |p| <= 1 + 3
    rays[:, 6], rays[:, 7] = 0.5, 3.0
    v = rays[:, 3:6] / rays[:, 3:6].norm(dim=1, keepdim=True)
    rays[:, 8:11] = v
    z = torch.rand((n, S), generator=g).sort(1)[0] * 3
    return rays, z


def _ray_grad_shares(idn, dev, pc, vc, d_x, rays, z, d_norm):
    n, S = z.shape
    d_x, rays, z, d_norm = (t.to(dev).contiguous() for t in (d_x.view(n * S, pc + vc), rays, z, d_norm))
    out = bt.run_ray_grad(idn, d_x, pc, vc, rays, z, d_norm)
    truth, U, dn = bt.ray_grad_reference(d_x, pc, vc, rays, z, d_norm)
    bound = 18 * EPS * U
    bound[:, 3:6] += 3 * EPS * dn[:, None]
    err = (out.double() - truth).abs()
    assert bool((err[bound == 0] == 0).all()), "an output without any non-zero input is not exactly zero"
    return err / bound.clamp_min(1e-300), float(p32_max(rays, z))


def p32_max(rays, z):
    return (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).abs().max()


@pytest.mark.parametrize("S", [65, 512])
@pytest.mark.parametrize("widths", [(63, 27), (27, 15)], ids=lambda w: f"{w[0]}+{w[1]}")
def test_ray_grad_encoding_backward_band_by_band(idn, dev, widths, S):
    """T4: one ray per (band, axis, sine / cosine) of the point encoding and then of the view encoding, its d_x Gaussian in
    that one column alone (S = 65: two chunks; 512: eight), against fp64 of 2^k (cos(t) g_sin - sin(t) g_cos) at the kernel's own argument
    t = 2^k fl32(o + fl32(d z)); bound 18 EPS U with U of that column.  The worst share per band is recorded."""
    pc, vc = widths
    cols = [(f"pts band {k} {'sin' if c == cs else 'cos'}", k, c) for k, a, cs, cc in bt.pe_columns((pc - 3) // 6) for c in (cs, cc)]
    cols += [(f"view band {k} {'sin' if c == cs else 'cos'}", k, pc + c) for k, a, cs, cc in bt.pe_columns((vc - 3) // 6) for c in (cs, cc)]
    n = len(cols)
    g = bt.gen(200 + pc + S)
    rays, z = _graded_rays(n, S, g)
    d_x = torch.zeros(n, S, pc + vc)
    for r, (_, _, c) in enumerate(cols):
        d_x[r, :, c] = torch.randn(S, generator=g)
    share, pmax = _ray_grad_shares(idn, dev, pc, vc, d_x, rays, z, torch.zeros(n))
    assert 3.0 < pmax <= 4.0, pmax
    per_band = {}
    for r, (name, k, c) in enumerate(cols):
        key = name.rsplit(" ", 1)[0]
        per_band[key] = max(per_band.get(key, 0.0), float(share[r].max()))
    print(f"\n  ray_grad_kernel {widths} S {S}, band by band (max |p| {pmax:.2f}): worst |err| / bound per band")
    print("    " + "  ".join(f"{k}: {v:.3f}" for k, v in per_band.items()))
    bt.record(f"T4/bands/{pc}+{vc}/S{S}", per_band)
    assert max(per_band.values()) <= 1.0, per_band


@pytest.mark.parametrize("S", [65, 512])
@pytest.mark.parametrize("widths", [(63, 27), (27, 15)], ids=lambda w: f"{w[0]}+{w[1]}")
def test_ray_grad_rounding_vs_fp64(idn, dev, widths, S):
    """T4: every column of d_x Gaussian, a Gaussian dL / d |rays_d|: each component of d o, d d, d v within 18 EPS U
    (+ 3 EPS |d_norm| on d d) of fp64."""
    pc, vc = widths
    n = 6
    g = bt.gen(300 + S + pc)
    rays, z = _graded_rays(n, S, g)
    d_x = torch.randn((n, S, pc + vc), generator=g)
    share, pmax = _ray_grad_shares(idn, dev, pc, vc, d_x, rays, z, torch.randn(n, generator=g) * 10)
    worst = {k: float(share[:, s].max()) for k, s in (("d_o", slice(0, 3)), ("d_d", slice(3, 6)), ("d_v", slice(8, 11)))}
    print(f"\n  ray_grad_kernel {widths} S {S} (max |p| {pmax:.2f}): worst |err| / bound " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    bt.record(f"T4/gauss/{pc}+{vc}/S{S}", worst)
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------- T5
FOLD_CASES = [((64, 76, 32), (63, 27)), ((64, 79, 32), (27, 15)), ((106, 0, 0), (63, 27)), ((64, 0, 0), (33, 9))]


def _fold_case(idn, dev, dims3, widths, exact, seed):
    pc, vc = widths
    a, e, l = dims3
    g = bt.gen(seed)
    draw = (lambda *s: bt.ints(s, -8, 8, g)) if exact else (lambda *s: torch.randn(s, generator=g))
    sd = bt.nan_net(pc, vc, dims3, dev)
    blocks = bt.cond_blocks(sd, pc, vc, dims3)
    for b in blocks:
        b.copy_(draw(*b.shape).to(dev))
    cond = [draw(d).to(dev) if d else None for d in dims3]
    if exact and e:
        cond[1] = cond[1] * 3                                   # expr = 3 x integer: expr * 1 / 3 is exact
    db0, db5, dbv = draw(256).to(dev), draw(256).to(dev), draw(128).to(dev)
    return dict(sd=sd, p=idn.ops.params_struct(sd, *dims3, pts_ch=pc, views_ch=vc), blocks=blocks, cond=cond, db=(db0, db5, dbv),
                ref=bt.fold_reference(blocks, dims3, cond, db0, db5, dbv), draw=draw)


def _run_fold(idn, dev, c, dims3, widths, full, d_old, dbv=None, want_expr=True):
    """One call of ops.fold_bwd: gradient tensors in sentinel-filled guarded buffers (full) or none, the three d * in guarded
    buffers pre-filled with d_old.  -> (gW views or None, [d_aud, d_expr, d_latent])."""
    pc, vc = widths
    a, e, l = dims3
    C = a + e + l
    gws = wholes = None
    if full:
        pairs = [guarded(s, dev) for s in ((256, pc + C), (256, pc + C + 256), (128, 256 + vc + e))]
        wholes, gws = [w for w, _ in pairs], [v for _, v in pairs]
    d_wholes, ds = [], []
    for i, dim in enumerate(dims3):
        if dim == 0 or (i == 1 and not want_expr):
            d_wholes.append(None), ds.append(None)
            continue
        w, v = guarded((dim,), dev)
        v.copy_(d_old[i])
        d_wholes.append(w), ds.append(v)
    db0, db5, dbv0 = c["db"]
    idn.ops.fold_bwd(c["p"], *c["cond"], db0, db5, dbv0 if dbv is None else dbv, *(gws or (None, None, None)),
                     d_aud=ds[0], d_expr=ds[1], d_latent=ds[2])
    for w in (wholes or []) + [w for w in d_wholes if w is not None]:
        assert guards_intact(w), "a write outside an output of the fold"
    return gws, ds


@pytest.mark.parametrize("dims3,widths", FOLD_CASES, ids=lambda v: "x".join(map(str, v)))
def test_fold_bwd_exact(idn, dev, dims3, widths):
    """T5: integer db, aud, latent and weights, expr = 3 x integers.  The conditioning columns of gW0 / gW5 / gWv0 equal
    db (x) cond and every other element still holds the sentinel's bits; d aud / d latent = old + the fp64 sum and d expr =
    old + fl32((s + sv) / 3); without d_expr the others are the same bits; the cond-only launch gives the same three d * without
    gradient tensors, and with d_expr None reads no dbv (NaN there)."""
    pc, vc = widths
    a, e, l = dims3
    C = a + e + l
    c = _fold_case(idn, dev, dims3, widths, True, 40 + a + e)
    r = c["ref"]
    d_old = [c["draw"](d).to(dev) if d else None for d in dims3]
    gws, ds = _run_fold(idn, dev, c, dims3, widths, True, d_old)
    for gw, want, cols, name in ((gws[0], r["gW0c"], slice(pc, pc + C), "gW0"), (gws[1], r["gW5c"], slice(pc, pc + C), "gW5"),
                                 (gws[2], r["gWvc"], slice(256 + vc, 256 + vc + e), "gWv0")):
        assert torch.equal(gw[:, cols], want.float()), (name, dims3)
        assert bt.sentinel_outside(gw, cols), f"{name}: an element outside the conditioning columns was written"
    assert float(r["unit"].max()) < 2 ** 24
    s32 = r["s"].float()
    want_d = [None if a == 0 else d_old[0] + s32[:a],
              None if e == 0 else d_old[1] + ((r["s"][a:a + e] + r["sv"]) / 3.0).float(),
              None if l == 0 else d_old[2] + s32[a + e:]]
    for got, want, name in zip(ds, want_d, ("d_aud", "d_expr", "d_latent")):
        assert (got is None) == (want is None)
        if got is not None:
            assert torch.equal(got, want), (name, dims3, (got != want).nonzero()[:4].tolist())
    nan_dbv = torch.full((128,), NAN, device=dev)
    # the frozen launch: the same three bits, no gradient tensor
    _, ds_c = _run_fold(idn, dev, c, dims3, widths, False, d_old)
    for got, want, name in zip(ds_c, ds, ("d_aud", "d_expr", "d_latent")):
        assert (got is None) == (want is None) and (got is None or torch.equal(got.view(torch.int32), want.view(torch.int32))), name
    # without d_expr the expression's share leaves no trace, on either launch (the frozen one does not even read dbv)
    for full, dbv in ((True, None), (False, nan_dbv)):
        _, ds_n = _run_fold(idn, dev, c, dims3, widths, full, d_old, dbv=dbv, want_expr=False)
        assert ds_n[1] is None
        for i in (0, 2):
            assert (ds_n[i] is None) == (ds[i] is None) and (ds[i] is None or torch.equal(ds_n[i].view(torch.int32), ds[i].view(torch.int32))), (full, i)


def test_fold_bwd_without_conditioning_writes_nothing(idn, dev):
    """T5, dims (0, 0, 0): neither launch writes anything."""
    sd = bt.nan_net(63, 27, (0, 0, 0), dev)
    p = idn.ops.params_struct(sd, 0, 0, 0)
    db = [torch.ones(256, device=dev), torch.ones(256, device=dev), torch.ones(128, device=dev)]
    pairs = [guarded(s, dev) for s in ((256, 63), (256, 63 + 256), (128, 256 + 27))]
    idn.ops.fold_bwd(p, None, None, None, *db, *(v for _, v in pairs))
    idn.ops.fold_bwd(p, None, None, None, *db)
    torch.cuda.synchronize(dev)
    for w, _ in pairs:
        assert bool((w == SENTINEL).all())


@pytest.mark.parametrize("dims3,widths", FOLD_CASES, ids=lambda v: "x".join(map(str, v)))
def test_fold_bwd_rounding_vs_fp64(idn, dev, dims3, widths):
    """T5: Gaussian operands.  d cond (accumulated into zeros) within 2 EPS of fp64 relative to sum |w| |db| -- for d expr a
    third of the sum over its three layers --, the conditioning columns of the gradient tensors within 3 EPS relative."""
    pc, vc = widths
    a, e, l = dims3
    C = a + e + l
    c = _fold_case(idn, dev, dims3, widths, False, 60 + a + e)
    r = c["ref"]
    zeros = [torch.zeros(d, device=dev) if d else None for d in dims3]
    gws, ds = _run_fold(idn, dev, c, dims3, widths, True, zeros)
    truth = [r["s"][:a], (r["s"][a:a + e] + r["sv"]) / 3.0, r["s"][a + e:]]
    unit = [r["unit"][:a], (r["unit"][a:a + e] + r["unit_v"]) / 3.0, r["unit"][a + e:]]
    shares = {}
    for got, t, u, name in zip(ds, truth, unit, ("d_aud", "d_expr", "d_latent")):
        if got is not None:
            assert float(u.min()) > 0
            shares[name] = float(((got.double() - t).abs() / (2 * EPS * u)).max())
    for gw, want, cols, name in ((gws[0], r["gW0c"], slice(pc, pc + C), "gW0"), (gws[1], r["gW5c"], slice(pc, pc + C), "gW5"),
                                 (gws[2], r["gWvc"], slice(256 + vc, 256 + vc + e), "gWv0")):
        assert bt.sentinel_outside(gw, cols), name
        if want.numel():
            assert float(want.abs().min()) > 0
            shares[name] = float(((gw[:, cols].double() - want).abs() / (3 * EPS * want.abs())).max())
    print(f"\n  fold {dims3} {widths}: worst |err| / bound " + "  ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    bt.record(f"T5/{a}x{e}x{l}", shares)
    assert max(shares.values()) <= 1.0, shares


# ---------------------------------------------------------------------------------------------- T6
@pytest.mark.parametrize("P,p_pad", [(128, 128), (129, 256), (1000, 1024), (65600, 65664)])
def test_cond_colsums_exact(idn, dev, P, p_pad):
    """T6: integer matrices in [-8, 8]: db0' / db5' are the sums over all p_pad rows, dbv' the sum of columns 0..127 over the
    first P rows alone (NaN in rows P.. and in columns 128..255 of dV0).  At 65664 rows a block takes 256 rows and the last
    dbv' block ends inside its range.  Equalities; either group alone gives the same bits."""
    g = torch.Generator(device=dev).manual_seed(P)
    draw = lambda: torch.randint(-8, 9, (p_pad, 256), generator=g, device=dev).float()
    dA0, dA5, dV0 = draw(), draw(), draw()
    want_db = torch.stack([dA0.sum(0, dtype=torch.float64), dA5.sum(0, dtype=torch.float64)]).float()
    want_dbv = dV0[:P, :128].sum(0, dtype=torch.float64).float()
    dV0[P:] = NAN
    dV0[:, 128:] = NAN
    w_db, db = guarded((2, 256), dev)
    w_dbv, dbv = guarded((128,), dev)
    idn.ops.cond_colsums(dA0, dA5, dV0, P, db=db, dbv=dbv)
    assert guards_intact(w_db) and guards_intact(w_dbv)
    assert torch.equal(db, want_db), (db != want_db).nonzero()[:4].tolist()
    assert torch.equal(dbv, want_dbv), (dbv != want_dbv).nonzero()[:4].tolist()
    db2, none = idn.ops.cond_colsums(dA0, dA5, None, P)
    none2, dbv2 = idn.ops.cond_colsums(None, None, dV0, P)
    assert none is None and none2 is None and torch.equal(db2, want_db) and torch.equal(dbv2, want_dbv)


# ---------------------------------------------------------------------------------------------- T7
def test_the_aids_are_the_pass(idn, dev):
    """T7: the 37 x (64 + 128) case of tests/ray_grad_common.py, its fine network on 192 samples per ray.  ops.pass_bwd_ex with
    ray, expression and conditioning gradients; then dA[0], dA[5], dV0 from its workspace (carve_bwd: [p_pad, 256] matrices --
    eight dA, dV2 | dV1, dV0) through ops.input_grad, that d_x and the compositing backward's dL / d |rays_d| through
    ops.ray_grad, the pass's bias gradients through ops.fold_bwd: each result is the pass's bit for bit, on the backward pipe
    of this process."""
    import ray_grad_common as rg
    import test_cond_grad_gpu as tcg
    import test_ray_grad_gpu as trg
    from idealnerf_amd import autograd as ag
    from idealnerf_amd.helper import linspace01
    ops = idn.ops
    sc = rg.scene("37x64+128")
    _, _, fine = trg._network(idn, dev, sc)
    to = lambda t: t.to(dev)
    rays, bc = to(sc["rays"]).contiguous(), to(sc["bc"]).contiguous()
    aud, expr, lat = to(sc["aud"]), to(sc["expr"]), to(sc["latent"])
    n, S = sc["n"], sc["S"] + sc["Ni"]
    z = ops.coarse_depths(rays, linspace01(S, dev))
    raw, acts = ag._train_query(fine, fine.folded_bias(aud, expr, lat), rays, z)
    rs = np.random.RandomState(9)
    g_rgb = torch.from_numpy(rs.standard_normal((n, 3)).astype(np.float32)).to(dev)
    g_acc = torch.from_numpy(rs.standard_normal(n).astype(np.float32)).to(dev)
    sd = fine.kernel_tensors()
    p = fine.kernel_params()
    grads = {k: torch.full_like(sd[k], NAN) for k in ag.PARAM_KEYS}
    start = [torch.from_numpy(rs.standard_normal(d).astype(np.float32)).to(dev) for d in (64, 76, 32)]
    d_aud, d_expr, d_lat = (t.clone() for t in start)
    d_rays = torch.full((n, 11), NAN, device=dev)
    ops.pass_bwd_ex(p, grads, aud, expr, lat, acts, raw, z, rays, bc, g_rgb, None, None, g_acc, d_aud, d_lat, d_expr=d_expr, d_rays=d_rays)
    P = n * S
    Pp = (P + 127) // 128 * 128
    words = tcg._workspace(idn, dev, n, S).view(torch.float32)
    mat = lambda i: words[i * Pp * 256:(i + 1) * Pp * 256].view(Pp, 256)
    dA0, dA5, dV0 = mat(0).clone(), mat(5).clone(), mat(9).clone()
    pass_d_x = mat(1).reshape(-1)[:P * 90].view(P, 90).clone()   # launch_pass_bwd puts d_x into the delta matrix of pts_linears.1
    assert bool(torch.isfinite(pass_d_x).all()) and float(pass_d_x.abs().max()) > 0
    d_x, blocks = ops.input_grad(p, dA0, dA5, dV0, P)
    assert blocks == min((Pp // 32 + 15) // 16, torch.cuda.get_device_properties(dev).multi_processor_count)
    assert torch.equal(d_x.view(torch.int32), pass_d_x.view(torch.int32)), "ops.input_grad is not the pass's d_x"
    d_norm = torch.zeros((n, 11), device=dev)
    ops.composite_bwd(raw, z, rays, bc, g_rgb, None, None, g_acc, d_rgb=torch.empty((P, 64), device=dev),
                      d_sig=torch.empty((P, 256), device=dev), sig_col=128, d_norm=d_norm, norm_col=6)
    assert float(d_norm[:, 6].abs().min()) > 0
    mine = torch.full((n, 11), NAN, device=dev)
    mine[:, 6] = d_norm[:, 6]
    ops.ray_grad(d_x, 63, 27, rays, z, mine)
    assert torch.equal(mine.view(torch.int32), d_rays.view(torch.int32)), "ops.ray_grad is not the pass's d_rays"
    gws = [torch.full_like(grads[k], NAN) for k in ("pts_linears.0.weight", "pts_linears.5.weight", "views_linears.0.weight")]
    mine_d = [t.clone() for t in start]
    ops.fold_bwd(p, aud, expr, lat, grads["pts_linears.0.bias"], grads["pts_linears.5.bias"], grads["views_linears.0.bias"], *gws,
                 d_aud=mine_d[0], d_expr=mine_d[1], d_latent=mine_d[2])
    for got, want, old, name in zip(mine_d, (d_aud, d_expr, d_lat), start, ("d_aud", "d_expr", "d_latent")):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not torch.equal(got, old), name
    for gw, key, cols in zip(gws, ("pts_linears.0.weight", "pts_linears.5.weight", "views_linears.0.weight"),
                             (slice(63, 63 + 172), slice(63, 63 + 172), slice(283, 283 + 76))):
        assert torch.equal(gw[:, cols].contiguous().view(torch.int32), grads[key][:, cols].contiguous().view(torch.int32)), key
    # the frozen plan's column sums and fold: ops.pass_bwd_ex(grads=None) against the two aids on the same deltas
    f_aud, f_expr, f_lat = (t.clone() for t in start)
    d_vb = torch.full((128,), NAN, device=dev)
    ops.pass_bwd_ex(p, None, aud, expr, lat, acts, raw, z, rays, bc, g_rgb, None, None, g_acc, f_aud, f_lat, d_expr=f_expr, d_views0_bias=d_vb)
    db, dbv = ops.cond_colsums(mat(0), mat(5), mat(9), P)
    assert torch.equal(dbv.view(torch.int32), d_vb.view(torch.int32)), "ops.cond_colsums is not the frozen plan's d_views0_bias"
    mine_f = [t.clone() for t in start]
    ops.fold_bwd(p, aud, expr, lat, db[0], db[1], dbv, d_aud=mine_f[0], d_expr=mine_f[1], d_latent=mine_f[2])
    for got, want, name in zip(mine_f, (f_aud, f_expr, f_lat), ("d_aud", "d_expr", "d_latent")):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), ("frozen", name)


def test_the_aids_are_the_pass_on_the_other_backward_pipe(dev):
    """T7 again in a fresh process on the other backward pipe (IDN_BACKWARD_PIPE is read once per process)."""
    other = "x6" if os.environ.get("IDN_BACKWARD_PIPE") == "f32" else "f32"
    env = dict(os.environ, IDN_BACKWARD_PIPE=other)
    env.pop("IDN_BACKWARD_TAIL_RECORD", None)
    child = subprocess.Popen([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-k", "test_the_aids_are_the_pass and not other"],
                             env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True,
                             cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        out, err = child.communicate(timeout=180)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.wait()
        pytest.fail("the child run did not finish within 180 s")
    assert child.returncode == 0 and "1 passed" in out, out[-3000:] + err[-2000:]
