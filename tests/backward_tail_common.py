"""Shared by tests/test_backward_tail_gpu.py (not collected by pytest): operands and fp64 references of what a training
backward runs after the delta chain -- dx_kernel, ray_grad_kernel, fold_bwd_kernel and the two column-sum kernels."""
import json
import os

import torch

from test_delta_chain_gpu import SENTINEL, guarded, guards_intact

NAN = float("nan")
EPS = 2.0 ** -24
WIDTHS = [(63, 27), (3, 3), (27, 15), (33, 9)]                 # (pts_ch, views_ch)
ROWS = [(1, 128), (33, 128), (128, 128), (129, 256), (185, 256)]   # (n, p_pad)
DIMS = [(64, 76, 32), (106, 0, 0)]                             # (dim_aud, dim_expr, dim_latent): ld0 / ld5 / ldv differ


def record(key, value):
    path = os.environ.get("IDN_BACKWARD_TAIL_RECORD")
    if not path:
        return
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(old, open(path, "w"), indent=1, sort_keys=True)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# ---------------------------------------------------------------------------------------------- networks
def nan_net(pts_ch, views_ch, dims3, dev):
    """All 24 tensors of a network of these widths in state-dict layout on the device, every element NaN: a test fills the
    blocks its kernel may read and leaves the NaN everywhere else."""
    a, e, l = dims3
    C = a + e + l
    sd = {}
    for i in range(8):
        fan_in = pts_ch + C if i == 0 else (256 + pts_ch + C if i == 5 else 256)
        sd[f"pts_linears.{i}.weight"] = torch.full((256, fan_in), NAN, device=dev)
        sd[f"pts_linears.{i}.bias"] = torch.full((256,), NAN, device=dev)
    sd["views_linears.0.weight"] = torch.full((128, 256 + views_ch + e), NAN, device=dev)
    sd["views_linears.1.weight"] = torch.full((128, 128), NAN, device=dev)
    sd["views_linears.2.weight"] = torch.full((128, 128), NAN, device=dev)
    for i in range(3):
        sd[f"views_linears.{i}.bias"] = torch.full((128,), NAN, device=dev)
    sd["alpha_linear.weight"], sd["alpha_linear.bias"] = torch.full((1, 256), NAN, device=dev), torch.full((1,), NAN, device=dev)
    sd["rgb_linear.weight"], sd["rgb_linear.bias"] = torch.full((3, 128), NAN, device=dev), torch.full((3,), NAN, device=dev)
    return sd


def dx_blocks(sd, pts_ch, views_ch):
    """Views of the three weight blocks dx_kernel reads: W0[:, :pts_ch], W5[:, :pts_ch], Wv0[:, 256:256 + views_ch]."""
    return (sd["pts_linears.0.weight"][:, :pts_ch], sd["pts_linears.5.weight"][:, :pts_ch],
            sd["views_linears.0.weight"][:, 256:256 + views_ch])


# ---------------------------------------------------------------------------------------------- dx_kernel
def dx_deltas(n, p_pad, fill, dev):
    """dA0, dA5, dV0 [p_pad, 256] with fill(rows, cols) in the rows below n (dV0: columns 0..127) and NaN in everything the
    kernel must not read or may only read into columns it does not store: rows n.., and columns 128..255 of dV0."""
    out = []
    for cols in (256, 256, 128):
        m = torch.full((p_pad, 256), NAN)
        m[:n, :cols] = fill(n, cols)
        out.append(m.to(dev))
    return out


def dx_reference(deltas, blocks, n):
    """fp64 d_x [n, pts_ch + views_ch] and the element's unit sum_k |delta_k| |w_k|, same shape."""
    dA0, dA5, dV0 = (d[:n].double() for d in deltas)
    W0, W5, Wv = (b.double() for b in blocks)
    ref = torch.cat([dA0 @ W0 + dA5 @ W5, dV0[:, :128] @ Wv], 1)
    unit = torch.cat([dA0.abs() @ W0.abs() + dA5.abs() @ W5.abs(), dV0[:, :128].abs() @ Wv.abs()], 1)
    return ref, unit


def run_dx(idn, p, deltas, n, cols, max_blocks=0):
    """One call of ops.input_grad into a guarded [n, cols] buffer: the guards (and so every row at or past n) hold the
    sentinel afterwards and every element below is finite.  -> (d_x, blocks)."""
    whole, d_x = guarded((n, cols), deltas[0].device)
    got, blocks = idn.ops.input_grad(p, *deltas, n, d_x=d_x, max_blocks=max_blocks)
    assert got.data_ptr() == d_x.data_ptr()
    assert guards_intact(whole), "a write outside d_x (at or past row n, or in front of row 0)"
    assert bool(torch.isfinite(d_x).all()), "an element of d_x was not written, or a NaN the kernel must not read reached it"
    return d_x, blocks


def first_difference(got, ref):
    bad = (got != ref).nonzero()
    row, col = (int(v) for v in bad[0])
    return bad.shape[0], row, col


# ---------------------------------------------------------------------------------------------- ray_grad_kernel
def pe_columns(L):
    """Column of gamma_L's (band k, axis a) sine and cosine: 3 + 6 k + a, 6 + 6 k + a."""
    return [(k, a, 3 + 6 * k + a, 6 + 6 * k + a) for k in range(L) for a in range(3)]


def ray_grad_reference(d_x, pts_ch, views_ch, rays, z, d_norm):
    """fp64 truth of ray_grad_kernel and the unit of its bound, both [n, 11] (columns 6, 7 zero).  The point is the forward's:
    p = fl32(o + fl32(d z)), so 2^k p is the kernel's own argument; everything after it is fp64.
      truth: per sample  acc = g_id + sum_k 2^k (cos(2^k p) g_sin - sin(2^k p) g_cos);  d o = sum_s acc, d d = sum_s z_s acc +
             d_norm d / |d| (0 for a zero direction), d v = sum_s acc_v
      unit:  U = sum_s (|g_id| + sum_k 2^k (|g_sin| + |g_cos|)), times |z_s| for d d; -> (truth, U, |d_norm| per ray)"""
    n, S = z.shape
    L, Lv = (pts_ch - 3) // 6, (views_ch - 3) // 6
    o, d, v = rays[:, None, 0:3], rays[:, None, 3:6], rays[:, None, 8:11]
    p32 = o + d * z[:, :, None]                                 # two fp32 roundings (eager: a product kernel, then a sum kernel)
    assert p32.dtype == torch.float32
    g = d_x.double().view(n, S, pts_ch + views_ch)
    z64 = z.double()[:, :, None]

    def backward(gg, x64, bands):
        acc, unit = gg[..., 0:3].clone(), gg[..., 0:3].abs()
        for k in range(bands):
            f = 2.0 ** k
            gs, gc = gg[..., 3 + 6 * k:6 + 6 * k], gg[..., 6 + 6 * k:9 + 6 * k]
            acc = acc + f * (torch.cos(f * x64) * gs - torch.sin(f * x64) * gc)
            unit = unit + f * (gs.abs() + gc.abs())
        return acc, unit
    acc, unit = backward(g[..., :pts_ch], p32.double(), L)
    accv, unitv = backward(g[..., pts_ch:], v.double().expand(n, S, 3), Lv)
    d64 = rays[:, 3:6].double()
    norm = d64.norm(dim=1, keepdim=True)
    gn = torch.where(norm > 0, d_norm.double()[:, None] / norm.clamp_min(1e-300), torch.zeros_like(norm))
    truth = torch.zeros((n, 11), dtype=torch.float64, device=z.device)
    U = torch.zeros_like(truth)
    truth[:, 0:3], U[:, 0:3] = acc.sum(1), unit.sum(1)
    truth[:, 3:6], U[:, 3:6] = (z64 * acc).sum(1) + gn * d64, (z64.abs() * unit).sum(1)
    truth[:, 8:11], U[:, 8:11] = accv.sum(1), unitv.sum(1)
    return truth, U, torch.where(norm[:, 0] > 0, d_norm.double().abs(), torch.zeros_like(norm[:, 0]))


def run_ray_grad(idn, d_x, pts_ch, views_ch, rays, z, d_norm):
    """One call of ops.ray_grad on a guarded d_rays that holds the sentinel in every column but 6 (= d_norm): afterwards the
    guards are intact, columns 6 and 7 are +0.0 and every other column is finite.  -> d_rays [n, 11]."""
    n = z.shape[0]
    whole, d_rays = guarded((n, 11), z.device)
    d_rays[:, 6] = d_norm
    assert int((d_rays.view(torch.int32) == SENTINEL).sum()) == 10 * n
    got = idn.ops.ray_grad(d_x, pts_ch, views_ch, rays, z, d_rays)
    assert got.data_ptr() == d_rays.data_ptr()
    assert guards_intact(whole), "a write outside d_rays"
    assert bool((d_rays[:, 6:8].contiguous().view(torch.int32) == 0).all()), "columns 6 and 7 are not +0.0"
    assert bool(torch.isfinite(d_rays).all()), "a column of d_rays was not written"
    return d_rays


# ---------------------------------------------------------------------------------------------- fold
def cond_blocks(sd, pts_ch, views_ch, dims3):
    """Views of the blocks fold_bwd_kernel reads: W0[:, pts_ch:pts_ch + C], W5[:, pts_ch:pts_ch + C], Wv0[:, 256 + views_ch:]."""
    C = sum(dims3)
    return (sd["pts_linears.0.weight"][:, pts_ch:pts_ch + C], sd["pts_linears.5.weight"][:, pts_ch:pts_ch + C],
            sd["views_linears.0.weight"][:, 256 + views_ch:])


def fold_reference(blocks, dims3, cond, db0, db5, dbv):
    """fp64: (s [C] = the d cond sums, sv [e] = the views_linears.0 share of d expr, unit [C], unit_v [e], the outer products
    gW0c / gW5c [256, C] and gWvc [128, e]).  cond = (aud, expr, latent) as the forward takes them (expr enters as expr / 3)."""
    a, e, l = dims3
    W0c, W5c, Wvc = (b.double() for b in blocks)
    cv = torch.cat([t.double() / (3.0 if i == 1 else 1.0) for i, t in enumerate(cond) if t is not None]) if sum(dims3) else db0.new_zeros(0).double()
    d0, d5, dv = db0.double(), db5.double(), dbv.double()
    s = d0 @ W0c + d5 @ W5c
    unit = d0.abs() @ W0c.abs() + d5.abs() @ W5c.abs()
    sv, unit_v = dv @ Wvc, dv.abs() @ Wvc.abs()
    return dict(s=s, sv=sv, unit=unit, unit_v=unit_v, gW0c=d0[:, None] * cv[None, :], gW5c=d5[:, None] * cv[None, :],
                gWvc=dv[:, None] * cv[None, a:a + e])


def sentinel_outside(whole_view, cols):
    """True where every element of the [rows, ld] float view outside the column range still holds the sentinel's bits."""
    w = whole_view.view(torch.int32)
    keep = torch.ones(w.shape[1], dtype=torch.bool, device=w.device)
    keep[cols] = False
    return bool((w[:, keep] == SENTINEL).all())
