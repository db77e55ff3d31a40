"""Tensor-level entry points over the C ABI.  torch is plumbing here: device memory,
the HIP stream of the tensors' device and nothing else.  Every function requires CUDA
(ROCm) fp32 contiguous tensors of the documented shapes, all on ONE device, and raises
``IdealNerfError`` otherwise -- before the C call, and with no silent fallback.  The launch
happens on the tensors' own device and on that device's current stream, whatever the
process-wide current device is (``Network.to('cuda:1')`` without ``set_device(1)`` is legal,
as it is for the reference's torch ops).
"""
import contextlib
import ctypes as C
import os
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import IDN_PREC_F32, RAY_FLOATS, IdealNerfError, check

PTS_CH, VIEWS_CH, W_HID = 63, 27, 256   # the widest encodings (multires 10 / multires_views 4): the defaults


def embed_channels(multires: int, views: bool = False) -> int:
    """Input channels of an encoding of `multires` octaves: 3 + 6 multires, helper.get_embedder's out_dim.  Raises
    NotImplementedError naming the flag outside 0..10 (points) / 0..4 (view directions), the compiled input tiles."""
    limit = _lib.MAX_MULTIRES_VIEWS if views else _lib.MAX_MULTIRES
    name = "multires_views" if views else "multires"
    if not 0 <= int(multires) <= limit:
        raise NotImplementedError(f"{name}={multires}: libidealnerf is compiled for {name} in 0..{limit} "
                                  f"({3 + 6 * limit} input channels at the most)")
    return 3 + 6 * int(multires)


def check_input_channels(input_ch: int, input_ch_views: int):
    """The widths a FaceNeRF / FaceNeRFAgg may have: 3 + 6 L with L in 0..10 (points) and 0..4 (view directions)."""
    for ch, name, flag, limit in ((input_ch, "input_ch", "multires", _lib.MAX_MULTIRES),
                                  (input_ch_views, "input_ch_views", "multires_views", _lib.MAX_MULTIRES_VIEWS)):
        if ch != int(ch) or ch < 3 or (ch - 3) % 6 or (ch - 3) // 6 > limit:
            raise NotImplementedError(f"{name}={ch}: libidealnerf is compiled for {name} = 3 + 6 {flag} with {flag} in "
                                      f"0..{limit} (at most {3 + 6 * limit})")


def widths(p):
    """(pts_ch, views_ch) of an idn_facenerf_params struct; 63 / 27 for one that leaves the two fields zero."""
    m, v = p.multires_plus1, p.multires_views_plus1
    return (6 * m - 3 if m else PTS_CH), (6 * v - 3 if v else VIEWS_CH)


def _ptr(t: Optional[torch.Tensor], name="tensor", dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise IdealNerfError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise IdealNerfError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise IdealNerfError(f"{name} must be contiguous")
    return t.data_ptr()


def _shape(t: Optional[torch.Tensor], name: str, *shape):
    """t must have exactly this shape (None = any size in that position)."""
    if t is None:
        return
    got = tuple(t.shape)
    if len(got) != len(shape) or any(s is not None and int(s) != g for s, g in zip(shape, got)):
        want = "[" + ", ".join("*" if s is None else str(int(s)) for s in shape) + "]"
        raise IdealNerfError(f"{name} must be {want}, got {list(got)}")


class _Launch:
    """One C call: every tensor argument on one GPU; that GPU current for the duration of the call
    (the library launches on the calling thread's current HIP device) and its current stream."""

    def __init__(self, *tensors, device=None):
        devs = {t.device for t in tensors if t is not None and t.is_cuda}
        if device is not None:
            d = torch.device(device)
            if d.type != "cuda":
                raise IdealNerfError(f"the HIP path renders on the GPU (got device {device}); there is no CPU fallback")
            devs.add(torch.device("cuda", torch.cuda.current_device() if d.index is None else d.index))
        if len(devs) > 1:
            raise IdealNerfError("all tensors of one call must live on the same GPU, got " +
                                 ", ".join(sorted(str(d) for d in devs)))
        self.device = devs.pop() if devs else None
        self._ctx = contextlib.nullcontext()

    def __enter__(self):
        if self.device is not None:
            self._ctx = torch.cuda.device(self.device)
            self._ctx.__enter__()
            self.stream = torch.cuda.current_stream(self.device).cuda_stream
        else:   # only CPU tensors: let _ptr raise the "must live on the GPU" error
            self.stream = None
        return self

    def __exit__(self, *exc):
        return self._ctx.__exit__(*exc)


def _precision(precision):
    if precision not in (_lib.IDN_PREC_F32, _lib.IDN_PREC_BF16X3, _lib.IDN_PREC_BF16, _lib.IDN_PREC_FP16X3, _lib.IDN_PREC_BF16X6):
        raise IdealNerfError(f"unknown precision code {precision}")
    return int(precision)


def _net_buffers(lib, packed, folded, precision, which=""):
    """The two per-network device buffers must have the sizes the kernels walk."""
    if packed is not None:
        _shape(packed, f"packed{which}", lib.idealnerf_packed_weight_floats(_precision(precision)))
    if folded is not None:
        _shape(folded, f"folded{which}", lib.idealnerf_folded_bias_floats())


def params_struct(sd: Dict[str, torch.Tensor], dim_aud: int, dim_expr: int, dim_latent: int, prefix: str = "",
                  pts_ch: int = PTS_CH, views_ch: int = VIEWS_CH):
    """state_dict-keyed tensors (models/face_nerf.py:27-37 names) -> idn_facenerf_params.  pts_ch / views_ch: the
    network's input widths (FaceNeRF's input_ch / input_ch_views), 3 + 6 multires each."""
    check_input_channels(pts_ch, views_ch)
    p = _lib.FaceNerfParams()
    C_all = pts_ch + dim_aud + dim_expr + dim_latent

    def get(key, shape):
        t = sd[prefix + key]
        if tuple(t.shape) != shape:
            raise IdealNerfError(f"{key}: shape {tuple(t.shape)} != {shape} (D=8, W=256, skips=[4] with "
                                 f"{pts_ch} point and {views_ch} direction channels)")
        return _ptr(t, key)

    for i in range(8):
        fan_in = C_all if i == 0 else (W_HID + C_all if i == 5 else W_HID)
        p.pts_w[i] = get(f"pts_linears.{i}.weight", (W_HID, fan_in))
        p.pts_b[i] = get(f"pts_linears.{i}.bias", (W_HID,))
    p.views_w[0] = get("views_linears.0.weight", (W_HID // 2, W_HID + views_ch + dim_expr))
    p.views_b[0] = get("views_linears.0.bias", (W_HID // 2,))
    for i in (1, 2):
        p.views_w[i] = get(f"views_linears.{i}.weight", (W_HID // 2, W_HID // 2))
        p.views_b[i] = get(f"views_linears.{i}.bias", (W_HID // 2,))
    p.alpha_w = get("alpha_linear.weight", (1, W_HID))
    p.alpha_b = get("alpha_linear.bias", (1,))
    p.rgb_w = get("rgb_linear.weight", (3, W_HID // 2))
    p.rgb_b = get("rgb_linear.bias", (3,))
    p.dim_aud, p.dim_expr, p.dim_latent = dim_aud, dim_expr, dim_latent
    p.multires_plus1, p.multires_views_plus1 = (pts_ch - 3) // 6 + 1, (views_ch - 3) // 6 + 1
    return p


def pack_weights(p, device, precision=IDN_PREC_F32) -> torch.Tensor:
    """`p` holds raw addresses: the caller (FaceNeRF.packed_weights) guarantees they live on `device`."""
    lib = _lib.load()
    with _Launch(device=device) as L:
        out = torch.empty(lib.idealnerf_packed_weight_floats(_precision(precision)), dtype=torch.float32, device=L.device)
        check(lib.idealnerf_pack_weights(C.byref(p), precision, out.data_ptr(), L.stream))
    return out


def fold_conditioning(p, aud, expr, latent, device) -> torch.Tensor:
    lib = _lib.load()
    _shape(aud, "aud", p.dim_aud)
    _shape(expr, "expr", p.dim_expr)
    _shape(latent, "latent", p.dim_latent)
    if aud is None and p.dim_aud:
        raise IdealNerfError(f"aud is None but the network was built with dim_aud={p.dim_aud}")
    with _Launch(aud, expr, latent, device=device) as L:
        out = torch.empty(lib.idealnerf_folded_bias_floats(), dtype=torch.float32, device=L.device)
        check(lib.idealnerf_fold_conditioning(C.byref(p), _ptr(aud, "aud"), _ptr(expr, "expr"), _ptr(latent, "latent"),
                                              out.data_ptr(), L.stream))
    return out


def facenerf_fwd(packed, folded, x, precision=IDN_PREC_F32, pts_ch=PTS_CH, views_ch=VIEWS_CH) -> torch.Tensor:
    """x [n, pts_ch + views_ch] -> [n, 4]; `packed` must be the stream of a network of those widths."""
    lib = _lib.load()
    check_input_channels(pts_ch, views_ch)
    _shape(x, "x", None, pts_ch + views_ch)
    _net_buffers(lib, packed, folded, precision)
    with _Launch(packed, folded, x) as L:
        out = torch.empty((x.shape[0], 4), dtype=torch.float32, device=x.device)
        check(lib.idealnerf_facenerf_fwd_ch(_ptr(packed, "packed"), _ptr(folded, "folded"), precision, _ptr(x, "x"),
                                            pts_ch, views_ch, x.shape[0], out.data_ptr(), L.stream))
    return out


def facenerf_train_fwd(packed, folded, x, precision=_lib.IDN_PREC_BF16X6, pts_ch=PTS_CH, views_ch=VIEWS_CH):
    """FaceNeRF.forward that also records the backward's activation slab (idealnerf_facenerf_train_fwd_ch):
    x [n, pts_ch + views_ch] -> (out [n, 4], acts [idealnerf_train_acts_floats(n)]).  precision: IDN_PREC_F32 or
    IDN_PREC_BF16X6 only."""
    lib = _lib.load()
    check_input_channels(pts_ch, views_ch)
    _shape(x, "x", None, pts_ch + views_ch)
    if precision not in (_lib.IDN_PREC_F32, _lib.IDN_PREC_BF16X6):
        raise IdealNerfError(f"the training forward runs IDN_PREC_F32 or IDN_PREC_BF16X6 only (got {precision})")
    _net_buffers(lib, packed, folded, precision)
    n = x.shape[0]
    with _Launch(packed, folded, x) as L:
        out = torch.empty((n, 4), dtype=torch.float32, device=x.device)
        acts = torch.empty(lib.idealnerf_train_acts_floats(n), dtype=torch.float32, device=x.device)
        check(lib.idealnerf_facenerf_train_fwd_ch(_ptr(packed, "packed"), _ptr(folded, "folded"), precision, _ptr(x, "x"),
                                                  pts_ch, views_ch, n, out.data_ptr(), acts.data_ptr(), L.stream))
    return out, acts


def grads_struct(grads: Dict[str, torch.Tensor]):
    """state_dict-keyed gradient tensors (the 24 of idn_facenerf_params) -> idn_facenerf_grads."""
    g = _lib.FaceNerfGrads()
    for i in range(8):
        g.pts_w[i] = grads[f"pts_linears.{i}.weight"].data_ptr()
        g.pts_b[i] = grads[f"pts_linears.{i}.bias"].data_ptr()
    for i in range(3):
        g.views_w[i] = grads[f"views_linears.{i}.weight"].data_ptr()
        g.views_b[i] = grads[f"views_linears.{i}.bias"].data_ptr()
    g.alpha_w, g.alpha_b = grads["alpha_linear.weight"].data_ptr(), grads["alpha_linear.bias"].data_ptr()
    g.rgb_w, g.rgb_b = grads["rgb_linear.weight"].data_ptr(), grads["rgb_linear.bias"].data_ptr()
    return g


def facenerf_bwd(p, grads, aud, expr, latent, acts, g_out, d_x=None, d_aud=None, d_expr=None, d_latent=None):
    """Backward of FaceNeRF.forward (idealnerf_facenerf_bwd) from the slab of facenerf_train_fwd.  p: params_struct of the
    module; grads: state_dict-keyed tensors of the parameters' shapes, OVERWRITTEN; g_out [n, 4] = dL/d out;
    d_x [n, pts_ch + views_ch] of the network `p` describes (overwritten) and d_aud / d_expr / d_latent (accumulated) may each be None."""
    lib = _lib.load()
    _shape(g_out, "g_out", None, 4)
    n = g_out.shape[0]
    _shape(acts, "acts", lib.idealnerf_train_acts_floats(n))
    _shape(d_x, "d_x", n, sum(widths(p)))
    for t, name, dim in ((aud, "aud", p.dim_aud), (expr, "expr", p.dim_expr), (latent, "latent", p.dim_latent),
                         (d_aud, "d_aud", p.dim_aud), (d_expr, "d_expr", p.dim_expr), (d_latent, "d_latent", p.dim_latent)):
        _shape(t, name, dim)
    for k, t in grads.items():
        _ptr(t, f"grad {k}")
    with _Launch(aud, expr, latent, acts, g_out, d_x, d_aud, d_expr, d_latent, *grads.values()) as L:
        ptrs = [_ptr(t, name) for t, name in ((aud, "aud"), (expr, "expr"), (latent, "latent"), (acts, "acts"))]
        ptrs += [n, _ptr(g_out, "g_out")]
        ptrs += [_ptr(t, name) for t, name in ((d_x, "d_x"), (d_aud, "d_aud"), (d_expr, "d_expr"), (d_latent, "d_latent"))]
        ws = _workspace(lib.idealnerf_facenerf_bwd_workspace_bytes(n), g_out.device, L.stream)
        check(lib.idealnerf_facenerf_bwd(C.byref(p), C.byref(grads_struct(grads)), *ptrs, ws.data_ptr(), ws.numel(), L.stream))
    return grads


def query_rays_train_fwd(packed, folded, rays, z, precision=_lib.IDN_PREC_BF16X6, pts_ch=PTS_CH, views_ch=VIEWS_CH):
    """query_rays_fwd that also records the backward's activation slab (idealnerf_query_rays_train_fwd_ch):
    -> (raw [n, S, 4], acts [idealnerf_train_acts_floats(n * S)]).  pts_ch / views_ch: the widths of the network `packed`
    is the stream of; the slab's x0 / dir matrices hold zeros beyond them."""
    lib = _lib.load()
    check_input_channels(pts_ch, views_ch)
    _shape(z, "z", None, None)
    n, S = z.shape
    _shape(rays, "rays", n, RAY_FLOATS)
    with _Launch(packed, folded, rays, z) as L:
        raw = torch.empty((n, S, 4), dtype=torch.float32, device=z.device)
        acts = torch.empty(lib.idealnerf_train_acts_floats(n * S), dtype=torch.float32, device=z.device)
        check(lib.idealnerf_query_rays_train_fwd_ch(_ptr(packed, "packed"), _ptr(folded, "folded"), precision, _ptr(rays, "rays"),
                                                    _ptr(z, "z"), n, S, pts_ch, views_ch, raw.data_ptr(), acts.data_ptr(), L.stream))
    return raw, acts


def _pass_bwd(p, grads, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent, d_views0_bias=None,
              d_rays=None, with_rays=False, d_expr=None, ex=False):
    """The checks and the call behind `pass_bwd` (grads: a dict), `pass_bwd_rays` (with_rays), `pass_bwd_cond` (grads: None)
    and `pass_bwd_ex` (ex: either plan through idealnerf_pass_bwd_ex, with d_expr / d_rays / d_views0_bias as its extras)."""
    lib = _lib.load()
    if grads is None:
        grads = {}
    n, S = z.shape
    for t, name, shape in ((raw, "raw", (n, S, 4)), (rays, "rays", (n, RAY_FLOATS)), (bc, "bc_rgb", (n, 3)),
                           (g_rgb, "g_rgb_map", (n, 3)), (g_fg, "g_rgb_fg", (n, 3)), (g_lw, "g_last_weight", (n,)),
                           (g_acc, "g_acc", (n,)), (d_rays, "d_rays", (n, RAY_FLOATS)), (d_expr, "d_expr", (p.dim_expr,))):
        _shape(t, name, *shape)
    tensors = (aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent)
    with _Launch(*tensors, d_rays, d_expr, d_views0_bias if ex else None, *grads.values()) as L:
        ws = _workspace(lib.idealnerf_pass_bwd_workspace_bytes(n, S), z.device, L.stream)   # scratch of this (device, stream): two streams training on one GPU do not share it
        ptrs = [_ptr(t) for t in tensors]
        if ex:
            _shape(d_views0_bias, "d_views0_bias", W_HID // 2)
            extra = _lib.PassBwdExtra(_ptr(d_expr, "d_expr"), _ptr(d_rays, "d_rays"), _ptr(d_views0_bias, "d_views0_bias"))
            check(lib.idealnerf_pass_bwd_ex(C.byref(p), C.byref(grads_struct(grads)) if grads else None, *ptrs[:8], n, S, *ptrs[8:],
                                            C.byref(extra), ws.data_ptr(), ws.numel(), L.stream))
        elif with_rays:
            check(lib.idealnerf_pass_bwd_rays(C.byref(p), C.byref(grads_struct(grads)), *ptrs[:8], n, S, *ptrs[8:], _ptr(d_rays, "d_rays"),
                                              ws.data_ptr(), ws.numel(), L.stream))
        elif grads:
            check(lib.idealnerf_pass_bwd(C.byref(p), C.byref(grads_struct(grads)), *ptrs[:8], n, S, *ptrs[8:], ws.data_ptr(), ws.numel(), L.stream))
        else:
            check(lib.idealnerf_pass_bwd_cond(C.byref(p), *ptrs[:8], n, S, *ptrs[8:], ws.data_ptr(), ws.numel(), L.stream))
    return grads


def pass_bwd(p, grads, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent):
    """Backward of one render pass (idealnerf_pass_bwd) from the slab of query_rays_train_fwd.  grads: as facenerf_bwd,
    OVERWRITTEN; g_* = dL/d (rgb_map, rgb_fg, last_weight, acc_map), each may be None; d_aud / d_latent: accumulated."""
    return _pass_bwd(p, grads, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent)


def pass_bwd_rays(p, grads, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent, d_rays):
    """`pass_bwd` that also returns the gradient of the ray records (idealnerf_pass_bwd_rays): d_rays [n, 11], OVERWRITTEN --
    columns 0:3 d rays_o, 3:6 d rays_d, 8:11 d viewdirs, 6:8 zeros.  d_rays None: the entry behaves as `pass_bwd`."""
    return _pass_bwd(p, grads, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent,
                     d_rays=d_rays, with_rays=True)


def pass_bwd_cond(p, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent, d_views0_bias=None):
    """`pass_bwd` for a network none of whose parameters takes a gradient (idealnerf_pass_bwd_cond): the same compositing
    backward and delta chain, then only the column sums and the fold range d aud / d latent need.  d_aud / d_latent:
    accumulated; nothing else is written.

    d_views0_bias [128] (optional, OVERWRITTEN): the gradient of views_linears.0's bias -- what `pass_bwd` returns as that
    entry of `grads` -- for a network whose conditioning also reaches that bias (FaceNeRFAgg).  That entry does not return it:
    with it the call goes through idealnerf_pass_bwd_ex, which sums the deltas' columns itself (fp64, fixed order, the pass's
    real rows).  Needs d_aud or d_latent: with both None the entry launches nothing."""
    if d_views0_bias is not None and d_aud is None and d_latent is None:
        raise IdealNerfError("pass_bwd_cond: d_views0_bias needs d_aud or d_latent (with neither the pass is not run)")
    _pass_bwd(p, None, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent, d_views0_bias,
              ex=d_views0_bias is not None)


def pass_bwd_ex(p, grads, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent, d_expr=None,
                d_rays=None, d_views0_bias=None):
    """The pass backward with every optional gradient (idealnerf_pass_bwd_ex).  grads: a dict as `pass_bwd` takes it (the
    training plan), or None (the frozen plan of `pass_bwd_cond`: it runs when any of d_aud / d_latent / d_expr is given).
      d_expr [dim_expr]: ACCUMULATED, like d_aud -- the gradient of the expression the pass was conditioned on;
      d_rays [n, 11]: OVERWRITTEN, as `pass_bwd_rays` (the training plan only);
      d_views0_bias [128]: OVERWRITTEN, the bias gradient of views_linears.0, written by the entry itself (the frozen plan only).
    Every other output is bit for bit what `pass_bwd` / `pass_bwd_rays` / `pass_bwd_cond` return on the same inputs.  The
    background needs no call: d bc = g_rgb * last_weight[:, None] of the pass's forward."""
    return _pass_bwd(p, grads, aud, expr, latent, acts, raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_aud, d_latent,
                     d_views0_bias=d_views0_bias, d_rays=d_rays, d_expr=d_expr, ex=True)


def query_rays_fwd(packed, folded, rays, z, precision=IDN_PREC_F32) -> torch.Tensor:
    lib = _lib.load()
    _shape(z, "z", None, None)
    n, S = z.shape
    _shape(rays, "rays", n, RAY_FLOATS)
    _net_buffers(lib, packed, folded, precision)
    with _Launch(packed, folded, rays, z) as L:
        raw = torch.empty((n, S, 4), dtype=torch.float32, device=z.device)
        check(lib.idealnerf_query_rays_fwd(_ptr(packed, "packed"), _ptr(folded, "folded"), precision, _ptr(rays, "rays"),
                                           _ptr(z, "z"), n, S, raw.data_ptr(), L.stream))
    return raw


def query_points_fwd(packed, folded, pts, viewdirs, precision=IDN_PREC_F32) -> torch.Tensor:
    lib = _lib.load()
    _shape(pts, "pts", None, None, 3)
    n, S, _ = pts.shape
    _shape(viewdirs, "viewdirs", n, 3)
    _net_buffers(lib, packed, folded, precision)
    with _Launch(packed, folded, pts, viewdirs) as L:
        raw = torch.empty((n, S, 4), dtype=torch.float32, device=pts.device)
        check(lib.idealnerf_query_points_fwd(_ptr(packed, "packed"), _ptr(folded, "folded"), precision, _ptr(pts, "pts"),
                                             _ptr(viewdirs, "viewdirs"), n, S, raw.data_ptr(), L.stream))
    return raw


def frame_rays(c2w, H, W, focal, near, far, row0=0, nrows=None, cx=None, cy=None, device="cuda") -> torch.Tensor:
    lib = _lib.load()
    nrows = H - row0 if nrows is None else nrows
    if not (0 <= row0 and 0 <= nrows and row0 + nrows <= H and W > 0):
        raise IdealNerfError(f"rows [{row0}, {row0 + nrows}) are outside a {H}x{W} frame")
    if tuple(c2w.shape[-2:]) not in ((3, 4), (4, 4)) or c2w.dim() != 2:
        raise IdealNerfError(f"c2w must be [3, 4] or [4, 4], got {list(c2w.shape)}")
    m = (C.c_float * 12)(*[float(v) for v in c2w[:3, :4].reshape(-1).tolist()])
    with _Launch(device=device) as L:
        out = torch.empty((nrows * W, RAY_FLOATS), dtype=torch.float32, device=L.device)
        check(lib.idealnerf_frame_rays(m, H, W, float(focal), -1.0 if cx is None else float(cx),
                                       -1.0 if cy is None else float(cy), float(near), float(far), row0, nrows,
                                       out.data_ptr(), L.stream))
    return out


def to8b(rgb, swap_rb=False, nonfinite_flag=None) -> torch.Tensor:
    """helper.py:154 on the device: [..., 3] fp32 -> [..., 3] uint8.  `nonfinite_flag` (int32[1] on
    the device) is OR-ed with 1 when the frame holds a NaN/Inf."""
    lib = _lib.load()
    if rgb.shape[-1] != 3:
        raise IdealNerfError(f"to8b expects [..., 3], got {tuple(rgb.shape)}")
    if nonfinite_flag is not None and (nonfinite_flag.dtype != torch.int32 or not nonfinite_flag.is_cuda
                                       or nonfinite_flag.numel() < 1):
        raise IdealNerfError("nonfinite_flag must be an int32 device tensor")
    with _Launch(rgb, nonfinite_flag) as L:
        out = torch.empty(rgb.shape, dtype=torch.uint8, device=rgb.device)
        check(lib.idealnerf_to8b(_ptr(rgb, "rgb"), rgb.numel() // 3, int(bool(swap_rb)), out.data_ptr(),
                                 nonfinite_flag.data_ptr() if nonfinite_flag is not None else None, L.stream))
    return out


def compose_to8b(rgb_head, last_weight, rgb_fg, swap_rb=False, nonfinite_flag=None, want_fg=False):
    """Tail of the head + torso clip loop in one kernel (idealnerf_compose_to8b):
    ``to8b(rgb_head * last_weight[..., None] + rgb_fg)``, [..., 3] / [...] / [..., 3] fp32 -> [..., 3] uint8, the bytes of
    `to8b` on the eager expression.  A non-finite composite value is written as 0 and sets `nonfinite_flag`.
    ``want_fg=True`` returns ``(out, to8b(rgb_fg))``: the torso-only still of the same frame."""
    lib = _lib.load()
    if rgb_head.shape[-1] != 3:
        raise IdealNerfError(f"compose_to8b expects rgb_head [..., 3], got {tuple(rgb_head.shape)}")
    _shape(rgb_fg, "rgb_fg", *rgb_head.shape)
    _shape(last_weight, "last_weight", *rgb_head.shape[:-1])
    if nonfinite_flag is not None and (nonfinite_flag.dtype != torch.int32 or not nonfinite_flag.is_cuda
                                       or nonfinite_flag.numel() < 1):
        raise IdealNerfError("nonfinite_flag must be an int32 device tensor")
    with _Launch(rgb_head, last_weight, rgb_fg, nonfinite_flag) as L:
        ptrs = (_ptr(rgb_head, "rgb_head"), _ptr(last_weight, "last_weight"), _ptr(rgb_fg, "rgb_fg"))
        out = torch.empty(rgb_head.shape, dtype=torch.uint8, device=rgb_head.device)
        fg_out = torch.empty_like(out) if want_fg else None
        check(lib.idealnerf_compose_to8b(*ptrs, rgb_head.numel() // 3, int(bool(swap_rb)), out.data_ptr(),
                                         fg_out.data_ptr() if want_fg else None,
                                         nonfinite_flag.data_ptr() if nonfinite_flag is not None else None, L.stream))
    return (out, fg_out) if want_fg else out


def coarse_depths(rays, t_vals, t_rand=None, lindisp=False) -> torch.Tensor:
    lib = _lib.load()
    _shape(rays, "rays", None, RAY_FLOATS)
    _shape(t_vals, "t_vals", None)
    n, S = rays.shape[0], t_vals.shape[0]
    _shape(t_rand, "t_rand", n, S)
    with _Launch(rays, t_vals, t_rand) as L:
        z = torch.empty((n, S), dtype=torch.float32, device=rays.device)
        check(lib.idealnerf_coarse_depths(_ptr(rays, "rays"), _ptr(t_vals, "t_vals"), _ptr(t_rand, "t_rand"),
                                          int(bool(lindisp)), n, S, z.data_ptr(), L.stream))
    return z


def composite_fwd(raw, z, rays, bc_rgb, with_fg=False, with_weights=True, sigma_noise=None,
                  white_bkgd=False) -> Dict[str, torch.Tensor]:
    lib = _lib.load()
    _shape(z, "z", None, None)
    n, S = z.shape
    _shape(raw, "raw", n, S, 4)
    _shape(rays, "rays", n, RAY_FLOATS)
    _shape(bc_rgb, "bc_rgb", n, 3)
    _shape(sigma_noise, "sigma_noise", n, S)
    dev = z.device
    with _Launch(raw, z, rays, bc_rgb, sigma_noise) as L:
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        o = dict(rgb_map=new(n, 3), disp_map=new(n), acc_map=new(n), depth_map=new(n), last_weight=new(n))
        if with_weights:
            o["weights"] = new(n, S)
        if with_fg:
            o["rgb_fg"] = new(n, 3)
        co = _lib.CompositeOut(**{k: v.data_ptr() for k, v in o.items()})
        check(lib.idealnerf_composite_fwd(_ptr(raw, "raw"), _ptr(z, "z"), _ptr(rays, "rays"), _ptr(bc_rgb, "bc_rgb"),
                                          _ptr(sigma_noise, "sigma_noise"), int(bool(white_bkgd)), n, S, C.byref(co), L.stream))
    return o


def _u_shape(u, n, n_importance=None):
    """u: [Ni] shared by all rays (the deterministic linspace) or [n, Ni] per ray."""
    if u.dim() == 2:
        _shape(u, "u", n, n_importance)
        return 1
    _shape(u, "u", n_importance)
    return 0


def sample_pdf_fwd(z, weights, u, n_importance) -> Dict[str, torch.Tensor]:
    lib = _lib.load()
    _shape(z, "z", None, None)
    n, S = z.shape
    _shape(weights, "weights", n, S)
    per_ray = _u_shape(u, n, n_importance)
    dev = z.device
    with _Launch(z, weights, u) as L:
        o = dict(z_samples=torch.empty((n, n_importance), dtype=torch.float32, device=dev),
                 inds=torch.empty((n, n_importance), dtype=torch.int64, device=dev),
                 cdf=torch.empty((n, S - 1), dtype=torch.float32, device=dev),
                 z_fine=torch.empty((n, S + n_importance), dtype=torch.float32, device=dev),
                 z_std=torch.empty((n,), dtype=torch.float32, device=dev))
        check(lib.idealnerf_sample_pdf_fwd(_ptr(z, "z"), _ptr(weights, "weights"), _ptr(u, "u"), per_ray, n, S,
                                           n_importance, o["z_samples"].data_ptr(), o["inds"].data_ptr(),
                                           o["cdf"].data_ptr(), o["z_fine"].data_ptr(), o["z_std"].data_ptr(), L.stream))
    return o


def march_fwd(raw, z, rays, bc_rgb, u, n_importance, with_fg=False, with_weights=False, sigma_noise=None,
              white_bkgd=False) -> Dict[str, torch.Tensor]:
    """Coarse raw2outputs + sample_pdf + merge as one kernel (audio_exp_nerf.py:335-349): the union of
    composite_fwd's and sample_pdf_fwd's outputs; `weights` only when asked for."""
    lib = _lib.load()
    _shape(z, "z", None, None)
    n, S = z.shape
    _shape(raw, "raw", n, S, 4)
    _shape(rays, "rays", n, RAY_FLOATS)
    _shape(bc_rgb, "bc_rgb", n, 3)
    _shape(sigma_noise, "sigma_noise", n, S)
    per_ray = _u_shape(u, n, n_importance)
    dev = z.device
    with _Launch(raw, z, rays, bc_rgb, u, sigma_noise) as L:
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        o = dict(rgb_map=new(n, 3), disp_map=new(n), acc_map=new(n), depth_map=new(n), last_weight=new(n))
        if with_weights:
            o["weights"] = new(n, S)
        if with_fg:
            o["rgb_fg"] = new(n, 3)
        co = _lib.CompositeOut(**{k: v.data_ptr() for k, v in o.items()})
        o.update(z_samples=new(n, n_importance), inds=torch.empty((n, n_importance), dtype=torch.int64, device=dev),
                 cdf=new(n, S - 1), z_fine=new(n, S + n_importance), z_std=new(n))
        check(lib.idealnerf_march_fwd(_ptr(raw, "raw"), _ptr(z, "z"), _ptr(rays, "rays"), _ptr(bc_rgb, "bc_rgb"),
                                      _ptr(sigma_noise, "sigma_noise"), int(bool(white_bkgd)), _ptr(u, "u"), per_ray, n, S,
                                      n_importance, C.byref(co), o["z_samples"].data_ptr(), o["inds"].data_ptr(),
                                      o["cdf"].data_ptr(), o["z_fine"].data_ptr(), o["z_std"].data_ptr(), L.stream))
    return o


def sample_pdf_bins_fwd(bins, weights, u) -> Dict[str, torch.Tensor]:
    """helper.sample_pdf's own argument list (helper.py:269): bins [n, nb], weights [n, nb-1] (already
    the interior weights), u [Ni] or [n, Ni] -> z_samples, inds, cdf -- pdf, cdf and inversion all by
    the kernel that Network.render_rays runs."""
    lib = _lib.load()
    _shape(bins, "bins", None, None)
    n, nb = bins.shape
    _shape(weights, "weights", n, nb - 1)
    per_ray = _u_shape(u, n)
    ni = u.shape[-1]
    dev = bins.device
    with _Launch(bins, weights, u) as L:
        o = dict(z_samples=torch.empty((n, ni), dtype=torch.float32, device=dev),
                 inds=torch.empty((n, ni), dtype=torch.int64, device=dev),
                 cdf=torch.empty((n, nb), dtype=torch.float32, device=dev))
        check(lib.idealnerf_sample_pdf_bins_fwd(_ptr(bins, "bins"), _ptr(weights, "weights"), _ptr(u, "u"), per_ray, n,
                                                nb, ni, o["z_samples"].data_ptr(), o["inds"].data_ptr(),
                                                o["cdf"].data_ptr(), L.stream))
    return o


def invert_cdf(cdf, bins, u):
    lib = _lib.load()
    _shape(cdf, "cdf", None, None)
    n, nb = cdf.shape
    _shape(bins, "bins", n, nb)
    per_ray = _u_shape(u, n)
    ni = u.shape[-1]
    with _Launch(cdf, bins, u) as L:
        zs = torch.empty((n, ni), dtype=torch.float32, device=cdf.device)
        inds = torch.empty((n, ni), dtype=torch.int64, device=cdf.device)
        check(lib.idealnerf_invert_cdf(_ptr(cdf, "cdf"), _ptr(bins, "bins"), _ptr(u, "u"), per_ray, n, nb, ni,
                                       zs.data_ptr(), inds.data_ptr(), L.stream))
    return zs, inds


def dw_gemm(delta, acts, pipe=0, with_bias=True):
    """Test aid: one 256 x 256 weight-gradient product of the training step in isolation (idealnerf_dw_gemm):
    delta [rows, >= 256], acts [rows, >= 256] (row pitch = their width) -> dW [256, 256] = delta[:, :256]^T acts[:, :256]
    and db [256] = column sums of delta.  pipe 0: six bf16 piece products (what the step runs), 1: fp32 MFMA."""
    lib = _lib.load()
    _shape(delta, "delta", None, None)
    rows = delta.shape[0]
    _shape(acts, "acts", rows, None)
    with _Launch(delta, acts) as L:
        dW = torch.empty((256, 256), dtype=torch.float32, device=delta.device)
        db = torch.empty(256, dtype=torch.float32, device=delta.device) if with_bias else None
        nbytes = lib.idealnerf_dw_gemm_workspace_bytes()
        ws = _workspace(nbytes, delta.device, L.stream)
        check(lib.idealnerf_dw_gemm(_ptr(delta, "delta"), delta.shape[1], _ptr(acts, "acts"), acts.shape[1], rows, dW.data_ptr(),
                                    None if db is None else db.data_ptr(), int(pipe), ws.data_ptr(), ws.numel(), L.stream))
    return dW, db


DW_SHAPES = ((256, 256), (256, 64), (128, 256), (128, 64), (128, 128), (64, 128))   # N x K with a kernel (csrc/dw_gemm.hip)
DW_MAX_X6_ITEMS, DW_MAX_REDUCE_ITEMS = 12, 32                                         # kMaxTnBatch, kMaxReduceItems (csrc/dw_gemm.h)


_dw_products_ws = {}


def dw_products(rows, products, pipe=0, x6_items=1):
    """Test aid: a list of weight-gradient products through one pass plan, as a training pass runs them (idealnerf_dw_products).
    Each product is a dict:
        delta [rows, ld_delta], N, acts [rows, ld_acts], K   ->  block = delta[:, :N]^T acts[:, :K]  (N x K one of DW_SHAPES)
        delta_col0 (optional, a multiple of 4): the product's delta columns start there, delta[:, delta_col0 : delta_col0 + N]
        acts2 [rows, ld_acts] (optional; pipe 0, 256 x 256): output columns 128..255 from acts2[:, :128], 0..127 from acts[:, :128]
               (the two matrices less than 2 GiB apart, or the library refuses: take them from ONE allocation, as a pass's are)
        colsum (bool): keep the column sums of delta[:, :N]
        takes: [(row0, col0, n_rows, n_cols, out, out_row0, out_col0)]: out[out_row0 + r, out_col0 + c] = block[row0 + r, col0 + c],
               out 2-D (its width is the pitch); nothing else of out is written
        colsum_takes: [(col0, n_cols, out, out0)]: out[out0 + c] = column sum col0 + c, out 1-D
    pipe 0: the 256 x 256 products as six bf16 piece products, the CUs divided among x6_items of them; 1: all on the fp32 pipe.
    Returns [(splits, chunks_per_split)], the plan each product ran with."""
    lib = _lib.load()
    E = IdealNerfError
    if not 1 <= len(products) <= _lib.DW_MAX_PRODUCTS:
        raise E(f"dw_products: {len(products)} products outside [1, {_lib.DW_MAX_PRODUCTS}]")
    if pipe not in (0, 1):
        raise E(f"dw_products: pipe {pipe}")
    if rows <= 0 or rows % 128:
        raise E(f"dw_products: rows {rows} is not a positive multiple of 128")
    if pipe == 0 and not 1 <= x6_items <= DW_MAX_X6_ITEMS:
        raise E(f"dw_products: x6_items {x6_items} outside [1, {DW_MAX_X6_ITEMS}]")
    n_x6 = n_red = 0
    tensors = []
    for i, t in enumerate(products):
        N, K = int(t["N"]), int(t["K"])
        if (N, K) not in DW_SHAPES:
            raise E(f"dw_products: product {i}: no instantiation for {N} x {K}")
        _shape(t["delta"], f"product {i}: delta", rows, None)
        _shape(t["acts"], f"product {i}: acts", rows, None)
        b_cols = K if t.get("acts2") is None else 128   # a split B: two 128-column matrices
        if t["delta"].shape[1] < N or t["acts"].shape[1] < b_cols:
            raise E(f"dw_products: product {i}: row pitch {t['delta'].shape[1]} / {t['acts'].shape[1]} < {N} / {b_cols}")
        d0 = int(t.get("delta_col0", 0))
        if d0 < 0 or d0 % 4 or d0 + N > t["delta"].shape[1]:
            raise E(f"dw_products: product {i}: delta columns {d0} .. {d0 + N} of {t['delta'].shape[1]}")
        x6 = pipe == 0 and (N, K) == (256, 256)
        if t.get("acts2") is not None:
            if not x6:
                raise E(f"dw_products: product {i}: a split B needs the 256 x 256 bf16-piece kernel")
            _shape(t["acts2"], f"product {i}: acts2", rows, t["acts"].shape[1])
        n_x6 += x6
        if n_x6 > x6_items:
            raise E(f"dw_products: more 256 x 256 products than x6_items ({x6_items})")
        takes, ctakes = t.get("takes", ()), t.get("colsum_takes", ())
        if len(takes) > _lib.DW_MAX_TAKES or len(ctakes) > _lib.DW_MAX_COLSUM_TAKES:
            raise E(f"dw_products: product {i}: {len(takes)} takes / {len(ctakes)} column-sum takes")
        if ctakes and not t.get("colsum"):
            raise E(f"dw_products: product {i} kept no column sums")
        n_red += len(takes) + len(ctakes)
        if n_red > DW_MAX_REDUCE_ITEMS:
            raise E(f"dw_products: more than {DW_MAX_REDUCE_ITEMS} takes in one pass")
        for j, (row0, col0, nr, nc, out, o_r, o_c) in enumerate(takes):
            if min(row0, col0) < 0 or min(nr, nc) < 1 or row0 + nr > N or col0 + nc > K:
                raise E(f"dw_products: product {i} take {j} leaves the {N} x {K} block")
            _shape(out, f"product {i} take {j}: out", None, None)
            if min(o_r, o_c) < 0 or o_r + nr > out.shape[0] or o_c + nc > out.shape[1]:
                raise E(f"dw_products: product {i} take {j} does not fit out {list(out.shape)}")
            tensors.append(out)
        for j, (col0, nc, out, o0) in enumerate(ctakes):
            if col0 < 0 or nc < 1 or col0 + nc > N:
                raise E(f"dw_products: product {i} column-sum take {j} leaves the {N} columns")
            _shape(out, f"product {i} column-sum take {j}: out", None)
            if o0 < 0 or o0 + nc > out.shape[0]:
                raise E(f"dw_products: product {i} column-sum take {j} does not fit out {list(out.shape)}")
            tensors.append(out)
        tensors += [t["delta"], t["acts"], t.get("acts2")]
    with _Launch(*tensors) as L:
        recs = (_lib.DwProduct * len(products))()
        for r, t in zip(recs, products):
            r.delta, r.ld_delta, r.N = _ptr(t["delta"], "delta") + 4 * int(t.get("delta_col0", 0)), t["delta"].shape[1], int(t["N"])
            r.acts, r.ld_acts, r.K = _ptr(t["acts"], "acts"), t["acts"].shape[1], int(t["K"])
            r.acts2, r.want_colsum = _ptr(t.get("acts2"), "acts2"), int(bool(t.get("colsum")))
            takes, ctakes = t.get("takes", ()), t.get("colsum_takes", ())
            r.n_takes, r.n_colsum_takes = len(takes), len(ctakes)
            for k, (row0, col0, nr, nc, out, o_r, o_c) in zip(r.takes, takes):
                k.row0, k.col0, k.rows, k.cols, k.ldo = row0, col0, nr, nc, out.shape[1]
                k.out = _ptr(out, "out") + 4 * (o_r * out.shape[1] + o_c)
            for k, (col0, nc, out, o0) in zip(r.colsum_takes, ctakes):
                k.col0, k.cols, k.out = col0, nc, _ptr(out, "out") + 4 * o0
        nbytes = lib.idealnerf_dw_products_workspace_bytes()
        # pools of its own: the tests put NaN into operand columns no gradient may depend on, and so into partial blocks -- not
        # into the scratch a later backward on this stream multiplies whole delta matrices from (_workspace)
        key = (str(L.device), int(L.stream))
        ws = _dw_products_ws.get(key)
        if ws is None:
            ws = _dw_products_ws[key] = torch.zeros(nbytes, dtype=torch.uint8, device=L.device)
        check(lib.idealnerf_dw_products(rows, int(pipe), int(x6_items), recs, len(products), ws.data_ptr(), ws.numel(), L.stream))
        return [(r.splits, r.chunks_per_split) for r in recs]


_delta_chain_ws = {}


def delta_chain(p, pipe, acts, d_rgb, dv0, max_blocks=0, dv21=None, da=None):
    """Test aid: the backward delta chain of a training pass alone (idealnerf_delta_chain): the transposed-weight pack and the
    fused chain kernel of `pipe` (0: six bf16 piece products, what a pass runs; 1: fp32 MFMA) on the caller's matrices.
        p: params_struct of the network;  acts [idealnerf_train_acts_floats(p_pad)]: only its mask tail is read
        d_rgb [p_pad, 64]: columns 0..2 = d raw rgb;  dv0 [p_pad, 256]: column 128 = d raw sigma, columns 0..127 are WRITTEN
        max_blocks: 0 = the grid of a pass (min(p_pad / 128, CUs)); k > 0: at most k workgroups
        dv21 [p_pad, 256], da [8, p_pad, 256]: optional outputs to write into (views into larger buffers are welcome)
    p_pad = dv0.shape[0], a positive multiple of 128.  Returns (dv21, da, blocks): views_linears.2's | views_linears.1's delta
    side by side, da[l] = delta of pts_linears.l, and the grid that ran."""
    lib = _lib.load()
    E = IdealNerfError
    if not isinstance(p, _lib.FaceNerfParams):
        raise E("delta_chain: p must be a params_struct")
    if pipe not in (0, 1):
        raise E(f"delta_chain: pipe {pipe}")
    if isinstance(max_blocks, bool) or not isinstance(max_blocks, int) or max_blocks < 0:
        raise E(f"delta_chain: max_blocks {max_blocks} < 0")
    _shape(dv0, "dv0", None, 256)
    p_pad = dv0.shape[0]
    if p_pad <= 0 or p_pad % 128 or p_pad > 1 << 24:
        raise E(f"delta_chain: p_pad {p_pad} is not a positive multiple of 128 up to 2^24")
    _shape(acts, "acts", lib.idealnerf_train_acts_floats(p_pad))
    _shape(d_rgb, "d_rgb", p_pad, 64)
    _shape(dv21, "dv21", p_pad, 256)
    _shape(da, "da", 8, p_pad, 256)
    for t, name in ((acts, "acts"), (d_rgb, "d_rgb"), (dv0, "dv0"), (dv21, "dv21"), (da, "da")):
        if t is not None and t.dtype != torch.float32:
            raise E(f"{name} must be {torch.float32} (got {t.dtype})")
    with _Launch(acts, d_rgb, dv0, dv21, da) as L:
        ptrs = [_ptr(t, name) for t, name in ((acts, "acts"), (d_rgb, "d_rgb"), (dv0, "dv0"))]   # raises for CPU tensors
        if dv21 is None:
            dv21 = torch.empty((p_pad, 256), dtype=torch.float32, device=L.device)
        if da is None:
            da = torch.empty((8, p_pad, 256), dtype=torch.float32, device=L.device)
        ptrs += [_ptr(dv21, "dv21"), _ptr(da, "da")]
        if any(q % 16 for q in ptrs):
            raise E("delta_chain: operands are not 16-byte aligned")
        # a stream buffer of its own: the tests put NaN into weight columns the chain must not read
        key = str(L.device)   # (one per device: calls on other streams of it are the caller's to order)
        ws = _delta_chain_ws.get(key)
        if ws is None:
            ws = _delta_chain_ws[key] = torch.zeros(lib.idealnerf_delta_chain_workspace_bytes(), dtype=torch.uint8, device=L.device)
        blocks = C.c_int(0)
        check(lib.idealnerf_delta_chain(C.byref(p), int(pipe), ptrs[0], p_pad, ptrs[1], ptrs[2], ptrs[3], ptrs[4], int(max_blocks),
                                        C.byref(blocks), ws.data_ptr(), ws.numel(), L.stream))
    return dv21, da, blocks.value


def composite_bwd(raw, z, rays, bc, g_rgb=None, g_fg=None, g_lw=None, g_acc=None, d_rgb=None, d_sig=None, sig_col=0, d_norm=None,
                  norm_col=0):
    """Test aid: the compositing backward of a training pass alone (idealnerf_composite_bwd), through the dispatch a pass runs.
        raw [n, S, 4], z [n, S], rays [n, 11], bc [n, 3];  g_* = dL/d (rgb_map [n, 3], rgb_fg [n, 3], last_weight [n], acc_map [n]),
        each may be None
        d_rgb [rows >= n S, ld_rgb >= 3]: columns 0..2 of row ray * S + s are WRITTEN with d raw rgb
        d_sig [rows >= n S, ld_sig]: column sig_col of that row is WRITTEN with d raw sigma (d_sig may be d_rgb itself)
        d_norm [n, ld_norm]: optional; column norm_col of row r is WRITTEN with dL / d |rays_d| (given: the kernels of a pass with
        a ray gradient; None: the others)
    With neither d_rgb nor d_sig, both go into one new [n, S, 4] tensor (pitches 4 and 4).  A pass itself runs d_rgb [p_pad, 64],
    d_sig [p_pad, 256] at sig_col 128 and d_norm = d_rays [n, 11] at norm_col 6.  Returns (d_rgb, d_sig, d_norm) as given, or the
    new tensor twice."""
    lib = _lib.load()
    E = IdealNerfError
    if z is None:
        raise E("composite_bwd: z is None")
    _shape(z, "z", None, None)
    n, S = z.shape
    for t, name, shape in ((raw, "raw", (n, S, 4)), (rays, "rays", (n, RAY_FLOATS)), (bc, "bc_rgb", (n, 3)), (g_rgb, "g_rgb_map", (n, 3)),
                           (g_fg, "g_rgb_fg", (n, 3)), (g_lw, "g_last_weight", (n,)), (g_acc, "g_acc", (n,)), (d_rgb, "d_rgb", (None, None)),
                           (d_sig, "d_sig", (None, None)), (d_norm, "d_norm", (n, None))):
        if t is None and name in ("raw", "rays", "bc_rgb"):
            raise E(f"composite_bwd: {name} is None")
        _shape(t, name, *shape)
    if not 2 <= S <= 512:
        raise E(f"composite_bwd: n_samples {S} outside [2, 512]")
    if (d_rgb is None) != (d_sig is None):
        raise E("composite_bwd: d_rgb and d_sig come together")
    for t, name, col in ((d_sig, "sig_col", sig_col), (d_norm, "norm_col", norm_col)):
        if isinstance(col, bool) or not isinstance(col, int) or col < 0 or (t is None and col != 0) or (t is not None and col >= t.shape[1]):
            raise E(f"composite_bwd: {name} {col} is not a column of its matrix")
    if d_rgb is not None and (d_rgb.shape[0] < n * S or d_sig.shape[0] < n * S or d_rgb.shape[1] < 3):
        raise E(f"composite_bwd: d_rgb {list(d_rgb.shape)} / d_sig {list(d_sig.shape)} hold fewer than {n * S} rows or d_rgb fewer than 3 columns")
    with _Launch(raw, z, rays, bc, g_rgb, g_fg, g_lw, g_acc, d_rgb, d_sig, d_norm) as L:
        ptrs = [_ptr(t, name) for t, name in ((raw, "raw"), (z, "z"), (rays, "rays"), (bc, "bc_rgb"))]   # raises for CPU tensors
        grad_ptrs = [_ptr(t, name) for t, name in ((g_rgb, "g_rgb_map"), (g_fg, "g_rgb_fg"), (g_lw, "g_last_weight"), (g_acc, "g_acc"))]
        if d_rgb is None:
            d_rgb = d_sig = torch.empty((n, S, 4), dtype=torch.float32, device=L.device)
            out = (d_rgb.data_ptr(), 4, d_rgb.data_ptr() + 12, 4)
        else:
            out = (_ptr(d_rgb, "d_rgb"), d_rgb.shape[1], _ptr(d_sig, "d_sig") + 4 * sig_col, d_sig.shape[1])
        norm = (None, 0) if d_norm is None else (_ptr(d_norm, "d_norm") + 4 * norm_col, d_norm.shape[1])
        check(lib.idealnerf_composite_bwd(*ptrs, n, S, *grad_ptrs, *out, *norm, L.stream))
    return d_rgb, d_sig, d_norm


def _all_f32(*named):
    for t, name in named:
        if t is not None and t.dtype != torch.float32:
            raise IdealNerfError(f"{name} must be {torch.float32} (got {t.dtype})")


def input_grad(p, dA0, dA5, dV0, n, d_x=None, max_blocks=0):
    """Test aid: the input-row gradient of a backward alone (idealnerf_input_grad: dx_kernel through the launch of a pass).
        p: params_struct of the network -- only pts_linears.0 / .5's encoding columns and views_linears.0's direction columns are read
        dA0, dA5, dV0 [p_pad, 256]: the deltas of pts_linears.0, pts_linears.5 and views_linears.0 (dV0: columns 0..127 are read)
        n: the rows that get a gradient, 1 <= n <= p_pad;  d_x [n, pts_ch + views_ch]: optional output to write into
        max_blocks: 0 = the grid of a pass (min(ceil(p_pad / 512), CUs)); k > 0: at most k workgroups
    p_pad = dA0.shape[0], a positive multiple of 128.  Returns (d_x, blocks): the gradient and the grid that ran."""
    lib = _lib.load()
    E = IdealNerfError
    if not isinstance(p, _lib.FaceNerfParams):
        raise E("input_grad: p must be a params_struct")
    if isinstance(max_blocks, bool) or not isinstance(max_blocks, int) or max_blocks < 0:
        raise E(f"input_grad: max_blocks {max_blocks} < 0")
    _shape(dA0, "dA0", None, 256)
    p_pad = dA0.shape[0]
    if p_pad <= 0 or p_pad % 128 or p_pad > 1 << 24:
        raise E(f"input_grad: p_pad {p_pad} is not a positive multiple of 128 up to 2^24")
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= p_pad:
        raise E(f"input_grad: n {n} outside [1, p_pad = {p_pad}]")
    _shape(dA5, "dA5", p_pad, 256)
    _shape(dV0, "dV0", p_pad, 256)
    _shape(d_x, "d_x", n, sum(widths(p)))
    _all_f32((dA0, "dA0"), (dA5, "dA5"), (dV0, "dV0"), (d_x, "d_x"))
    with _Launch(dA0, dA5, dV0, d_x) as L:
        ptrs = [_ptr(t, name) for t, name in ((dA0, "dA0"), (dA5, "dA5"), (dV0, "dV0"))]   # raises for CPU tensors
        if any(q % 16 for q in ptrs):
            raise E("input_grad: the delta matrices are not 16-byte aligned")
        if d_x is None:
            d_x = torch.empty((n, sum(widths(p))), dtype=torch.float32, device=L.device)
        blocks = C.c_int(0)
        check(lib.idealnerf_input_grad(C.byref(p), *ptrs, n, p_pad, _ptr(d_x, "d_x"), int(max_blocks), C.byref(blocks), L.stream))
    return d_x, blocks.value


def ray_grad(d_x, pts_ch, views_ch, rays, z, d_rays):
    """Test aid: the encoding backward and the per-ray reduction of a pass alone (idealnerf_ray_grad).
        d_x [n * S, pts_ch + views_ch]: the input-row gradient of the pass's points;  rays [n, 11], z [n, S]
        d_rays [n, 11]: column 6 holds dL / d |rays_d| on entry; columns 0:3 d rays_o, 3:6 d rays_d, 8:11 d viewdirs are WRITTEN,
        6:8 with zeros
    S in [2, 512].  Returns d_rays."""
    lib = _lib.load()
    E = IdealNerfError
    for ch, name, limit in ((pts_ch, "pts_ch", PTS_CH), (views_ch, "views_ch", VIEWS_CH)):
        if isinstance(ch, bool) or not isinstance(ch, int) or ch < 3 or ch > limit or ch % 6 != 3:
            raise E(f"ray_grad: {name} {ch} is not 3 + 6 L up to {limit}")
    if z is None or d_rays is None:
        raise E("ray_grad: z / d_rays is None")
    _shape(z, "z", None, None)
    n, S = z.shape
    if not 2 <= S <= 512:
        raise E(f"ray_grad: n_samples {S} outside [2, 512]")
    for t, name, shape in ((d_x, "d_x", (n * S, pts_ch + views_ch)), (rays, "rays", (n, RAY_FLOATS)), (d_rays, "d_rays", (n, RAY_FLOATS))):
        if t is None:
            raise E(f"ray_grad: {name} is None")
        _shape(t, name, *shape)
    _all_f32((d_x, "d_x"), (rays, "rays"), (z, "z"), (d_rays, "d_rays"))
    with _Launch(d_x, rays, z, d_rays) as L:
        ptrs = [_ptr(t, name) for t, name in ((d_x, "d_x"), (rays, "rays"), (z, "z"), (d_rays, "d_rays"))]
        check(lib.idealnerf_ray_grad(ptrs[0], pts_ch, views_ch, ptrs[1], ptrs[2], n, S, ptrs[3], L.stream))
    return d_rays


def fold_bwd(p, aud, expr, latent, db0, db5, dbv, gW0=None, gW5=None, gWv0=None, d_aud=None, d_expr=None, d_latent=None):
    """Test aid: the conditioning fold's backward alone (idealnerf_fold_bwd).
        p: params_struct of the network -- only the conditioning columns of pts_linears.0 / .5 and the expression columns of
        views_linears.0 are read;  aud / expr / latent: the vectors the forward was folded with (None where the width is 0)
        db0, db5 [256], dbv [128]: the bias gradients of pts_linears.0 / .5 and views_linears.0
        gW0 [256, pts_ch + C], gW5 [256, pts_ch + C + 256], gWv0 [128, 256 + views_ch + dim_expr]: the three layers' gradient
        tensors, whose conditioning columns are WRITTEN.  All three None: the launch of a frozen network (d cond alone);
        dbv is then read only with d_expr
        d_aud / d_expr / d_latent: ACCUMULATED, each may be None."""
    lib = _lib.load()
    E = IdealNerfError
    if not isinstance(p, _lib.FaceNerfParams):
        raise E("fold_bwd: p must be a params_struct")
    given = sum(t is not None for t in (gW0, gW5, gWv0))
    if given not in (0, 3):
        raise E(f"fold_bwd: {given} of the three gradient tensors (all three, or none)")
    pc, vc = widths(p)
    Cc = p.dim_aud + p.dim_expr + p.dim_latent
    for t, name, dim in ((aud, "aud", p.dim_aud), (expr, "expr", p.dim_expr), (latent, "latent", p.dim_latent)):
        if (t is None) != (dim == 0):
            raise E(f"fold_bwd: {name} is {'None' if t is None else 'given'} but the network's width is {dim}")
        _shape(t, name, dim)
    for t, name, dim in ((d_aud, "d_aud", p.dim_aud), (d_expr, "d_expr", p.dim_expr), (d_latent, "d_latent", p.dim_latent)):
        if t is not None and dim == 0:
            raise E(f"fold_bwd: {name} for a width of 0")
        _shape(t, name, dim)
    if db0 is None or db5 is None or (dbv is None and p.dim_expr > 0 and (given or d_expr is not None)):
        raise E("fold_bwd: db0 / db5 / dbv is None")
    for t, name, shape in ((db0, "db0", (W_HID,)), (db5, "db5", (W_HID,)), (dbv, "dbv", (W_HID // 2,)), (gW0, "gW0", (W_HID, pc + Cc)),
                           (gW5, "gW5", (W_HID, pc + Cc + W_HID)), (gWv0, "gWv0", (W_HID // 2, W_HID + vc + p.dim_expr))):
        _shape(t, name, *shape)
    named = ((aud, "aud"), (expr, "expr"), (latent, "latent"), (db0, "db0"), (db5, "db5"), (dbv, "dbv"), (gW0, "gW0"), (gW5, "gW5"),
             (gWv0, "gWv0"), (d_aud, "d_aud"), (d_expr, "d_expr"), (d_latent, "d_latent"))
    _all_f32(*named)
    with _Launch(*(t for t, _ in named)) as L:
        check(lib.idealnerf_fold_bwd(C.byref(p), *(_ptr(t, name) for t, name in named), L.stream))


_cond_colsums_ws = {}


def cond_colsums(dA0, dA5, dV0, P, db=None, dbv=None):
    """Test aid: the column sums a frozen network's backward feeds the fold with (idealnerf_cond_colsums).
        dA0, dA5 [p_pad, 256] -> db [2, 256]: their column sums over all p_pad rows (both None: left out)
        dV0 [p_pad, 256] -> dbv [128]: the sums of its columns 0..127 over the first P rows (None: left out)
    p_pad a positive multiple of 128, 1 <= P <= p_pad.  Returns (db, dbv); an output is None where its matrices are."""
    lib = _lib.load()
    E = IdealNerfError
    if (dA0 is None) != (dA5 is None):
        raise E("cond_colsums: dA0 and dA5 come together")
    first = dA0 if dA0 is not None else dV0
    if first is None:
        raise E("cond_colsums: no matrix")
    _shape(first, "dA0" if dA0 is not None else "dV0", None, 256)
    p_pad = first.shape[0]
    if p_pad <= 0 or p_pad % 128 or p_pad > 1 << 24:
        raise E(f"cond_colsums: p_pad {p_pad} is not a positive multiple of 128 up to 2^24")
    if isinstance(P, bool) or not isinstance(P, int) or not 1 <= P <= p_pad:
        raise E(f"cond_colsums: P {P} outside [1, p_pad = {p_pad}]")
    if (db is not None and dA0 is None) or (dbv is not None and dV0 is None):
        raise E("cond_colsums: an output without its matrices")
    for t, name, shape in ((dA5, "dA5", (p_pad, 256)), (dV0, "dV0", (p_pad, 256)), (db, "db", (2, 256)), (dbv, "dbv", (128,))):
        _shape(t, name, *shape)
    named = ((dA0, "dA0"), (dA5, "dA5"), (dV0, "dV0"), (db, "db"), (dbv, "dbv"))
    _all_f32(*named)
    with _Launch(*(t for t, _ in named)) as L:
        ptrs = [_ptr(t, name) for t, name in named[:3]]   # raises for CPU tensors
        if db is None and dA0 is not None:
            db = torch.empty((2, 256), dtype=torch.float32, device=L.device)
        if dbv is None and dV0 is not None:
            dbv = torch.empty((128,), dtype=torch.float32, device=L.device)
        key = (str(L.device), int(L.stream))
        ws = _cond_colsums_ws.get(key)
        if ws is None:
            ws = _cond_colsums_ws[key] = torch.zeros(lib.idealnerf_cond_colsums_workspace_bytes(), dtype=torch.uint8, device=L.device)
        check(lib.idealnerf_cond_colsums(*ptrs, P, p_pad, _ptr(db, "db"), _ptr(dbv, "dbv"), ws.data_ptr(), ws.numel(), L.stream))
    return db, dbv


AUDIO_NET_MAX_BWD_WINDOWS = 8


def _audio_params_struct(params, dim_aud):
    """params: encoder_conv.{0,2,4,6}.{weight,bias} then encoder_fc1.{0,2}.{weight,bias} (12 tensors, nn layout)."""
    shapes = [(32, 29, 3), (32,), (32, 32, 3), (32,), (64, 32, 3), (64,), (64, 64, 3), (64,), (64, 64), (64,), (dim_aud, 64), (dim_aud,)]
    if len(params) != 12:
        raise IdealNerfError(f"AudioNet has 12 parameter tensors, got {len(params)}")
    for i, (t, shp) in enumerate(zip(params, shapes)):
        _shape(t, f"AudioNet parameter {i}", *shp)
    p = _lib.AudioNetParams()
    for i in range(4):
        p.conv_w[i], p.conv_b[i] = _ptr(params[2 * i], "conv weight"), _ptr(params[2 * i + 1], "conv bias")
    for i in range(2):
        p.fc_w[i], p.fc_b[i] = _ptr(params[8 + 2 * i], "fc weight"), _ptr(params[9 + 2 * i], "fc bias")
    p.dim_aud = int(dim_aud)
    return p


def audio_net_fwd(params, windows, dim_aud, save=False):
    """AudioNet.forward (models/audio_net.py:43-69) on [n, 16, 29] windows as one kernel -> ([n, dim_aud], saved or None)."""
    lib = _lib.load()
    _shape(windows, "windows", None, 16, 29)
    n = windows.shape[0]
    with _Launch(windows, *params) as L:
        p = _audio_params_struct(params, dim_aud)
        out = torch.empty((n, dim_aud), dtype=torch.float32, device=windows.device)
        saved = torch.empty(lib.idealnerf_audio_net_saved_floats(n), dtype=torch.float32, device=windows.device) if save else None
        check(lib.idealnerf_audio_net_fwd(C.byref(p), _ptr(windows, "windows"), n, out.data_ptr(),
                                          None if saved is None else saved.data_ptr(), L.stream))
    return out, saved


def audio_net_bwd(params, windows, saved, d_out, dim_aud):
    """-> the 12 parameter gradients (summed over the n <= 8 windows), in the order of `params`."""
    lib = _lib.load()
    n = windows.shape[0]
    _shape(windows, "windows", None, 16, 29)
    _shape(d_out, "d_out", n, dim_aud)
    _shape(saved, "saved", lib.idealnerf_audio_net_saved_floats(n))
    with _Launch(windows, saved, d_out, *params) as L:
        p = _audio_params_struct(params, dim_aud)
        grads = [torch.empty_like(t) for t in params]
        g = _lib.AudioNetGrads()
        for i in range(4):
            g.conv_w[i], g.conv_b[i] = grads[2 * i].data_ptr(), grads[2 * i + 1].data_ptr()
        for i in range(2):
            g.fc_w[i], g.fc_b[i] = grads[8 + 2 * i].data_ptr(), grads[9 + 2 * i].data_ptr()
        check(lib.idealnerf_audio_net_bwd(C.byref(p), C.byref(g), _ptr(windows, "windows"), _ptr(saved, "saved"), _ptr(d_out, "d_out"),
                                          n, L.stream))
    return grads


SCORE_GROUPS = ("frame", "rect", "outside", "mouth", "torso")    # rows of a score table: the whole frame, then dataset.REGION_NAMES
SCORE_COLUMNS = ("n_pixels", "sse", "n_windows", "ssim_sum")
SCORE_TILE = _lib.SCORE_TILE                                      # edge of the pixel tile one workgroup scores


def frame_scores_workspace_doubles(H, W) -> int:
    return _lib.load().idealnerf_frame_scores_workspace_bytes(int(H), int(W)) // 8


def frame_scores(pred, truth_u8, regions=None, out=None, workspace=None) -> torch.Tensor:
    """Squared error and SSIM of a rendered frame against its ground truth (idealnerf_frame_scores): pred [H, W, 3] fp32,
    truth_u8 [H, W, 3] uint8, regions [H, W] uint8 (``dataset.region_byte_map``) or None -> float64 [5, 4] on the device: rows
    SCORE_GROUPS, columns SCORE_COLUMNS (``summarise_scores`` turns them into mse / psnr / ssim).  fp64 sums, no atomics: the
    same inputs give the same 160 bytes.  `out` (float64 [5, 4], e.g. a row of a caller's table) and `workspace` (float64
    [>= frame_scores_workspace_doubles(H, W)]): the caller's buffers, for a call that allocates nothing; nothing is read back."""
    lib = _lib.load()
    if pred.dim() != 3 or pred.shape[-1] != 3:
        raise IdealNerfError(f"pred must be [H, W, 3], got {list(pred.shape)}")
    H, W = int(pred.shape[0]), int(pred.shape[1])
    _shape(truth_u8, "truth_u8", H, W, 3)
    _shape(regions, "regions", H, W)
    _shape(out, "out", 5, 4)
    with _Launch(pred, truth_u8, regions, out, workspace) as L:
        ptrs = (_ptr(pred, "pred"), _ptr(truth_u8, "truth_u8", torch.uint8), _ptr(regions, "regions", torch.uint8))
        need = lib.idealnerf_frame_scores_workspace_bytes(H, W)
        if out is None:
            out = torch.empty((5, 4), dtype=torch.float64, device=pred.device)
        if workspace is None:
            workspace = torch.empty(need // 8, dtype=torch.float64, device=pred.device)
        if workspace.numel() * 8 < need:
            raise IdealNerfError(f"workspace must hold {need // 8} float64 for a {H} x {W} frame, got {workspace.numel()}")
        check(lib.idealnerf_frame_scores(*ptrs, H, W, _ptr(out, "out", torch.float64), _ptr(workspace, "workspace", torch.float64),
                                         workspace.numel() * 8, L.stream))
    return out


def summarise_scores(table):
    """Score table(s) [..., 5, 4] (tensor or array; a device tensor is copied to the host here) -> dict of float64 arrays [..., 5]:
    ``mse = sse / (3 n_pixels)``, ``psnr = -10 log10(mse)`` (helper.mse2psnr), ``ssim = ssim_sum / (3 n_windows)``.  A group
    without pixels (windows) has mse and psnr (ssim) nan; mse == 0 gives psnr = inf."""
    import numpy as np
    t = np.asarray(table.detach().cpu() if isinstance(table, torch.Tensor) else table, dtype=np.float64)
    if t.ndim < 2 or t.shape[-2:] != (5, 4):
        raise ValueError(f"a score table is [..., 5, 4], got {list(t.shape)}")
    n_pix, sse, n_win, ssim_sum = (t[..., c] for c in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = np.where(n_pix > 0, sse / (3.0 * n_pix), np.nan)
        psnr = -10.0 * np.log10(mse)
        ssim = np.where(n_win > 0, ssim_sum / (3.0 * n_win), np.nan)
    return dict(mse=mse, psnr=psnr, ssim=ssim)


_workspaces: Dict[tuple, torch.Tensor] = {}


def _workspace(nbytes: int, device, stream) -> torch.Tensor:
    """Scratch of one (device, stream): calls on one stream are ordered, so they can share it."""
    key = (str(device), int(stream))
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        # zeros, once per allocation: the backward multiplies whole 256-column delta matrices of which it writes 129 columns
        # (csrc/train.hip, bwd_tail: views_linears.0 + alpha_linear, a product of csrc/dw_gemm.hip); what the other columns hold is never read back, but it must be
        # DEFINED data (zeros now, values our own kernels wrote later), not whatever the allocator hands out
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


_FUSED_NAMES = {"0": 0, "1": 1, "2": 2, "split": 2}


def _fused_code(fused, where) -> int:
    """False / 0 -> 0 (kernel sequence), True / 1 -> 1 (one kernel), "split" / 2 -> 2 (two kernels); anything else is named."""
    if isinstance(fused, str) and fused.strip().lower() in _FUSED_NAMES:
        return _FUSED_NAMES[fused.strip().lower()]
    if isinstance(fused, (bool, int)) and int(fused) in (0, 1, 2):
        return int(fused)
    raise IdealNerfError(f"{where} must be one of 0 / False (kernel sequence), 1 / True (one fused kernel), 2 / 'split' "
                         f"(two fused kernels); got {fused!r}")


# read once: the arrangement of the fp32 64 + 128 path where `fused` is not given
FUSED_MARCH_DEFAULT = _fused_code(os.environ.get("IDN_FUSED_MARCH", "0") or "0", "IDN_FUSED_MARCH")


# read once: whether the fp32 kernel sequence launches its colour-gated network kernels where `colour_gate` is not given
COLOUR_GATE_DEFAULT = (os.environ.get("IDN_COLOUR_GATE", "1") or "1").strip() != "0"


def make_frame(c2w, H, W, focal, near, far, row0=0, nrows=None, cx=None, cy=None):
    """The camera of a full-frame render (idn_frame): rays of rows [row0, row0 + nrows) are derived on the device."""
    nrows = H - row0 if nrows is None else nrows
    if not (0 <= row0 and 0 <= nrows and row0 + nrows <= H and W > 0):
        raise IdealNerfError(f"rows [{row0}, {row0 + nrows}) are outside a {H}x{W} frame")
    if c2w.dim() != 2 or tuple(c2w.shape[-2:]) not in ((3, 4), (4, 4)):
        raise IdealNerfError(f"c2w must be [3, 4] or [4, 4], got {list(c2w.shape)}")
    f = _lib.Frame()
    f.c2w = (C.c_float * 12)(*[float(v) for v in c2w[:3, :4].reshape(-1).tolist()])
    f.H, f.W, f.focal = int(H), int(W), float(focal)
    f.cx, f.cy = -1.0 if cx is None else float(cx), -1.0 if cy is None else float(cy)
    f.near_, f.far_, f.row0, f.nrows = float(near), float(far), int(row0), int(nrows)
    f.rays_out = None
    return f


def philox_uniform(seed, which, row0, n_rows, n_cols, device) -> torch.Tensor:
    """Rows [row0, row0 + n_rows) of the table the in-kernel draws come from (`draws=` of render_rays_fwd) as a tensor:
    which = 0 the stratified offsets t_rand, 1 the importance draws u (include/idealnerf.h: idealnerf_philox_uniform)."""
    lib = _lib.load()
    with _Launch(device=device) as L:   # (raises for a CPU device: there is no CPU path)
        out = torch.empty((int(n_rows), int(n_cols)), dtype=torch.float32, device=L.device)
        check(lib.idealnerf_philox_uniform(int(seed) & (2 ** 64 - 1), int(which), int(row0), int(n_rows), int(n_cols), _ptr(out, "out"), L.stream))
    return out


def sample_counts(n_rand, mouth_rays, torso_rays, sample_rate):
    """(rect, outside, mouth, torso) picks of one batch, computed as upstream does (audio_exp_nerf.py:176-178)."""
    sample_num = int(n_rand) - int(mouth_rays) - int(torso_rays)
    rect_num = int(sample_num * sample_rate)
    return rect_num, sample_num - rect_num, int(mouth_rays), int(torso_rays)


def camera_floats(c2w):
    """[3, 4] / [4, 4] camera matrix (tensor, array or nested list) -> the 12 host floats the ray kernels take as arguments."""
    if isinstance(c2w, C.Array):
        return c2w
    m = torch.as_tensor(c2w, dtype=torch.float32).detach().cpu()
    if m.dim() != 2 or tuple(m.shape) not in ((3, 4), (4, 4)):
        raise IdealNerfError(f"c2w must be [3, 4] or [4, 4], got {list(m.shape)}")
    return (C.c_float * 12)(*[float(v) for v in m[:3, :4].reshape(-1).tolist()])


def sample_pixels(region_map, counts, seed, draw, out=None, workspace=None) -> torch.Tensor:
    """The region-weighted pixel draw of the training loader on the device (idealnerf_sample_pixels): region_map uint8 [H, W]
    (bit 0 rect minus mouth, 1 outside rect, 2 mouth, 3 torso), counts = (rect, outside, mouth, torso) -> int64 [sum(counts)] flat
    pixel indices in that order; a function of (region_map, counts, seed, draw) alone.  `out` / `workspace` (int32 [>= 4], receives
    the region populations): the caller's buffers, for a call that allocates nothing."""
    lib = _lib.load()
    if region_map.dim() != 2:
        raise IdealNerfError(f"region_map must be [H, W], got {list(region_map.shape)}")
    counts = [int(c) for c in counts]
    if len(counts) != 4 or min(counts) < 0:
        raise IdealNerfError(f"counts must be four non-negative numbers (rect, outside, mouth, torso), got {counts}")
    if max(counts) > _lib.SAMPLE_MAX_REGION:
        raise IdealNerfError(f"a region count of {max(counts)} exceeds the sampler's {_lib.SAMPLE_MAX_REGION} picks per region")
    H, W = region_map.shape
    n = sum(counts)
    _shape(out, "out", n)
    with _Launch(region_map, out, workspace) as L:
        mp = _ptr(region_map, "region_map", torch.uint8)
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=region_map.device)
        if workspace is None:
            workspace = torch.empty(4, dtype=torch.int32, device=region_map.device)
        if workspace.numel() < 4:
            raise IdealNerfError("workspace must hold four int32")
        check(lib.idealnerf_sample_pixels(mp, H, W, *counts, int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1),
                                          _ptr(workspace, "workspace", torch.int32), workspace.numel() * 4,
                                          _ptr(out, "out", torch.int64), L.stream))
    return out


_byte_tables: Dict[str, tuple] = {}


def byte_tables(device):
    """(target_table, background_table), fp32 [256] on `device`: what a byte becomes in GetData -- the target as
    `uint8 tensor -> device -> float() / 255.0`, evaluated by that very expression on that device; the background as numpy's
    `uint8 / 255.0` in float64, rounded to fp32 (the cast Network.forward applies)."""
    import numpy as np
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = str(device)
    t = _byte_tables.get(key)
    if t is None:
        target = torch.arange(256, dtype=torch.int32).to(torch.uint8).to(device).float() / 255.0
        background = torch.tensor(np.arange(256, dtype=np.uint8) / 255.0).to(device).to(torch.float32)
        t = _byte_tables[key] = (target.contiguous(), background.contiguous())
    return t


def gather_rays(sel, c2w, H, W, focal, image, background, cx=None, cy=None, c2w_torso=None):
    """Rays and colours of the pixels `sel` (int64 [n], flat row-major) of one training frame (idealnerf_gather_rays) ->
    (batch_rays [2, n, 3], target_s [n, 3], bc_rgb [n, 3]) fp32.  image / background: uint8 [H, W, 3] on the device; c2w: the
    camera on the HOST (it travels as kernel arguments), or `camera_floats` of it.  No [H W, 11] ray tensor exists.
    c2w_torso: `gather_ray_pairs`."""
    lib = _lib.load()
    _shape(sel, "sel", None)
    _shape(image, "image", H, W, 3)
    _shape(background, "background", H, W, 3)
    n = sel.shape[0]
    cams = [camera_floats(c2w)] + ([] if c2w_torso is None else [camera_floats(c2w_torso)])
    with _Launch(sel, image, background) as L:
        tt, tb = byte_tables(L.device)
        rays = [torch.empty((2, n, 3), dtype=torch.float32, device=sel.device) for _ in cams]
        target_s = torch.empty((n, 3), dtype=torch.float32, device=sel.device)
        bc_rgb = torch.empty((n, 3), dtype=torch.float32, device=sel.device)
        entry = lib.idealnerf_gather_rays if c2w_torso is None else lib.idealnerf_gather_ray_pairs
        check(entry(_ptr(sel, "sel", torch.int64), n, *cams, int(H), int(W), float(focal),
                    -1.0 if cx is None else float(cx), -1.0 if cy is None else float(cy),
                    _ptr(image, "image", torch.uint8), _ptr(background, "background", torch.uint8),
                    _ptr(tt, "target table"), _ptr(tb, "background table"),
                    *[r.data_ptr() for r in rays], target_s.data_ptr(), bc_rgb.data_ptr(), L.stream))
    return (*rays, target_s, bc_rgb)


def gather_ray_pairs(sel, c2w, c2w_torso, H, W, focal, image, background, cx=None, cy=None):
    """`gather_rays` with the torso stage's second camera for the same pixels, in the same launch (idealnerf_gather_ray_pairs)
    -> (batch_rays, batch_rays_torso, target_s, bc_rgb); batch_rays_torso [2, n, 3] is what `gather_rays` returns for c2w_torso,
    bit for bit."""
    return gather_rays(sel, c2w, H, W, focal, image, background, cx, cy, c2w_torso=c2w_torso)


PATCH_MAX, PATCH_MIN_P, PATCH_MAX_P = _lib.PATCH_MAX, _lib.PATCH_MIN_P, _lib.PATCH_MAX_P


def _check_patches(n_patches, p):
    n_patches, p = int(n_patches), int(p)
    if not 1 <= n_patches <= PATCH_MAX:
        raise IdealNerfError(f"n_patches {n_patches} is outside 1..{PATCH_MAX}")
    if not PATCH_MIN_P <= p <= PATCH_MAX_P:
        raise IdealNerfError(f"patch edge {p} is outside {PATCH_MIN_P}..{PATCH_MAX_P}")
    return n_patches, p


def patch_set(origins, p):
    """[(oy, ox), ...] top-left corners (host numbers) and the edge p -> the idn_patch_set the kernel takes as arguments."""
    origins = [(int(oy), int(ox)) for oy, ox in origins]
    k, p = _check_patches(len(origins), p)
    s = _lib.PatchSet()
    s.n_patches, s.p = k, p
    for i, (oy, ox) in enumerate(origins):
        s.oy[i], s.ox[i] = oy, ox
    return s


def patch_pixels(origins, p, W, out=None, device=None) -> torch.Tensor:
    """The flat row-major pixel indices of k p x p patches (idealnerf_patch_pixels): origins [(oy, ox), ...] on the HOST (they
    travel as kernel arguments) or a ``patch_set`` of them -> int64 [k p p], patch by patch, row-major inside a patch.  `out`:
    the caller's buffer (e.g. the tail of a loader's selection), for a call that allocates nothing; without it the result is
    allocated on `device` (default: the current GPU).  k outside 1..16, p outside 11..48 or a patch that leaves the W columns
    raise IdealNerfError."""
    lib = _lib.load()
    s = origins if isinstance(origins, _lib.PatchSet) else patch_set(origins, p)
    k, p = _check_patches(s.n_patches, s.p)
    _shape(out, "out", k * p * p)
    with _Launch(out, device=None if out is not None else (device or "cuda")) as L:
        if out is None:
            out = torch.empty(k * p * p, dtype=torch.int64, device=L.device)
        check(lib.idealnerf_patch_pixels(C.byref(s), int(W), _ptr(out, "out", torch.int64), L.stream))
    return out


def _patch_rows(t, name, n_patches, p):
    if t.numel() != n_patches * p * p * 3 or t.shape[-1] != 3:
        raise IdealNerfError(f"{name} must hold [{n_patches}, {p}, {p}, 3] values in rows of 3, got {list(t.shape)}")


def ssim_patch_fwd(pred, truth, n_patches, p, out=None) -> torch.Tensor:
    """The patch SSIM loss (idealnerf_ssim_patch_fwd): pred, truth fp32 [n_patches, p, p, 3] (or the [n_patches p p, 3] rows a
    render and a gather return for ``patch_pixels``) -> float64 [n_patches + 1] on the device: each patch's mean SSIM index over
    its 3 (p - 10)^2 windows, then the loss 1 - mean.  ``frame_scores``' index; fp64 sums in a fixed order, no atomics."""
    lib = _lib.load()
    n_patches, p = _check_patches(n_patches, p)
    _patch_rows(pred, "pred", n_patches, p)
    _patch_rows(truth, "truth", n_patches, p)
    _shape(out, "out", n_patches + 1)
    with _Launch(pred, truth, out) as L:
        ptrs = (_ptr(pred, "pred"), _ptr(truth, "truth"))
        if out is None:
            out = torch.empty(n_patches + 1, dtype=torch.float64, device=pred.device)
        check(lib.idealnerf_ssim_patch_fwd(*ptrs, n_patches, p, _ptr(out, "out", torch.float64), L.stream))
    return out


def ssim_patch_bwd(pred, truth, n_patches, p, g=1.0, out=None) -> torch.Tensor:
    """g * d loss / d pred of ``ssim_patch_fwd``'s loss (idealnerf_ssim_patch_bwd) -> fp32, pred's shape, each element rounded
    once from fp64; g is a host number.  truth gets no gradient."""
    lib = _lib.load()
    n_patches, p = _check_patches(n_patches, p)
    _patch_rows(pred, "pred", n_patches, p)
    _patch_rows(truth, "truth", n_patches, p)
    if out is not None:
        _shape(out, "out", *pred.shape)
    with _Launch(pred, truth, out) as L:
        ptrs = (_ptr(pred, "pred"), _ptr(truth, "truth"))
        if out is None:
            out = torch.empty_like(pred)
        check(lib.idealnerf_ssim_patch_bwd(*ptrs, n_patches, p, float(g), _ptr(out, "out"), L.stream))
    return out


def render_rays_fwd(rays, bc_rgb, packed_c, folded_c, packed_f, folded_f, t_vals, u, n_importance,
                    t_rand=None, with_fg=False, taps=False, precision=IDN_PREC_F32, precision_fine=None, lindisp=False,
                    white_bkgd=False, noise_coarse=None, noise_fine=None, fused=None, frame=None, draws=None,
                    colour_gate=None, gate_counters=None) -> Dict[str, torch.Tensor]:
    """Network.render_rays forward (audio_exp_nerf.py:297-371) as one C call.  `precision_fine` (default: the
    same as `precision`) selects the fine network's arithmetic; packed_f must be packed for it.
    `fused`: the arrangement of the kernels (same results bit for bit).  False / 0: the kernel sequence
    (network, march, network, compositing) -- the default.  True / 1: the whole path as ONE kernel with a ray's samples, raw
    outputs, weights and cdf in LDS (csrc/render_fused.hip): 0-0.5 % faster on a full frame, six times the HBM bytes (it
    re-fetches a network's 2.4 MB weight stream into every L2 at each change of network).  "split" / 2: the same kernel as
    two launches (coarse network + march | fine network + compositing): half the sequence's bytes, 0.5 % slower.  1 and 2 are
    built for fp32, 64 + 128 samples, no density noise -- anything else raises.  None: IDN_FUSED_MARCH (0 / 1 / 2, read once)
    wherever the fused kernel applies, else the sequence.
    `frame` (ops.make_frame) with `rays=None`: full-frame mode (idealnerf_render_frame_fwd) -- the ray records of the frame's
    row band are derived on the device pass by pass; with `taps` they come back as `tap_rays`.
    `draws=(seed, ray0)` with `u=None, t_rand=None`: the perturb > 0 draws are made inside the kernels (rng_mode 1 of
    idn_render_args), ray r using row ray0 + r of the table `philox_uniform` writes out -- no [n, S] / [n, Ni] random tensors.
    `colour_gate` (idn_render_opts): the fp32 kernel sequence skips the colour branch of every 128-point tile whose colours
    cannot reach a pixel (same results bit for bit; off wherever noise or a raw tap is given).  None: IDN_COLOUR_GATE (1 / 0,
    read once, default 1).  `gate_counters`: int64 [2, 2] on the device, (coarse, fine) x (tiles, skipped); the gated launches
    add to it."""
    lib = _lib.load()
    if gate_counters is not None:
        _shape(gate_counters, "gate_counters", 2, 2)
    if draws is not None and (u is not None or t_rand is not None):
        raise IdealNerfError("draws=(seed, ray0) replaces BOTH t_rand and u: pass them as None")
    _shape(t_vals, "t_vals", None)
    if frame is not None:
        if rays is not None:
            raise IdealNerfError("frame mode derives the rays from the camera: pass rays=None")
        n = frame.nrows * frame.W
    else:
        _shape(rays, "rays", None, RAY_FLOATS)
        n = rays.shape[0]
    S, Ni = t_vals.shape[0], int(n_importance)
    _shape(bc_rgb, "bc_rgb", n, 3)
    _shape(t_rand, "t_rand", n, S)
    _shape(noise_coarse, "noise_coarse", n, S)
    _shape(noise_fine, "noise_fine", n, S + Ni)
    _net_buffers(lib, packed_c, folded_c, precision, "_coarse")
    if Ni > 0:
        if (u is None and draws is None) or packed_f is None or folded_f is None:
            raise IdealNerfError("n_importance > 0 needs u (or draws=) and the fine network's packed / folded buffers")
        if u is not None:
            _u_shape(u, n, Ni)
        _net_buffers(lib, packed_f, folded_f, precision if precision_fine is None else precision_fine, "_fine")
    dev = bc_rgb.device
    with _Launch(rays, bc_rgb, packed_c, folded_c, packed_f, folded_f, t_vals, u, t_rand, noise_coarse, noise_fine, gate_counters) as L:
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        opts = _lib.RenderOpts()
        opts.colour_gate = int(COLOUR_GATE_DEFAULT if colour_gate is None else bool(colour_gate))
        opts.gate_counters = _ptr(gate_counters, "gate_counters", torch.int64)
        out = dict(rgb_map=new(n, 3), disp_map=new(n), acc_map=new(n))
        if Ni > 0:
            out.update(rgb0=new(n, 3), disp0=new(n), acc0=new(n), z_std=new(n), last_weight=new(n))
        if with_fg:
            out["rgb_fg"] = new(n, 3)
            if Ni > 0:
                out.update(rgb_fg0=new(n, 3), last_weight0=new(n))
        if taps:
            out.update(tap_z_coarse=new(n, S), tap_raw_coarse=new(n, S, 4), tap_weights_coarse=new(n, S))
            if Ni > 0:
                out.update(tap_cdf=new(n, S - 1), tap_inds=torch.empty((n, Ni), dtype=torch.int64, device=dev),
                           tap_z_samples=new(n, Ni), tap_z_fine=new(n, S + Ni), tap_raw_fine=new(n, S + Ni, 4),
                           tap_weights_fine=new(n, S + Ni))
        a = _lib.RenderArgs()
        a.rays, a.bc_rgb, a.n_rays = _ptr(rays, "rays"), _ptr(bc_rgb, "bc_rgb"), n
        a.n_samples, a.n_importance, a.precision = S, Ni, _precision(precision)
        a.precision_fine_plus1 = 0 if precision_fine is None else _precision(precision_fine) + 1
        a.packed_coarse, a.folded_coarse = _ptr(packed_c, "packed_coarse"), _ptr(folded_c, "folded_coarse")
        a.packed_fine, a.folded_fine = _ptr(packed_f, "packed_fine"), _ptr(folded_f, "folded_fine")
        a.t_vals, a.t_rand = _ptr(t_vals, "t_vals"), _ptr(t_rand, "t_rand")
        a.u = _ptr(u, "u") if u is not None else None
        a.u_per_ray = 1 if (u is not None and u.dim() == 2) else 0
        a.lindisp, a.white_bkgd = int(bool(lindisp)), int(bool(white_bkgd))
        a.noise_coarse, a.noise_fine = _ptr(noise_coarse, "noise_coarse"), _ptr(noise_fine, "noise_fine")
        if draws is not None:
            a.rng_mode, a.rng_seed, a.rng_ray0 = 1, int(draws[0]) & (2 ** 64 - 1), int(draws[1])
        if fused is None:
            applies = (S == 64 and Ni == 128 and noise_coarse is None and noise_fine is None and
                       _precision(precision) == IDN_PREC_F32 and (precision_fine is None or _precision(precision_fine) == IDN_PREC_F32))
            fused = FUSED_MARCH_DEFAULT if applies else 0
        a.fused_march = _fused_code(fused, "render_rays_fwd(fused=)")
        for k, v in out.items():
            setattr(a, k, v.data_ptr())
        if frame is None:
            nbytes = lib.idealnerf_render_workspace_bytes(n, S, Ni)
            ws = _workspace(nbytes, dev, L.stream or 0)
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
            check(lib.idealnerf_render_rays_fwd_opts(C.byref(a), C.byref(opts), L.stream))
        else:
            tap_rays = new(n, RAY_FLOATS) if taps else None
            frame.rays_out = None if tap_rays is None else tap_rays.data_ptr()
            nbytes = lib.idealnerf_render_frame_workspace_bytes(n, S, Ni)
            ws = _workspace(nbytes, dev, L.stream or 0)
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
            check(lib.idealnerf_render_frame_fwd_opts(C.byref(a), C.byref(frame), C.byref(opts), L.stream))
            frame.rays_out = None
            if tap_rays is not None:
                out["tap_rays"] = tap_rays
    return out


# ---- ray cull (csrc/cull.hip; cull.py builds and uses the grid) ----------------------------------------------------------
def _cull_G(G):
    if isinstance(G, bool) or not isinstance(G, int) or G < 32 or G > 1024 or G % 32:
        raise IdealNerfError(f"G = {G!r}: the grid edge is a multiple of 32 in 32..1024")
    return G


def cull_mark(raw, sigma_min, corners) -> torch.Tensor:
    """corners[i] |= raw[i, 3] > sigma_min (idealnerf_cull_mark): raw [n, 4] fp32, corners uint8 [n], updated in place."""
    lib = _lib.load()
    _shape(raw, "raw", None, 4)
    n = raw.shape[0]
    _shape(corners, "corners", n)
    with _Launch(raw, corners) as L:
        check(lib.idealnerf_cull_mark(_ptr(raw, "raw"), n, float(sigma_min), _ptr(corners, "corners", torch.uint8), L.stream))
    return corners


def cull_cells(corners, G, dilate) -> torch.Tensor:
    """Marked lattice corners uint8 [(G+1)^3] -> cell bits int32 [G^3 / 32], 32 cells per word along x (idealnerf_cull_cells):
    a cell is set when a corner of a cell within `dilate` cells of it (Chebyshev) is marked."""
    lib = _lib.load()
    G = _cull_G(G)
    if isinstance(dilate, bool) or not isinstance(dilate, int) or dilate < 0:
        raise IdealNerfError(f"dilate = {dilate!r}: a whole number of cells >= 0")
    _shape(corners, "corners", (G + 1) ** 3)
    with _Launch(corners) as L:
        ptr = _ptr(corners, "corners", torch.uint8)
        bits = torch.empty(G ** 3 // 32, dtype=torch.int32, device=corners.device)
        check(lib.idealnerf_cull_cells(ptr, G, dilate, bits.data_ptr(), L.stream))
    return bits


def _cull_grid_struct(bits, G, lo, cell):
    G = _cull_G(G)
    _shape(bits, "bits", G ** 3 // 32)
    if not float(cell) > 0.0:
        raise IdealNerfError(f"cell = {cell!r} must be positive")
    g = _lib.CullGridStruct()
    g.bits, g.G, g.cell = _ptr(bits, "bits", torch.int32), G, float(cell)
    g.lo = (C.c_float * 3)(*[float(v) for v in lo])
    return g


def cull_classify(bits, G, lo, cell, frame, dz, K, sel=None, n_live=None):
    """The live pixels of the frame's row band (idealnerf_cull_classify): -> (sel int64 [nrows W], n_live int32 [1]), both on
    the device; sel[:n_live] holds the live pixels (row-major in the band) in ascending order, the rest is not written.
    dz, K: the march z_k = near + k dz, k < K, z_K = far (`cull.march_steps` chooses them)."""
    lib = _lib.load()
    npix = frame.nrows * frame.W
    _shape(sel, "sel", npix)
    _shape(n_live, "n_live", 1)
    if not float(dz) > 0.0 or int(K) < 1 or int(K) > 1 << 20:
        raise IdealNerfError(f"a march of K = {K} steps of dz = {dz} (K in 1..2^20, dz > 0)")
    with _Launch(bits, sel, n_live) as L:
        g = _cull_grid_struct(bits, G, lo, cell)
        if sel is None:
            sel = torch.empty(npix, dtype=torch.int64, device=bits.device)
        if n_live is None:
            n_live = torch.empty(1, dtype=torch.int32, device=bits.device)
        ws = _workspace(lib.idealnerf_cull_classify_workspace_bytes(npix), bits.device, L.stream or 0)
        check(lib.idealnerf_cull_classify(C.byref(g), C.byref(frame), float(dz), int(K), _ptr(sel, "sel", torch.int64),
                                          _ptr(n_live, "n_live", torch.int32), ws.data_ptr(), ws.numel(), L.stream))
    return sel, n_live


def cull_gather(sel, frame, bc_rgb):
    """(rays [n, 11], bc_live [n, 3]) of the band's pixels `sel` (int64 [n]): each ray row is the row `frame_rays` writes for
    that pixel, bit for bit (idealnerf_cull_gather).  bc_rgb [nrows W, 3]: the band's background."""
    lib = _lib.load()
    _shape(sel, "sel", None)
    n, npix = sel.shape[0], frame.nrows * frame.W
    _shape(bc_rgb, "bc_rgb", npix, 3)
    if n > npix:
        raise IdealNerfError(f"sel holds {n} pixels, the band has {npix}")
    with _Launch(sel, bc_rgb) as L:
        ptrs = (_ptr(sel, "sel", torch.int64), _ptr(bc_rgb, "bc_rgb"))
        rays = torch.empty((n, RAY_FLOATS), dtype=torch.float32, device=sel.device)
        bc_live = torch.empty((n, 3), dtype=torch.float32, device=sel.device)
        check(lib.idealnerf_cull_gather(ptrs[0], n, C.byref(frame), ptrs[1], rays.data_ptr(), bc_live.data_ptr(), L.stream))
    return rays, bc_live


def cull_scatter(sel, n_live, bc_rgb, outputs) -> Dict[str, torch.Tensor]:
    """fill + scatter (idealnerf_cull_scatter).  outputs: name -> (live [n_live, ...] or None when n_live == 0, channels, fill)
    with fill = "bc" (the background pixel; channels 3) or a float.  -> name -> dense [n_pixels(, 3)]: the fill in every pixel,
    row i of live at pixel sel[i]."""
    lib = _lib.load()
    npix, n_live = bc_rgb.shape[0], int(n_live)
    _shape(bc_rgb, "bc_rgb", npix, 3)
    if not 0 <= n_live <= npix or (n_live and (sel is None or sel.dim() != 1 or sel.shape[0] < n_live)):
        raise IdealNerfError(f"n_live = {n_live} with {npix} pixels and sel {None if sel is None else list(sel.shape)}")
    if len(outputs) > _lib.CULL_MAX_OUTPUTS:
        raise IdealNerfError(f"{len(outputs)} outputs: one call takes {_lib.CULL_MAX_OUTPUTS}")
    for name, (live, ch, fill) in outputs.items():
        if ch not in (1, 3) or (fill == "bc" and ch != 3):
            raise IdealNerfError(f"{name}: channels {ch} / fill {fill!r}")
        if n_live:
            _shape(live, name, *((n_live, 3) if ch == 3 else (n_live,)))
    lives = [v[0] for v in outputs.values() if n_live]
    with _Launch(sel, bc_rgb, *lives) as L:
        bc_ptr, sel_ptr = _ptr(bc_rgb, "bc_rgb"), _ptr(sel, "sel", torch.int64)
        recs = (_lib.CullOutput * max(len(outputs), 1))()
        dense = {}
        for r, (name, (live, ch, fill)) in zip(recs, outputs.items()):
            dense[name] = torch.empty((npix, 3) if ch == 3 else (npix,), dtype=torch.float32, device=bc_rgb.device)
            r.dense, r.live, r.channels = dense[name].data_ptr(), _ptr(live, name) if n_live else None, ch
            r.fill_background, r.value = int(fill == "bc"), 0.0 if fill == "bc" else float(fill)
        check(lib.idealnerf_cull_scatter(sel_ptr, n_live, npix, bc_ptr, recs, len(outputs), L.stream))
    return dense


# ---- sample cull of the live rays (csrc/cull.hip) ---------------------------------------------------
def _cull_points(rays, z):
    _shape(z, "z", None, None)
    n, S = z.shape
    _shape(rays, "rays", n, RAY_FLOATS)
    if n * S >= 2 ** 31:
        raise IdealNerfError(f"{n} rays of {S} samples: one sample cull takes fewer than 2^31 points")
    return n, S


def cull_sample_classify(bits, G, lo, cell, rays, z, sel=None, n_live=None):
    """The live points of a network pass over rays [n, 11] / z [n, S] (idealnerf_cull_sample_classify): -> (sel int64 [n S],
    n_live int32 [1]), both on the device; sel[:n_live] holds the live points P = ray S + s in ascending order, the rest is not
    written.  A point is skipped when its cell is clear and it is its ray's last sample or its spacing is at most
    idealnerf_colour_gate_max_dist(); every other point (occupied cell, outside the box, wider spacing, NaN) is live."""
    lib = _lib.load()
    n, S = _cull_points(rays, z)
    _shape(sel, "sel", n * S)
    _shape(n_live, "n_live", 1)
    with _Launch(bits, rays, z, sel, n_live) as L:
        g = _cull_grid_struct(bits, G, lo, cell)
        ptrs = (_ptr(rays, "rays"), _ptr(z, "z"))
        if sel is None:
            sel = torch.empty(n * S, dtype=torch.int64, device=bits.device)
        if n_live is None:
            n_live = torch.empty(1, dtype=torch.int32, device=bits.device)
        ws = _workspace(lib.idealnerf_cull_classify_workspace_bytes(n * S), bits.device, L.stream or 0)
        check(lib.idealnerf_cull_sample_classify(C.byref(g), *ptrs, n, S, _ptr(sel, "sel", torch.int64),
                                                 _ptr(n_live, "n_live", torch.int32), ws.data_ptr(), ws.numel(), L.stream))
    return sel, n_live


def cull_sample_gather(sel, rays, z):
    """(pts [m, 3], dirs [m, 3]) of the points `sel` (int64 [m]) of rays [n, 11] / z [n, S]: the position the network kernels
    form for the point, bit for bit, and its ray's view direction (idealnerf_cull_sample_gather) -- `query_points_fwd`'s
    inputs as pts.view(m, 1, 3), dirs."""
    lib = _lib.load()
    n, S = _cull_points(rays, z)
    _shape(sel, "sel", None)
    m = sel.shape[0]
    if m > n * S:
        raise IdealNerfError(f"sel holds {m} points, the pass has {n * S}")
    with _Launch(sel, rays, z) as L:
        ptrs = (_ptr(sel, "sel", torch.int64), _ptr(rays, "rays"), _ptr(z, "z"))
        pts = torch.empty((m, 3), dtype=torch.float32, device=sel.device)
        dirs = torch.empty((m, 3), dtype=torch.float32, device=sel.device)
        check(lib.idealnerf_cull_sample_gather(ptrs[0], m, ptrs[1], ptrs[2], n, S, pts.data_ptr(), dirs.data_ptr(), L.stream))
    return pts, dirs


def cull_sample_scatter(sel, m, raw_live, n, S, device=None) -> torch.Tensor:
    """The dense raw [n, S, 4] of a sparse pass (idealnerf_cull_sample_scatter): row j of raw_live [m, 4] at point sel[j],
    +0.0 in all four channels elsewhere.  m == 0: zeros on `device` (sel and raw_live may be None)."""
    lib = _lib.load()
    m, n, S = int(m), int(n), int(S)
    if n < 0 or S < 1 or n * S >= 2 ** 31 or not 0 <= m <= n * S or (m and (sel is None or sel.dim() != 1 or sel.shape[0] < m)):
        raise IdealNerfError(f"m = {m} live points of {n} x {S} with sel {None if sel is None else list(sel.shape)}")
    if m:
        _shape(raw_live, "raw_live", m, 4)
    with _Launch(*((sel, raw_live) if m else ()), device=device) as L:
        ptrs = (_ptr(sel, "sel", torch.int64), _ptr(raw_live, "raw_live")) if m else (None, None)
        raw = torch.empty((n, S, 4), dtype=torch.float32, device=L.device)
        check(lib.idealnerf_cull_sample_scatter(ptrs[0], m, ptrs[1], n * S, raw.data_ptr(), L.stream))
    return raw


def _sparse_pass(grid, packed, folded, rays, z, precision):
    """One network pass over the live points only: classify, read the count (the pass's one host read), gather, the points
    mode of the network's kernel, scatter.  -> raw [n, S, 4]."""
    n, S = z.shape
    sel, n_dev = cull_sample_classify(grid.bits, grid.G, grid.lo, grid.cell, rays, z)
    m = int(n_dev.item())
    grid.points_seen += n * S
    grid.points_evaluated += m
    raw_live = None
    if m:
        pts, dirs = cull_sample_gather(sel[:m], rays, z)
        raw_live = query_points_fwd(packed, folded, pts.view(m, 1, 3), dirs, precision).view(m, 4)
    return cull_sample_scatter(sel if m else None, m, raw_live, n, S, device=z.device)


def render_rays_sparse_fwd(grid, rays, bc_rgb, packed_c, folded_c, packed_f, folded_f, t_vals, u, n_importance, t_rand=None,
                           with_fg=False, precision=IDN_PREC_F32, precision_fine=None, draws=None, chunk=32768, taps=False,
                           lindisp=False, white_bkgd=False, noise_coarse=None, noise_fine=None, fused=None) -> Dict[str, torch.Tensor]:
    """`render_rays_fwd` (rays mode, kernel sequence) with both network passes evaluated only at the samples the occupancy
    `grid` (cull.CullGrid) cannot rule out: the same outputs under the same names, bit for bit while
    sigma_raw <= 0 in the grid's clear cells.  Per `chunk` rays: coarse_depths, sparse coarse pass, march_fwd, sparse fine pass,
    composite_fwd (n_importance == 0: the coarse pass and composite_fwd); two host reads per chunk (the passes' live counts),
    which the grid adds to `points_seen` / `points_evaluated`.  `draws=(seed, ray0)`: the rows of the two draw tables are
    materialised with `philox_uniform`, so the numbers are the in-kernel ones.  taps, density noise, white_bkgd, lindisp and
    the fused arrangements are refused, as by `cull.refuse`."""
    bad = [name for name, on in (("taps", taps), ("white_bkgd", white_bkgd), ("lindisp", lindisp),
                                 ("density noise", noise_coarse is not None or noise_fine is not None),
                                 ("a fused arrangement", (FUSED_MARCH_DEFAULT if fused is None else _fused_code(fused, "fused=")) != 0)) if on]
    if bad:
        raise IdealNerfError(f"{', '.join(bad)} with the sample cull: a skipped sample has no raw output to tap, and its argument "
                             "holds for the plain kernel sequence without density noise or a white background")
    if draws is not None and (u is not None or t_rand is not None):
        raise IdealNerfError("draws=(seed, ray0) replaces BOTH t_rand and u: pass them as None")
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise IdealNerfError(f"chunk = {chunk!r}: a whole number of rays >= 1")
    _shape(t_vals, "t_vals", None)
    _shape(rays, "rays", None, RAY_FLOATS)
    n, S, Ni = rays.shape[0], t_vals.shape[0], int(n_importance)
    _shape(bc_rgb, "bc_rgb", n, 3)
    _shape(t_rand, "t_rand", n, S)
    if Ni > 0:
        if (u is None and draws is None) or packed_f is None or folded_f is None:
            raise IdealNerfError("n_importance > 0 needs u (or draws=) and the fine network's packed / folded buffers")
        if u is not None:
            _u_shape(u, n, Ni)
    prec_f = precision if precision_fine is None else precision_fine
    # render_rays_fwd's names: the last compositing's outputs, and in front of a fine pass the march's under their *0 names
    last = ("rgb_map", "disp_map", "acc_map") + (("last_weight",) if Ni > 0 else ()) + (("rgb_fg",) if with_fg else ())
    first = dict(rgb_map="rgb0", disp_map="disp0", acc_map="acc0", z_std="z_std") if Ni > 0 else {}
    if Ni > 0 and with_fg:
        first.update(rgb_fg="rgb_fg0", last_weight="last_weight0")
    parts: Dict[str, list] = {k: [] for k in last + tuple(first.values())}
    for r0 in range(0, n, chunk):
        r, bc = rays[r0:r0 + chunk], bc_rgb[r0:r0 + chunk]
        c = r.shape[0]
        tr, uc = (None if t_rand is None else t_rand[r0:r0 + chunk]), (u[r0:r0 + chunk] if u is not None and u.dim() == 2 else u)
        if draws is not None:
            tr = philox_uniform(draws[0], 0, int(draws[1]) + r0, c, S, rays.device)
            uc = philox_uniform(draws[0], 1, int(draws[1]) + r0, c, Ni, rays.device) if Ni > 0 else None
        z = coarse_depths(r, t_vals, tr)
        raw = _sparse_pass(grid, packed_c, folded_c, r, z, precision)
        if Ni > 0:
            m = march_fwd(raw, z, r, bc, uc, Ni, with_fg=with_fg)
            for old, new in first.items():
                parts[new].append(m[old])
            z = m["z_fine"]
            raw = _sparse_pass(grid, packed_f, folded_f, r, z, prec_f)
        f = composite_fwd(raw, z, r, bc, with_fg=with_fg, with_weights=False)
        for k in last:
            parts[k].append(f[k])
    empty = lambda k: torch.empty((0, 3) if k.startswith("rgb") else (0,), dtype=torch.float32, device=bc_rgb.device)   # (no rays)
    return {k: (torch.cat(v, 0) if len(v) > 1 else v[0] if v else empty(k)) for k, v in parts.items()}


def profile_begin():
    """Start counting the network-kernel launches (idealnerf_profile_begin)."""
    _lib.load().idealnerf_profile_begin()


def profile_end():
    """-> (total_ms, launches, points) of the network-kernel launches since `profile_begin` (idealnerf_profile_end)."""
    ms, launches, points = C.c_double(0), C.c_int64(0), C.c_int64(0)
    check(_lib.load().idealnerf_profile_end(C.byref(ms), C.byref(launches), C.byref(points)))
    return ms.value, launches.value, points.value
