"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports exactly
what include/idealnerf.h declares, the ctypes mirrors have the C layout, the host layer
keeps the reference's names/shapes/semantics, the product path refuses CPU tensors, and
the multi-rank tiling works over gloo with world_size 2.  No GPU compute here."""
import ctypes as C
import os
import time
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "idealnerf.h")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    return idealnerf_amd


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(idealnerf_\w+)\s*\(", src)))


def test_library_exports_every_declared_symbol(idn):
    lib = idn._lib.load()
    names = header_functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/idealnerf.h but not exported"
    assert sorted(idn._lib.PROTOTYPES) == names, "ctypes prototypes and header are out of sync"
    assert lib.idealnerf_version() == 4
    assert lib.idealnerf_folded_bias_floats() == 3136   # 2496 biases + alpha_linear (256) and rgb_linear (3 x 128) weight rows
    assert lib.idealnerf_packed_weight_floats(0) == 2304 * 256
    assert lib.idealnerf_packed_weight_floats(99) == 0


def test_ctypes_structs_match_c_layout(idn, tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "idealnerf.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(idn_facenerf_params), '
        'sizeof(idn_composite_out), sizeof(idn_render_args), offsetof(idn_facenerf_params, dim_aud), '
        'offsetof(idn_render_args, t_vals), offsetof(idn_render_args, tap_inds), '
        'offsetof(idn_render_args, workspace_bytes), offsetof(idn_render_args, precision_fine_plus1), '
        'sizeof(idn_frame), offsetof(idn_frame, focal), offsetof(idn_frame, rays_out), sizeof(idn_audio_net_params), '
        'offsetof(idn_audio_net_params, dim_aud), sizeof(idn_audio_net_grads), offsetof(idn_render_args, rng_mode), '
        'offsetof(idn_render_args, rng_seed), offsetof(idn_render_args, rng_ray0), '
        'sizeof(idn_dw_take), offsetof(idn_dw_take, out), offsetof(idn_dw_take, ldo), sizeof(idn_dw_colsum_take), sizeof(idn_dw_product), '
        'offsetof(idn_dw_product, acts2), offsetof(idn_dw_product, takes), offsetof(idn_dw_product, colsum_takes), '
        'offsetof(idn_dw_product, chunks_per_split));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    L = idn._lib
    want = [C.sizeof(L.FaceNerfParams), C.sizeof(L.CompositeOut), C.sizeof(L.RenderArgs),
            L.FaceNerfParams.dim_aud.offset, L.RenderArgs.t_vals.offset, L.RenderArgs.tap_inds.offset,
            L.RenderArgs.workspace_bytes.offset, L.RenderArgs.precision_fine_plus1.offset,
            C.sizeof(L.Frame), L.Frame.focal.offset, L.Frame.rays_out.offset,
            C.sizeof(L.AudioNetParams), L.AudioNetParams.dim_aud.offset, C.sizeof(L.AudioNetGrads),
            L.RenderArgs.rng_mode.offset, L.RenderArgs.rng_seed.offset, L.RenderArgs.rng_ray0.offset,
            C.sizeof(L.DwTake), L.DwTake.out.offset, L.DwTake.ldo.offset, C.sizeof(L.DwColsumTake), C.sizeof(L.DwProduct),
            L.DwProduct.acts2.offset, L.DwProduct.takes.offset, L.DwProduct.colsum_takes.offset, L.DwProduct.chunks_per_split.offset]
    assert got == want
    hdr = open(HEADER).read()
    for name, val in (("PRODUCTS", L.DW_MAX_PRODUCTS), ("TAKES", L.DW_MAX_TAKES), ("COLSUM_TAKES", L.DW_MAX_COLSUM_TAKES)):
        assert re.search(rf"#define IDN_DW_MAX_{name} {val}\b", hdr), name


def test_c_abi_argument_errors_without_gpu(idn):
    lib = idn._lib.load()
    # NULL params: rejected before any HIP call
    assert lib.idealnerf_pack_weights(None, 0, None, None) == -1
    assert b"NULL" in lib.idealnerf_last_error()
    p = idn._lib.FaceNerfParams()
    assert lib.idealnerf_pack_weights(C.byref(p), 0, None, None) == -1
    a = idn._lib.RenderArgs()
    a.precision = 7
    assert lib.idealnerf_render_rays_fwd(C.byref(a), None) == -2  # IDN_EUNSUPPORTED
    assert lib.idealnerf_render_workspace_bytes(0, 64, 128) == 0
    # in-kernel draws: the mode is validated, and it excludes the tensors it replaces
    a = idn._lib.RenderArgs()
    a.n_rays, a.n_samples, a.n_importance = 4, 64, 128
    a.bc_rgb = a.t_vals = a.packed_coarse = a.folded_coarse = a.packed_fine = a.folded_fine = a.rays = 1
    a.rng_mode = 2
    assert lib.idealnerf_render_rays_fwd(C.byref(a), None) == -1 and b"rng_mode" in lib.idealnerf_last_error()
    a.rng_mode, a.u = 1, 1
    assert lib.idealnerf_render_rays_fwd(C.byref(a), None) == -1 and b"must be NULL" in lib.idealnerf_last_error()
    a.u, a.rng_ray0 = None, -1
    assert lib.idealnerf_render_rays_fwd(C.byref(a), None) == -1 and b"rng_ray0" in lib.idealnerf_last_error()
    a.rng_ray0 = 0   # (draws on, no u: accepted up to the next check, the workspace)
    assert lib.idealnerf_render_rays_fwd(C.byref(a), None) == -4 and b"workspace" in lib.idealnerf_last_error()
    assert lib.idealnerf_philox_uniform(1, 2, 0, 4, 4, None, None) == -1 and b"which" in lib.idealnerf_last_error()
    assert lib.idealnerf_philox_uniform(1, 0, -1, 4, 4, None, None) == -1
    assert lib.idealnerf_philox_uniform(1, 0, 0, 4, 4, None, None) == -1 and b"NULL" in lib.idealnerf_last_error()
    assert lib.idealnerf_philox_uniform(1, 0, 0, 0, 4, None, None) == 0
    # AudioNet kernels: NULL parameters, a dim_aud the kernel is not built for and more windows than the backward holds in LDS
    ap = idn._lib.AudioNetParams()
    assert lib.idealnerf_audio_net_fwd(C.byref(ap), None, 1, None, None, None) == -1 and b"NULL" in lib.idealnerf_last_error()
    for i in range(4):
        ap.conv_w[i] = ap.conv_b[i] = 1
    for i in range(2):
        ap.fc_w[i] = ap.fc_b[i] = 1
    ap.dim_aud = 500
    assert lib.idealnerf_audio_net_fwd(C.byref(ap), 1, 1, 1, None, None) == -2 and b"dim_aud" in lib.idealnerf_last_error()
    ap.dim_aud = 64
    ag = idn._lib.AudioNetGrads()
    for i in range(4):
        ag.conv_w[i] = ag.conv_b[i] = 1
    for i in range(2):
        ag.fc_w[i] = ag.fc_b[i] = 1
    assert lib.idealnerf_audio_net_bwd(C.byref(ap), C.byref(ag), 1, 1, 1, 9, None) == -2 and b"windows" in lib.idealnerf_last_error()
    assert lib.idealnerf_audio_net_saved_floats(8) == 8 * 640 and lib.idealnerf_audio_net_fwd(C.byref(ap), None, 0, None, None, None) == 0
    # frame mode: the camera replaces the ray records -- a rays pointer, rows outside the frame or a ray count that is not
    # the band's are refused before any HIP call
    f = idn._lib.Frame()
    f.H, f.W, f.row0, f.nrows = 32, 32, 8, 4
    a = idn._lib.RenderArgs()
    a.n_rays = 4 * 32
    a.rays = 1
    assert lib.idealnerf_render_frame_fwd(C.byref(a), C.byref(f), None) == -1 and b"must be NULL" in lib.idealnerf_last_error()
    a.rays = None
    a.n_rays = 5 * 32
    assert lib.idealnerf_render_frame_fwd(C.byref(a), C.byref(f), None) == -1 and b"nrows * W" in lib.idealnerf_last_error()
    f.nrows = 30
    assert lib.idealnerf_render_frame_fwd(C.byref(a), C.byref(f), None) == -1 and b"bad frame" in lib.idealnerf_last_error()
    assert lib.idealnerf_render_frame_workspace_bytes(1000, 64, 128) == lib.idealnerf_render_workspace_bytes(1000, 64, 128) + 1000 * 44 // 256 * 256 + 256
    per_ray = lib.idealnerf_render_workspace_bytes(1000, 64, 128) / 1000
    assert 5000 < per_ray < 5500  # 5*S + 5*(S+Ni) floats per ray (z and raw of both passes), rounded up per buffer
    assert lib.idealnerf_render_workspace_bytes(10 ** 6, 64, 128) == lib.idealnerf_render_workspace_bytes(32768, 64, 128)
    # a list of dW products through one pass plan: everything that needs no device is refused before any HIP call
    L = idn._lib
    ws_bytes = lib.idealnerf_dw_products_workspace_bytes()
    assert ws_bytes == 256 * (9 * 65536 + 6 * 16384 + 4 * 8192) * 4 + 256 * 256 * 16 * 4   # the two pools of a pass (csrc/dw_gemm.h)

    def product(N=256, K=256, ld_delta=256, ld_acts=None, acts2=None, colsum=True, takes=((0, 0, 1, 1, 4096, 256),), ctakes=()):
        r = L.DwProduct()
        r.delta, r.ld_delta, r.N, r.acts, r.ld_acts, r.K = 4096, ld_delta, N, 8192, K if ld_acts is None else ld_acts, K
        r.acts2, r.want_colsum, r.n_takes, r.n_colsum_takes = acts2, int(colsum), len(takes), len(ctakes)
        for k, v in zip(r.takes, takes):
            k.row0, k.col0, k.rows, k.cols, k.out, k.ldo = v
        for k, v in zip(r.colsum_takes, ctakes):
            k.col0, k.cols, k.out = v
        return r

    def refused(recs, rows=256, pipe=0, x6_items=1, n=None, ws=4096, nbytes=ws_bytes):
        arr = (L.DwProduct * len(recs))(*recs)
        rc = lib.idealnerf_dw_products(rows, pipe, x6_items, arr, len(recs) if n is None else n, ws, nbytes, None)
        return rc, lib.idealnerf_last_error()

    assert lib.idealnerf_dw_products(256, 0, 1, None, 1, 4096, ws_bytes, None) == -1 and b"NULL" in lib.idealnerf_last_error()
    for n in (0, -1, L.DW_MAX_PRODUCTS + 1):
        rc, msg = refused([product()], n=n)
        assert rc == -1 and b"products outside" in msg, n
    rc, msg = refused([product()], pipe=2)
    assert rc == -1 and b"pipe" in msg
    for rows in (0, -128, 100, 192):
        rc, msg = refused([product()], rows=rows)
        assert rc == -1 and b"multiple of 128" in msg, rows
    for x6_items in (0, 13):     # kMaxTnBatch = 12
        rc, msg = refused([product()], x6_items=x6_items)
        assert rc == -1 and b"x6_items" in msg
    r = product()
    r.acts = None
    rc, msg = refused([r])
    assert rc == -1 and b"NULL" in msg
    for N, K in ((64, 64), (64, 256), (256, 128), (128, 32), (0, 0), (255, 256)):
        for pipe in (0, 1):
            rc, msg = refused([product(N=N, K=K)], pipe=pipe)
            assert rc == -2 and b"no instantiation" in msg, (N, K)
    for N in (64, 128, 256):      # the host layer's table of shapes is the library's: the others stop at the workspace check
        for K in (64, 128, 256):
            rc, _ = refused([product(N=N, K=K, takes=())], pipe=1, nbytes=0)
            assert rc == (-4 if (N, K) in idn.ops.DW_SHAPES else -2), (N, K)
    for kw in (dict(N=128, K=64, ld_delta=124), dict(N=128, K=64, ld_delta=256, ld_acts=60), dict(ld_delta=252)):
        rc, msg = refused([product(**kw)], pipe=1)
        assert rc == -1 and b"row pitch" in msg, kw
    rc, msg = refused([product(N=128, K=64, ld_delta=130)], pipe=1)     # rows of 16-byte pieces
    assert rc == -1 and b"aligned" in msg
    rc, msg = refused([product(acts2=12288)], pipe=1)
    assert rc == -1 and b"split B" in msg
    rc, msg = refused([product(N=128, K=128, acts2=12288)], pipe=0)
    assert rc == -1 and b"split B" in msg
    for far in (8192 + (1 << 31), 8192 + (5 << 30)):     # acts at 8192: 32-bit byte offsets from the lower of the two
        rc, msg = refused([product(acts2=far)], pipe=0)
        assert rc == -2 and b"2 GiB apart" in msg
    r = product(acts2=8192 + (1 << 31) - 16)             # (the last distance that fits: on to the workspace check)
    assert refused([r], nbytes=0)[0] == -4
    r.acts, r.acts2 = r.acts2, r.acts                    # ... and with acts2 below acts
    assert refused([r], nbytes=0)[0] == -4
    r.acts += 16
    rc, msg = refused([r], nbytes=0)
    assert rc == -2 and b"2 GiB apart" in msg
    rc, msg = refused([product(), product()], x6_items=1)
    assert rc == -1 and b"x6_items" in msg
    rc, msg = refused([product()] * 13, x6_items=12)
    assert rc == -1 and b"x6_items" in msg
    r = product()
    r.n_takes = L.DW_MAX_TAKES + 1
    rc, msg = refused([r])
    assert rc == -1 and b"takes" in msg
    four = ((0, 0, 1, 1, 4096, 256),) * 4
    rc, msg = refused([product(N=64, K=128, takes=four, ctakes=((0, 1, 4096),))] * 7, pipe=1)     # 35 reductions > kMaxReduceItems = 32
    assert rc == -1 and b"more than 32 takes" in msg
    for take in ((0, 0, 65, 128, 4096, 128), (1, 0, 64, 128, 4096, 128), (0, 1, 64, 128, 4096, 128), (-1, 0, 1, 1, 4096, 128),
                 (0, 0, 0, 1, 4096, 128), (0, 0, 3, 128, 4096, 127), (0, 0, 3, 128, None, 128)):
        rc, msg = refused([product(N=64, K=128, takes=(take,))], pipe=1)
        assert rc == -1 and (b"leaves the 64 x 128 block" in msg or b"NULL" in msg), take
    rc, msg = refused([product(N=64, K=128, colsum=False, ctakes=((0, 3, 4096),))], pipe=1)
    assert rc == -1 and b"kept no column sums" in msg
    for ctake in ((62, 3, 4096), (-1, 1, 4096), (0, 0, 4096), (0, 3, None)):
        rc, msg = refused([product(N=64, K=128, ctakes=(ctake,))], pipe=1)
        assert rc == -1 and (b"leaves the 64 columns" in msg or b"NULL" in msg), ctake
    rc, msg = refused([product()] * 12, pipe=1)      # twelve 256 x 256 blocks per split: more than the pools of a pass hold
    assert rc == -4 and b"pools of a pass" in msg
    rc, msg = refused([product()], nbytes=ws_bytes - 1)
    assert rc == -4 and b"workspace" in msg
    rc, msg = refused([product()], ws=None)
    assert rc == -4 and b"workspace" in msg
    # the delta chain alone: the same, in the order NULL, p_pad, pipe, max_blocks, alignment, workspace
    dc_bytes = lib.idealnerf_delta_chain_workspace_bytes()
    assert dc_bytes == 3264 * 256 * 4     # the six-piece transposed stream: 3264 fragments of 64 lanes x 4 floats
    fp_ = idn._lib.FaceNerfParams()

    def chain(p=fp_, pipe=0, acts=4096, p_pad=256, d_rgb=8192, dv0=12288, dv21=16384, da=20480, max_blocks=0, ws=24576, nbytes=dc_bytes):
        blocks = C.c_int(-7)
        rc = lib.idealnerf_delta_chain(None if p is None else C.byref(p), pipe, acts, p_pad, d_rgb, dv0, dv21, da, max_blocks,
                                       C.byref(blocks), ws, nbytes, None)
        assert blocks.value == -7         # (nothing ran)
        return rc, lib.idealnerf_last_error()

    rc, msg = chain(p=None)
    assert rc == -1 and b"params is NULL" in msg
    rc, msg = chain()
    assert rc == -1 and b"pts_linears.0 is NULL" in msg
    for i in range(8):
        fp_.pts_w[i] = fp_.pts_b[i] = 4096
    for i in range(3):
        fp_.views_w[i] = fp_.views_b[i] = 4096
    fp_.alpha_w = fp_.alpha_b = fp_.rgb_w = fp_.rgb_b = 4096
    for name in ("acts", "d_rgb", "dv0", "dv21", "da"):
        rc, msg = chain(**{name: None})
        assert rc == -1 and b"NULL" in msg, name
    for p_pad in (0, -128, 100, 192):
        rc, msg = chain(p_pad=p_pad)
        assert rc == -1 and b"multiple of 128" in msg, p_pad
    rc, msg = chain(p_pad=(1 << 24) + 128)
    assert rc == -2 and b"2^24" in msg
    for pipe in (-1, 2):                  # (IDN_DW_PIPE_BF16X6_PASS is a dw_gemm split count, not a chain)
        rc, msg = chain(pipe=pipe)
        assert rc == -1 and b"pipe" in msg
    rc, msg = chain(max_blocks=-1)
    assert rc == -1 and b"max_blocks" in msg
    for name in ("acts", "d_rgb", "dv0", "dv21", "da", "ws"):
        rc, msg = chain(**{name: 4096 + 4})
        assert rc == -1 and b"aligned" in msg, name
    for kw in (dict(nbytes=dc_bytes - 1), dict(nbytes=0), dict(ws=None)):
        rc, msg = chain(pipe=1, p_pad=1 << 24, **kw)
        assert rc == -4 and b"workspace" in msg, kw
    # the compositing backward alone: n_rays, then NULL operands, alignment, pitches, n_samples; the four gradients may be NULL
    def comp(raw=4096, z=8192, rays=12288, bc=16384, n=4, S=64, g=(None, None, None, None), d_rgb=20480, ld_rgb=4, d_sig=20492, ld_sig=4,
             d_norm=None, ld_norm=0):
        rc = lib.idealnerf_composite_bwd(raw, z, rays, bc, n, S, *g, d_rgb, ld_rgb, d_sig, ld_sig, d_norm, ld_norm, None)
        return rc, lib.idealnerf_last_error()

    rc, msg = comp(n=-1)
    assert rc == -1 and b"n_rays < 0" in msg
    assert comp(n=0)[0] == 0 and comp(n=0, raw=None, d_rgb=None, S=0)[0] == 0          # nothing to do: OK, as idealnerf_pass_bwd
    for name in ("raw", "z", "rays", "bc", "d_rgb", "d_sig"):
        rc, msg = comp(**{name: None})
        assert rc == -1 and b"composite_bwd: NULL" in msg, name
    rc, msg = comp(raw=4096 + 4)
    assert rc == -1 and b"aligned" in msg
    for kw in (dict(ld_rgb=2), dict(ld_rgb=0), dict(ld_sig=0), dict(ld_sig=-4), dict(d_norm=24576, ld_norm=0), dict(d_norm=24576, ld_norm=-11)):
        rc, msg = comp(**kw)
        assert rc == -1 and b"row pitch" in msg, kw
    rc, msg = comp(n=1 << 31)
    assert rc == -2 and b"2^31-1" in msg
    for S in (-1, 0, 1, 513, 1024):     # with and without d_norm, with and without gradients: refused before the launch
        for kw in ({}, dict(d_norm=24576, ld_norm=11), dict(g=(4096, 4096, 4096, 4096), ld_rgb=64, ld_sig=256)):
            rc, msg = comp(S=S, **kw)
            assert rc == -2 and b"n_samples" in msg and b"[2, 512]" in msg, (S, kw)
    # the backward's tail alone.  The input gradient: params, NULL, p_pad, n, max_blocks, alignment
    def dx(p=fp_, dA0=4096, dA5=8192, dV0=12288, n=100, p_pad=256, d_x=16384, max_blocks=0):
        blocks = C.c_int(-7)
        rc = lib.idealnerf_input_grad(None if p is None else C.byref(p), dA0, dA5, dV0, n, p_pad, d_x, max_blocks, C.byref(blocks), None)
        assert blocks.value == -7         # (nothing ran)
        return rc, lib.idealnerf_last_error()

    rc, msg = dx(p=None)
    assert rc == -1 and b"params is NULL" in msg
    for name in ("dA0", "dA5", "dV0", "d_x"):
        rc, msg = dx(**{name: None})
        assert rc == -1 and b"input_grad: NULL" in msg, name
    for p_pad in (0, -128, 100, 192):
        rc, msg = dx(p_pad=p_pad, n=1)
        assert rc == -1 and b"multiple of 128" in msg, p_pad
    rc, msg = dx(p_pad=(1 << 24) + 128)
    assert rc == -2 and b"2^24" in msg
    for n in (257, 0, -1):
        rc, msg = dx(n=n)
        assert rc == -1 and b"outside [1, p_pad = 256]" in msg, n
    rc, msg = dx(max_blocks=-1)
    assert rc == -1 and b"max_blocks" in msg
    for name in ("dA0", "dA5", "dV0"):
        rc, msg = dx(**{name: 4096 + 4})
        assert rc == -1 and b"aligned" in msg, name
    # the ray gradient: n_rays, NULL, widths, n_samples
    def rgrad(d_x=4096, pts_ch=63, views_ch=27, rays=8192, z=12288, n=4, S=64, d_rays=16384):
        rc = lib.idealnerf_ray_grad(d_x, pts_ch, views_ch, rays, z, n, S, d_rays, None)
        return rc, lib.idealnerf_last_error()

    rc, msg = rgrad(n=-1)
    assert rc == -1 and b"n_rays < 0" in msg
    assert rgrad(n=0)[0] == 0 and rgrad(n=0, d_x=None, S=0, pts_ch=4)[0] == 0
    for name in ("d_x", "rays", "z", "d_rays"):
        rc, msg = rgrad(**{name: None})
        assert rc == -1 and b"ray_grad: NULL" in msg, name
    for kw in (dict(pts_ch=4), dict(views_ch=4), dict(pts_ch=27, views_ch=4), dict(pts_ch=4, views_ch=27), dict(pts_ch=69), dict(views_ch=33),
               dict(pts_ch=0), dict(views_ch=-3)):
        rc, msg = rgrad(**kw)
        assert rc == -1 and b"row widths" in msg, kw
    for S in (-1, 0, 1, 513, 1024):
        for kw in ({}, dict(pts_ch=27, views_ch=15), dict(pts_ch=3, views_ch=3)):
            rc, msg = rgrad(S=S, **kw)
            assert rc == -2 and b"n_samples" in msg and b"[2, 512]" in msg, (S, kw)
    # the fold's backward: params, conditioning pointers against the widths, a partial set of gradient tensors, NULL bias gradients
    def fold(p=fp_, dims=(64, 76, 32), cond=(4096, 8192, 12288), db=(16384, 20480, 24576), gw=(28672, 32768, 36864), d=(None, None, None)):
        if p is not None:
            p.dim_aud, p.dim_expr, p.dim_latent = dims
        rc = lib.idealnerf_fold_bwd(None if p is None else C.byref(p), *cond, *db, *gw, *d, None)
        return rc, lib.idealnerf_last_error()

    rc, msg = fold(p=None)
    assert rc == -1 and b"params is NULL" in msg
    for cond in ((None, 8192, 12288), (4096, None, 12288), (4096, 8192, None)):
        rc, msg = fold(cond=cond)
        assert rc == -1 and b"conditioning pointers" in msg, cond
    rc, msg = fold(dims=(106, 0, 0))
    assert rc == -1 and b"conditioning pointers" in msg
    for gw in ((None, 32768, 36864), (28672, None, 36864), (28672, 32768, None), (28672, None, None), (None, 32768, None), (None, None, 36864)):
        rc, msg = fold(gw=gw)
        assert rc == -1 and b"of the three gradient tensors" in msg, gw
        rc, msg = fold(gw=gw, dims=(0, 0, 0), cond=(None, None, None))
        assert rc == -1 and b"of the three gradient tensors" in msg, gw
    rc, msg = fold(dims=(106, 0, 0), cond=(4096, None, None), d=(None, 4096, None))
    assert rc == -1 and b"does not have" in msg
    for db in ((None, 20480, 24576), (16384, None, 24576)):
        for gw in ((28672, 32768, 36864), (None, None, None)):
            rc, msg = fold(db=db, gw=gw)
            assert rc == -1 and b"NULL bias gradient" in msg, (db, gw)
    rc, msg = fold(db=(16384, 20480, None))
    assert rc == -1 and b"views_linears.0" in msg
    rc, msg = fold(db=(16384, 20480, None), gw=(None, None, None), d=(None, 4096, None))
    assert rc == -1 and b"views_linears.0" in msg
    assert fold(dims=(0, 0, 0), cond=(None, None, None), db=(None, None, None))[0] == 0     # nothing to fold: OK, nothing runs
    fp_.dim_aud = fp_.dim_expr = fp_.dim_latent = 0
    # the frozen plan's column sums: a NULL inside a group, p_pad, P, workspace
    cs_bytes = lib.idealnerf_cond_colsums_workspace_bytes()
    assert cs_bytes == 512 * 512 * 8      # 512 row blocks x [2][256] fp64 partial sums

    def colsums(dA0=4096, dA5=8192, dV0=12288, P=100, p_pad=256, db=16384, dbv=20480, ws=24576, nbytes=cs_bytes):
        rc = lib.idealnerf_cond_colsums(dA0, dA5, dV0, P, p_pad, db, dbv, ws, nbytes, None)
        return rc, lib.idealnerf_last_error()

    for kw in (dict(dA0=None), dict(dA5=None), dict(db=None), dict(dV0=None), dict(dbv=None), dict(dA0=None, dA5=None), dict(dA0=None, db=None)):
        rc, msg = colsums(**kw)
        assert rc == -1 and b"NULL pointer inside a pair" in msg, kw
    for p_pad in (0, -128, 100, 192):
        rc, msg = colsums(p_pad=p_pad, P=1)
        assert rc == -1 and b"multiple of 128" in msg, p_pad
    rc, msg = colsums(p_pad=(1 << 24) + 128)
    assert rc == -2 and b"2^24" in msg
    for P in (257, 0, -1):
        rc, msg = colsums(P=P)
        assert rc == -1 and b"outside [1, p_pad = 256]" in msg, P
    assert colsums(dA0=None, dA5=None, db=None, dV0=None, dbv=None, ws=None)[0] == 0         # neither group: nothing runs
    for kw in (dict(nbytes=cs_bytes - 1), dict(nbytes=0), dict(ws=None), dict(ws=24576 + 4)):
        for groups in ({}, dict(dA0=None, dA5=None, db=None), dict(dV0=None, dbv=None)):
            rc, msg = colsums(**kw, **groups)
            assert rc == -4 and b"workspace" in msg, (kw, groups)


def test_product_path_refuses_cpu_tensors(idn):
    x = torch.zeros(4, 90)
    with pytest.raises(idn._lib.IdealNerfError, match="GPU"):
        lib = idn._lib.load()
        idn.ops.facenerf_fwd(torch.zeros(lib.idealnerf_packed_weight_floats(0)), torch.zeros(lib.idealnerf_folded_bias_floats()), x)
    net = idn.FaceNeRF(dim_aud=64, dim_latent=32, dim_expr=76)
    with torch.no_grad(), pytest.raises(idn._lib.IdealNerfError):
        net(x, torch.zeros(64), torch.zeros(76), torch.zeros(32))


def test_facenerf_state_dict_contract(idn):
    for v in (dict(dim_aud=64, dim_expr=76, dim_latent=32), dict(dim_aud=106, dim_expr=0, dim_latent=0),
              dict(dim_aud=64, dim_expr=0, dim_latent=0)):
        net = idn.FaceNeRF(**v)
        shapes = {k: tuple(t.shape) for k, t in net.state_dict().items()}
        assert shapes == oracle.facenerf_param_shapes(oracle.facenerf_dims(**v))
    assert "feature_linear.weight" in shapes  # never applied upstream, still part of checkpoints
    with pytest.raises(NotImplementedError):
        idn.FaceNeRF(D=4)
    with pytest.raises(NotImplementedError):
        idn.FaceNeRF(W=128)


def test_network_contract(idn):
    from idealnerf_amd.audio_exp_nerf import Network, init_weights
    from idealnerf_amd.helper import RenderConfig
    net = Network(450, 450, 1200.0, 0.3, 0.9, 8192, None, 64, 128)  # positional, typo'd N_samlpes included
    tops = sorted(set(k.split(".")[0] for k in net.state_dict()))
    assert tops == ["aud_att_net", "aud_net", "ds_aud_net", "face_nerf_coarse", "face_nerf_fine"]
    ref_keys = {"aud_net.encoder_conv.0.weight", "aud_net.encoder_fc1.2.bias", "aud_att_net.attentionConvNet.8.weight",
                "aud_att_net.attentionNet.0.weight", "ds_aud_net.encoder_fc.0.weight",
                "face_nerf_fine.views_linears.2.bias", "face_nerf_coarse.pts_linears.5.weight"}
    assert ref_keys <= set(net.state_dict())
    assert net.state_dict()["face_nerf_coarse.pts_linears.5.weight"].shape == (256, 491)
    net.apply(init_weights)
    assert float(net.face_nerf_fine.rgb_linear.bias[0]) == pytest.approx(0.01)
    cfg = RenderConfig()
    assert (cfg.N_samples, cfg.N_importance, cfg.perturb, cfg.chunk, cfg.netchunk) == (64, 128, 1.0, 8192, 65536)


def test_draw_randoms_follow_reference_rules(idn):
    from idealnerf_amd.audio_exp_nerf import Network
    t, u = Network.draw_randoms(5, 64, 128, 0.0, False, "cpu")
    assert t is None and torch.equal(u, torch.linspace(0.0, 1.0, 128))
    t, u = Network.draw_randoms(5, 64, 128, 1.0, True, "cpu")  # reference's pytest=True: numpy seed 0 for both
    np.random.seed(0)
    assert np.array_equal(t.numpy(), np.random.rand(5, 64).astype(np.float32))
    np.random.seed(0)
    assert np.array_equal(u.numpy(), np.random.rand(5, 128).astype(np.float32))
    t, u = Network.draw_randoms(5, 64, 0, 1.0, False, "cpu")
    assert u is None and t.shape == (5, 64)


def test_audio_nets_match_reference(idn, golden):
    from idealnerf_amd.models.audio_net import AudioAttNet, AudioNet, DeepSpeechAudNet
    g = golden("audio_nets")
    nets = {"aud": AudioNet(64, 16), "att": AudioAttNet(), "ds": DeepSpeechAudNet()}
    for tag, m in nets.items():
        sd = {k[len(tag) + 4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(tag + "_sd_")}
        m.load_state_dict(sd, strict=True)
    auds = torch.from_numpy(g["aud_in"])
    with torch.no_grad():
        out8 = nets["aud"](auds)
        np.testing.assert_allclose(out8.numpy(), g["aud_out8"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(nets["aud"](auds[3:4]).numpy(), g["aud_out1"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(nets["att"](out8).numpy(), g["att_out"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(nets["ds"](auds[3:4]).numpy(), g["ds_out"], rtol=1e-5, atol=1e-6)


def test_get_embedder_matches_golden(idn, golden):
    from idealnerf_amd.helper import get_embedder
    g = golden("pe")
    for L, key in ((10, "pe10"), (4, "pe4"), (3, "pe3")):
        fn, dim = get_embedder(L, 0)
        out = fn(torch.from_numpy(g["x"]))
        assert dim == g[key].shape[1]
        np.testing.assert_array_equal(out.numpy(), g[key])


def test_row_bands_tile_the_frame(idn):
    from idealnerf_amd.parallel import all_bands
    for H in (512, 450, 7, 8, 9):
        for world in (1, 2, 3, 4, 8):
            b = all_bands(H, world)
            assert b[0][0] == 0 and b[-1][1] == H
            assert all(b[i][1] == b[i + 1][0] for i in range(world - 1))
            sizes = [y - x for x, y in b]
            assert max(sizes) - min(sizes) <= 1
    assert all_bands(512, 8) == [(64 * r, 64 * r + 64) for r in range(8)]


def _gloo_worker(rank, world, H, port, ok):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from idealnerf_amd.parallel import gather_rows, row_band
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        W = 6
        full = torch.arange(H * W * 3, dtype=torch.float32).reshape(H, W, 3)
        r0, r1 = row_band(H, rank, world)
        out = gather_rows(full[r0:r1].clone(), H)
        ok[rank] = int(torch.equal(out, full))
    finally:
        dist.destroy_process_group()


def _gloo_grad_worker(rank, world, port, ok):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from idealnerf_amd.parallel import average_gradients
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        torch.manual_seed(0)
        ps = [torch.nn.Parameter(torch.zeros(3, 5)), torch.nn.Parameter(torch.zeros(7)), torch.nn.Parameter(torch.zeros(2, 2))]
        ps[0].grad = torch.full((3, 5), float(rank + 1))
        ps[1].grad = torch.arange(7, dtype=torch.float32) * (rank + 1)
        if rank == 0:
            ps[2].grad = torch.ones(2, 2)            # rank 1 never touched this parameter
        average_gradients(ps)
        good = (torch.allclose(ps[0].grad, torch.full((3, 5), 1.5)) and
                torch.allclose(ps[1].grad, torch.arange(7, dtype=torch.float32) * 1.5) and
                torch.allclose(ps[2].grad, torch.full((2, 2), 0.5)))
        ok[rank] = int(good)
    finally:
        dist.destroy_process_group()


def test_average_gradients_gloo_two_ranks():
    """Data-parallel training: one bucketed all-reduce averages every gradient, missing ones count as zero."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ok = ctx.Array("i", [0, 0])
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_gloo_grad_worker, args=(r, 2, port, ok)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert list(ok) == [1, 1]


@pytest.mark.parametrize("world,H", [(2, 8), (2, 9), (8, 450), (8, 512)])
def test_gather_rows_gloo(world, H):
    """N>1 path on CPU: the ranks render disjoint row bands and all-gather them -- two ranks (even and uneven split), and
    the eight ranks of BASELINE configs[3] on the reference's real frame height 450 (bands of 57 and 56 rows:
    audio_exp_nerf.py:453) and on the bench's 512 (equal bands: the gathered buffer is returned as the frame)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ok = ctx.Array("i", [0] * world)
    port = 29500 + (os.getpid() + 7 * H + world) % 2000
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, H, port, ok)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    assert list(ok) == [1] * world


def test_inline_asm_loads_are_never_touched_in_flight(tmp_path):
    """The MLP kernels read weight fragments with inline-asm ds_read_b128 retired by counted waits
    (DESIGN.md): compile both kernels to ISA and check that no compiler-generated instruction
    reads or writes a destination register while its read is still in flight
    (tools/audit_asm_loads.py; a dangling prefetch once let hipcc reuse such registers as a
    global address -> memory fault)."""
    import concurrent.futures
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        import torch
        assert not torch.cuda.is_available(), "a GPU box without hipcc: the counted waits of the kernels it runs cannot be audited"
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "ideal-nerf_amd", "csrc")

    def compile_s(name):
        out = tmp_path / (name + ".s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                        "--cuda-device-only", os.path.join(csrc, name + ".hip"), "-o", str(out)], check=True)
        return str(out)

    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        files = list(ex.map(compile_s, ["mlp_f32", "mlp_bf16x3", "mlp_bf16x6", "render_fused", "mlp_f32_bwd", "train", "dw_gemm"]))
    for f in files:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_loads.py"), f, ""],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        assert "0 suspicious touches" in r.stdout
        # every device function is inlined into its kernel: a real call passes the register-resident layer state through
        # scratch memory (a generic lambda called eight times was once left out of line: 11x slower, same results)
        isa = open(f).read()
        assert "s_swappc_b64" not in isa, f    # (s_setpc_b64 alone is a long branch, not a return)
    # the auditor's second check (inline-asm VALU reading a VGPR an MFMA has just written: the
    # plain-bf16 kernel keeps its accumulators in VGPRs) must fire on a known-bad sequence
    bad = tmp_path / "bad.s"
    bad.write_text("_Z11fake_kernelv:\n\tv_mfma_f32_32x32x16_bf16 v[0:15], v[20:23], v[24:27], v[0:15]\n"
                   "\t;;#ASMSTART\n\tv_max_f32 v3, 0, v3\n\t;;#ASMEND\n\ts_endpgm\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_loads.py"), str(bad)],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "written by an MFMA" in r.stdout
    # the first check follows branches: a read that is only retired on the fall-through path is caught on the taken one
    loop = tmp_path / "loop.s"
    loop.write_text("_Z12fake_kernel2v:\n.LBB0_1:\n\t;;#ASMSTART\n\tds_read_b128 v[0:3], v9\n\t;;#ASMEND\n"
                    "\ts_cbranch_scc1 .LBB0_3\n\t;;#ASMSTART\n\ts_waitcnt lgkmcnt(0)\n\t;;#ASMEND\n"
                    ".LBB0_3:\n\tv_add_f32_e32 v8, v1, v8\n\ts_cbranch_scc0 .LBB0_1\n\ts_endpgm\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_loads.py"), str(loop)],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "still in flight" in r.stdout
    ok = tmp_path / "ok.s"
    ok.write_text(loop.read_text().replace("s_cbranch_scc1 .LBB0_3\n", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_loads.py"), str(ok)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    # the same for inline-asm buffer loads into registers, retired by counted vmcnt waits (the bf16 dW GEMM reloads
    # its row registers in place): a copy of a register whose load is still in flight is flagged, a copy behind the
    # counted wait that covers it is not
    vm = tmp_path / "vm.s"
    vm.write_text("_Z12fake_kernel3v:\n.LBB0_1:\n\t;;#ASMSTART\n\tbuffer_load_dword v5, v1, s[8:11], s24 offen\n\t;;#ASMEND\n"
                  "\t;;#ASMSTART\n\tbuffer_load_dword v6, v1, s[8:11], s25 offen\n\t;;#ASMEND\n"
                  "\t;;#ASMSTART\n\ts_waitcnt vmcnt(1)\n\t;;#ASMEND\n"
                  "\tv_mov_b32_e32 v7, v6\n\t;;#ASMSTART\n\ts_waitcnt vmcnt(0)\n\t;;#ASMEND\n\ts_cbranch_scc0 .LBB0_1\n\ts_endpgm\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_loads.py"), str(vm)], capture_output=True, text=True)
    assert r.returncode == 1 and "asm load at line" in r.stdout, r.stdout
    vm.write_text(vm.read_text().replace("v_mov_b32_e32 v7, v6", "v_mov_b32_e32 v7, v5"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_loads.py"), str(vm)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    # third check: a counted vmcnt in front of a slice barrier (the training kernels keep their row stores in flight
    # across it) must not reach back into the LDS-DMA pieces: three stores since the last piece cannot justify vmcnt(4),
    # on the path that skips the fourth one
    cw = tmp_path / "cw.s"
    cw.write_text("_Z16fake_mlp_kernel4v:\n.LBB0_1:\n\tbuffer_load_dwordx4 v36, s[8:11], s28 offen lds\n"
                  "\tglobal_store_dwordx4 v[0:1], v[2:5], off\n\tglobal_store_dwordx4 v[0:1], v[2:5], off offset:16\n"
                  "\tglobal_store_dwordx4 v[0:1], v[2:5], off offset:32\n\ts_cbranch_scc1 .LBB0_2\n"
                  "\tglobal_store_dwordx4 v[0:1], v[2:5], off offset:48\n.LBB0_2:\n"
                  "\t;;#ASMSTART\n\ts_waitcnt vmcnt(4)\n\t;;#ASMEND\n\ts_barrier\n\ts_cbranch_scc0 .LBB0_1\n\ts_endpgm\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_loads.py"), str(cw)], capture_output=True, text=True)
    assert r.returncode == 1 and "a piece may still be in flight" in r.stdout, r.stdout
    cw.write_text(cw.read_text().replace("\ts_cbranch_scc1 .LBB0_2\n", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_loads.py"), str(cw)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout


def test_config_files_parse_like_the_reference(idn):
    """Every shipped audio_expr_nerf config, resolved by the reference's own parser (golden), vs
    idealnerf_amd.config: same values, and the same files are rejected (stale keys)."""
    import json
    from idealnerf_amd import config
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "configs_parsed.json")))
    assert len(gold) >= 20
    n_rejected = 0
    for rel, g in gold.items():
        text = "\n".join(g["lines"])
        if g["parsed"] is None:
            n_rejected += 1
            with pytest.raises(ValueError):
                config.load_config(text=text)
            continue
        ns = config.load_config(text=text)
        got = {k: v for k, v in vars(ns).items() if k != "config"}
        assert got == g["parsed"], rel
    assert n_rejected >= 1
    # prefix matching, CLI override, render subset
    ns = config.load_config(text="N_sample=32\nN_importance = 16\nnear=0.5\ndim_aud=64\n# comment\n", argv=["--perturb", "0"])
    assert (ns.N_samples, ns.N_importance, ns.near, ns.perturb, ns.chunk) == (32, 16, 0.5, 0.0, 8192)
    rc = config.to_render_config(ns)
    assert (rc.N_samples, rc.dim_aud, rc.perturb, rc.dim_latent) == (32, 64, 0.0, 32)
    with pytest.raises(ValueError):
        config.load_config(text="no_such_flag=1\n")


def test_fused_arrangement_flag_is_validated(idn):
    """`fused=` / IDN_FUSED_MARCH: 0, 1, 2, False, True and "split" are the arrangements; anything else is named (round 3:
    IDN_FUSED_MARCH=split raised ValueError at import, =3 an EINVAL from the C side on every render)."""
    f = idn.ops._fused_code
    assert [f(v, "x") for v in (0, 1, 2, False, True, "split", "0", "1", "2", " Split ")] == [0, 1, 2, 0, 1, 2, 0, 1, 2, 2]
    for bad in (3, -1, "both", "", None, 1.5):
        with pytest.raises(idn._lib.IdealNerfError, match="must be one of"):
            f(bad, "fused")
    env = dict(os.environ, IDN_FUSED_MARCH="sideways", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", "import idealnerf_amd"], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "IDN_FUSED_MARCH must be one of" in r.stderr
    r = subprocess.run([sys.executable, "-c", "import idealnerf_amd; print(idealnerf_amd.ops.FUSED_MARCH_DEFAULT)"],
                       env=dict(env, IDN_FUSED_MARCH="split"), capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "2", r.stderr


def _smoother_network(idn, g, dev):
    from idealnerf_amd.audio_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    net = Network(12, 12, float(g["focal"]), 0.5772005200386048, 1.1772005200386046, 512, None, 64, 128,
                  args=RenderConfig(perturb=0.0, chunk=512, near=0.5772005200386048, far=1.1772005200386046))
    net.aud_net.load_state_dict({k[len("audnet."):]: T(v) for k, v in g.items() if k.startswith("audnet.")})
    net.aud_att_net.load_state_dict({k[len("attnet."):]: T(v) for k, v in g.items() if k.startswith("attnet.")})
    return net.to(dev).eval()


def _smoother_data(g, idx):
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return (torch.zeros(1, 2, 1, 3), torch.zeros(1, 3), T(g["bg"])[None], T(g["auds"])[None], torch.zeros(1, 12, 12, 3), T(g["pose"])[None],
            T(g["expr"])[None], T(g["latent"]), torch.tensor([idx]))


def test_forward_smoother_window_matches_the_reference(idn):
    """`Network.forward` behind `nosmo_iters` (audio_exp_nerf.py:235-264): the window of eight DeepSpeech frames around `index`,
    zero-padded at the clip's ends, AudioNet on the window, AudioAttNet on its output.  Golden = the reference's own forward
    (tests/golden/smoother.npz: the audio feature it hands to its renderer for a frame at the start, in the middle and at the
    end of a 10-frame clip); here on the CPU with the renderer stubbed out -- the render itself is held to the same fixture in -m gpu."""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "smoother.npz")))
    net = _smoother_network(idn, g, "cpu")
    seen = {}
    net.render_dynamic_face = lambda *a, **k: seen.update(aud=k["aud_para"].detach().clone(), expr=k["expr"]) or [None] * 5
    for idx in g["frames"]:
        with torch.no_grad():
            net([_smoother_data(g, int(idx)), int(g["nosmo_iters"]), 10])
        np.testing.assert_allclose(seen["aud"].numpy(), g[f"aud_feature_{int(idx)}"], rtol=1e-5, atol=1e-6, err_msg=f"frame {idx}")
        assert seen["expr"].shape == (76,)
    # one step before the switch the feature is AudioNet's of the frame's own window
    with torch.no_grad():
        net([_smoother_data(g, 5), int(g["nosmo_iters"]) - 1, 10])
        own = net.aud_net(torch.from_numpy(g["auds"])[5:6])
    assert torch.allclose(seen["aud"], own) and not np.allclose(own.numpy(), g["aud_feature_5"], atol=1e-3)


@pytest.fixture
def process_flags():
    """Tests that parse flags into the process-wide slot leave it, sys.argv and helper.args as they found them."""
    from idealnerf_amd import config, helper
    argv, cur = list(sys.argv), dict(config._current)
    yield config
    sys.argv[:] = argv
    config._current.clear()
    config._current.update(cur)
    for k in ("args", "parser"):
        vars(helper).pop(k, None)


def test_unchanged_caller_gets_its_config(idn, tmp_path, process_flags):
    """The reference's caller, unchanged but for the import line (audio_exp_nerf.py:14,25-26,479-480): `from ...helper import *`
    parses `sys.argv` (helper.py:141-142), and `Network(H, W, focal, near=..., ..., N_samlpes=..., N_importance=...)` -- no
    `args=` -- builds the networks the `--config` file names: obama3's paper model has dim_expr 79 and its own near / far,
    not the May constants (round 3: the call silently got RenderConfig() defaults)."""
    import json
    config = process_flags
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "configs_parsed.json")))
    rel = "NeRFs/HeadNeRF/configs/audio_expr_nerf/obama3/paper_model/torso_bg.txt"
    cfg = tmp_path / "torso_bg.txt"
    cfg.write_text("\n".join(gold[rel]["lines"]))
    sys.argv[:] = ["audio_exp_nerf.py", "--config", str(cfg), "--N_rand", "1024"]
    scope = {}
    exec("from idealnerf_amd.helper import *\nfrom idealnerf_amd.audio_exp_nerf import Network\n"
         "parser = config_parser()\nargs = parser.parse_args()\n"
         "network = Network(450, 450, 1200., near=args.near, far=args.far, chunk=args.chunk, intrinsic=None,\n"
         "                  N_samlpes=args.N_samples, N_importance=args.N_importance)\n", scope)
    args, net = scope["args"], scope["network"]
    want = dict(gold[rel]["parsed"], N_rand=1024)               # the command line outranks the file
    assert {k: v for k, v in vars(args).items() if k != "config"} == want and args.config == str(cfg)
    assert (args.dim_expr, args.near, args.far) == (79, gold[rel]["parsed"]["near"], gold[rel]["parsed"]["far"]) and args.near != 0.3
    assert (net.args.dim_aud, net.args.dim_expr, net.args.near, net.args.far, net.args.perturb) == (64, 79, args.near, args.far, args.perturb)
    assert net.face_nerf_coarse.pts_linears[0].weight.shape == (256, 63 + 64 + 79 + 32)
    assert net.face_nerf_fine.views_linears[0].weight.shape == (128, 27 + 256 + 79)
    for name in ("nn", "F", "np", "torch", "get_embedder", "get_rays", "sample_pdf", "img2mse", "mse2psnr", "to8b", "write_config"):
        assert name in scope, name                                # what upstream's scripts take from the star import
    # the module attributes are upstream's import-time globals, evaluated on first access
    from idealnerf_amd import helper
    assert helper.args.dim_expr == 79 and helper.args is helper.args
    # an explicit RenderConfig that contradicts the parsed config is refused by name, not rendered
    from idealnerf_amd.audio_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    with pytest.raises(ValueError, match="dim_expr: config 79 != network 76"):
        Network(450, 450, 1200., 0.3, 0.9, 8192, None, 64, 128, args=RenderConfig())
    Network(450, 450, 1200., 0.3, 0.9, 8192, None, 64, 128, args=RenderConfig(dim_expr=79))
    # stale keys end the run as upstream's parser does (several shipped configs carry `use_highlight`)
    bad = tmp_path / "bad.txt"
    bad.write_text("dim_aud = 64\nuse_highlight = True\n")
    with pytest.raises(SystemExit):
        helper.config_parser().parse_args(["--config", str(bad)])
    # without any flags anywhere the paper model's dimensions are used (and said so)
    config.set_current_args(None)
    sys.argv[:] = ["pytest"]
    assert Network(32, 32, 100., 0.3, 0.9, 512, None, 64, 128).args.dim_expr == 76
    # ... and with --config on the command line but no parse_args() call, the command line is parsed as upstream does on import
    sys.argv[:] = ["eval.py", "--config", str(cfg), "--my_own_flag", "7"]     # (a flag of the caller's own does not break the implicit path)
    assert Network(32, 32, 100., 0.3, 0.9, 512, None, 64, 128).args.dim_expr == 79


def test_unchanged_torso_caller_gets_its_config(idn, tmp_path, process_flags):
    """NeRFs/TorsoNeRF/train_torso.py's constructor call (:185,200-221) with the TorsoNeRF parser's flags
    (run_nerf_helpers.py:231-365): dim_aud / dim_aud_body from the config, the head pair's dim_expr 79 a literal."""
    cfg = tmp_path / "torso.txt"
    cfg.write_text("N_samples = 64\nN_importance = 128\nchunk = 1024\nperturb = 0.0\nwin_size = 16\ndim_aud = 76\ndim_aud_body = 32\n"
                   "near = 0.55\nfar = 1.15\nuse_highlight = True\n")
    from idealnerf_amd import train_torso
    args = train_torso.config_parser().parse_args(["--config", str(cfg)])
    assert (args.dim_aud, args.dim_aud_body, args.chunk, args.testskip, args.lrate, args.use_highlight) == (76, 32, 1024, 1, 5e-4, True)
    net = train_torso.Network(450, 450, 1200., args.near, args.far, args.chunk, args.N_samples, args.N_importance)
    assert (net.args.dim_aud, net.args.dim_expr, net.dim_aud_body, net.args.perturb) == (76, 79, 32, 0.0)
    assert net.face_nerf_coarse.pts_linears[0].weight.shape == (256, 63 + 76 + 79 + 32)
    assert net.torso_fine_nerf.pts_linears[0].weight.shape == (256, 63 + 32 + 42)
    assert net.aud_net.encoder_fc1[-1].out_features == 76 if hasattr(net.aud_net, "encoder_fc1") else True


def test_checkpoint_round_trip_and_adnerf_warm_start(idn, tmp_path):
    from idealnerf_amd import checkpoint, train as T_
    from idealnerf_amd.audio_exp_nerf import Network
    torch.manual_seed(0)
    net = Network(32, 32, 100.0, 0.3, 0.9, 512, None, 64, 128)
    lat = torch.randn(5, 32, requires_grad=True)
    opt = T_.make_optimizer(net, lat)
    run = tmp_path / "logs" / "exp"
    for step in (5000, 10000, 900):
        checkpoint.save_checkpoint(str(run / f"head_{step}.tar"), net, opt, lat, step)
    assert checkpoint.latest_checkpoint(str(run)).endswith("head_10000.tar")  # natural, not lexical, order
    assert checkpoint.latest_checkpoint(str(tmp_path / "nope")) is None
    ck = torch.load(str(run / "head_900.tar"), weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer", "latent_codes"}
    net2 = Network(32, 32, 100.0, 0.3, 0.9, 512, None, 64, 128)
    step, lat2 = checkpoint.load_checkpoint(str(run / "head_10000.tar"), net2, T_.make_optimizer(net2, torch.zeros(5, 32, requires_grad=True)))
    assert step == 10000 and torch.equal(lat2, lat.data)
    for (k, a), (_, b) in zip(net.state_dict().items(), net2.state_dict().items()):
        assert torch.equal(a, b), k
    # AD-NeRF checkpoint: audio only network (input widths 127 / 383 / 283), first/skip/view layers dropped
    ad = idn.FaceNeRF(dim_aud=64, dim_latent=0, dim_expr=0)
    ft = {"network_fn_state_dict": ad.state_dict(), "network_fine_state_dict": ad.state_dict(),
          "network_audnet_state_dict": net.aud_net.state_dict(), "network_audattnet_state_dict": net.aud_att_net.state_dict()}
    net3 = Network(32, 32, 100.0, 0.3, 0.9, 512, None, 64, 128)
    before = net3.face_nerf_coarse.pts_linears[0].weight.clone()
    checkpoint.load_adnerf_finetune(ft, net3)
    assert torch.equal(net3.face_nerf_coarse.pts_linears[3].weight, ad.pts_linears[3].weight)
    assert torch.equal(net3.face_nerf_coarse.pts_linears[0].weight, before)  # width differs: kept as initialised


def test_pixel_selection_matches_reference_sampler(idn, golden):
    """Region-weighted pixel selection (GetData.sample_rays) against the reference run with the
    same numpy seed: identical pixels in identical order (checked through the gathered targets
    and backgrounds, which are unique per pixel)."""
    from idealnerf_amd.dataset import select_pixels
    g = golden("sample_rays")
    H, W = g["parse"].shape[:2]
    np.random.seed(int(g["seed"]))
    sel = select_pixels(H, W, g["rect"], g["landmark"], g["parse"], int(g["N_rand"]), int(g["mouth_rays"]),
                        int(g["torso_rays"]), float(g["sample_rate"]))
    assert sel.shape == (96, 2)
    np.testing.assert_array_equal(g["target"][sel[:, 0], sel[:, 1]], g["target_s"])
    np.testing.assert_array_equal(g["bc"][sel[:, 0], sel[:, 1]], g["bc_s"])
    # rays of those pixels with the dataset's principal point (oracle = reference get_rays restated)
    ro, rd = oracle.camera_rays(H, W, float(g["focal"]), torch.from_numpy(g["pose"]).float(), float(g["cx"]), float(g["cy"]))
    np.testing.assert_allclose(rd.numpy()[sel[:, 0], sel[:, 1]], g["batch_rays"][1], rtol=1e-6, atol=1e-7)


def test_dataset_reader_on_synthetic_directory(idn, tmp_path):
    """The on-disk format end to end with a tiny generated dataset (no GPU: pixel selection, metadata,
    audio window table, natural fields of the 8-tuple up to the device-side ray gather)."""
    from PIL import Image
    from idealnerf_amd import dataset
    from types import SimpleNamespace
    rs = np.random.RandomState(0)
    H = W = 64
    d = tmp_path / "May"
    for sub in ("head_imgs", "ori_imgs", "parsing"):
        (d / sub).mkdir(parents=True)
    frames = []
    for i in range(3):
        Image.fromarray(rs.randint(0, 255, (H, W, 3), dtype=np.uint8)).save(d / "head_imgs" / f"{i}.jpg")
        par = np.zeros((H, W, 3), np.uint8); par[50:, 4:60] = (255, 0, 0)
        Image.fromarray(par).save(d / "parsing" / f"{i}.png")
        lms = rs.uniform(6, 58, (68, 2)); lms[48:] = rs.uniform(28, 36, (20, 2))
        np.savetxt(d / "ori_imgs" / f"{i}.lms", lms)
        frames.append({"img_id": i, "aud_id": i + 5, "transform_matrix": np.eye(4).tolist(), "face_rect": [4, 4, 50, 50],
                       "exp": rs.standard_normal(76).tolist()})
    Image.fromarray(rs.randint(0, 255, (H, W, 3), dtype=np.uint8)).save(d / "bc.jpg")
    np.save(d / "aud.npy", rs.standard_normal((6, 16, 29)).astype(np.float32))
    json_meta = {"focal_len": 100.0, "cx": W / 2, "cy": H / 2, "frames": frames}
    import json
    for mode in ("train", "val"):
        (d / f"transforms_exp_{mode}.json").write_text(json.dumps(json_meta))
    args = SimpleNamespace(gt_dirs="head_imgs", testskip=2, N_rand=64, sample_rate=0.95, mouth_rays=8, torso_rays=4)
    ds = dataset.GetData(str(d), "aud.npy", "train", args, device="cpu")
    assert len(ds) == 3 and (ds.H, ds.W, ds.focal) == (64, 64, 100.0)
    assert ds.auds.shape == (3, 16, 29)
    assert torch.equal(ds.auds[1], torch.from_numpy(np.load(d / "aud.npy")[5]))   # aud_id clamped to the table
    np.random.seed(3)
    sel = dataset.select_pixels(H, W, ds.all_face_rects[0], np.loadtxt(ds.all_landmarks[0]),
                                np.asarray(Image.open(ds.all_parse_imgs[0])), 64, 8, 4, 0.95)
    assert sel.shape == (64, 2) and len({tuple(r) for r in sel[:49]}) == 49       # no replacement inside a region
    with pytest.raises(idn._lib.IdealNerfError):
        ds[0]  # ray generation is a device kernel: a CPU dataset must fail loudly, not fall back


# --------------------------------------------------------------------------- 8(f) items 3 and 4 (host side)
def test_raw_avi_writer_round_trip(tmp_path):
    """The container FrameSink writes: RIFF/AVI, 'DIB ' BI_RGB 24-bit, bottom-up rows padded to 4 bytes."""
    import struct
    from idealnerf_amd.frame_io import RawAviWriter
    H, W, N = 6, 5, 3  # W*3 = 15 -> padded rows of 16 bytes
    rs = np.random.RandomState(0)
    frames = [rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(N)]
    path = str(tmp_path / "v.avi")
    w = RawAviWriter(path, W, H, fps=25.0)
    for f in frames:
        w.write(f)
    w.release()
    blob = open(path, "rb").read()
    assert blob[:4] == b"RIFF" and blob[8:12] == b"AVI " and struct.unpack("<I", blob[4:8])[0] == len(blob) - 8
    avih = blob.index(b"avih")
    usec, _, _, flags, total, _, streams, _, width, height = struct.unpack("<10I", blob[avih + 8: avih + 48])
    assert (usec, total, streams, width, height) == (40000, N, 1, W, H) and flags & 0x10
    strf = blob.index(b"strf")
    size, bw, bh, planes, bits, comp = struct.unpack("<IiiHHI", blob[strf + 8: strf + 28])
    assert (size, bw, bh, planes, bits, comp) == (40, W, H, 1, 24, 0)
    pos = blob.index(b"movi") + 4
    for f in frames:
        assert blob[pos:pos + 4] == b"00db" and struct.unpack("<I", blob[pos + 4:pos + 8])[0] == 16 * H
        rows = np.frombuffer(blob[pos + 8: pos + 8 + 16 * H], dtype=np.uint8).reshape(H, 16)[:, :15].reshape(H, W, 3)
        np.testing.assert_array_equal(rows[::-1], f)
        pos += 8 + 16 * H
    assert blob[pos:pos + 4] == b"idx1" and struct.unpack("<I", blob[pos + 4:pos + 8])[0] == 16 * N
    with pytest.raises(ValueError):
        RawAviWriter(str(tmp_path / "w.avi"), W, H).write(np.zeros((H, W + 1, 3), np.uint8))


def test_clip_audio_features_match_reference_loop(golden):
    """One batched pass over the clip == the reference's frame-by-frame loop (test_torso.py:478-498),
    including the ends, where the padded slots carry AudioNet(0) rather than zeros."""
    from idealnerf_amd.models import AudioNet, AudioAttNet, clip_audio_features
    g = golden("audio_clip")
    aud_net, att_net = AudioNet(64, 16), AudioAttNet()
    aud_net.load_state_dict({k[len("audnet."):]: torch.from_numpy(g[k]) for k in g if k.startswith("audnet.")})
    att_net.load_state_dict({k[len("attnet."):]: torch.from_numpy(g[k]) for k in g if k.startswith("attnet.")})
    with torch.no_grad():
        out = clip_audio_features(aud_net, att_net, torch.from_numpy(g["auds"]))
    assert out.shape == g["out"].shape == (21, 64)
    assert np.abs(out.numpy() - g["out"]).max() < 2e-6 * max(1.0, np.abs(g["out"]).max())
    with pytest.raises(ValueError):
        clip_audio_features(aud_net, att_net, torch.zeros(5, 16, 29))


# --- the self-launching bench (`python bench.py --gpus N`, the driver's scaling command) ------------

def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("idn_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("n", [2, 8])
def test_bench_plain_start_launches_its_own_ranks(n):
    """`python bench.py --gpus N ...` started as ONE plain process (no torch.distributed.run around it):
    the parent starts N ranks (2, and the 8 of BASELINE configs[3]), they rendezvous over gloo (no GPU here), the flags
    reach the ranks and rank 0's line -- and only that line -- comes back on stdout with every rank's row band."""
    import json
    env = dict(os.environ, IDN_DIST_BACKEND="gloo", OMP_NUM_THREADS="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    size = 9 if n == 2 else 512
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "7", "--warmup", "3",
                        "--size", str(size), "--workload", "rendezvous"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == n and res["ranks"] == n and res["backend"] == "gloo"
    assert res["steps"] == 7 and res["warmup"] == 3
    assert res["bands"] == ([[0, 5], [5, 9]] if n == 2 else [[64 * r, 64 * r + 64] for r in range(8)])


def test_bench_launcher_propagates_a_failed_rank(tmp_path, capsys):
    """A rank that dies makes the parent exit non-zero and print no result line; a run whose ranks all
    succeed but print nothing is a failure too."""
    bench = _bench_module()
    bad = tmp_path / "bad_rank.py"
    bad.write_text("import os, sys, json\n"
                   "if os.environ['RANK'] == '1':\n    sys.exit(3)\n"
                   "print(json.dumps({'metric': 'm', 'value': 1.0}))\n")
    rc = bench.launch_ranks(2, [], script=str(bad), timeout=300)
    out = capsys.readouterr()
    assert rc != 0 and out.out.strip() == ""
    quiet = tmp_path / "quiet_rank.py"
    quiet.write_text("print('hello from a rank')\n")
    rc = bench.launch_ranks(2, [], script=str(quiet), timeout=300)
    out = capsys.readouterr()
    assert rc == 1 and out.out.strip() == "" and "hello from a rank" in out.err
    hang = tmp_path / "hang_rank.py"
    hang.write_text("import os, time\nopen(os.environ['IDN_TEST_PIDFILE'] + os.environ['RANK'], 'w').write(str(os.getpid()))\ntime.sleep(600)\n")
    os.environ["IDN_TEST_PIDFILE"] = str(tmp_path / "pid")
    try:
        t0 = time.time()
        rc = bench.launch_ranks(2, [], script=str(hang), timeout=20)
        out = capsys.readouterr()
        assert rc == 124 and out.out.strip() == "" and time.time() - t0 < 90
        time.sleep(1.0)
        for r in ("0", "1"):      # the ranks went down with the launcher (killed by process-group id)
            pid = int(open(str(tmp_path / "pid") + r).read())
            assert not os.path.exists(f"/proc/{pid}") or open(f"/proc/{pid}/stat").read().split()[2] == "Z", pid
    finally:
        os.environ.pop("IDN_TEST_PIDFILE", None)
    good = tmp_path / "good_rank.py"
    good.write_text("import os, sys, json\n"
                    "assert os.environ['WORLD_SIZE'] == '2' and os.environ['MASTER_ADDR'] == '127.0.0.1'\n"
                    "print('1')\nprint('[3]')\nprint('\"metric\"')\n"   # log fragments that happen to be valid JSON
                    "if os.environ['RANK'] == '0':\n"
                    "    print(json.dumps({'metric': 'm', 'value': 2.0, 'argv': sys.argv[1:]}))\n")
    rc = bench.launch_ranks(2, ["--steps", "4"], script=str(good), timeout=300)
    out = capsys.readouterr()
    assert rc == 0 and len(out.out.strip().splitlines()) == 1
    import json
    assert json.loads(out.out.strip())["argv"] == ["--steps", "4"]


def test_bench_parent_never_touches_the_gpu_before_launching():
    """The launcher branch must run before any torch.cuda / HIP call: in the source, the WORLD_SIZE test
    and launch_ranks() precede every `torch.cuda` use of main(), and launch_ranks itself has none."""
    import inspect
    bench = _bench_module()
    src = inspect.getsource(bench.main)
    assert src.index("launch_ranks(") < src.index("init_ranks(")
    assert "torch.cuda" not in src[:src.index("launch_ranks(")]
    assert "torch.cuda" not in inspect.getsource(bench.launch_ranks).split('"""')[2]
    assert "os.exec" not in open(os.path.join(ROOT, "bench.py")).read()


def test_bench_dump_outputs_keep_every_kth_pixel_under_the_limit(tmp_path):
    """`--dump-outputs`: float32 .npy files of the given shapes while they fit; past the byte limit every array keeps
    the same every-k-th pixel, and all files together stay within the limit."""
    bench = _bench_module()
    g = torch.Generator().manual_seed(0)
    arrays = {"frame_rgb": torch.rand(8, 8, 3, generator=g), "rgb_map": torch.rand(64, 3, generator=g),
              "disp_map": torch.rand(64, generator=g, dtype=torch.float64)}
    assert bench.dump_outputs(str(tmp_path / "all"), arrays) == 1
    for k, v in arrays.items():
        a = np.load(tmp_path / "all" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(v.shape) and np.array_equal(a, v.float().numpy())
    limit = 300   # 64 pixels x (3 + 3 + 1) floats = 1792 bytes: every 7th pixel (10 of them, 280 bytes) is the first stride that fits
    assert bench.dump_outputs(str(tmp_path / "few"), arrays, limit=limit) == 7
    got = {k: np.load(tmp_path / "few" / f"{k}.npy") for k in arrays}
    assert sum(a.nbytes for a in got.values()) <= limit
    assert np.array_equal(got["frame_rgb"], arrays["frame_rgb"].reshape(-1, 3)[::7].numpy())
    assert np.array_equal(got["rgb_map"], arrays["rgb_map"][::7].numpy())
    assert np.array_equal(got["disp_map"], arrays["disp_map"][::7].float().numpy())


def test_bench_refuses_zero_steps():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--workload", "rendezvous"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--steps must be >= 1" in p.stderr


def test_bench_rejects_a_world_size_that_contradicts_gpus():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "rendezvous"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "WORLD_SIZE=3" in p.stderr


def test_ops_validate_shapes_before_the_c_call(idn):
    """Shape errors surface as IdealNerfError before any pointer is taken (so even on CPU tensors); a
    well-shaped CPU call is then refused for its device.  An 8-column ray batch -- which the reference's
    render_rays accepts -- is named as such instead of being read out of bounds."""
    E = idn._lib.IdealNerfError
    ops = idn.ops
    raw, z, rays, bc = torch.zeros(4, 8, 4), torch.zeros(4, 8), torch.zeros(4, 11), torch.zeros(4, 3)
    with pytest.raises(E, match=r"rays must be \[4, 11\], got \[4, 8\]"):
        ops.composite_fwd(raw, z, rays[:, :8].contiguous(), bc)
    with pytest.raises(E, match=r"bc_rgb must be \[4, 3\]"):
        ops.composite_fwd(raw, z, rays, torch.zeros(3, 3))
    with pytest.raises(E, match="must live on the GPU"):
        ops.composite_fwd(raw, z, rays, bc)
    with pytest.raises(E, match=r"x must be \[\*, 90\]"):
        ops.facenerf_fwd(None, None, torch.zeros(5, 63))
    with pytest.raises(E, match="u must be"):
        ops.invert_cdf(torch.zeros(4, 7), torch.zeros(4, 7), torch.zeros(3, 16))
    with pytest.raises(E, match="no CPU fallback"):
        ops.frame_rays(torch.eye(4), 8, 8, 10.0, 0.1, 1.0, device="cpu")
    with pytest.raises(E, match="t_vals"):
        ops.render_rays_fwd(rays, bc, None, None, None, None, torch.zeros(8, 2), None, 0)
    # a list of dW products: the refusals of the C entry, on CPU tensors, before any pointer is taken
    d256, a256, a64, a128 = torch.zeros(256, 256), torch.zeros(256, 256), torch.zeros(256, 64), torch.zeros(256, 128)
    o2, o1 = torch.zeros(300, 300), torch.zeros(300)

    def prod(**kw):
        return dict(dict(delta=d256, N=256, acts=a256, K=256, colsum=True, takes=[(0, 0, 256, 256, o2, 0, 0)]), **kw)

    for bad, kw, match in (
            ([], {}, "products outside"), ([prod()] * 17, dict(pipe=1), "products outside"),
            ([prod()], dict(pipe=2), "pipe 2"), ([prod()], dict(x6_items=0), "x6_items"), ([prod()], dict(x6_items=13), "x6_items"),
            ([prod(N=64, K=64)], {}, "no instantiation for 64 x 64"), ([prod(N=256, K=128)], dict(pipe=1), "no instantiation"),
            ([prod(delta=torch.zeros(128, 256))], {}, r"delta must be \[256, \*\]"),
            ([prod(acts=torch.zeros(128, 256))], {}, r"acts must be \[256, \*\]"),
            ([prod(delta=a128)], {}, "row pitch 128 / 256 < 256 / 256"), ([prod(N=128, K=128, acts=a64)], dict(pipe=1), "row pitch"),
            ([prod(acts2=a256)], dict(pipe=1), "split B"), ([prod(N=128, K=128, acts2=a256)], {}, "split B"),
            ([prod(acts=a64, acts2=a64)], {}, "row pitch 256 / 64 < 256 / 128"), ([prod(acts=a128, acts2=a256)], {}, r"acts2 must be \[256, 128\]"), ([prod(acts2=a128)], {}, r"acts2 must be \[256, 256\]"),
            ([prod(), prod()], dict(x6_items=1), "more 256 x 256 products than x6_items"),
            ([prod(takes=[(0, 0, 1, 1, o2, 0, 0)] * 5)], {}, "5 takes"),
            ([prod(colsum_takes=[(0, 1, o1, 0)] * 3)], {}, "3 column-sum takes"),
            ([prod(N=64, K=128, acts=a128, takes=[(0, 0, 1, 1, o2, 0, 0)] * 4, colsum_takes=[(0, 1, o1, 0)])] * 7, dict(pipe=1), "more than 32 takes"),
            ([prod(takes=[(1, 0, 256, 256, o2, 0, 0)])], {}, "leaves the 256 x 256 block"),
            ([prod(takes=[(0, 200, 3, 57, o2, 0, 0)])], {}, "leaves the 256 x 256 block"),
            ([prod(takes=[(0, 0, 256, 256, o2, 45, 0)])], {}, "does not fit out"),
            ([prod(takes=[(0, 0, 256, 256, o2, 0, 45)])], {}, "does not fit out"),
            ([prod(takes=[(0, 0, 256, 256, o1, 0, 0)])], {}, r"out must be \[\*, \*\]"),
            ([prod(colsum=False, colsum_takes=[(0, 256, o1, 0)])], {}, "kept no column sums"),
            ([prod(colsum_takes=[(1, 256, o1, 0)])], {}, "leaves the 256 columns"),
            ([prod(colsum_takes=[(0, 256, o1, 45)])], {}, "does not fit out")):
        with pytest.raises(E, match=match):
            ops.dw_products(256, bad, **kw)
    for rows in (0, 100, 192):
        with pytest.raises(E, match="multiple of 128"):
            ops.dw_products(rows, [prod()])
    with pytest.raises(E, match="must live on the GPU"):
        ops.dw_products(256, [prod(colsum_takes=[(0, 256, o1, 0)])])
    # the delta chain alone: every shape, dtype and device, on CPU tensors
    lib = idn._lib.load()
    pp = idn._lib.FaceNerfParams()
    slab = lambda rows: torch.zeros(lib.idealnerf_train_acts_floats(rows))
    assert slab(256).numel() == 256 * (2560 + 88)

    def chain(p=pp, pipe=0, acts=None, d_rgb=None, dv0=None, **kw):
        return ops.delta_chain(p, pipe, slab(256) if acts is None else acts, torch.zeros(256, 64) if d_rgb is None else d_rgb,
                               torch.zeros(256, 256) if dv0 is None else dv0, **kw)

    for kw, match in (
            (dict(p=None), "params_struct"), (dict(pipe=2), "pipe 2"), (dict(max_blocks=-1), "max_blocks"), (dict(max_blocks=1.5), "max_blocks"),
            (dict(dv0=torch.zeros(256, 128)), r"dv0 must be \[\*, 256\]"), (dict(dv0=torch.zeros(256 * 256)), r"dv0 must be \[\*, 256\]"),
            (dict(dv0=torch.zeros(192, 256)), "multiple of 128"), (dict(dv0=torch.zeros(0, 256)), "multiple of 128"),
            (dict(acts=slab(128)), r"acts must be \[677888\]"), (dict(acts=slab(256)[:-1]), r"acts must be \[677888\]"),
            (dict(acts=slab(256).reshape(256, -1)), r"acts must be \[677888\]"),
            (dict(d_rgb=torch.zeros(256, 3)), r"d_rgb must be \[256, 64\]"), (dict(d_rgb=torch.zeros(128, 64)), r"d_rgb must be \[256, 64\]"),
            (dict(dv21=torch.zeros(256, 128)), r"dv21 must be \[256, 256\]"), (dict(dv21=torch.zeros(128, 256)), r"dv21 must be \[256, 256\]"),
            (dict(da=torch.zeros(8, 128, 256)), r"da must be \[8, 256, 256\]"), (dict(da=torch.zeros(7, 256, 256)), r"da must be \[8, 256, 256\]"),
            (dict(da=torch.zeros(8 * 256, 256)), r"da must be \[8, 256, 256\]"),
            (dict(acts=slab(256).double()), "acts must be torch.float32"), (dict(d_rgb=torch.zeros(256, 64, dtype=torch.float16)), "d_rgb must be torch.float32"),
            (dict(dv0=torch.zeros(256, 256, dtype=torch.float64)), "dv0 must be torch.float32"),
            (dict(dv21=torch.zeros(256, 256, dtype=torch.int32)), "dv21 must be torch.float32"),
            (dict(da=torch.zeros(8, 256, 256, dtype=torch.bfloat16)), "da must be torch.float32"),
            ({}, "must live on the GPU"), (dict(dv21=torch.zeros(256, 256), da=torch.zeros(8, 256, 256)), "must live on the GPU")):
        with pytest.raises(E, match=match):
            chain(**kw)
    # the compositing backward alone: every shape, column and device, on CPU tensors
    def comp(n=4, S=64, **kw):
        args = dict(raw=torch.zeros(n, S, 4), z=torch.zeros(n, S), rays=torch.zeros(n, 11), bc=torch.zeros(n, 3))
        args.update(kw)
        return ops.composite_bwd(**args)

    m4, m64, m256 = torch.zeros(256, 4), torch.zeros(256, 64), torch.zeros(256, 256)
    for kw, match in (
            (dict(z=torch.zeros(4 * 64)), r"z must be \[\*, \*\]"), (dict(raw=torch.zeros(4, 64, 3)), r"raw must be \[4, 64, 4\]"),
            (dict(raw=None), "raw is None"), (dict(z=None), "z is None"), (dict(rays=torch.zeros(4, 8)), r"rays must be \[4, 11\]"), (dict(bc=torch.zeros(3, 3)), r"bc_rgb must be \[4, 3\]"),
            (dict(g_rgb=torch.zeros(4)), r"g_rgb_map must be \[4, 3\]"), (dict(g_fg=torch.zeros(4, 4)), r"g_rgb_fg must be \[4, 3\]"),
            (dict(g_lw=torch.zeros(4, 1)), r"g_last_weight must be \[4\]"), (dict(g_acc=torch.zeros(5)), r"g_acc must be \[4\]"),
            (dict(S=1), "outside"), (dict(S=513), "outside"),
            (dict(d_rgb=m4), "come together"), (dict(d_sig=m4), "come together"),
            (dict(d_rgb=torch.zeros(4, 64, 4), d_sig=m4), r"d_rgb must be \[\*, \*\]"),
            (dict(d_rgb=torch.zeros(255, 4), d_sig=m4), "fewer than 256 rows"), (dict(d_rgb=m4, d_sig=torch.zeros(255, 4)), "fewer than 256 rows"),
            (dict(d_rgb=torch.zeros(256, 2), d_sig=m4), "fewer than 3 columns"),
            (dict(d_rgb=m4, d_sig=m4, sig_col=4), "sig_col 4"), (dict(d_rgb=m64, d_sig=m256, sig_col=256), "sig_col 256"),
            (dict(d_rgb=m4, d_sig=m4, sig_col=-1), "sig_col -1"), (dict(sig_col=3), "sig_col 3"), (dict(norm_col=6), "norm_col 6"),
            (dict(d_norm=torch.zeros(3, 11)), r"d_norm must be \[4, \*\]"), (dict(d_norm=torch.zeros(4, 11), norm_col=11), "norm_col 11"),
            ({}, "must live on the GPU"), (dict(d_rgb=m64, d_sig=m256, sig_col=128, d_norm=torch.zeros(4, 11), norm_col=6), "must live on the GPU"),
            (dict(raw=torch.zeros(4, 64, 4, dtype=torch.float64)), "must live on the GPU")):
        with pytest.raises(E, match=match):
            comp(**kw)
    # the backward's tail alone: every shape, dtype and device, on CPU tensors
    def dx(p=pp, dA0=m256, dA5=m256, dV0=m256, n=100, **kw):
        return ops.input_grad(p, dA0, dA5, dV0, n, **kw)

    narrow = idn._lib.FaceNerfParams()
    narrow.multires_plus1, narrow.multires_views_plus1 = 5, 3                        # 27 / 15 columns
    for kw, match in (
            (dict(p=None), "params_struct"), (dict(max_blocks=-1), "max_blocks"), (dict(max_blocks=True), "max_blocks"),
            (dict(dA0=torch.zeros(256, 128)), r"dA0 must be \[\*, 256\]"), (dict(dA0=torch.zeros(192, 256)), "multiple of 128"),
            (dict(dA0=torch.zeros(0, 256)), "multiple of 128"), (dict(dA5=torch.zeros(128, 256)), r"dA5 must be \[256, 256\]"),
            (dict(dV0=torch.zeros(256, 129)), r"dV0 must be \[256, 256\]"), (dict(n=257), "n 257 outside"), (dict(n=0), "n 0 outside"),
            (dict(n=2.0), "outside"), (dict(d_x=torch.zeros(100, 63)), r"d_x must be \[100, 90\]"), (dict(d_x=torch.zeros(99, 90)), r"d_x must be \[100, 90\]"),
            (dict(p=narrow, d_x=torch.zeros(100, 90)), r"d_x must be \[100, 42\]"),
            (dict(dA0=m256.double()), "dA0 must be torch.float32"), (dict(dV0=m256.half()), "dV0 must be torch.float32"),
            (dict(d_x=torch.zeros(100, 90, dtype=torch.float64)), "d_x must be torch.float32"),
            ({}, "must live on the GPU"), (dict(d_x=torch.zeros(100, 90)), "must live on the GPU")):
        with pytest.raises(E, match=match):
            dx(**kw)

    def rgrad(n=4, S=64, pts_ch=63, views_ch=27, **kw):
        args = dict(d_x=torch.zeros(n * S, pts_ch + views_ch), rays=torch.zeros(n, 11), z=torch.zeros(n, S), d_rays=torch.zeros(n, 11))
        args.update(kw)
        return ops.ray_grad(args["d_x"], pts_ch, views_ch, args["rays"], args["z"], args["d_rays"])

    for kw, match in (
            (dict(pts_ch=4), "pts_ch 4"), (dict(views_ch=4), "views_ch 4"), (dict(pts_ch=27, views_ch=4), "views_ch 4"),
            (dict(pts_ch=4, views_ch=27), "pts_ch 4"), (dict(pts_ch=69), "pts_ch 69"), (dict(views_ch=33), "views_ch 33"),
            (dict(S=1), "outside"), (dict(S=513), "outside"), (dict(z=None), "is None"), (dict(d_rays=None), "is None"),
            (dict(d_x=None), "d_x is None"), (dict(rays=None), "rays is None"), (dict(z=torch.zeros(256)), r"z must be \[\*, \*\]"),
            (dict(d_x=torch.zeros(256, 63)), r"d_x must be \[256, 90\]"), (dict(d_x=torch.zeros(255, 90)), r"d_x must be \[256, 90\]"),
            (dict(pts_ch=27, views_ch=15, d_x=torch.zeros(256, 90)), r"d_x must be \[256, 42\]"),
            (dict(rays=torch.zeros(4, 8)), r"rays must be \[4, 11\]"), (dict(d_rays=torch.zeros(4, 3)), r"d_rays must be \[4, 11\]"),
            (dict(d_x=torch.zeros(256, 90, dtype=torch.float64)), "d_x must be torch.float32"), (dict(z=torch.zeros(4, 64).half()), "z must be torch.float32"),
            ({}, "must live on the GPU"), (dict(pts_ch=3, views_ch=3, S=2), "must live on the GPU")):
        with pytest.raises(E, match=match):
            rgrad(**kw)

    head = idn._lib.FaceNerfParams()
    head.dim_aud, head.dim_expr, head.dim_latent = 64, 76, 32
    torso = idn._lib.FaceNerfParams()
    torso.dim_aud = 106
    z = torch.zeros

    def fold(p=head, **kw):
        q = head if p is None else p
        args = dict(aud=z(q.dim_aud) if q.dim_aud else None, expr=z(q.dim_expr) if q.dim_expr else None,
                    latent=z(q.dim_latent) if q.dim_latent else None, db0=z(256), db5=z(256), dbv=z(128))
        args.update(kw)
        return ops.fold_bwd(p, **args)

    g0, g5, gv = z(256, 235), z(256, 491), z(128, 359)
    for kw, match in (
            (dict(p=None), "params_struct"), (dict(gW0=g0), "1 of the three"), (dict(gW5=g5), "1 of the three"), (dict(gWv0=gv), "1 of the three"),
            (dict(gW0=g0, gW5=g5), "2 of the three"), (dict(gW0=g0, gWv0=gv), "2 of the three"), (dict(gW5=g5, gWv0=gv), "2 of the three"),
            (dict(aud=None), "aud is None"), (dict(expr=None), "expr is None"), (dict(latent=None), "latent is None"),
            (dict(p=torso, expr=z(76)), "expr is given"), (dict(aud=z(63)), r"aud must be \[64\]"), (dict(expr=z(79)), r"expr must be \[76\]"),
            (dict(p=torso, d_expr=z(76)), "d_expr for a width of 0"), (dict(p=torso, d_latent=z(32)), "d_latent for a width of 0"),
            (dict(d_aud=z(65)), r"d_aud must be \[64\]"), (dict(d_expr=z(3, 76)), r"d_expr must be \[76\]"),
            (dict(db0=None), "is None"), (dict(db5=None), "is None"), (dict(dbv=None, gW0=g0, gW5=g5, gWv0=gv), "is None"),
            (dict(dbv=None, d_expr=z(76)), "is None"), (dict(db0=z(255)), r"db0 must be \[256\]"), (dict(db5=z(1, 256)), r"db5 must be \[256\]"),
            (dict(dbv=z(256)), r"dbv must be \[128\]"), (dict(gW0=z(256, 234), gW5=g5, gWv0=gv), r"gW0 must be \[256, 235\]"),
            (dict(gW0=g0, gW5=z(256, 235), gWv0=gv), r"gW5 must be \[256, 491\]"), (dict(gW0=g0, gW5=g5, gWv0=z(128, 283)), r"gWv0 must be \[128, 359\]"),
            (dict(p=torso, gW0=g0, gW5=g5, gWv0=gv), r"gW0 must be \[256, 169\]"),
            (dict(db0=z(256).double()), "db0 must be torch.float32"), (dict(d_aud=z(64).half()), "d_aud must be torch.float32"),
            ({}, "must live on the GPU"), (dict(gW0=g0, gW5=g5, gWv0=gv, d_aud=z(64), d_expr=z(76), d_latent=z(32)), "must live on the GPU"),
            (dict(p=torso, dbv=None, d_aud=z(106)), "must live on the GPU")):
        with pytest.raises(E, match=match):
            fold(**kw)

    def colsums(dA0=m256, dA5=m256, dV0=m256, P=100, **kw):
        return ops.cond_colsums(dA0, dA5, dV0, P, **kw)

    for kw, match in (
            (dict(dA0=None), "come together"), (dict(dA5=None), "come together"), (dict(dA0=None, dA5=None, dV0=None), "no matrix"),
            (dict(dA0=torch.zeros(256, 128)), r"dA0 must be \[\*, 256\]"), (dict(dA0=None, dA5=None, dV0=torch.zeros(256, 128)), r"dV0 must be \[\*, 256\]"),
            (dict(dA0=torch.zeros(192, 256)), "multiple of 128"), (dict(dA5=torch.zeros(128, 256)), r"dA5 must be \[256, 256\]"),
            (dict(dV0=torch.zeros(384, 256)), r"dV0 must be \[256, 256\]"), (dict(P=257), "P 257 outside"), (dict(P=0), "P 0 outside"),
            (dict(dA0=None, dA5=None, db=torch.zeros(2, 256)), "without its matrices"), (dict(dV0=None, dbv=torch.zeros(128)), "without its matrices"),
            (dict(db=torch.zeros(512)), r"db must be \[2, 256\]"), (dict(dbv=torch.zeros(256)), r"dbv must be \[128\]"),
            (dict(dA5=m256.double()), "dA5 must be torch.float32"), (dict(dbv=torch.zeros(128, dtype=torch.float64)), "dbv must be torch.float32"),
            ({}, "must live on the GPU"), (dict(dA0=None, dA5=None), "must live on the GPU"), (dict(dV0=None, db=torch.zeros(2, 256)), "must live on the GPU")):
        with pytest.raises(E, match=match):
            colsums(**kw)
