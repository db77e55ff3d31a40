"""Shared by tests/test_multires_cpu.py and tests/test_multires_gpu.py (not collected by pytest): networks whose encoding
widths are not the default 10 / 4 octaves.

The oracle takes the widths everywhere (``oracle.facenerf_dims(input_ch=, input_ch_views=)``) except in
``oracle.render_oracle._query``, which writes 10 and 4 literally and which ``render_rays`` / ``render_frame`` (and
tests/parity_proof.py, tests/ray_grad_common.py) look up as a module global.  ``install`` puts a width-aware replacement
there for the duration of a test."""
import torch

import oracle

# (multires, multires_views).  (5, 2): the reference's shipped ablation config -- 33 point columns, one past the 32-column split
# of the input-gradient kernel; (4, 1): 27, below that split; (0, 0): no octave, the raw columns (and ``i_embed = -1``);
# (10, 2) and (3, 4): asymmetric, so that a point / direction mix-up cannot cancel.
PAIRS = [(5, 2), (4, 1), (0, 0), (10, 2), (3, 4)]
CONFIG = "NeRFs/HeadNeRF/configs/audio_expr_nerf/may/ablation/positional_encoding.txt"


def channels(octaves: int) -> int:
    return 3 + 6 * octaves


def dims_of(pair, **cond):
    """oracle.facenerf_dims at the pair's widths (cond: dim_aud / dim_expr / dim_latent, the head model's by default)."""
    return oracle.facenerf_dims(input_ch=channels(pair[0]), input_ch_views=channels(pair[1]), **cond)


def embed(x: torch.Tensor, octaves: int) -> torch.Tensor:
    """gamma_L(x); with no octave the raw 3 columns."""
    return x if octaves == 0 else oracle.positional_encoding(x, octaves)


def query_for(pair):
    """``oracle.render_oracle._query`` for a network of ``pair`` octaves (same signature, same chunking)."""
    L, Lv = pair

    def _query(p, pts, viewdirs, aud, expr, latent, dims, netchunk: int = 1 << 16):
        n, s, _ = pts.shape
        dirs = viewdirs[:, None, :].expand(n, s, 3).reshape(-1, 3)
        emb = torch.cat([embed(pts.reshape(-1, 3), L), embed(dirs, Lv)], dim=-1)
        outs = [oracle.facenerf_forward(p, emb[i:i + netchunk], aud, expr, latent, dims)
                for i in range(0, emb.shape[0], netchunk)]
        return torch.cat(outs, dim=0).reshape(n, s, 4)

    return _query


def install(monkeypatch, pair):
    """The oracle renders networks of ``pair`` octaves until the test ends."""
    monkeypatch.setattr(oracle.render_oracle, "_query", query_for(pair))


def widen(params, pair, dims):
    """The 10 / 4 network that computes what the narrow one does: the same weights, zeros in the columns the narrow one does
    not have (state-dict tensors of a FaceNeRF with ``dims``' conditioning widths)."""
    pc, vc = channels(pair[0]), channels(pair[1])
    out = {k: v.clone() for k, v in params.items()}
    for k in ("pts_linears.0.weight", "pts_linears.5.weight"):
        w = params[k]
        out[k] = torch.cat([w[:, :pc], w.new_zeros(w.shape[0], 63 - pc), w[:, pc:]], dim=1)
    w = params["views_linears.0.weight"]
    W = dims["W"]
    # face_nerf.py:67: [h | gamma(dir) | expr / 3]
    out["views_linears.0.weight"] = torch.cat([w[:, :W + vc], w.new_zeros(w.shape[0], 27 - vc), w[:, W + vc:]], dim=1)
    return out
