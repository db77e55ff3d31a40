"""SSIM as a training term: ``ssim_patch_loss`` on the patch rows of a ray batch (no counterpart upstream, whose image-level
terms -- loss/vgg_loss.py, loss/vgg_face_loss.py, loss/landmark_loss.py -- need external weights), and the host-side recipe
that decides where a step's patches lie (``patch_origins``).

The loss and its gradient are HIP kernels (csrc/ssim_loss.hip): the scorer's index (``ops.frame_scores``) on p x p patches,
all arithmetic beyond the loads in fp64, fixed summation order.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import ops

PATCH_REGIONS = ("rect", "frame")


class _SsimPatchLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_rows, truth_rows, n_patches, p):
        pred, truth = pred_rows.detach().contiguous(), truth_rows.detach().contiguous()
        out = ops.ssim_patch_fwd(pred, truth, n_patches, p)
        ctx.save_for_backward(pred, truth)
        ctx.patches = (int(n_patches), int(p))
        return out[int(n_patches)].to(torch.float32)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        pred, truth = ctx.saved_tensors
        # the incoming scalar enters the kernel as its argument g (a host number: one read of one float), so that every element
        # of the gradient is rounded to fp32 once
        return ops.ssim_patch_bwd(pred, truth, *ctx.patches, g=float(g_out)), None, None, None


def ssim_patch_loss(pred_rows, truth_rows, n_patches, p):
    """1 - mean SSIM of n_patches p x p patches -> float32 scalar with a gradient for ``pred_rows`` only.  pred_rows, truth_rows:
    fp32 [n_patches p p, 3] (or [n_patches, p, p, 3]), the rows a render and a gather return for ``ops.patch_pixels`` -- patch by
    patch, row-major inside a patch.  Each patch's index is the mean over its 3 (p - 10)^2 "valid" 11 x 11 windows, as
    ``ops.frame_scores`` computes it.  Raises ``IdealNerfError`` off the device: there is no CPU path."""
    return _SsimPatchLoss.apply(pred_rows, truth_rows, n_patches, p)


def check_patches(patches):
    """(k, p) of ``patches=`` as two ints; ValueError for anything the kernels do not take."""
    try:
        k, p = (int(v) for v in patches)
    except (TypeError, ValueError):
        raise ValueError(f"patches must be (k, p): k patches of p x p pixels, got {patches!r}") from None
    if not 1 <= k <= ops.PATCH_MAX or not ops.PATCH_MIN_P <= p <= ops.PATCH_MAX_P:
        raise ValueError(f"patches = ({k}, {p}): k must be in 1..{ops.PATCH_MAX} and p in {ops.PATCH_MIN_P}..{ops.PATCH_MAX_P}")
    return k, p


def origin_range(lo, hi, p, size):
    """The top-left coordinates a p-wide patch may take along one axis of `size` pixels so that it lies inside the pixels
    [lo, hi] (inclusive, clipped to the axis) -> (first, count).  Where the clipped range is narrower than p the patch is
    centred on it and clamped to the axis: one coordinate."""
    if p > size:
        raise ValueError(f"a patch of {p} pixels does not fit an axis of {size}")
    lo, hi = max(int(lo), 0), min(int(hi), size - 1)
    if hi - lo + 1 >= p:
        return lo, hi - lo + 1 - p + 1
    return min(max(lo + (hi - lo + 1 - p) // 2, 0), size - p), 1


def patch_origins(seed, frame, draw, k, p, H, W, face_rect=None, region="rect"):
    """The top-left corners [(oy, ox)] * k of draw `draw` on frame `frame`: a function of (seed, frame, draw) alone (and of the
    frame's geometry), computed on the host from a counter-based generator -- numpy's Philox with key = seed and counter =
    (draw, frame, 0, 0) -- so that a resumed run and every rank's draw index reproduce them without any state.

    region = "rect": uniform over the origins for which the patch lies inside the face rect clipped to the frame -- pixel rows
    [face_rect[0], face_rect[0] + face_rect[2]], columns [face_rect[1], face_rect[1] + face_rect[3]], the loader's convention
    (``dataset.region_masks``); along an axis where that is narrower than p the patch is centred on the rect and clamped to the
    frame.  region = "frame": uniform over the frame.  Patches of one draw are drawn independently and may overlap."""
    if region not in PATCH_REGIONS:
        raise ValueError(f"patch_region must be one of {PATCH_REGIONS}, got {region!r}")
    if region == "rect":
        if face_rect is None:
            raise ValueError("patch_region 'rect' needs the frame's face_rect")
        y0, ny = origin_range(face_rect[0], face_rect[0] + face_rect[2], p, H)
        x0, nx = origin_range(face_rect[1], face_rect[1] + face_rect[3], p, W)
    else:
        y0, ny = origin_range(0, H - 1, p, H)
        x0, nx = origin_range(0, W - 1, p, W)
    mask = (1 << 64) - 1
    gen = np.random.Generator(np.random.Philox(key=int(seed) & mask, counter=[int(draw) & mask, int(frame) & mask, 0, 0]))
    picks = gen.integers(0, [ny, nx], size=(int(k), 2))
    return [(y0 + int(a), x0 + int(b)) for a, b in picks]
