"""Shared by tests/test_ssim_loss_cpu.py and tests/test_ssim_loss_gpu.py (not collected by pytest): the fp64 reference of the
patch SSIM loss, the test inputs, ``patch_pixels`` restated in numpy and the measured-maxima record."""
import json
import os

import numpy as np
import torch

C1, C2 = 1e-4, 9e-4
SHAPES = [(k, p) for p in (11, 12, 32, 48) for k in (1, 3)]
CASES = ("uniform", "flat_noise", "equal")
MAXIMA = {}   # what the GPU tests measured, by name: written to $IDN_SSIM_LOSS_RECORD (profiles/ssim_loss_parity.json)


def gauss_taps():
    """The eleven weights as the comment in csrc/metrics.hip says: exp(-(k - 5)^2 / 4.5), normalised in fp64, rounded to fp32."""
    w = np.exp(-(np.arange(11, dtype=np.float64) - 5.0) ** 2 / 4.5)
    return (w / w.sum()).astype(np.float32)


def ssim_patches64(pred, truth, k, p):
    """pred, truth [k, p, p, 3] (any float dtype, any device) -> float64 [k] mean SSIM of each patch on the CPU, differentiable
    in pred: the fp32 weights widened, their outer product in fp64, conv2d in float64, "valid" windows."""
    w = torch.from_numpy(gauss_taps().astype(np.float64))
    win = torch.outer(w, w)[None, None]
    x = pred.reshape(k, p, p, 3).permute(0, 3, 1, 2).reshape(k * 3, 1, p, p)
    t = truth.reshape(k, p, p, 3).permute(0, 3, 1, 2).reshape(k * 3, 1, p, p)
    f = lambda a: torch.nn.functional.conv2d(a, win)
    mx, mt = f(x), f(t)
    vx, vt, cov = f(x * x) - mx * mx, f(t * t) - mt * mt, f(x * t) - mx * mt
    s = ((2.0 * mx * mt + C1) * (2.0 * cov + C2)) / ((mx * mx + mt * mt + C1) * (vx + vt + C2))
    return s.reshape(k, -1).mean(dim=1)


def reference(pred32, truth32, k, p):
    """fp32 inputs (CPU or device) -> (out float64 [k + 1] as idealnerf_ssim_patch_fwd defines it, d loss / d pred float64,
    pred's shape) on the CPU, by torch autograd in fp64."""
    x = pred32.detach().cpu().double().requires_grad_(True)
    t = truth32.detach().cpu().double()
    per_patch = ssim_patches64(x, t, k, p)
    loss = 1.0 - per_patch.mean()
    (g,) = torch.autograd.grad(loss, x)
    return torch.cat([per_patch.detach(), loss.detach()[None]]), g


def inputs(case, k, p, seed=0):
    """-> (pred, truth) fp32 [k, p, p, 3] on the CPU.  uniform: both uniform random; flat_noise: a flat 0.6 truth with
    prediction = truth + sigma-0.02 noise (the cancellation case: E[tt] - mu_t^2 is zero up to rounding); equal: pred == truth."""
    gen = torch.Generator().manual_seed(1000 * p + 10 * k + seed)
    if case == "uniform":
        return torch.rand((k, p, p, 3), generator=gen), torch.rand((k, p, p, 3), generator=gen)
    if case == "flat_noise":
        truth = torch.full((k, p, p, 3), 0.6)
        return truth + 0.02 * torch.randn((k, p, p, 3), generator=gen), truth
    if case == "equal":
        truth = torch.rand((k, p, p, 3), generator=gen)
        return truth.clone(), truth
    raise ValueError(case)


def patch_pixels_reference(origins, p, W):
    """include/idealnerf.h: idealnerf_patch_pixels, restated: patch by patch, row-major inside a patch."""
    out = []
    for oy, ox in origins:
        rows, cols = np.meshgrid(np.arange(oy, oy + p, dtype=np.int64), np.arange(ox, ox + p, dtype=np.int64), indexing="ij")
        out.append((rows * W + cols).reshape(-1))
    return np.concatenate(out)


def record(name, value):
    """Keep the largest `value` seen under `name`; with $IDN_SSIM_LOSS_RECORD set, the table is rewritten there each time."""
    MAXIMA[name] = max(float(value), MAXIMA.get(name, 0.0))
    path = os.environ.get("IDN_SSIM_LOSS_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump(MAXIMA, f, indent=1, sort_keys=True)
