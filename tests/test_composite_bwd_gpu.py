"""The compositing backward of the training step (csrc/train.hip: composite_bwd_kernel<SPL, kNorm>) alone, element by element
against the fp64 autograd of ``oracle.composite``.  ``ops.composite_bwd`` runs the kernel through the dispatch of a pass
(launch_composite_bwd: SPL = ceil(S / 64) = 1..8, the kNorm kernels where dL / d |rays_d| is asked for); every S below sits at
an end of a bucket, so all sixteen kernels run, each at both ragged ends.

Reference: ``oracle.composite`` on ``oracle.to_f64`` inputs, differentiated by torch with respect to raw and to the norm of
rays_d (the rays of the reference are (m, 0, 0) with the leaf m = |rays_d|: torch.norm is then the identity with derivative 1,
and the last spacing, 1e10 m, has alpha saturated -- asserted -- so that its share of d m is exactly 0).  The same in fp32 is the
reference's own distance from fp64, e32 (``oracle.fp32_noise_floor``).  The fp32 oracle is evaluated by torch on the device, so
that e32 is the same number wherever the test runs, and twice: |rays_d| is no fp32 number, an fp32 evaluation holds one of its
two fp32 neighbours according to how it orders the squares, the sum and the root (the kernel's sqrtf and torch.norm need not
agree), and that choice moves every exponent sigma dist of the ray by one part in 2^24.  e32 is the larger of the two distances,
m = the neighbour below and the neighbour above: on an output of a few numbers (d_norm at n <= 5) either one alone can land on
fp64 by chance and ask of the kernel less than the rounding of its inputs costs.  The kernel is held to
    bound = FACTOR max(e32, 2^-23),  FACTOR = 4
under the metric e32 is measured in, separately for d rgb [n, S, 3], d sigma [n, S] and d_norm [n]:
    sharp scene   max |got - ref| / max |ref| over the whole tensor
    mild scene    that ratio per ray, scaled by the ray's own max |ref|; the largest over all rays
(a reference that is zero throughout -- d rgb of a loss on acc alone -- demands zeros).

Scenes (seeded, CPU): |rays_d| >= 1 and never 1, random colours, background and incoming gradients (normal).
    mild    depths jittered in [0.3, 1.1]; optical depth per sample (0.2 .. 2) 4 / S; a quarter of the sigmas negated (never sample 0)
    sharp   raw_sigma = 300 randn; spacings 0.8 x 2^(-8 v^2), v uniform per sample -- between 0.8 and 0.003, a third of them above
            0.4 -- so that at every S a ray mixes samples whose sigma dist is near 1 (they carry the tensor's largest gradients)
            with samples at which fp32 exp(-sigma dist) is exactly 0.  The scene asserts from the fp64 forward that it holds a ray
            with such a sample before its last one (every n and S) and a ray whose transmittance falls below fp32's smallest
            normal number (S >= 63: every factor is at least 1e-10, so at S = 2 and 3 none can, and at S = 5 it takes four
            opaque samples in a row).  The JSON record counts both kinds of ray per scene.

What the tensor-scaled metric found: the kernel used to form the suffix sums sum_{t > s} dw_t w_t as total - inclusive prefix, in
fp64, which leaves 1e-16 of the ray's total in every one of them; divided by the sample's own transmittance factor that put
|d sigma| ~ 1e-16 dist on samples behind an opaque one, whose true gradient vanishes with their transmittance.  Invisible beside a
gradient of order 1 -- but on a batch whose every ray is opaque at its first samples the whole tensor is that small: with those
suffix sums the kernel measured, on the MI355X, 1.8e-2 of the largest d sigma on sharp 1 x 100 (bound 5.7e-5) and 1.8e-4 on sharp
5 x 64 (bound 5.5e-6).  The suffix sums are now added up from the ray's far end: 1.4e-5 and
6.1e-7 on the same two cases.  test_occluded_samples_have_vanishing_gradients holds the property itself, without a
yardstick: |d sigma| and |d rgb| below 1e-27 wherever the fp64 transmittance is below 1e-30.

Measured on an MI355X.  Every recorded launch -- every (scene, n, S, variant) and every gradient subset -- is in
profiles/composite_bwd_parity.json ($IDN_COMPOSITE_BWD_RECORD names the file the figures are merged into); the table below holds
the n = 37 rows alone, every S on both scenes, as  e32 -> kernel  per output (the kNorm kernels' d rgb and d sigma are the plain
kernels' bit for bit, so one row serves both variants):
      S  SPL  scene   d rgb  e32 -> kernel     d sigma  e32 -> kernel    d_norm  e32 -> kernel    (bound = 4 max(e32, 1.19e-7))
      2   1   mild    3.8e-07 -> 2.6e-07        3.2e-06 -> 1.3e-06        3.2e-06 -> 1.2e-06
      3   1   mild    1.9e-07 -> 1.9e-07        2.4e-06 -> 1.5e-06        6.2e-06 -> 2.3e-06
      5   1   mild    3.0e-07 -> 1.8e-07        1.6e-06 -> 2.6e-06        7.0e-06 -> 2.4e-06
     63   1   mild    6.7e-07 -> 5.7e-07        1.0e-06 -> 6.1e-07        3.8e-06 -> 1.7e-06
     64   1   mild    4.5e-07 -> 3.8e-07        1.9e-06 -> 9.0e-07        1.6e-05 -> 4.1e-06
     65   2   mild    4.5e-07 -> 4.6e-07        8.9e-07 -> 5.7e-07        1.1e-03 -> 9.8e-04
    100   2   mild    6.5e-07 -> 6.1e-07        1.9e-06 -> 1.5e-06        4.9e-06 -> 4.4e-06
    128   2   mild    7.1e-07 -> 7.0e-07        1.3e-06 -> 6.4e-07        4.0e-05 -> 1.3e-05
    129   3   mild    9.0e-07 -> 7.2e-07        1.2e-06 -> 7.6e-07        1.2e-05 -> 3.5e-06
    192   3   mild    1.2e-06 -> 1.1e-06        1.6e-06 -> 6.1e-07        2.9e-05 -> 1.9e-06
    193   4   mild    1.1e-06 -> 1.1e-06        1.4e-06 -> 8.3e-07        1.8e-05 -> 3.1e-06
    256   4   mild    1.5e-06 -> 1.6e-06        2.1e-06 -> 4.9e-07        1.4e-05 -> 1.9e-05
    257   5   mild    1.5e-06 -> 1.4e-06        2.0e-06 -> 6.8e-07        5.8e-05 -> 2.1e-05
    320   5   mild    1.7e-06 -> 1.6e-06        4.1e-06 -> 2.6e-06        7.7e-06 -> 2.7e-06
    321   6   mild    1.6e-06 -> 1.6e-06        2.7e-06 -> 7.8e-07        3.3e-05 -> 3.6e-06
    384   6   mild    2.0e-06 -> 2.1e-06        1.5e-06 -> 7.6e-07        2.1e-04 -> 9.8e-06
    385   7   mild    1.9e-06 -> 1.8e-06        1.5e-06 -> 5.2e-07        2.9e-05 -> 1.8e-05
    448   7   mild    2.2e-06 -> 2.1e-06        1.6e-06 -> 6.9e-07        4.9e-05 -> 2.8e-05
    449   8   mild    2.6e-06 -> 2.3e-06        3.1e-06 -> 1.0e-06        2.0e-05 -> 4.5e-06
    511   8   mild    2.6e-06 -> 2.6e-06        1.7e-06 -> 6.5e-07        7.7e-05 -> 1.1e-05
    512   8   mild    3.3e-06 -> 3.3e-06        1.6e-06 -> 6.6e-07        1.0e-05 -> 9.8e-06
      2   1   sharp   9.9e-08 -> 9.9e-08        7.1e-08 -> 7.1e-08        9.6e-08 -> 8.2e-08
      3   1   sharp   7.9e-08 -> 7.9e-08        3.4e-07 -> 3.4e-07        2.3e-07 -> 2.3e-07
      5   1   sharp   8.7e-08 -> 1.3e-07        1.1e-07 -> 4.0e-07        1.4e-07 -> 3.6e-07
     63   1   sharp   1.1e-07 -> 1.1e-07        2.3e-07 -> 2.9e-07        3.8e-07 -> 3.5e-07
     64   1   sharp   1.6e-07 -> 1.6e-07        3.9e-07 -> 1.8e-07        3.4e-07 -> 3.6e-07
     65   2   sharp   1.1e-07 -> 8.1e-08        1.3e-07 -> 1.3e-07        1.5e-07 -> 1.3e-07
    100   2   sharp   1.5e-07 -> 1.3e-07        1.7e-07 -> 6.2e-08        6.4e-07 -> 7.3e-08
    128   2   sharp   9.1e-08 -> 7.9e-08        1.4e-07 -> 1.4e-07        3.3e-07 -> 2.7e-07
    129   3   sharp   8.0e-08 -> 8.0e-08        2.0e-07 -> 1.9e-07        6.5e-07 -> 2.6e-07
    192   3   sharp   7.9e-08 -> 7.9e-08        3.5e-07 -> 3.6e-07        2.7e-07 -> 1.7e-07
    193   4   sharp   8.2e-08 -> 8.2e-08        5.4e-07 -> 4.3e-07        4.2e-07 -> 1.8e-07
    256   4   sharp   8.5e-08 -> 1.2e-07        2.5e-07 -> 4.9e-07        1.0e-07 -> 8.6e-08
    257   5   sharp   1.1e-07 -> 1.1e-07        1.4e-07 -> 9.3e-08        2.3e-07 -> 7.0e-08
    320   5   sharp   1.3e-07 -> 1.3e-07        1.1e-07 -> 2.2e-07        2.7e-07 -> 9.1e-08
    321   6   sharp   9.1e-08 -> 1.2e-07        2.8e-07 -> 4.8e-07        4.5e-07 -> 1.6e-07
    384   6   sharp   1.1e-07 -> 1.1e-07        2.9e-07 -> 1.0e-07        2.0e-07 -> 1.8e-07
    385   7   sharp   1.2e-07 -> 1.5e-07        7.0e-07 -> 3.2e-07        1.1e-06 -> 1.1e-07
    448   7   sharp   1.3e-07 -> 1.3e-07        4.6e-07 -> 1.5e-07        1.2e-07 -> 2.1e-07
    449   8   sharp   8.7e-08 -> 1.1e-07        3.7e-07 -> 3.7e-07        2.4e-07 -> 1.9e-07
    511   8   sharp   8.2e-08 -> 1.6e-07        7.8e-07 -> 1.6e-07        1.8e-06 -> 3.5e-07
    512   8   sharp   7.0e-08 -> 6.6e-08        2.3e-07 -> 3.1e-07        2.7e-07 -> 2.8e-07
Over all 164 recorded launches the kernel's largest share of its bound is 0.84 (sharp/n37/S5/plain, d sigma: a bound
that is the floor 4 x 2^-23).
"""
import json
import os

import pytest
import torch

import oracle
from test_delta_chain_gpu import SENTINEL, guarded, guards_intact

pytestmark = pytest.mark.gpu

FACTOR = 4.0                 # as tests/test_ray_grad_gpu.py
EPS = 2.0 ** -23             # one fp32 epsilon: a single correctly rounded result already sits at 2^-24 of the scale
S_ALL = [2, 3, 5, 63, 64, 65, 100, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 511, 512]   # both ends of all 8 buckets
N_ALL = [1, 3, 4, 5, 37, 130]                                                                              # 4 rays to a workgroup
S_FOR_N = [64, 100, 449]
SHAPES = [(37, S) for S in S_ALL] + [(n, S) for n in N_ALL if n != 37 for S in S_FOR_N]
OUTPUTS = ("rgb", "fg", "lw", "acc")
SUBSETS = [("rgb",), ("rgb", "fg", "lw"), ("acc",), ("lw",), OUTPUTS]
GROUPS = ("d_rgb", "d_sigma", "d_norm")
NEAR, FAR = 0.3, 1.1
SEED = 0
EXTRA_ROWS = 5               # sentinel rows behind the n S rows of every output matrix


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()  # fail loudly if the HIP library is missing
    return idealnerf_amd


def _record(key, value):
    path = os.environ.get("IDN_COMPOSITE_BWD_RECORD")
    if not path:
        return
    old = {}
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
    old[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(old, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------------------------- scenes
_scenes = {}


def scene(kind, n, S):
    """One seeded scene (CPU fp32): raw [n, S, 4], z [n, S], rays [n, 11], bc [n, 3] and the four incoming gradients g; built
    once and never written again.  The references of its gradient subsets are cached in it (``reference``)."""
    key = (kind, n, S)
    if key in _scenes:
        return _scenes[key]
    g = torch.Generator().manual_seed(SEED + 100003 * S + 17 * n + (1 if kind == "sharp" else 0))
    rnd = lambda *shape: torch.rand(shape, generator=g)
    d = torch.randn((n, 3), generator=g) * 0.5
    d[:, 2] = -1.0 - 0.5 * rnd(n)
    norm = torch.norm(d, dim=-1)
    assert float(norm.min()) >= 1.0 and float((norm - 1).abs().min()) > 0
    one = torch.ones(n, 1)
    rays = torch.cat([torch.randn((n, 3), generator=g) * 0.1, d, NEAR * one, FAR * one, d / norm[:, None]], -1).contiguous()
    raw = torch.randn((n, S, 4), generator=g)
    if kind == "mild":
        u = (torch.arange(S)[None, :] + 0.1 + 0.8 * rnd(n, S)) / S             # jittered, spacings of at least 0.2 / S
        z = NEAR + (FAR - NEAR) * u
        dz = z[:, 1:] - z[:, :-1]
        dist = torch.cat([dz, dz[:, -1:]], -1) * norm[:, None]                 # (the last sample: the spacing in front of it)
        sigma = (0.2 + 1.8 * rnd(n, S)) * (4.0 / S) / dist
        off = rnd(n, S) < 0.25
        off[:, 0] = False
        raw[..., 3] = torch.where(off, -sigma, sigma)
    else:
        dz = (FAR - NEAR) * torch.exp2(-8.0 * rnd(n, S) ** 2)                  # 0.8 .. 0.003, a third of them above 0.4
        z = NEAR + torch.cumsum(dz, -1)
        raw[..., 3] *= 300.0
    assert bool((z[:, 1:] > z[:, :-1]).all())
    sc = dict(kind=kind, n=n, S=S, raw=raw.contiguous(), z=z.contiguous(), rays=rays, bc=rnd(n, 3),
              g=dict(rgb=torch.randn((n, 3), generator=g), fg=torch.randn((n, 3), generator=g), lw=torch.randn(n, generator=g),
                     acc=torch.randn(n, generator=g)), refs={})
    if kind == "sharp":
        x, T = _forward64(sc)
        sc["rays_exp0"] = int((x[:, :-1] > 104.0).any(1).sum())               # fp32 exp(-x) is 0 from x = 103.98 on
        sc["rays_T_underflow"] = int((T < 2.0 ** -126).any(1).sum())
        assert sc["rays_exp0"] >= 1, "no ray with a sample whose fp32 exp is exactly 0 before the last sample"
        assert S < 63 or sc["rays_T_underflow"] >= 1, "no ray whose transmittance underflows fp32"
    _scenes[key] = sc
    return sc


def _forward64(sc):
    """(sigma' dist [n, S], transmittance [n, S]) of the fp64 forward."""
    raw, z, rays = oracle.to_f64((sc["raw"], sc["z"], sc["rays"]))
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((sc["n"], 1), 1e10, dtype=torch.float64)], -1) * torch.norm(rays[:, 3:6], dim=-1)[:, None]
    x = (torch.relu(raw[..., 3]) + 1e-6) * dist
    tf = 1.0 - (1.0 - torch.exp(-x)) + 1e-10
    T = torch.cumprod(torch.cat([torch.ones((sc["n"], 1), dtype=torch.float64), tf], -1), -1)[:, :-1]
    return x, T


# ---------------------------------------------------------------------------------------------- reference
def norm_neighbours(sc):
    """The two fp32 numbers next to the exact |rays_d| of every ray, (below, above) -- the same number twice where the norm is one."""
    m64 = torch.norm(sc["rays"][:, 3:6].double(), dim=-1)
    near = m64.float()
    inf = torch.full_like(near, float("inf"))
    return (torch.where(near.double() > m64, torch.nextafter(near, -inf), near),
            torch.where(near.double() < m64, torch.nextafter(near, inf), near))


def _autograd(sc, dtype, subset, device="cpu", side=None):
    """d (sum over `subset` of <output, g>) / d (raw, |rays_d|) by torch autograd of oracle.composite in `dtype`, evaluated by torch
    on `device` (the tensors oracle.composite makes itself are made there too) -> fp64 tensors on the CPU.  side: None -- |rays_d|
    as `dtype` computes it (the fp64 reference); 0 / 1 -- the fp32 number below / above it (norm_neighbours)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.device(device):
            to = lambda t: t.to(device=device, dtype=dtype)
            raw = to(sc["raw"]).clone().requires_grad_(True)
            m = torch.norm(to(sc["rays"][:, 3:6]), dim=-1) if side is None else to(norm_neighbours(sc)[side])
            m = m.clone().requires_grad_(True)
            zero = torch.zeros_like(m)
            rgb_map, _, acc, weights, _, rgb_fg = oracle.composite(raw, to(sc["z"]), torch.stack([m, zero, zero], -1), to(sc["bc"]),
                                                                    with_fg=True)
            outs = dict(rgb=rgb_map, fg=rgb_fg, lw=weights[:, -1], acc=acc)
            loss = sum((outs[k] * to(sc["g"][k])).sum() for k in subset)
            d_raw, d_m = torch.autograd.grad(loss, (raw, m))
            # the last spacing is 1e10 m: its alpha is saturated, so m reaches the loss through the first S - 1 spacings alone
            assert float(torch.exp(-(torch.relu(raw[:, -1, 3]) + 1e-6) * 1e10 * m).detach().max()) == 0.0
        return dict(d_rgb=d_raw[..., :3].double().cpu(), d_sigma=d_raw[..., 3].double().cpu(), d_norm=d_m.double().cpu())
    finally:
        torch.set_default_dtype(old)


def distance(kind, got, ref):
    """The scene's metric for one output: oracle.fp32_noise_floor (max |got - ref| / max |ref|) of the whole tensor (sharp) or of
    every ray's own part, the largest of them (mild)."""
    if kind == "sharp":
        return oracle.fp32_noise_floor(got, ref)
    return max(oracle.fp32_noise_floor(got[r], ref[r]) for r in range(ref.shape[0]))


def reference(sc, dev, subset=OUTPUTS):
    """(fp64 gradients, e32 per output) of a gradient subset; computed once per scene and subset.  The fp64 reference is
    evaluated on the CPU; e32 is the larger of the fp32 oracle's two distances from it, evaluated on `dev` with |rays_d| as the
    fp32 number below and as the one above the exact norm (module docstring)."""
    if subset not in sc["refs"]:
        g64 = _autograd(sc, torch.float64, subset)
        e32 = dict.fromkeys(GROUPS, 0.0)
        for side in (0, 1):
            g32 = _autograd(sc, torch.float32, subset, dev, side)
            for k in GROUPS:
                assert bool(torch.isfinite(g64[k]).all()) and bool(torch.isfinite(g32[k]).all()), k
                e32[k] = max(e32[k], distance(sc["kind"], g32[k], g64[k]))
        sc["refs"][subset] = (g64, e32)
    return sc["refs"][subset]


# ---------------------------------------------------------------------------------------------- running the aid
def on_device(sc, dev):
    if "dev" not in sc:
        sc["dev"] = dict(raw=sc["raw"].to(dev), z=sc["z"].to(dev), rays=sc["rays"].to(dev), bc=sc["bc"].to(dev),
                         g={k: v.to(dev) for k, v in sc["g"].items()})
    return sc["dev"]


def run(idn, dev, t, subset=OUTPUTS, norm=True, layout="packed"):
    """One launch on fresh sentinel-guarded outputs.  t: device tensors raw, z, rays, bc, g (on_device, or made of it); subset: the
    incoming gradients handed over (the others are NULL); norm: the kNorm kernels, d_norm in column 6 of an [n, 11] matrix as in
    a pass.  layout "packed": pitches (4, 4), one [n S + EXTRA_ROWS, 4] matrix; "pass": d rgb at pitch 64, d sigma in column 128 at
    pitch 256.  Afterwards every word no output is addressed to holds the sentinel bit for bit -- the other columns, the rows
    from n S on, the guards, d_norm's other columns -- and every output is finite.
    -> dict(d_rgb [n, S, 3], d_sigma [n, S], d_norm [n] or None) on the CPU."""
    n, S = t["z"].shape
    rows = n * S + EXTRA_ROWS
    g = [t["g"][k] if k in subset else None for k in OUTPUTS]
    wn, dn = guarded((n, 11), dev) if norm else (None, None)
    if layout == "packed":
        wo, out = guarded((rows, 4), dev)
        idn.ops.composite_bwd(t["raw"], t["z"], t["rays"], t["bc"], *g, d_rgb=out, d_sig=out, sig_col=3, d_norm=dn, norm_col=6 if norm else 0)
        assert guards_intact(wo), "a write outside the output matrix"
        d_rgb, d_sig = out[:n * S, :3], out[:n * S, 3]
        untouched = [out[n * S:]]
    else:
        wr, m_rgb = guarded((rows, 64), dev)
        ws, m_sig = guarded((rows, 256), dev)
        idn.ops.composite_bwd(t["raw"], t["z"], t["rays"], t["bc"], *g, d_rgb=m_rgb, d_sig=m_sig, sig_col=128, d_norm=dn, norm_col=6 if norm else 0)
        assert guards_intact(wr) and guards_intact(ws), "a write outside the output matrices"
        d_rgb, d_sig = m_rgb[:n * S, :3], m_sig[:n * S, 128]
        untouched = [m_rgb[:, 3:], m_rgb[n * S:], m_sig[:, :128], m_sig[:, 129:], m_sig[n * S:]]
    if norm:
        assert guards_intact(wn), "a write outside d_norm's matrix"
        untouched += [dn[:, :6], dn[:, 7:]]
    for u in untouched:
        assert bool((u.contiguous().view(torch.int32) == SENTINEL).all()), "a word no output is addressed to was written"
    res = dict(d_rgb=d_rgb.reshape(n, S, 3).cpu(), d_sigma=d_sig.reshape(n, S).cpu(), d_norm=dn[:, 6].cpu() if norm else None)
    for k, v in res.items():
        assert v is None or bool(torch.isfinite(v).all()), f"{k}: not every element was written with a finite value"
    return res


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def is_plus_zero(a):
    return bool((a.contiguous().view(torch.int32) == 0).all())


def is_zero(a):
    """Zero bit for bit but for the sign: where the kernel's zero is a product with an exact 0 (d alpha x exp x dist at a saturated
    sample, or anything times zero incoming gradients) its sign is the other factors', and -0.0 is as exact a zero as +0.0."""
    return bool((a.contiguous().view(torch.int32) & 0x7fffffff == 0).all())


def check_against_fp64(sc, dev, got, subset, tag):
    """Every output of one launch against the fp64 autograd under the scene's metric; prints and records the figures, then
    asserts them."""
    g64, e32 = reference(sc, dev, subset)
    err, bound = {}, {}
    for k in GROUPS:
        if got[k] is not None:
            err[k], bound[k] = distance(sc["kind"], got[k], g64[k]), FACTOR * max(e32[k], EPS)
    print(f"\n  {tag}: " + "  ".join(f"{k} e32 {e32[k]:.2e} bound {bound[k]:.2e} kernel {err[k]:.2e}" for k in err))
    _record(tag, dict(e32={k: e32[k] for k in err}, bound=bound, kernel=err, n=sc["n"], S=sc["S"], spl=(sc["S"] + 63) // 64,
                      **{k: sc[k] for k in ("rays_exp0", "rays_T_underflow") if k in sc}))
    for k in err:
        assert err[k] <= bound[k], (tag, k, err[k], bound[k], e32[k])


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("n,S", SHAPES, ids=[f"{n}x{S}" for n, S in SHAPES])
@pytest.mark.parametrize("kind", ["mild", "sharp"])
def test_every_element_vs_fp64(idn, dev, kind, n, S):
    """All four incoming gradients; the plain and the kNorm kernel of the shape's bucket, whose d rgb and d sigma are the same bits.
    Every ray's last sample has d rgb = +0 and d sigma = 0 of either sign (is_zero: d alpha x exp x dist with exp exactly 0), and
    d sigma is +0 bit for bit wherever raw_sigma <= 0."""
    sc = scene(kind, n, S)
    t = on_device(sc, dev)
    plain, normed = run(idn, dev, t, norm=False), run(idn, dev, t, norm=True)
    assert same_bits(plain["d_rgb"], normed["d_rgb"]) and same_bits(plain["d_sigma"], normed["d_sigma"])
    for variant, got in (("plain", plain), ("norm", normed)):
        assert is_plus_zero(got["d_rgb"][:, -1]) and is_zero(got["d_sigma"][:, -1]), "a ray's last sample"
        assert is_plus_zero(got["d_sigma"][sc["raw"][..., 3] <= 0]), "d sigma behind a ReLU that is off"
        check_against_fp64(sc, dev, got, OUTPUTS, f"{kind}/n{n}/S{S}/{variant}")
    assert kind == "sharp" or float(normed["d_norm"].abs().min()) > 0


@pytest.mark.parametrize("S", [65, 192])
@pytest.mark.parametrize("kind", ["mild", "sharp"])
def test_gradient_subsets_vs_fp64(idn, dev, kind, S):
    """{rgb}, {rgb, fg, lw} (the torso loss), {acc}, {lw} and all four, the other pointers NULL: each against the fp64 autograd of
    exactly those outputs.  {acc} is a check of another kind than the rest: acc = 1 - prod(1 - alpha + 1e-10) is 1 to within the
    last factor, so its fp64 gradient is some 1e-10 of any other here, while an fp32 evaluation -- the oracle's and the kernel's
    alike -- leaves the rounding of g_acc T - suffix / (1 - alpha + 1e-10), two numbers that cancel.  e32 is then many times the
    reference's largest entry, and what the bound holds is that cancellation: the kernel's d sigma and d_norm stay within 4 x the
    fp32 oracle's own residue (and d rgb is +0 bit for bit)."""
    sc = scene(kind, 37, S)
    t = on_device(sc, dev)
    for subset in SUBSETS:
        got = run(idn, dev, t, subset=subset)
        check_against_fp64(sc, dev, got, subset, f"{kind}/n37/S{S}/norm/" + "+".join(subset))
        if "rgb" not in subset and "fg" not in subset:
            assert is_plus_zero(got["d_rgb"])


# ---------------------------------------------------------------------------------------------- equalities
def with_sigma(t, sigma):
    raw = t["raw"].clone()
    raw[..., 3] = sigma.to(raw.device)
    return dict(t, raw=raw)


def test_relu_off_values_and_extreme_sigma(idn, dev):
    """raw_sigma = +0.0, -0.0 and -1e30 (every third sample each way, never sample 0) give d sigma = +0 bit for bit, on both
    scenes; on the sharp scene every output stays finite, also with raw_sigma = 1e30 in every other sample and throughout."""
    for kind in ("mild", "sharp"):
        sc = scene(kind, 37, 100)
        t = on_device(sc, dev)
        sigma = sc["raw"][..., 3].clone()
        special = torch.tensor([0.0, -0.0, -1e30])
        idx = torch.arange(1, 100)
        sigma[:, 1:] = torch.where((idx % 2 == 1)[None, :], special[(idx // 2) % 3][None, :], sigma[:, 1:])
        assert all(int((sigma.view(torch.int32) == v.view(torch.int32)).sum()) >= 37 * 16 for v in special)
        got = run(idn, dev, with_sigma(t, sigma))
        assert is_plus_zero(got["d_sigma"][sigma <= 0]) and (kind == "sharp" or bool((got["d_sigma"][:, 0] != 0).all()))
    for S in (5, 100, 449):
        sc = scene("sharp", 37, S)
        t = on_device(sc, dev)
        sigma = sc["raw"][..., 3].clone()
        sigma[:, ::2] = 1e30
        for s in (sigma, torch.full_like(sigma, 1e30)):
            got = run(idn, dev, with_sigma(t, s))          # (run asserts that every output is finite)
            assert is_plus_zero(got["d_rgb"][:, -1]) and is_zero(got["d_sigma"][:, -1])


@pytest.mark.parametrize("n,S", [(1, 100), (5, 64), (37, 449)])
def test_occluded_samples_have_vanishing_gradients(idn, dev, n, S):
    """Behind transmittance T a sample's gradients are at most of order T: |d alpha_s| <= T_s (|dw_s| + max |dw|), so with
    |dw| <= sum |g| <= 25 on these scenes, e <= 1 and dist <= 0.8 |rays_d| <= 4: |d sigma| <= 200 T, and |d rgb| <= 2 T.  Held, whatever
    the rest of the tensor holds, at every sample whose fp64 transmittance is below 1e-30 -- more than half of the sharp scene:
    both below 1e-27.  (Suffix sums formed as total - prefix left 1e-16 dist there.)"""
    sc = scene("sharp", n, S)
    assert sum(float(v.abs().max()) for v in sc["g"].values()) <= 25.0 and float(torch.norm(sc["rays"][:, 3:6], dim=-1).max()) <= 5.0
    dark = _forward64(sc)[1] < 1e-30
    assert int(dark.sum()) > n * S // 2
    got = run(idn, dev, on_device(sc, dev))
    assert float(got["d_sigma"][dark].abs().max()) <= 1e-27 and float(got["d_rgb"][dark].abs().max()) <= 1e-27


def test_zero_gradients_give_zero_outputs(idn, dev):
    """A ray whose four incoming gradients are all 0 has all-zero outputs while its neighbours do not; with the gradients one-hot
    over the rays only that ray has any; with all four pointers NULL everything written is +0."""
    for kind, S in (("mild", 100), ("sharp", 65)):
        sc = scene(kind, 5, S)
        t = on_device(sc, dev)
        full = run(idn, dev, t)
        for r in range(5):
            hot = torch.zeros(5, device=dev)
            hot[r] = 1.0
            for keep in (hot, 1.0 - hot):
                g = {k: (v * (keep[:, None] if v.dim() == 2 else keep)).contiguous() for k, v in t["g"].items()}
                got = run(idn, dev, dict(t, g=g))
                for q in range(5):
                    for k in GROUPS:
                        if float(keep[q]) == 0.0:
                            assert is_zero(got[k][q]), (kind, r, q, k)
                        else:
                            assert same_bits(got[k][q], full[k][q]) and bool((got[k][q] != 0).any()), (kind, r, q, k)
        got = run(idn, dev, t, subset=())
        assert all(is_plus_zero(got[k]) for k in GROUPS)


def rows_of(t, idx):
    return dict(raw=t["raw"][idx].contiguous(), z=t["z"][idx].contiguous(), rays=t["rays"][idx].contiguous(), bc=t["bc"][idx].contiguous(),
                g={k: v[idx].contiguous() for k, v in t["g"].items()})


@pytest.mark.parametrize("kind,S", [("mild", 100), ("sharp", 449), ("sharp", 64)])
def test_a_rays_bits_do_not_depend_on_its_place(idn, dev, kind, S):
    """A ray's outputs are the same bits in a second launch, with 1, 2 or 3 other rays in front of it (another wave of the
    workgroup) and in a batch of another size."""
    sc = scene(kind, 130, S)
    t = on_device(sc, dev)
    base = run(idn, dev, t)
    again = run(idn, dev, t)
    assert all(same_bits(base[k], again[k]) for k in GROUPS), "a second launch gave other bits"
    for front in (1, 2, 3):
        idx = torch.cat([torch.arange(129, 129 - front, -1), torch.arange(37)]).to(dev)
        got = run(idn, dev, rows_of(t, idx))
        assert all(same_bits(got[k][front:], base[k][:37]) for k in GROUPS), front
    for n in (1, 5, 37):
        got = run(idn, dev, rows_of(t, torch.arange(n, device=dev)))
        assert all(same_bits(got[k], base[k][:n]) for k in GROUPS), n
    got = run(idn, dev, rows_of(t, torch.arange(7, 12, device=dev)))
    assert all(same_bits(got[k], base[k][7:12]) for k in GROUPS)


# ---------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("kind,n,S", [("mild", 37, 100), ("sharp", 5, 449)])
def test_the_pass_layout_is_the_packed_one(idn, dev, kind, n, S):
    """Pitches (4, 4) into one [n, S, 4] tensor, and the pass's own -- d rgb at pitch 64, d sigma at pitch 256 in column 128,
    d_norm at pitch 11 in column 6: the same bits, and (run) every sentinel around and between them intact."""
    t = on_device(scene(kind, n, S), dev)
    packed, passed = run(idn, dev, t, layout="packed"), run(idn, dev, t, layout="pass")
    assert all(same_bits(packed[k], passed[k]) for k in GROUPS)
    d_raw, d_sig, d_norm = idn.ops.composite_bwd(t["raw"], t["z"], t["rays"], t["bc"], *(t["g"][k] for k in OUTPUTS))
    assert d_raw is d_sig and d_norm is None and d_raw.shape == (n, S, 4)
    assert same_bits(d_raw[..., :3].cpu(), packed["d_rgb"]) and same_bits(d_raw[..., 3].cpu(), packed["d_sigma"])
