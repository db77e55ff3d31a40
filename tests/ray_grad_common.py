"""Shared by tests/test_ray_grad_gpu.py and its child process (not collected by pytest): the scenes of the ray-gradient cases and
the CPU oracle's d loss / d rays at GIVEN sample depths, in float32 and float64."""
import math

import numpy as np
import torch

import oracle

NEAR, FAR = 0.5772005200386048, 1.1772005200386046
# n rays x (S + Ni) samples; fg: the torso variant (rgb_map_fg in the loss, the torso pair's widths); seed: of the scene's
# camera, rays, weights and loss.  Why these shapes: tests/test_ray_grad_gpu.py.  The torso variant's seed was chosen with the
# oracle alone: its first scene (seed 3) gave e32 = 1.07e-3 -- above the 1e-3 at which a scene counts as too sharp -- at the
# depths of a GPU forward; of the next candidates (14, 24, 34, 44) seed 24 is the one whose e32 stays at 9e-5 on the CPU when
# the fine depths are moved by a few ulps (the others: 2.7e-3, 1.4e-3, 9.4e-4).
CASES = {
    "3x64+128": dict(n=3, S=64, Ni=128, fg=False, seed=4),
    "37x64+128": dict(n=37, S=64, Ni=128, fg=False, seed=2),
    "26x5": dict(n=26, S=5, Ni=0, fg=False, seed=0),
    "2x256+256": dict(n=2, S=256, Ni=256, fg=False, seed=1),
    "37x64+128fg": dict(n=37, S=64, Ni=128, fg=True, seed=24),
}
# Density head of the scenes (alpha_linear.weight x GAIN, bias BIAS on Xavier weights): chosen on the CPU, with the oracle alone,
# so that every case's e32 (the fp32 oracle against the fp64 oracle) stays below 1e-3 and the |rays_d| term of raw2outputs
# carries far more than the bound (the measured figures stand in test_ray_grad_gpu.py's docstring).
GAIN, BIAS = 30.0, 0.1
BLOCKS = {"o": slice(0, 3), "d": slice(3, 6), "viewdirs": slice(8, 11)}


def rotated_camera(seed):
    """[3, 4]: a seeded rotation of ~0.3 rad about a seeded axis, origin near (0, 0, 0.877)."""
    rs = np.random.RandomState(seed)
    axis = rs.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = 0.3
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    t = np.array([0.03, -0.02, 0.877]) + 0.01 * rs.standard_normal(3)
    return torch.from_numpy(np.concatenate([R, t[:, None]], 1).astype(np.float32))


def scene(name):
    """Everything a case needs, on the CPU in float32: ray records of a rotated 32 x 32 camera with a short focal length
    (|rays_d| from 1.0 to ~1.1, never 1 everywhere), background, conditioning, the two networks' weights and the fixed
    random linear functional of (rgb_map, rgb0, acc_map[, rgb_map_fg]) that is the loss."""
    c = CASES[name]
    seed = c["seed"]
    rs = np.random.RandomState(100 + seed)
    n = c["n"]
    ro, rd = oracle.camera_rays(32, 32, 50.0, rotated_camera(seed))
    sel = torch.from_numpy(rs.choice(1024, size=n, replace=False))
    rays = oracle.ray_records(ro, rd, NEAR, FAR)[sel].contiguous()
    norm = rays[:, 3:6].norm(dim=-1)
    assert float(norm.min()) >= 1.0 and float(norm.max()) > 1.02, (float(norm.min()), float(norm.max()))
    T = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    if c["fg"]:
        dims = oracle.facenerf_dims(dim_aud=106, dim_expr=0, dim_latent=0)
        aud, expr, latent = T(rs.standard_normal(106) * 0.5), None, None
    else:
        dims = oracle.facenerf_dims()
        aud, expr, latent = T(rs.standard_normal(64)), T(rs.standard_normal(76)), torch.ones(32)

    def params(s):
        p = oracle.xavier_facenerf_params(s, dims)
        p["alpha_linear.weight"] = p["alpha_linear.weight"] * GAIN
        p["alpha_linear.bias"] = torch.full_like(p["alpha_linear.bias"], BIAS)
        return p
    keys = ["rgb_map", "acc_map"] + (["rgb0"] if c["Ni"] > 0 else []) + (["rgb_map_fg"] if c["fg"] else [])
    weights = {k: T(rs.standard_normal((n, 3) if k != "acc_map" else (n,))) for k in keys}
    return dict(c, name=name, dims=dims, rays=rays, bc=T(rs.uniform(0, 1, (n, 3))), aud=aud, expr=expr, latent=latent,
                coarse=params(40 + 2 * seed), fine=params(41 + 2 * seed), weights=weights)


def loss_of(out, weights):
    """The fixed linear functional; ``out`` has the reference's keys (either side's render)."""
    return sum((out[k] * w.to(out[k].device, out[k].dtype)).sum() for k, w in weights.items())


def oracle_outputs(sc, rays, z_c, z_f, detach_norm=False):
    """The oracle's render of ``rays`` [n, 11] AT GIVEN DEPTHS (z_c [n, S], z_f [n, S + Ni] or None), in rays' dtype: its query
    and composite functions on pts = o + d z, so that no importance index can flip between the two sides of a comparison.
    detach_norm: rays_d enters raw2outputs' dists = dz |rays_d| detached (what a backward without the norm term computes)."""
    f = oracle.to_f64 if rays.dtype == torch.float64 else (lambda x: x)
    o, d, view = rays[:, 0:3], rays[:, 3:6], rays[:, 8:11]
    aud, expr, lat, bc = f(sc["aud"]), f(sc["expr"]), f(sc["latent"]), f(sc["bc"])
    out = {}

    def one(params, z, tag0):
        pts = o[:, None, :] + d[:, None, :] * z[:, :, None]
        raw = oracle.render_oracle._query(f(params), pts, view, aud, expr, lat, sc["dims"])
        comp = oracle.composite(raw, z, d.detach() if detach_norm else d, bc, with_fg=sc["fg"])
        out["rgb" + tag0], out["acc" + tag0] = comp[0], comp[2]
        if sc["fg"]:
            out["rgb_map_fg" + ("0" if tag0 == "0" else "")] = comp[5]
    if z_f is None:
        one(sc["coarse"], z_c, "_map")
    else:
        one(sc["coarse"], z_c, "0")
        one(sc["fine"], z_f, "_map")
    return out


def oracle_d_rays(sc, z_c, z_f, dtype, detach_norm=False):
    """d loss / d rays [n, 11] by the oracle's autograd at the given depths, evaluated in ``dtype`` -> float64 tensor."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        rays = sc["rays"].to(dtype).clone().requires_grad_(True)
        cast = lambda z: None if z is None else z.detach().cpu().to(dtype)
        out = oracle_outputs(sc, rays, cast(z_c), cast(z_f), detach_norm)
        g, = torch.autograd.grad(loss_of(out, sc["weights"]), rays)
    finally:
        torch.set_default_dtype(old)
    return g.double()


def block_errors(got, ref64):
    """max |got - ref| / max |ref| per column block of the ray record (o, d, viewdirs) -> dict."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    return {k: float((got[:, s] - ref64[:, s]).abs().max() / ref64[:, s].abs().max().clamp_min(1e-30)) for k, s in BLOCKS.items()}


def oracle_depths(sc):
    """The oracle's own depths of the scene (perturb = 0): what the CPU-side choice of the scenes used in place of the HIP
    forward's, which need a GPU."""
    with torch.no_grad():
        o = oracle.render_rays(sc["rays"], sc["bc"], sc["coarse"], sc["fine"] if sc["Ni"] else None, sc["aud"], sc["expr"],
                               sc["latent"], n_samples=sc["S"], n_importance=sc["Ni"], dims=sc["dims"], with_fg=sc["fg"], taps=True)
    return o["tap_z_coarse"], o.get("tap_z_fine")
