"""Shared by tests/test_cond_grad_gpu.py, its child process and tests/test_cond_refine_cpu.py (not collected by pytest): the
CPU oracle's d loss / d expr and d loss / d bc at GIVEN sample depths, in float32 and float64, on the scenes of
ray_grad_common.py, and the oracle-only model of the background-recovery test."""
import numpy as np
import torch

import oracle
import ray_grad_common as rg

# every scene of the ray-gradient cases; the torso variant's pair takes no expression, so it checks d bc alone
CASES = list(rg.CASES)
FACTOR, FLOOR = 4.0, 5e-6   # bound per block: max(FACTOR * e32, FLOOR) (the issue's: test_ray_grad_gpu.py's margin, test_torso_train_gpu.py's d aud bound)
TOO_SHARP = 1e-3


def oracle_d_cond(sc, z_c, z_f, dtype):
    """d loss / d (expr [dim_expr] or None, bc [n, 3]) by the oracle's autograd at the given depths, evaluated in ``dtype``
    with both as leaves -> float64 tensors."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        leaf = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(True)
        expr, bc = leaf(sc["expr"]), leaf(sc["bc"])
        cast = lambda z: None if z is None else z.detach().cpu().to(dtype)
        out = rg.oracle_outputs(dict(sc, expr=expr, bc=bc), sc["rays"].to(dtype), cast(z_c), cast(z_f))
        g = torch.autograd.grad(rg.loss_of(out, sc["weights"]), [t for t in (expr, bc) if t is not None])
    finally:
        torch.set_default_dtype(old)
    return (g[0].double() if expr is not None else None), g[-1].double()


def rel(got, ref64):
    """max |got - ref| / max |ref|."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    return float((got - ref64).abs().max() / ref64.abs().max().clamp_min(1e-30))


def bound(e32):
    return max(FACTOR * e32, FLOOR)


# ---- background recovery: rgb_map = A + lw * B per ray, exactly linear in the background B ---------------------------------
RECOVERY_STEPS, RECOVERY_LR = 20, 2e-2


def recovery_run(lw_f, lw_c, b_true, noise, steps=RECOVERY_STEPS, lr=RECOVERY_LR):
    """The oracle-only model of the recovery test: with frozen networks the loss mse(rgb, tgt) + mse(rgb0, tgt) over a
    background B depends on it through rgb_map = A + lw_f B and rgb0 = A0 + lw_c B alone, and the targets are the renders over
    B*: loss(B) = mean((lw_f (B - B*))^2) + mean((lw_c (B - B*))^2).  Adam (the trainer's betas) on B from B* + 0.2 noise ->
    (|B - B*| per ray -- the row's largest channel -- before, after; loss before, after), float64."""
    lw_f, lw_c, b_true = lw_f.double()[:, None], lw_c.double()[:, None], b_true.double()
    B = (b_true + 0.2 * noise.double()).clone().requires_grad_(True)
    opt = torch.optim.Adam([B], lr=lr, betas=(0.9, 0.999))
    loss_of = lambda: ((lw_f * (B - b_true)) ** 2).mean() + ((lw_c * (B - b_true)) ** 2).mean()
    before, loss0 = (B - b_true).detach().abs().max(dim=1)[0], float(loss_of().detach())
    for _ in range(steps):
        opt.zero_grad()
        loss_of().backward()
        opt.step()
    return before, (B - b_true).detach().abs().max(dim=1)[0], loss0, float(loss_of().detach())


def recovery_scene(n=64, seed=5):
    """64 rays of a 32 x 32 camera at S = 16, Ni = 16 with the scenes' density head: (ray records, B* [n, 3], noise [n, 3],
    aud, expr, latent, coarse params, fine params), float32 on the CPU."""
    rs = np.random.RandomState(seed)
    ro, rd = oracle.camera_rays(32, 32, 50.0, rg.rotated_camera(seed))
    sel = torch.from_numpy(rs.choice(1024, size=n, replace=False))
    rays = oracle.ray_records(ro, rd, rg.NEAR, rg.FAR)[sel].contiguous()
    T = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    dims = oracle.facenerf_dims()

    def params(s):
        p = oracle.xavier_facenerf_params(s, dims)
        p["alpha_linear.weight"] = p["alpha_linear.weight"] * rg.GAIN
        p["alpha_linear.bias"] = torch.full_like(p["alpha_linear.bias"], rg.BIAS)
        return p
    return dict(n=n, S=16, Ni=16, fg=False, dims=dims, rays=rays, b_true=T(rs.uniform(0.2, 0.8, (n, 3))),
                noise=T(rs.standard_normal((n, 3))), aud=T(rs.standard_normal(64)), expr=T(rs.standard_normal(76)),
                latent=torch.ones(32), coarse=params(60), fine=params(61))


def recovery_weights(sc):
    """(last_weight of the fine pass, of the coarse pass) by the oracle's own render of the recovery scene (perturb 0)."""
    with torch.no_grad():
        o = oracle.render_rays(sc["rays"], sc["b_true"], sc["coarse"], sc["fine"], sc["aud"], sc["expr"], sc["latent"],
                               n_samples=sc["S"], n_importance=sc["Ni"], dims=sc["dims"], taps=True)
    return o["tap_weights_fine"][:, -1], o["tap_weights_coarse"][:, -1]
