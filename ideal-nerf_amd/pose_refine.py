"""Joint refinement of the per-frame camera poses during training (in the manner of NeRF-- and BARF; the reference has no
counterpart: it compensates the tracker's jitter with per-frame latent codes only).

The poses of ``transforms_exp_*.json`` come from a face tracker, frame by frame.  ``PoseRefiner`` holds one correction
``(omega, tau)`` per training frame, initialised to zero, and the refined camera of frame i is

    c2w'_i = [R(omega_i) . R_i | t_i + tau_i],          R(omega) = exp([omega]_x)   (Rodrigues)

Because the correction multiplies from the LEFT, it applies to any ray batch of frame i without pixel coordinates:

    rays_o' = rays_o + tau_i,        rays_d' = rays_d @ R(omega_i)^T

(``rays_d = dirs @ R_i^T``, helper.py:240, so ``dirs @ (R R_i)^T = rays_d @ R^T``): both loaders' batches are refined as
they are, the sampler and the gather kernel do not change.  The gradient reaches the deltas through the ray records:
``autograd.RenderRaysFn`` returns d rays when, and only when, the rays require one (``idealnerf_pass_bwd_rays``).
"""
import torch

# below this squared angle the coefficients come from their Taylor series: both branches are exact to fp64 rounding there
# (the first dropped term is theta^8 / 9! < 3e-22), and the series has a finite, correct gradient at omega = 0
SERIES_BELOW_SQ = 1e-4


def rotation(omega: torch.Tensor) -> torch.Tensor:
    """omega [..., 3] -> R [..., 3, 3] = I + A K + B K^2 with K = [omega]_x, t = |omega|^2, A = sin(theta) / theta and
    B = (1 - cos theta) / theta^2 = 2 sin^2(theta / 2) / t (no cancellation).  Written in t, never in theta alone: value and
    gradient are finite and correct at omega = 0, where R = I exactly."""
    t = (omega * omega).sum(-1)
    small = t < SERIES_BELOW_SQ
    ts = torch.where(small, torch.ones_like(t), t)       # the branch not taken still sees a safe argument (no NaN gradient)
    theta = torch.sqrt(ts)
    a_big = torch.sin(theta) / theta
    b_big = 2.0 * torch.sin(0.5 * theta) ** 2 / ts
    tt = torch.where(small, t, torch.zeros_like(t))
    a_small = 1.0 - tt / 6.0 * (1.0 - tt / 20.0 * (1.0 - tt / 42.0))
    b_small = 0.5 - tt / 24.0 * (1.0 - tt / 30.0 * (1.0 - tt / 56.0))
    A = torch.where(small, a_small, a_big)[..., None, None]
    B = torch.where(small, b_small, b_big)[..., None, None]
    x, y, z = omega[..., 0], omega[..., 1], omega[..., 2]
    o = torch.zeros_like(x)
    K = torch.stack([torch.stack([o, -z, y], -1), torch.stack([z, o, -x], -1), torch.stack([-y, x, o], -1)], -2)
    eye = torch.eye(3, dtype=omega.dtype, device=omega.device).expand(K.shape)
    return eye + A * K + B * (K @ K)


def apply_delta(delta: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor):
    """One frame's correction delta [6] = (omega, tau) on a ray batch of that frame: rays_o [..., 3], rays_d [..., 3] ->
    (rays_o + tau, rays_d @ R(omega)^T)."""
    R = rotation(delta[:3])
    return rays_o + delta[3:], rays_d @ R.transpose(-1, -2)


def refined_c2w(delta: torch.Tensor, c2w: torch.Tensor) -> torch.Tensor:
    """c2w [3 or 4, 4] -> [R(omega) R | t + tau] (rows beyond the third unchanged)."""
    top = torch.cat([rotation(delta[:3]) @ c2w[:3, :3], (c2w[:3, 3] + delta[3:])[:, None]], dim=1)
    return torch.cat([top, c2w[3:]], dim=0)


class PoseRefiner(torch.nn.Module):
    """``deltas[n_frames, 6] = (omega, tau)`` per training frame, zero at the start (the tracker's poses)."""

    def __init__(self, n_frames: int):
        super().__init__()
        self.deltas = torch.nn.Parameter(torch.zeros(int(n_frames), 6, dtype=torch.float32))

    def forward(self, index: int, batch_rays: torch.Tensor) -> torch.Tensor:
        """batch_rays [..., 2, n, 3] = (rays_o, rays_d) of frame ``index``, as either loader returns them -> the refined batch
        of the same shape, on the deltas' device, with the graph edge to ``deltas[index]``."""
        br = batch_rays.to(device=self.deltas.device, dtype=self.deltas.dtype)
        o, d = apply_delta(self.deltas[int(index)], br[..., 0, :, :], br[..., 1, :, :])
        return torch.stack([o, d], dim=-3)

    def c2w(self, index: int, c2w: torch.Tensor) -> torch.Tensor:
        return refined_c2w(self.deltas[int(index)].to(c2w.dtype), c2w.to(self.deltas.device))


def pose_errors(c2w_a: torch.Tensor, c2w_b: torch.Tensor):
    """Two stacks of cameras [n, 3+, 4] -> (rotation error in degrees [n], translation error [n])."""
    Ra, Rb = c2w_a[:, :3, :3].double(), c2w_b[:, :3, :3].double()
    rel = Ra @ Rb.transpose(1, 2)
    cos = ((rel.diagonal(dim1=1, dim2=2).sum(-1) - 1.0) * 0.5).clamp(-1.0, 1.0)
    return torch.rad2deg(torch.acos(cos)), (c2w_a[:, :3, 3].double() - c2w_b[:, :3, 3].double()).norm(dim=-1)
