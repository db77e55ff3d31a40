"""Pose refinement without a GPU: the rotation formula against ``torch.matrix_exp``, the rule that refines a ray batch
against rays built from the refined camera, the new C entry's argument checks, the checkpoint's ``pose_deltas`` and the
optimizer group's rate."""
import ctypes as C
import math

import pytest
import torch

import oracle
from test_facenerf_autograd_cpu import _fake_params

ANGLES = (0.0, 1e-9, 1e-4, 0.3, math.pi - 0.01)
# float64 agreement of Rodrigues' formula (pose_refine.rotation) and torch.matrix_exp of the skew matrix, measured on this
# code over the five angles x five seeded axes: value 7.5e-16, gradient 2.4e-15 (a few ulps of entries of size <= 1 and of
# gradients of size <= ~4).  The bounds leave a factor ~5 for another BLAS / libm.
TOL_VALUE, TOL_GRAD = 4e-15, 1.2e-14


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    return idealnerf_amd


def _skew(w):
    o = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([o, -w[2], w[1]]), torch.stack([w[2], o, -w[0]]), torch.stack([-w[1], w[0], o])])


def test_rotation_at_zero_is_the_identity_exactly(idn):
    from idealnerf_amd.pose_refine import rotation
    for dt in (torch.float32, torch.float64):
        assert torch.equal(rotation(torch.zeros(3, dtype=dt)), torch.eye(3, dtype=dt))
    assert torch.equal(rotation(torch.zeros(4, 3)), torch.eye(3).expand(4, 3, 3))


@pytest.mark.parametrize("angle", ANGLES)
def test_rotation_and_its_gradient_equal_matrix_exp(idn, angle):
    from idealnerf_amd.pose_refine import rotation
    gen = torch.Generator().manual_seed(0)
    for _ in range(5):
        axis = torch.randn(3, dtype=torch.float64, generator=gen)
        axis /= axis.norm()
        G = torch.randn(3, 3, dtype=torch.float64, generator=gen)
        w = (axis * angle).requires_grad_(True)
        R = rotation(w)
        g, = torch.autograd.grad((R * G).sum(), w)
        E = torch.matrix_exp(_skew(w))
        ge, = torch.autograd.grad((E * G).sum(), w)
        e_v, e_g = float((R - E).detach().abs().max()), float((g - ge).abs().max())
        print(f"angle {angle:g}: |R - expm| {e_v:.2e}  |dR - d expm| {e_g:.2e}")
        assert torch.isfinite(g).all()
        assert e_v <= TOL_VALUE and e_g <= TOL_GRAD
        assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).detach().abs().max()) < 1e-14


def test_delta_on_a_ray_batch_equals_rays_of_the_refined_camera(idn):
    """rays_o + tau, rays_d @ R(omega)^T against oracle.camera_rays of c2w' = [R(omega) R | t + tau] at the same pixels, in
    float64.  rays_d' = (dirs R_i^T) R^T on one side and dirs (R R_i)^T on the other: the two differ by the rounding of one
    3 x 3 product -- each entry is a 3-term dot product of 3-term dot products, |error| <= gamma_6 sum |terms| <= 6 eps 3 max|.|^2
    ~ 18 eps max|rays_d|; the bound is 32 eps max|rays_d|.  The origins are one addition on both sides: equal."""
    from idealnerf_amd.pose_refine import PoseRefiner, refined_c2w
    torch.set_default_dtype(torch.float64)
    try:
        syn = oracle.synthetic_frame(48, 80, seed=3)
        c2w = syn["c2w"].double()
        ref = PoseRefiner(4).double()
        with torch.no_grad():
            ref.deltas[2] = torch.tensor([0.02, -0.013, 0.007, 0.004, -0.002, 0.009], dtype=torch.float64)
        ro, rd = oracle.camera_rays(48, 80, syn["focal"], c2w, cx=30.25, cy=20.5)
        pix = torch.tensor([0, 17, 333, 48 * 80 - 1])
        batch = torch.stack([ro.reshape(-1, 3)[pix], rd.reshape(-1, 3)[pix]])            # [2, n, 3], as the loaders return it
        got = ref(2, batch)
        ro2, rd2 = oracle.camera_rays(48, 80, syn["focal"], ref.c2w(2, c2w), cx=30.25, cy=20.5)
        assert torch.equal(ref.c2w(2, c2w), refined_c2w(ref.deltas[2], c2w))
        assert got.shape == batch.shape
        assert torch.equal(got[0], ro2.reshape(-1, 3)[pix])
        bound = 32 * torch.finfo(torch.float64).eps * float(rd.abs().max())
        err = float((got[1] - rd2.reshape(-1, 3)[pix]).detach().abs().max())
        print(f"rays_d: {err:.2e} (bound {bound:.2e})")
        assert err <= bound
        assert float((got[1] - batch[1]).abs().max()) > 1e-3                             # the delta did something
        assert torch.equal(ref(0, batch), batch)                                         # a zero delta is the identity, exactly
        # a leading batch dimension (the reference loader behind a DataLoader) and the graph edge to the frame's row alone
        g, = torch.autograd.grad(ref(2, batch[None]).sum(), ref.deltas)
        assert g[2].abs().min() > 0 and float(g[[0, 1, 3]].abs().max()) == 0.0
    finally:
        torch.set_default_dtype(torch.float32)


def test_pass_bwd_rays_is_declared_and_checks_its_arguments(idn):
    """The new entry is exported, declared in _lib.PROTOTYPES, and answers argument errors before any HIP call (no GPU here)."""
    L = idn._lib
    lib = L.load()
    assert "idealnerf_pass_bwd_rays" in L.PROTOTYPES
    proto, base = L.PROTOTYPES["idealnerf_pass_bwd_rays"], L.PROTOTYPES["idealnerf_pass_bwd"]
    assert proto[0] is C.c_int and len(proto[1]) == len(base[1]) + 1            # idealnerf_pass_bwd's arguments + d_rays
    assert lib.idealnerf_pass_bwd_rays.argtypes == proto[1]
    assert lib.idealnerf_version() == L.ABI_VERSION                          # additive: the version did not move
    F = 256
    p, g = _fake_params(idn)
    ws_bytes = lib.idealnerf_pass_bwd_workspace_bytes(8, 64)

    def call(p_=C.byref(p), g_=C.byref(g), n=8, S=64, ws=F, nbytes=ws_bytes, **kw):
        a = dict(dict(aud=F, expr=F, latent=F, acts=F, raw=F, z=F, rays=F, bc=F), **kw)
        return lib.idealnerf_pass_bwd_rays(p_, g_, a["aud"], a["expr"], a["latent"], a["acts"], a["raw"], a["z"], a["rays"], a["bc"],
                                           n, S, None, None, None, None, None, None, F, ws, nbytes, None)

    assert call(p_=None) == -1 and call(g_=None) == -1
    assert call(g_=C.byref(L.FaceNerfGrads())) == -1
    for name in ("acts", "raw", "z", "rays", "bc"):
        assert call(**{name: None}) == -1, name                                  # IDN_EINVAL
        assert b"NULL" in lib.idealnerf_last_error()
    assert call(expr=None) == -1                                                 # dim_expr = 76 needs expr
    assert call(n=-1) == -1
    assert call(n=0) == 0
    assert call(nbytes=ws_bytes - 1) == -4                                       # IDN_EWORKSPACE
    assert b"workspace" in lib.idealnerf_last_error()
    assert call(ws=None) == -4
    assert call(S=1) == -2 and call(S=513) == -2                                 # IDN_EUNSUPPORTED: outside the compiled sizes
    # the workspace is the pass's own: the input-row gradient lives in a delta matrix the pass has finished with
    assert lib.idealnerf_pass_bwd_workspace_bytes(2, 512) == lib.idealnerf_facenerf_bwd_workspace_bytes(1024)


def test_checkpoint_carries_pose_deltas_only_when_asked(idn, tmp_path):
    from idealnerf_amd import checkpoint
    from idealnerf_amd.pose_refine import PoseRefiner
    net = torch.nn.Linear(3, 2)
    codes = torch.ones(6, 32, requires_grad=True)
    ref = PoseRefiner(6)
    with torch.no_grad():
        ref.deltas.copy_(torch.arange(36, dtype=torch.float32).reshape(6, 6) * 1e-3)
    opt = torch.optim.Adam(list(net.parameters()) + [codes], lr=8e-4)
    off, on = str(tmp_path / "off" / "head.tar"), str(tmp_path / "on" / "head.tar")
    checkpoint.save_checkpoint(off, net, opt, codes, 5)
    assert set(torch.load(off, weights_only=False)) == {"global_step", "model_state_dict", "optimizer", "latent_codes"}
    with pytest.raises(KeyError, match="pose_deltas"):
        checkpoint.load_pose_deltas(off)
    checkpoint.save_checkpoint(on, net, opt, codes, 5, pose_deltas=ref.deltas)
    ck = torch.load(on, weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer", "latent_codes", "pose_deltas"}
    back = checkpoint.load_pose_deltas(on)
    assert torch.equal(back, ref.deltas.detach()) and not back.requires_grad
    with torch.no_grad():
        ref.deltas.zero_()                                                       # the file holds a copy, not the parameter
    assert float(checkpoint.load_pose_deltas(on).abs().max()) > 0
    step, saved = checkpoint.load_checkpoint(on, torch.nn.Linear(3, 2), None)    # the other keys read as before
    assert step == 5 and torch.equal(saved, codes.detach())
    # the baseline's file: its three keys, or four
    base_off, base_on = str(tmp_path / "b_off.tar"), str(tmp_path / "b_on.tar")
    checkpoint.save_baseline_checkpoint(base_off, net, opt, 3)
    checkpoint.save_baseline_checkpoint(base_on, net, opt, 3, pose_deltas=ref.deltas)
    assert set(torch.load(base_off, weights_only=False)) == {"global_step", "model_state_dict", "optimizer"}
    assert set(torch.load(base_on, weights_only=False)) == {"global_step", "model_state_dict", "optimizer", "pose_deltas"}


def test_pose_group_decays_by_the_same_schedule_at_its_own_rate(idn):
    """The loop's update tail: a group with ``lr_scale`` (the pose deltas) gets scale x the decayed rate, every other group the
    decayed rate itself, as before."""
    from idealnerf_amd import train as T_
    from idealnerf_amd.pose_refine import PoseRefiner
    w = torch.nn.Parameter(torch.ones(3))
    ref = PoseRefiner(2)
    opt = torch.optim.Adam([w], lr=8e-4)
    opt.add_param_group({"params": [ref.deltas], "lr": 8e-5, "lr_scale": 0.1})
    loss = (w * w).sum() + (ref.deltas[1] * torch.arange(6.0)).sum()
    new = T_._backward_and_update(loss, opt, 300, 8e-4, 500)
    assert new == T_.decayed_lr(8e-4, 500, 300)
    assert opt.param_groups[0]["lr"] == new and "lr_scale" not in opt.param_groups[0]
    assert opt.param_groups[1]["lr"] == new * 0.1
    d = ref.deltas.detach()
    assert float(d[0].abs().max()) == 0.0                                        # the frame not visited did not move
    assert float(d[1, 0]) == 0.0 and torch.allclose(d[1, 1:], torch.full((5,), -8e-5), rtol=1e-4)   # Adam's first step: -lr sign(g)
