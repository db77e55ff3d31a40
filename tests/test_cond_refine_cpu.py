"""Expression and background refinement without a GPU: the new C entry's argument checks, ``ExprRefiner`` and ``Background``,
the checkpoint's ``expr_deltas`` / ``background``, the trainers' argument errors, and the oracle-only conditions the GPU tests
of tests/test_cond_grad_gpu.py stand on (no scene too sharp; the recovery run's margin)."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import cond_grad_common as cg
import ray_grad_common as rg
from test_facenerf_autograd_cpu import _fake_params


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    return idealnerf_amd


def test_pass_bwd_ex_is_declared_and_checks_its_arguments(idn):
    """The new entry is exported, declared in _lib.PROTOTYPES (idealnerf_pass_bwd's arguments + the struct pointer), and
    answers argument errors before any HIP call (there is no GPU here: a launch would fail otherwise)."""
    L = idn._lib
    lib = L.load()
    proto, base = L.PROTOTYPES["idealnerf_pass_bwd_ex"], L.PROTOTYPES["idealnerf_pass_bwd"]
    assert proto[0] is C.c_int and len(proto[1]) == len(base[1]) + 1
    assert lib.idealnerf_pass_bwd_ex.argtypes == proto[1]
    assert lib.idealnerf_version() == L.ABI_VERSION                          # additive: the version did not move
    assert [f[0] for f in L.PassBwdExtra._fields_] == ["d_expr", "d_rays", "d_views0_bias"]
    F = 256
    p, g = _fake_params(idn)
    p0, _ = _fake_params(idn, dims=(64, 0, 32))
    ws_bytes = lib.idealnerf_pass_bwd_workspace_bytes(8, 64)

    def call(p_=p, g_=g, extra=None, n=8, S=64, ws=F, nbytes=ws_bytes, d_aud=None, d_latent=None, **kw):
        a = dict(dict(aud=F, expr=F, latent=F, acts=F, raw=F, z=F, rays=F, bc=F), **kw)
        ex = None if extra is None else C.byref(L.PassBwdExtra(**extra))
        return lib.idealnerf_pass_bwd_ex(None if p_ is None else C.byref(p_), None if g_ is None else C.byref(g_), a["aud"],
                                         a["expr"], a["latent"], a["acts"], a["raw"], a["z"], a["rays"], a["bc"], n, S, None,
                                         None, None, None, d_aud, d_latent, ex, ws, nbytes, None)

    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
    assert call(p_=None) == EINVAL
    assert call(g_=L.FaceNerfGrads()) == EINVAL                                   # a grads struct with NULL entries
    # d_expr for a network without an expression
    assert call(p_=p0, expr=None, extra=dict(d_expr=F)) == EINVAL and b"d_expr" in lib.idealnerf_last_error()
    assert call(p_=p0, g_=None, expr=None, extra=dict(d_expr=F)) == EINVAL
    assert call(expr=None, extra=dict(d_expr=F)) == EINVAL                        # dim_expr = 76 needs expr
    # the frozen plan (grads NULL) has no ray gradient
    assert call(g_=None, extra=dict(d_rays=F), d_aud=F) == EUNSUPPORTED and b"ray" in lib.idealnerf_last_error()
    assert call(g_=None, extra=dict(d_rays=F)) == EUNSUPPORTED
    # d_views0_bias: the frozen plan only, and only beside a wanted conditioning gradient
    assert call(extra=dict(d_views0_bias=F)) == EINVAL
    assert call(g_=None, extra=dict(d_views0_bias=F)) == EINVAL
    # a short workspace, either plan, any extra
    for g_, extra, d_aud in ((g, None, None), (g, dict(d_expr=F), None), (g, dict(d_rays=F), None), (None, dict(d_expr=F), None),
                             (None, dict(d_views0_bias=F), F), (None, None, F)):
        assert call(g_=g_, extra=extra, d_aud=d_aud, nbytes=ws_bytes - 1) == EWORKSPACE, (g_, extra)
        assert b"workspace" in lib.idealnerf_last_error()
        assert call(g_=g_, extra=extra, d_aud=d_aud, ws=None) == EWORKSPACE
    for name in ("acts", "raw", "z", "rays", "bc"):
        assert call(extra=dict(d_expr=F), **{name: None}) == EINVAL, name
        assert call(g_=None, extra=dict(d_expr=F), **{name: None}) == EINVAL, name
    assert call(n=-1) == EINVAL and call(n=0) == 0
    assert call(S=1, extra=dict(d_expr=F)) == EUNSUPPORTED
    # the frozen plan with nothing wanted launches nothing: no workspace, no inputs needed
    assert call(g_=None, ws=None, nbytes=0, acts=None) == 0
    assert call(g_=None, extra=dict(), ws=None, nbytes=0, acts=None) == 0


def test_expr_refiner_is_the_identity_at_zero_and_its_gradient_reaches_one_row(idn):
    from idealnerf_amd.cond_refine import ExprRefiner
    ref = ExprRefiner(5, 76)
    assert ref.deltas.shape == (5, 76) and ref.deltas.dtype == torch.float32 and float(ref.deltas.detach().abs().max()) == 0.0
    expr = torch.randn(76, generator=torch.Generator().manual_seed(0))
    assert torch.equal(ref(3, expr), expr)                                       # zeros: the identity, exactly
    assert torch.equal(ref(3, expr[None]), expr[None])                           # a leading batch dimension (a DataLoader's)
    w = torch.arange(76, dtype=torch.float32)
    g, = torch.autograd.grad((ref(3, expr) * w).sum(), ref.deltas)
    assert torch.equal(g[3], w) and float(g[[0, 1, 2, 4]].abs().max()) == 0.0
    with torch.no_grad():
        ref.deltas[3] = 0.5
    assert torch.equal(ref(3, expr), expr + 0.5) and torch.equal(ref(2, expr), expr)
    assert ref(3, expr.double()).dtype == torch.float32


def test_background_starts_as_uint8_over_255_and_sums_repeated_indices(idn):
    from idealnerf_amd.cond_refine import Background
    img = torch.randint(0, 256, (4, 5, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    bg = Background(img)
    assert bg.image.dtype == torch.float32 and bg.image.shape == (4, 5, 3) and bg.image.requires_grad
    unit = (img.to(torch.float64) / 255.0).to(torch.float32)                    # numpy's uint8 / 255.0, then Network.forward's cast
    assert torch.equal(bg.image.detach(), unit) and float((unit - img.to(torch.float32) / 255.0).abs().max()) < 1e-7
    assert bg() is bg.image                                                      # the whole image for a full-frame render
    sel = torch.tensor([7, 0, 7, 19])
    rows = bg.rows(sel)
    assert torch.equal(rows.detach(), unit.reshape(-1, 3)[sel])
    w = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [10.0, 20.0, 30.0], [0.5, 0.25, 0.125]])
    g, = torch.autograd.grad((rows * w).sum(), bg.image)
    g = g.reshape(-1, 3)
    assert torch.equal(g[7], w[0] + w[2]) and torch.equal(g[0], w[1]) and torch.equal(g[19], w[3])
    others = [i for i in range(20) if i not in (0, 7, 19)]
    assert float(g[others].abs().max()) == 0.0
    with torch.no_grad():                                                        # nothing clamps the values
        bg.image[0, 0] = torch.tensor([-0.25, 1.5, 0.5])
    assert torch.equal(bg.rows(torch.tensor([0])).detach()[0], torch.tensor([-0.25, 1.5, 0.5]))
    with pytest.raises(ValueError):
        Background(torch.zeros(4, 5))


def test_checkpoint_carries_expr_deltas_and_background_only_when_asked(idn, tmp_path):
    from idealnerf_amd import checkpoint
    net = torch.nn.Linear(3, 2)
    codes = torch.ones(6, 32, requires_grad=True)
    deltas = torch.nn.Parameter(torch.arange(6 * 76, dtype=torch.float32).reshape(6, 76) * 1e-3)
    image = torch.nn.Parameter(torch.rand(4, 5, 3, generator=torch.Generator().manual_seed(2)) * 1.5 - 0.25)
    opt = torch.optim.Adam(list(net.parameters()) + [codes], lr=8e-4)
    base = {"global_step", "model_state_dict", "optimizer", "latent_codes"}
    off, on = str(tmp_path / "off" / "head.tar"), str(tmp_path / "on" / "head.tar")
    checkpoint.save_checkpoint(off, net, opt, codes, 5)
    assert set(torch.load(off, weights_only=False)) == base
    with pytest.raises(KeyError, match="expr_deltas"):
        checkpoint.load_expr_deltas(off)
    with pytest.raises(KeyError, match="background"):
        checkpoint.load_background(off)
    checkpoint.save_checkpoint(on, net, opt, codes, 5, expr_deltas=deltas, background=image)
    assert set(torch.load(on, weights_only=False)) == base | {"expr_deltas", "background"}
    back_e, back_b = checkpoint.load_expr_deltas(on), checkpoint.load_background(on)
    assert torch.equal(back_e, deltas.detach()) and not back_e.requires_grad
    assert torch.equal(back_b, image.detach()) and not back_b.requires_grad and back_b.dtype == torch.float32
    with torch.no_grad():
        deltas.zero_()                                                           # the file holds copies, not the parameters
        image.zero_()
    assert float(checkpoint.load_expr_deltas(on).abs().max()) > 0 and float(checkpoint.load_background(on).abs().max()) > 0
    with pytest.raises(KeyError, match="pose_deltas"):
        checkpoint.load_pose_deltas(on)
    step, saved = checkpoint.load_checkpoint(on, torch.nn.Linear(3, 2), None)    # the other keys read as before
    assert step == 5 and torch.equal(saved, codes.detach())
    one = str(tmp_path / "one.tar")
    checkpoint.save_checkpoint(one, net, opt, codes, 5, background=image)
    assert set(torch.load(one, weights_only=False)) == base | {"background"}
    # the baseline's file: its three keys, or four
    b_off, b_on = str(tmp_path / "b_off.tar"), str(tmp_path / "b_on.tar")
    checkpoint.save_baseline_checkpoint(b_off, net, opt, 3)
    checkpoint.save_baseline_checkpoint(b_on, net, opt, 3, background=image)
    assert set(torch.load(b_off, weights_only=False)) == {"global_step", "model_state_dict", "optimizer"}
    assert set(torch.load(b_on, weights_only=False)) == {"global_step", "model_state_dict", "optimizer", "background"}


def test_trainer_argument_errors_come_before_any_dataset_is_read(idn):
    from idealnerf_amd import train, train_agg, train_baseline
    args = SimpleNamespace(dim_expr=76, datadir="/nonexistent", basedir="/nonexistent", expname="x")
    with pytest.raises(ValueError, match="refine_expr"):
        train_baseline.train(args, refine_expr=True, device="cpu")
    for fn in (train.train, train_agg.train, train_baseline.train):
        with pytest.raises(ValueError, match="learn_background"):
            fn(args, loader="reference", learn_background=True, device="cpu")
    with pytest.raises(ValueError, match="refine_expr"):                          # a head network built without an expression
        train.train(SimpleNamespace(dim_expr=0), refine_expr=True, device="cpu")


def test_new_parameter_groups_decay_by_the_same_schedule_at_their_own_rates(idn):
    from idealnerf_amd import train as T_
    from idealnerf_amd.cond_refine import Background, ExprRefiner
    w = torch.nn.Parameter(torch.ones(3))
    ref, bg = ExprRefiner(2, 4), Background(torch.full((2, 2, 3), 128, dtype=torch.uint8))
    opt = torch.optim.Adam([w], lr=8e-4)
    opt.add_param_group({"params": [ref.deltas], "lr": 8e-5, "lr_scale": 0.1})
    opt.add_param_group({"params": [bg.image], "lr": 8e-4, "lr_scale": 1.0})
    loss = (w * w).sum() + ref(1, torch.zeros(4)).sum() + bg.rows(torch.tensor([3, 3])).sum()
    new = T_._backward_and_update(loss, opt, 300, 8e-4, 500)
    assert opt.param_groups[0]["lr"] == new and opt.param_groups[1]["lr"] == new * 0.1 and opt.param_groups[2]["lr"] == new * 1.0
    assert float(ref.deltas.detach()[0].abs().max()) == 0.0 and torch.allclose(ref.deltas.detach()[1], torch.full((4,), -8e-5), rtol=1e-4)
    moved = (bg.image.detach().reshape(-1, 3) - 128 / 255.0)
    assert float(moved[:3].abs().max()) == 0.0 and torch.allclose(moved[3], torch.full((3,), -8e-4), rtol=1e-3)


@pytest.mark.parametrize("name", cg.CASES)
def test_no_scene_is_too_sharp_for_d_expr_and_d_bc(name):
    """The fp32 oracle against the fp64 oracle at the oracle's own depths: e32 of d expr and of d bc stays below 1e-3 on every
    scene the GPU test uses, no ray has a zero d bc row and d expr is far above the bound's floor -- so a scene that cannot
    test these gradients fails here, without a GPU.  Measured: d expr 3.1e-7, 2.8e-5, 4.6e-7, 1.2e-6, n/a; d bc 6.0e-7, 2.4e-6,
    1.6e-6, 6.6e-7, 1.5e-6 (3x64+128, 37x64+128, 26x5, 2x256+256, 37x64+128fg)."""
    sc = rg.scene(name)
    z_c, z_f = rg.oracle_depths(sc)
    e64, b64 = cg.oracle_d_cond(sc, z_c, z_f, torch.float64)
    e32, b32 = cg.oracle_d_cond(sc, z_c, z_f, torch.float32)
    assert (e64 is None) == sc["fg"]
    floor_bc = cg.rel(b32, b64)
    print(f"\n{name}: e32 of d bc {floor_bc:.2e}" + ("" if e64 is None else f", of d expr {cg.rel(e32, e64):.2e}, max |d expr| {float(e64.abs().max()):.3f}"))
    assert floor_bc < cg.TOO_SHARP
    assert float(b64.abs().max(dim=1)[0].min()) > 0.0
    if e64 is not None:
        assert cg.rel(e32, e64) < cg.TOO_SHARP
        assert float(e64.abs().max()) > 0.01


def test_recovery_run_of_the_oracle_passes_with_a_factor_two_to_spare():
    """The step count and rate of the GPU's background-recovery test, chosen here with the oracle alone: on the oracle's own
    last weights the model run brings |B - B*| of every ray with last_weight > 0.1 below HALF of where it started (measured:
    the worst ray ends at 0.40 of its start after 20 Adam steps at 2e-2; the loss at 0.049 of its start)."""
    sc = cg.recovery_scene()
    lw_f, lw_c = cg.recovery_weights(sc)
    before, after, loss0, loss1 = cg.recovery_run(lw_f, lw_c, sc["b_true"], sc["noise"])
    m = lw_f > 0.1
    assert int(m.sum()) >= 32
    worst = float((after[m] / before[m]).max())
    print(f"\nrecovery: {int(m.sum())} rays above 0.1, worst after / before {worst:.3f}, loss {loss1 / loss0:.4f}")
    assert worst < 0.5 and loss1 < 0.5 * loss0


def test_learned_background_replaces_the_loaders_background_or_raises(idn, tmp_path):
    """drive's helper behind --learned_background: the checkpoint's background goes where the test-time loaders keep bc.jpg;
    no checkpoint -> ValueError, a checkpoint without one -> KeyError."""
    from idealnerf_amd import checkpoint, drive
    net, codes = torch.nn.Linear(3, 2), torch.ones(2, 32)
    image = torch.rand(4, 5, 3, generator=torch.Generator().manual_seed(4))
    off, on = str(tmp_path / "off.tar"), str(tmp_path / "on.tar")
    checkpoint.save_checkpoint(off, net, None, codes, 1)
    checkpoint.save_checkpoint(on, net, None, codes, 1, background=image)
    frames = SimpleNamespace(background_img=torch.zeros(4, 5, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="no checkpoint"):
        drive._learned_background(frames, None, "cpu")
    with pytest.raises(KeyError, match="background"):
        drive._learned_background(frames, off, "cpu")
    assert float(frames.background_img.abs().max()) == 0.0
    drive._learned_background(frames, on, "cpu")
    assert torch.equal(frames.background_img, image)
