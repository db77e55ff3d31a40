"""The render backward's gradients with respect to the expression and the background, and their refinement end to end (run
with ``-m gpu``).

Case 1 -- d expr and d bc of ``Network.render_rays`` against the CPU oracle's float64 autograd with both as leaves, evaluated at
the sample depths the HIP forward used (the method and the scenes of tests/test_ray_grad_gpu.py).  Bound per block:
max |HIP - fp64| / max |fp64| <= max(4 e32, 5e-6); e32 = the fp32 oracle's own distance from the fp64 oracle on that scene,
measured here; 4 x is test_ray_grad_gpu.py's margin, 5e-6 the bound tests/test_torso_train_gpu.py holds d aud / d latent to
(d expr comes out of the same fold).  Both training arithmetics: this process's and, in a child, the other one.  With the
ORACLE's depths on the CPU (tests/test_cond_refine_cpu.py) e32 of d expr is 3.1e-7, 2.8e-5, 4.6e-7, 1.2e-6 and of d bc 6.0e-7,
2.4e-6, 1.6e-6, 6.6e-7, 1.5e-6 in the order of ray_grad_common.CASES.  $IDN_COND_GRAD_RECORD names a JSON file the figures are
merged into (profiles/cond_grad_parity.json).
Case 2 -- nothing else moved: the 24 parameter gradients, d aud and d latent of ``ops.pass_bwd_ex`` are ``ops.pass_bwd``'s /
``ops.pass_bwd_rays``' bit for bit, whatever extras it is asked for.
Case 3 -- the frozen plan (``grads=None``) against fp64 column sums of the deltas it leaves in a poisoned workspace.
Case 4 -- the autograd surface: ``render_rays`` with ``expr`` / ``bc_rgb`` requiring gradients, the no-op path, a frozen pair,
``Background.rows`` with a repeated pixel.
Case 5 -- a noised background is recovered through a frozen pair.
Case 6 -- ``train(refine_expr=True, learn_background=True)``: both parameters move, the checkpoint, resume bit for bit; the agg
and the baseline trainer with the options.
"""
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import cond_grad_common as cg
import ray_grad_common as rg
import test_ray_grad_gpu as trg
from idealnerf_amd.synthetic import write_clip_directory
from test_delta_chain_gpu import SENTINEL
from train_loop_common import train_flags

pytestmark = pytest.mark.gpu

FROZEN_TOL = 5e-6   # the issue's: tests/test_torso_train_gpu.py's bound on d aud / d latent of the frozen plan


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()
    return idealnerf_amd


def _record(key, value):
    path = os.environ.get("IDN_COND_GRAD_RECORD")
    if not path:
        return
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(old, open(path, "w"), indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------ the HIP side of a case
_RUNS = {}


def _hip_d_cond(idn, dev, sc, expr_grad=True, bc_grad=True, entry="_render", cache=True):
    """One render of the case's rays in train mode and the backward of its loss -> dict(d_expr, d_bc, z_c, z_f, out, grads).
    entry: "_render" (either pair's shared body) or "render_rays" (the head Network's public method)."""
    from idealnerf_amd import autograd as ag
    key = (sc["name"], expr_grad, bc_grad, entry)
    if cache and key in _RUNS:
        return _RUNS[key]
    net, coarse, fine = trg._network(idn, dev, sc)
    g = lambda t: None if t is None else t.to(dev)
    rays = g(sc["rays"]).contiguous()
    bc = g(sc["bc"]).clone().requires_grad_(bc_grad)
    expr = None if sc["expr"] is None else g(sc["expr"]).clone().requires_grad_(expr_grad)
    zs = []
    real_query = ag._train_query
    ag._train_query = lambda net_, folded, r, z: (zs.append(z.detach().clone()), real_query(net_, folded, r, z))[1]
    try:
        for p in net.parameters():
            p.grad = None
        if entry == "render_rays":
            ret = net.render_rays(rays, bc, g(sc["aud"]), None, g(sc["latent"]), expr)
        else:
            ret = net._render(rays, bc, g(sc["aud"]), g(sc["latent"]), expr, coarse, fine, sc["fg"])
        rg.loss_of(ret, sc["weights"]).backward()
    finally:
        ag._train_query = real_query
    grads = {f"{tag}.{k}": p.grad.clone() for tag, m in (("c", coarse), ("f", fine)) for k, p in m.named_parameters()
             if p.grad is not None}
    run = dict(d_expr=None if expr is None or expr.grad is None else expr.grad.clone(),
               d_bc=None if bc.grad is None else bc.grad.clone(), z_c=zs[0], z_f=zs[1] if len(zs) > 1 else None,
               out={k: v.detach().clone() for k, v in ret.items()}, grads=grads)
    if cache:
        _RUNS[key] = run
    return run


_ORACLE = {}


def _oracle(sc, hip):
    """The fp64 and fp32 oracle gradients at the HIP forward's depths, once per scene (read-only afterwards)."""
    if sc["name"] not in _ORACLE:
        _ORACLE[sc["name"]] = (cg.oracle_d_cond(sc, hip["z_c"], hip["z_f"], torch.float64),
                               cg.oracle_d_cond(sc, hip["z_c"], hip["z_f"], torch.float32))
    return _ORACLE[sc["name"]]


# ------------------------------------------------------------------------------------------------ case 1
@pytest.mark.parametrize("name", cg.CASES)
def test_d_expr_and_d_bc_vs_fp64_oracle(idn, dev, name):
    from idealnerf_amd import autograd as ag
    sc = rg.scene(name)
    hip = _hip_d_cond(idn, dev, sc)
    (e64, b64), (e32, b32) = _oracle(sc, hip)
    d_bc, d_expr = hip["d_bc"], hip["d_expr"]
    assert d_bc is not None and d_bc.shape == (sc["n"], 3) and torch.isfinite(d_bc).all()
    assert (d_expr is None) == sc["fg"]                                          # the torso pair takes no expression
    figures = {"bc": (cg.rel(d_bc, b64), cg.rel(b32, b64))}
    if d_expr is not None:
        assert d_expr.shape == (76,) and torch.isfinite(d_expr).all()
        figures["expr"] = (cg.rel(d_expr, e64), cg.rel(e32, e64))
    print(f"\n{name} [{ag.TRAIN_PRECISION}]: " + "  ".join(f"d {k}: HIP {got:.2e} e32 {floor:.2e} bound {cg.bound(floor):.2e}"
                                                             for k, (got, floor) in figures.items()))
    _record(f"{name}/{ag.TRAIN_PRECISION}", {k: dict(hip=got, e32=floor, bound=cg.bound(floor)) for k, (got, floor) in figures.items()})
    assert float(b64.abs().max(dim=1)[0].min()) > 0.0                            # no ray has a zero d bc row
    for k, (got, floor) in figures.items():
        assert floor < cg.TOO_SHARP, "the scene is too sharp to test a gradient on"
        assert got <= cg.bound(floor), (name, k, got, cg.bound(floor))


def test_d_cond_cases_on_the_other_training_precision(idn, dev):
    """IDN_TRAIN_PRECISION is read once at import: the five cases again in a fresh process on the other arithmetic."""
    from idealnerf_amd import autograd as ag
    other = "f32" if ag.TRAIN_PRECISION == "bf16x6" else "bf16x6"
    env = dict(os.environ, IDN_TRAIN_PRECISION=other)
    child = subprocess.Popen([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-k",
                              "test_d_expr_and_d_bc_vs_fp64_oracle"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             text=True, start_new_session=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        out, err = child.communicate(timeout=180)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.wait()
        pytest.fail("the child run did not finish within 180 s")
    print(out[-4000:])
    assert child.returncode == 0 and f"{len(cg.CASES)} passed" in out, out[-4000:] + err[-2000:]


# ------------------------------------------------------------------------------------------------ cases 2 and 3: one pass
def _coarse_pass(idn, dev, name):
    """The coarse pass of a scene, forward done: everything ops.pass_bwd* takes, with seeded upstream gradients."""
    from idealnerf_amd import autograd as ag
    from idealnerf_amd.helper import linspace01
    ops = idn.ops
    sc = rg.scene(name)
    _, coarse, _ = trg._network(idn, dev, sc)
    g = lambda t: t.to(dev)
    rays, bc = g(sc["rays"]).contiguous(), g(sc["bc"]).contiguous()
    aud, expr, lat = g(sc["aud"]), g(sc["expr"]), g(sc["latent"])
    z = ops.coarse_depths(rays, linspace01(sc["S"], dev))
    raw, acts = ag._train_query(coarse, coarse.folded_bias(aud, expr, lat), rays, z)
    rs = np.random.RandomState(sc["S"])
    g_rgb = torch.from_numpy(rs.standard_normal((sc["n"], 3)).astype(np.float32)).to(dev)
    g_acc = torch.from_numpy(rs.standard_normal(sc["n"]).astype(np.float32)).to(dev)
    return dict(sc=sc, module=coarse, aud=aud, expr=expr, lat=lat, n=sc["n"], S=sc["S"],
                tail=(aud, expr, lat, acts, raw, z, rays, bc, g_rgb, None, None, g_acc))


@pytest.mark.parametrize("name", ["3x64+128", "26x5"])
def test_pass_bwd_ex_moves_nothing_else(idn, dev, name):
    """On 192 and 130 points (neither a multiple of the 128-row padding): with d_expr set, with every extra None and with
    d_rays set, the 24 parameter gradients, d aud and d latent of ops.pass_bwd_ex are ops.pass_bwd's bit for bit, d rays is
    ops.pass_bwd_rays' bit for bit, and d expr is the same whether or not d rays is computed beside it."""
    from idealnerf_amd import autograd as ag
    ops = idn.ops
    c = _coarse_pass(idn, dev, name)
    module, aud, lat = c["module"], c["aud"], c["lat"]
    sd = module.kernel_tensors()

    def run(fn, *extra, **kw):
        grads = {k: torch.full_like(sd[k], float("nan")) for k in ag.PARAM_KEYS}
        d_aud, d_lat = torch.zeros_like(aud), torch.zeros_like(lat)
        fn(module.kernel_params(), grads, *c["tail"], d_aud, d_lat, *extra, **kw)
        return dict(grads, d_aud=d_aud, d_lat=d_lat)
    base = run(ops.pass_bwd)
    d_rays_ref = torch.full((c["n"], 11), float("nan"), device=dev)
    run(ops.pass_bwd_rays, d_rays_ref)
    d_expr = torch.zeros(76, device=dev)
    d_expr2, d_rays = torch.zeros(76, device=dev), torch.full((c["n"], 11), float("nan"), device=dev)
    runs = {"d_expr": run(ops.pass_bwd_ex, d_expr=d_expr), "none": run(ops.pass_bwd_ex),
            "d_rays": run(ops.pass_bwd_ex, d_rays=d_rays.clone()), "both": run(ops.pass_bwd_ex, d_expr=d_expr2, d_rays=d_rays)}
    for tag, got in runs.items():
        for k in base:
            assert torch.isfinite(base[k]).all(), k
            assert torch.equal(base[k], got[k]), (name, tag, k)
    assert torch.equal(d_rays, d_rays_ref)
    assert torch.isfinite(d_expr).all() and float(d_expr.abs().max()) > 0 and torch.equal(d_expr, d_expr2)
    start = torch.from_numpy(np.random.RandomState(1).standard_normal(76).astype(np.float32)).to(dev)
    summed = start.clone()
    run(ops.pass_bwd_ex, d_expr=summed)
    assert torch.equal(summed, start + d_expr)                                   # accumulated: one fp32 addition per element


def _workspace(idn, dev, n, S):
    """This stream's backward scratch (ops._workspace), as int32 words."""
    lib = idn._lib.load()
    nbytes = lib.idealnerf_pass_bwd_workspace_bytes(n, S)
    ws = idn.ops._workspace(nbytes, dev, torch.cuda.current_stream(dev).cuda_stream)
    return ws[:nbytes // 4 * 4].view(torch.int32)


def _fp64_frozen_reference(idn, dev, module, n, S):
    """d cond [C], d expr [76] and dbv' [128] in float64 from the deltas the frozen plan has just left in the workspace
    (csrc/train.hip: carve_bwd -- [p_pad, 256] matrices: eight of pts_linears.l, one of views_linears.2 | .1, then dV0): column
    sums over the pass's real rows, then the fold's formulas."""
    P = n * S
    Pp = (P + 127) // 128 * 128
    words = _workspace(idn, dev, n, S).view(torch.float32)
    mat = lambda i: words[i * Pp * 256:(i + 1) * Pp * 256].view(Pp, 256)[:P].double()
    db0, db5, dbv = mat(0).sum(0), mat(5).sum(0), mat(9)[:, :128].sum(0)
    sd = {k: p.detach().double() for k, p in module.named_parameters()}
    W0, W5, Wv = sd["pts_linears.0.weight"], sd["pts_linears.5.weight"], sd["views_linears.0.weight"]
    C = W0.shape[1] - 63
    d_cond = db0 @ W0[:, 63:] + db5 @ W5[:, 63:63 + C]
    d_expr = (d_cond[64:64 + 76] + dbv @ Wv[:, 256 + 27:]) / 3.0
    return d_cond, d_expr, dbv


@pytest.mark.parametrize("name", ["26x5", "3x64+128"])
def test_frozen_plan_d_expr_and_views0_bias_vs_fp64_column_sums(idn, dev, name):
    """ops.pass_bwd_ex(grads=None) on a workspace filled with the sentinel of tests/test_delta_chain_gpu.py: d expr, d aud,
    d latent and d_views0_bias against fp64 column sums of the same saved deltas (relative 5e-6); d aud / d latent are
    ops.pass_bwd_cond's bit for bit; a second run from a freshly poisoned workspace gives the same bits."""
    ops = idn.ops
    c = _coarse_pass(idn, dev, name)
    module, aud, lat, n, S = c["module"], c["aud"], c["lat"], c["n"], c["S"]
    words = _workspace(idn, dev, n, S)

    def run():
        words.fill_(SENTINEL)
        out = dict(d_aud=torch.zeros_like(aud), d_lat=torch.zeros_like(lat), d_expr=torch.zeros(76, device=dev),
                   d_vb=torch.full((128,), float("nan"), device=dev))
        ops.pass_bwd_ex(module.kernel_params(), None, *c["tail"], out["d_aud"], out["d_lat"], d_expr=out["d_expr"],
                        d_views0_bias=out["d_vb"])
        return out
    try:
        a = run()
        d_cond, d_expr64, dbv64 = _fp64_frozen_reference(idn, dev, module, n, S)
        b = run()
        words.fill_(SENTINEL)
        old = dict(d_aud=torch.zeros_like(aud), d_lat=torch.zeros_like(lat))
        ops.pass_bwd_cond(module.kernel_params(), *c["tail"], old["d_aud"], old["d_lat"])
        only = torch.zeros(76, device=dev)
        words.fill_(SENTINEL)
        ops.pass_bwd_ex(module.kernel_params(), None, *c["tail"], None, None, d_expr=only)   # d expr alone runs the pass too
    finally:
        words.zero_()   # what the host layer promises later callers of this scratch: defined data
    errs = dict(d_expr=cg.rel(a["d_expr"], d_expr64), d_aud=cg.rel(a["d_aud"], d_cond[:64]), d_lat=cg.rel(a["d_lat"], d_cond[140:]),
                d_views0_bias=cg.rel(a["d_vb"], dbv64))
    print(f"\n{name}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, t in a.items():
        assert torch.isfinite(t).all(), k
        assert torch.equal(t, b[k]), k
    assert float(d_expr64.abs().max()) > 0 and float(dbv64.abs().max()) > 0
    for k, v in errs.items():
        assert v <= FROZEN_TOL, (name, k, v)
    assert torch.equal(a["d_aud"], old["d_aud"]) and torch.equal(a["d_lat"], old["d_lat"])
    assert torch.equal(only, a["d_expr"])


# ------------------------------------------------------------------------------------------------ case 4
def test_render_rays_returns_d_expr_and_d_bc_and_the_no_op_path_is_the_old_step(idn, dev):
    """Network.render_rays on 3x64+128 with expr and bc_rgb requiring gradients: .grad equals case 1's values bit for bit (the
    same function behind either entry) and so lies within case 1's bound; with neither requiring one, the outputs and all
    48 parameter gradients are bit-identical and ops.pass_bwd_ex is never called (with expr: once per pass)."""
    from idealnerf_amd import autograd as ag
    ops = idn.ops
    sc = rg.scene("3x64+128")
    first = _hip_d_cond(idn, dev, sc)
    calls = []
    real = ops.pass_bwd_ex
    ops.pass_bwd_ex = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    try:
        on = _hip_d_cond(idn, dev, sc, entry="render_rays", cache=False)
        n_on = len(calls)
        off = _hip_d_cond(idn, dev, sc, expr_grad=False, bc_grad=False, entry="render_rays", cache=False)
        only_bc = _hip_d_cond(idn, dev, sc, expr_grad=False, entry="render_rays", cache=False)
    finally:
        ops.pass_bwd_ex = real
    assert n_on == 2 and len(calls) == 2                                         # the other two runs never reach the entry
    assert torch.equal(on["d_expr"], first["d_expr"]) and torch.equal(on["d_bc"], first["d_bc"])
    (e64, b64), (e32, b32) = _oracle(sc, first)
    assert cg.rel(on["d_expr"], e64) <= cg.bound(cg.rel(e32, e64)) and cg.rel(on["d_bc"], b64) <= cg.bound(cg.rel(b32, b64))
    assert off["d_expr"] is None and off["d_bc"] is None
    assert only_bc["d_expr"] is None and torch.equal(only_bc["d_bc"], on["d_bc"])
    assert on["grads"].keys() == off["grads"].keys() and len(on["grads"]) == 2 * len(ag.PARAM_KEYS)
    for k in on["out"]:
        assert torch.equal(on["out"][k], off["out"][k]), k
    for k in on["grads"]:
        assert torch.equal(on["grads"][k], off["grads"][k]) and torch.equal(on["grads"][k], only_bc["grads"][k]), k


def test_frozen_pair_with_only_expr_requiring_grad_runs_the_frozen_plan(idn, dev):
    """Both networks frozen, expr the only input that requires a gradient: each pass goes through ops.pass_bwd_ex without
    gradient tensors, and expr.grad is the sum over the two passes of the fp64 fold of the deltas each leaves in the workspace,
    within the frozen plan's 5e-6; it also agrees with the trained pair's d expr of case 1 within twice that."""
    ops = idn.ops
    sc = rg.scene("3x64+128")
    trained = _hip_d_cond(idn, dev, sc)
    net, coarse, fine = trg._network(idn, dev, sc)
    ref64, plans = torch.zeros(76, dtype=torch.float64, device=dev), []
    real = ops.pass_bwd_ex

    def spy(p, grads, *a, **kw):
        plans.append(grads is None)
        out = real(p, grads, *a, **kw)
        z = a[5]
        module = fine if z.shape[1] > sc["S"] else coarse
        ref64.add_(_fp64_frozen_reference(idn, dev, module, z.shape[0], z.shape[1])[1])
        return out
    ops.pass_bwd_ex = spy
    net.requires_grad_(False)
    try:
        frozen = _hip_d_cond(idn, dev, sc, bc_grad=False, cache=False)
    finally:
        net.requires_grad_(True)
        ops.pass_bwd_ex = real
    assert plans == [True, True] and frozen["grads"] == {} and frozen["d_bc"] is None
    err, against_trained = cg.rel(frozen["d_expr"], ref64), cg.rel(frozen["d_expr"], trained["d_expr"])
    print(f"\nfrozen pair d expr: vs fp64 column sums {err:.2e}, vs the trained pair's {against_trained:.2e}")
    assert err <= FROZEN_TOL and against_trained <= 2 * FROZEN_TOL


def test_background_rows_with_a_repeated_pixel_sum_their_gradients(idn, dev):
    """bc_rgb = Background.rows(sel) with one pixel drawn for two rays: the image's gradient at that pixel is the sum of the two
    rays' d bc rows (exactly: two addends), every other drawn pixel holds its ray's row and the rest of the image zero."""
    from idealnerf_amd.cond_refine import Background
    sc = rg.scene("3x64+128")
    net, coarse, fine = trg._network(idn, dev, sc)
    g = lambda t: t.to(dev)
    image = torch.from_numpy(np.random.RandomState(3).uniform(0, 1, (4, 4, 3)).astype(np.float32))
    bg = Background(image).to(dev)
    sel = torch.tensor([5, 11, 5], device=dev)
    for p in net.parameters():
        p.grad = None
    ret = net.render_rays(g(sc["rays"]).contiguous(), bg.rows(sel), g(sc["aud"]), None, g(sc["latent"]), g(sc["expr"]))
    rg.loss_of(ret, sc["weights"]).backward()
    got = bg.image.grad.reshape(-1, 3)
    leaf = bg.image.detach().reshape(-1, 3)[sel].clone().requires_grad_(True)
    ret = net.render_rays(g(sc["rays"]).contiguous(), leaf, g(sc["aud"]), None, g(sc["latent"]), g(sc["expr"]))
    rg.loss_of(ret, sc["weights"]).backward()
    rows = leaf.grad
    assert float(rows.abs().min(dim=1)[0].max()) > 0
    assert torch.equal(got[5], rows[0] + rows[2]) and torch.equal(got[11], rows[1])
    others = [i for i in range(16) if i not in (5, 11)]
    assert float(got[others].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ case 5
def test_a_noised_background_is_recovered_through_a_frozen_pair(idn, dev):
    """rgb_map is linear in the background, so this is exact: 64 rays at S = 16, Ni = 16, perturb 0 through a frozen pair;
    the targets are the pair's own rgb_map / rgb0 over a known B*; ``Background`` starts at B* + 0.2 noise and is the only
    parameter of the trainer's Adam (betas 0.9 / 0.999).  After the steps |B - B*| (a ray's largest channel) has fallen on
    every ray whose last_weight > 0.1, and the loss has fallen.  Step count and rate (20 steps at 2e-2) were chosen on the CPU
    with the oracle alone -- cond_grad_common.recovery_run on the oracle's own last weights: the worst ray ends at 0.40 of its
    start, the loss at 0.049, a factor 2 to spare on both (tests/test_cond_refine_cpu.py asserts that)."""
    from idealnerf_amd.audio_exp_nerf import Network
    from idealnerf_amd.cond_refine import Background
    from idealnerf_amd.helper import RenderConfig, img2mse
    sc = cg.recovery_scene()
    torch.manual_seed(77)
    cfg = RenderConfig(perturb=0.0, chunk=512, near=rg.NEAR, far=rg.FAR, N_samples=sc["S"], N_importance=sc["Ni"])
    net = Network(32, 32, 50.0, rg.NEAR, rg.FAR, 512, None, sc["S"], sc["Ni"], args=cfg).to(dev)
    net.face_nerf_coarse.load_state_dict(sc["coarse"])
    net.face_nerf_fine.load_state_dict(sc["fine"])
    net.train()
    net.requires_grad_(False)
    g = lambda t: t.to(dev)
    rays, b_true = g(sc["rays"]).contiguous(), g(sc["b_true"])
    render = lambda bc: net.render_rays(rays, bc, g(sc["aud"]), None, g(sc["latent"]), g(sc["expr"]))
    truth = render(b_true)
    tgt, tgt0, lw = truth["rgb_map"].detach(), truth["rgb0"].detach(), truth["last_weight"].detach()
    bg = Background((sc["b_true"] + 0.2 * sc["noise"]).reshape(8, 8, 3)).to(dev)
    sel = torch.arange(64, device=dev)
    opt = torch.optim.Adam([bg.image], lr=cg.RECOVERY_LR, betas=(0.9, 0.999))
    dist = lambda: (bg.image.detach().reshape(-1, 3) - b_true).abs().max(dim=1)[0]
    before, losses = dist(), []
    for _ in range(cg.RECOVERY_STEPS + 1):    # (the last pass only evaluates the loss after the final step)
        out = render(bg.rows(sel))
        loss = img2mse(out["rgb_map"], tgt) + img2mse(out["rgb0"], tgt0)
        losses.append(loss.detach())
        if len(losses) <= cg.RECOVERY_STEPS:
            opt.zero_grad()
            loss.backward()
            opt.step()
    after = dist()
    m = lw > 0.1
    worst = float((after[m] / before[m]).max())
    print(f"\nrecovery: {int(m.sum())} of 64 rays above 0.1, worst after / before {worst:.3f}, loss {float(losses[-1] / losses[0]):.4f}")
    assert int(m.sum()) >= 32
    assert bool((after[m] < before[m]).all()) and float(losses[-1]) < float(losses[0])


# ------------------------------------------------------------------------------------------------ case 6
def _state(run):
    st = {"w." + k: v.detach().clone() for k, v in run["network"].state_dict().items()}
    st["latent"] = run["latent_codes"].detach().clone()
    st["expr_deltas"] = run["expr_refiner"].deltas.detach().clone()
    st["background"] = run["background"].image.detach().clone()
    osd = run["optimizer"].state_dict()
    for i, s in osd["state"].items():
        for k, v in s.items():
            st[f"opt.{i}.{k}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    st["opt.lr"] = torch.tensor([g["lr"] for g in osd["param_groups"]], dtype=torch.float64)
    return st


def test_train_with_expr_and_background_refinement_moves_both_checkpoints_and_resumes(idn, dev, tmp_path):
    """train(steps=3, refine_expr=True, learn_background=True, loader="resident") on 6 frames of 64 x 64 (the size of the
    existing train-loop tests' clip): the expression rows of frames 0..2 and the background have moved, only at drawn pixels;
    head.tar carries expr_deltas and background; 2 steps + 1 resumed step reproduce the 3-step run's deltas, background,
    weights, optimizer state and losses bit for bit; with the options off the file's keys and the optimizer's groups are what
    they were."""
    from idealnerf_amd import train as T_
    d = str(tmp_path / "clip")
    os.makedirs(d)
    flags, _ = write_clip_directory(d, 64, 6, seed=2, N_rand=48, mouth_rays=8, torso_rays=4)
    mk = lambda name: train_flags(d, tmp_path / "logs", name, flags, perturb=0.0, i_print=1, i_weights=1, N_iters=10, chunk=8192)
    losses = {}

    def run(name, steps, seed, **kw):
        torch.manual_seed(seed)
        return T_.train(mk(name), loader="resident", sample_seed=3, device=dev, steps=steps, val="reference",
                        on_step=lambda step, info: losses.setdefault(name, []).append(info["loss"].clone()), **kw)
    on = dict(refine_expr=True, learn_background=True)
    whole = run("whole", 3, 11, **on)
    deltas, image = whole["expr_refiner"].deltas.detach(), whole["background"].image.detach()
    assert whole["global_step"] == 3 and deltas.shape == (6, 76) and image.shape == (64, 64, 3)
    assert all(float(deltas[i].abs().max()) > 0 for i in range(3)) and float(deltas[3:].abs().max()) == 0.0
    ck = torch.load(str(tmp_path / "logs" / "whole" / "head.tar"), weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer", "latent_codes", "expr_deltas", "background"}
    assert ck["global_step"] == 3 and torch.equal(ck["expr_deltas"].to(dev), deltas) and torch.equal(ck["background"].to(dev), image)
    from idealnerf_amd import dataset
    start = dataset._imread(os.path.join(d, "bc.jpg"))
    moved = (image.cpu() != (torch.from_numpy(np.array(start)).to(torch.float64) / 255.0).to(torch.float32)).any(dim=-1)
    assert 0 < int(moved.sum()) <= 3 * 48                                          # only pixels a batch drew
    groups = whole["optimizer"].param_groups
    assert len(groups) == 3 and groups[1]["params"][0] is whole["expr_refiner"].deltas and groups[2]["params"][0] is whole["background"].image
    assert groups[1]["lr"] == pytest.approx(0.1 * groups[0]["lr"], rel=1e-12) and groups[2]["lr"] == pytest.approx(groups[0]["lr"], rel=1e-12)

    run("parts", 2, 11, **on)
    second = run("parts", 1, 999, **on)        # nothing of the last step may come from anywhere but head.tar
    assert second["global_step"] == 3
    a, b = _state(whole), _state(second)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    assert len(losses["parts"]) == 3 and all(torch.equal(x, y) for x, y in zip(losses["whole"], losses["parts"]))

    plain = run("plain", 1, 11)
    assert "expr_refiner" not in plain and "background" not in plain and len(plain["optimizer"].param_groups) == 1
    assert "lr_scale" not in plain["optimizer"].param_groups[0]
    ck = torch.load(str(tmp_path / "logs" / "plain" / "head.tar"), weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer", "latent_codes"}
    # the first step of both runs sees the same expression and the same background pixels: the same loss
    assert torch.equal(losses["plain"][0], losses["whole"][0])


def test_agg_and_baseline_trainers_take_the_options(idn, dev, tmp_path):
    """train_agg.train with both options on the flat 64 x 64 clip of its own loop test (79-wide expressions: the deltas take the
    model's width, not the head flag's, and their gradient arrives through agg_linears in torch) and train_baseline.train with
    learn_background: two steps each, the visited rows and the background have moved, the run files carry the new keys."""
    import json
    import shutil
    import agg_common as ac
    from idealnerf_amd import train_agg, train_baseline
    over = dict(perturb=0.0, i_print=1, i_weights=1, N_iters=10, chunk=8192)

    def split(d, meta):
        json.dump(dict(meta, frames=meta["frames"][:3]), open(os.path.join(d, "transforms_exp_train.json"), "w"))
        json.dump(dict(meta, frames=meta["frames"][3:]), open(os.path.join(d, "transforms_exp_val.json"), "w"))
    d = str(tmp_path / "agg")
    os.makedirs(d)
    flags, meta = write_clip_directory(d, 64, 5, seed=6, flat=True, N_rand=256, dim_expr=79, face_rect=ac.RECT64, mouth_range=ac.MOUTH64)
    split(d, meta)
    ns = train_flags(d, tmp_path / "logs", "agg", flags, **over)
    ns.use_highlight = True
    torch.manual_seed(1)
    run = train_agg.train(ns, loader="resident", sample_seed=3, device=dev, steps=2, refine_expr=True, learn_background=True)
    deltas = run["expr_refiner"].deltas.detach()
    assert deltas.shape == (3, 79) and float(deltas[0].abs().max()) > 0 and float(deltas[1].abs().max()) > 0
    assert float(deltas[2].abs().max()) == 0.0
    ck = torch.load(str(tmp_path / "logs" / "agg" / "000000_head.tar"), weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer", "latent_codes", "expr_deltas", "background"}
    assert torch.equal(ck["background"].to(dev), run["background"].image.detach()) and torch.isfinite(ck["background"]).all()

    d = str(tmp_path / "base")
    os.makedirs(d)
    flags, meta = write_clip_directory(d, 64, 5, seed=6, flat=True, N_rand=64)
    shutil.rmtree(os.path.join(d, "parsing"))
    for f in meta["frames"]:
        del f["exp"]
    split(d, meta)
    ns = train_flags(d, tmp_path / "logs", "base", flags, **over)
    torch.manual_seed(1)
    run = train_baseline.train(ns, loader="resident", sample_seed=3, device=dev, steps=2, learn_background=True)
    ck = torch.load(str(tmp_path / "logs" / "base" / "000000_head.tar"), weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer", "background"} and len(run["optimizer"].param_groups) == 2
    from idealnerf_amd import dataset
    image = run["background"].image.detach()
    start = (torch.from_numpy(np.array(dataset._imread(os.path.join(d, "bc.jpg")))).to(torch.float64) / 255.0).to(torch.float32)
    assert torch.equal(ck["background"].to(dev), image) and 0 < int((image.cpu() != start).any(dim=-1).sum()) <= 2 * 64
