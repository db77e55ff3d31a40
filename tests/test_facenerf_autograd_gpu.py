"""FaceNeRF.forward with gradients (models/face_nerf.py:40-80 as an ordinary differentiable module): weights, input rows
and the per-frame conditioning against autograd through the fp64 oracle, on the GPU."""
import os
import signal
import subprocess
import sys

import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

DIMS = [(64, 76, 32), (106, 0, 0), (64, 0, 0)]      # (dim_aud, dim_expr, dim_latent): head, torso, no expr / latent
SIZES = [1, 127, 128, 129, 4096, 40000]
# Each gradient within this multiple of the fp32 noise floor (torch fp32 vs fp64 on the same inputs).  Measured: d x within 2.5x
# at every n; the gradients that are sums over the rows (biases, weights, aud / expr / latent) within 9x up to 4096 rows and
# 33x at 40 000 -- the weight-gradient products accumulate the rows of a split in fp32 one after the other (hundreds per
# split) where torch's CPU reduction sums pairwise, so their error grows with n faster than the floor's.
GRAD_FLOOR_MULT = 64.0
KINK = 1e-5               # rows with a pre-activation this close to a ReLU kink get loss weight 0 (see _off_kinks)


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    return idealnerf_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(dims3, n, seed=0):
    a, e, l = dims3
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 90, generator=g) * 2 - 1
    cond = [torch.randn(d, generator=g) * 0.3 if d else None for d in (a, e, l)]
    w = torch.randn(n, 4, generator=g)
    return x, cond, w


def _off_kinks(params, dims, x, cond, w):
    """The gradient jumps where a pre-activation crosses 0, so a row whose fp64 pre-activation lies within rounding of a
    ReLU kink may be on either side of it in any fp32 evaluation, and it alone then moves a summed gradient by far more
    than the noise floor (one unit of one row flipped in 4096 rows: ~1e-2 of a bias gradient).  Such rows (about one in ten
    at KINK) get weight 0: they then contribute exactly nothing in every implementation."""
    near = torch.zeros(x.shape[0], dtype=torch.bool)
    relu = torch.relu

    def record(t):
        nonlocal near
        near = near | (t.detach().abs() < KINK).any(1)
        return relu(t)

    p = {k: v.detach().double() for k, v in params.items()}
    torch.relu = record
    try:
        oracle.facenerf_forward(p, x.double(), *[None if c is None else c.double() for c in cond], dims=dims)
    finally:
        torch.relu = relu
    return w * (~near)[:, None].to(w.dtype)


def _net(idn, dev, dims3, seed=5):
    a, e, l = dims3
    dims = oracle.facenerf_dims(dim_aud=a, dim_expr=e, dim_latent=l)
    params = oracle.xavier_facenerf_params(seed, dims)
    net = idn.FaceNeRF(dim_aud=a, dim_latent=l, dim_expr=e)
    net.load_state_dict(params)
    return net.to(dev), params, dims


def _oracle_grads(params, dims, x, cond, w, dtype, with_params=True):
    p = {k: v.detach().to(dtype).clone().requires_grad_(with_params) for k, v in params.items()}
    xs = x.to(dtype).clone().requires_grad_(True)
    cs = [None if c is None else c.to(dtype).clone().requires_grad_(True) for c in cond]
    out = oracle.facenerf_forward(p, xs, *cs, dims=dims)
    (out * w.to(dtype)).sum().backward()
    g = {k: v.grad for k, v in p.items() if v.grad is not None}
    g["x"] = xs.grad
    for name, c in zip(("aud", "expr", "latent"), cs):
        if c is not None:
            g[name] = c.grad
    return g


def _hip_grads(net, dev, x, cond, w):
    xs = x.to(dev).requires_grad_(True)
    cs = [None if c is None else c.to(dev).requires_grad_(True) for c in cond]
    net.zero_grad(set_to_none=True)
    out = net(xs, *cs)
    (out * w.to(dev)).sum().backward()
    g = {k: v.grad for k, v in net.named_parameters() if v.grad is not None}
    g["x"] = xs.grad
    for name, c in zip(("aud", "expr", "latent"), cs):
        if c is not None:
            g[name] = c.grad
    return g


def _err(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _check(got, g64, g32, ctx):
    assert "feature_linear.weight" not in got and set(got) == set(g64) - {"feature_linear.weight", "feature_linear.bias"}, ctx
    ratios = {}
    for k, ref in g64.items():
        if k.startswith("feature_linear"):
            continue
        floor = max(oracle.fp32_noise_floor(g32[k], ref), 2.0 ** -23)
        ratios[k] = _err(got[k], ref) / floor
    worst = max(ratios, key=ratios.get)
    print(f"\n{ctx}: worst gradient error / fp32 noise floor = {ratios[worst]:.2f} ({worst}); "
          f"x {ratios['x']:.2f}" + "".join(f", {k} {ratios[k]:.2f}" for k in ("aud", "expr", "latent") if k in ratios))
    return {k: r for k, r in ratios.items() if not r <= GRAD_FLOOR_MULT}


@pytest.mark.parametrize("dims3", DIMS)
def test_gradients_match_fp64_oracle(idn, dev, dims3, monkeypatch):
    """All 26 used parameter gradients plus d x, d aud, d expr and d latent, both training arithmetics, ragged and large n."""
    from idealnerf_amd import autograd
    net, params, dims = _net(idn, dev, dims3)
    bad = {}
    for n in SIZES:
        x, cond, w = _inputs(dims3, n, seed=n)
        w = _off_kinks(params, dims, x, cond, w)
        g64 = _oracle_grads(params, dims, x, cond, w, torch.float64)
        g32 = _oracle_grads(params, dims, x, cond, w, torch.float32)
        assert len([k for k in g64 if "linear" in k]) == 26      # feature_linear is never applied: no gradient
        for prec in ("bf16x6", "f32"):
            monkeypatch.setattr(autograd, "TRAIN_PRECISION", prec)
            ctx = f"dims {dims3} n {n} {prec}"
            bad.update({(ctx, k): r for k, r in _check(_hip_grads(net, dev, x, cond, w), g64, g32, ctx).items()})
    assert not bad, bad


def test_gradients_on_the_fp32_backward_pipe(dev):
    """IDN_BACKWARD_PIPE=f32 (fp32 delta chain and 256 x 256 products) is read once per process: the oracle test in a child."""
    env = dict(os.environ, IDN_BACKWARD_PIPE="f32")
    child = subprocess.Popen([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k",
                              "gradients_match_fp64_oracle or conditioning_only"],
                             env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True,
                             cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        out, err = child.communicate(timeout=600)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.wait()
        pytest.fail("the fp32-pipe child run did not finish within 600 s")
    assert child.returncode == 0 and "4 passed" in out, out[-3000:] + err[-2000:]


def test_forward_with_grad_matches_no_grad(idn, dev, monkeypatch):
    """The activation-saving forward returns what the inference forward returns at the same arithmetic: the same bits."""
    from idealnerf_amd import autograd
    net, _, _ = _net(idn, dev, DIMS[0])
    for n in (1, 129, 40000):
        x, cond, _ = _inputs(DIMS[0], n, seed=3)
        xd, cd = x.to(dev), [c.to(dev) for c in cond]
        for prec in ("bf16x6", "f32"):
            monkeypatch.setattr(autograd, "TRAIN_PRECISION", prec)
            out = net(xd.clone().requires_grad_(True), *cd)
            assert out.requires_grad
            net.precision = prec
            with torch.no_grad():
                ref = net(xd, *cd)
            assert torch.equal(out.detach(), ref), (n, prec, _err(out, ref))


def test_conditioning_only_gradients(idn, dev):
    """Frozen weights, per-frame codes optimised: only latent_code and expr require grad -- gradients arrive (the call used
    to return a tensor without a graph) and match the oracle; the parameters get none."""
    dims3 = DIMS[0]
    net, params, dims = _net(idn, dev, dims3)
    net.requires_grad_(False)
    n = 4096
    x, (aud, expr, lat), w = _inputs(dims3, n, seed=11)
    w = _off_kinks(params, dims, x, (aud, expr, lat), w)
    ex, la = expr.to(dev).requires_grad_(True), lat.to(dev).requires_grad_(True)
    out = net(x.to(dev), aud.to(dev), ex, la)
    assert out.requires_grad
    (out * w.to(dev)).sum().backward()
    assert all(p.grad is None for p in net.parameters())

    def ref(dtype):
        p = {k: v.detach().to(dtype) for k, v in params.items()}
        e, l = expr.to(dtype).clone().requires_grad_(True), lat.to(dtype).clone().requires_grad_(True)
        (oracle.facenerf_forward(p, x.to(dtype), aud.to(dtype), e, l, dims=dims) * w.to(dtype)).sum().backward()
        return e.grad, l.grad

    (e64, l64), (e32, l32) = ref(torch.float64), ref(torch.float32)
    for got, r64, r32 in ((ex.grad, e64, e32), (la.grad, l64, l32)):
        assert _err(got, r64) <= GRAD_FLOOR_MULT * max(oracle.fp32_noise_floor(r32, r64), 2.0 ** -23)


def test_padding_rows_are_defined(idn, dev):
    """A ragged n with a NaN-filled slab and workspace: every gradient finite (the padding rows carry zero deltas through
    activations the forward defined)."""
    from idealnerf_amd import autograd, ops
    lib = idn._lib.load()
    net, _, _ = _net(idn, dev, DIMS[0])
    n = 37 * 5
    x, cond, w = _inputs(DIMS[0], n, seed=2)
    x, cond, g_out = x.to(dev), [c.to(dev) for c in cond], w.to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    for prec, code in (("bf16x6", idn._lib.IDN_PREC_BF16X6), ("f32", idn._lib.IDN_PREC_F32)):
        folded = net.folded_bias(*cond)
        acts = torch.full((lib.idealnerf_train_acts_floats(n),), float("nan"), device=dev)
        out = torch.empty((n, 4), device=dev)
        rc = lib.idealnerf_facenerf_train_fwd(net.packed_weights(prec).data_ptr(), folded.data_ptr(), code, x.data_ptr(), n,
                                              out.data_ptr(), acts.data_ptr(), stream)
        assert rc == 0, lib.idealnerf_last_error()
        assert bool(torch.isfinite(acts[:256 * 2560]).all()) and bool(torch.isfinite(out).all()), prec
        nbytes = lib.idealnerf_facenerf_bwd_workspace_bytes(n)
        ws = torch.full((nbytes // 4,), float("nan"), device=dev)
        sd = dict(net.named_parameters())
        grads = {k: torch.full_like(sd[k], float("nan")) for k in autograd.PARAM_KEYS}
        d_x = torch.full((n, 90), float("nan"), device=dev)
        d_c = [torch.zeros_like(c) for c in cond]
        ptr = lambda t: t.data_ptr()
        import ctypes as C
        rc = lib.idealnerf_facenerf_bwd(C.byref(net.kernel_params()), C.byref(ops.grads_struct(grads)), *map(ptr, cond), ptr(acts),
                                        n, ptr(g_out), ptr(d_x), *map(ptr, d_c), ptr(ws), ws.numel() * 4, stream)
        assert rc == 0, lib.idealnerf_last_error()
        torch.cuda.synchronize()
        for k, g in list(grads.items()) + [("x", d_x), ("aud", d_c[0]), ("expr", d_c[1]), ("latent", d_c[2])]:
            assert bool(torch.isfinite(g).all()), (prec, k)


def test_backward_is_bit_reproducible(idn, dev):
    net, _, _ = _net(idn, dev, DIMS[0])
    x, cond, w = _inputs(DIMS[0], 40000, seed=4)
    first = _hip_grads(net, dev, x, cond, w)
    again = _hip_grads(net, dev, x, cond, w)
    for k in first:
        assert torch.equal(first[k], again[k]), k


def test_short_training_run_tracks_torch_eager(idn, dev):
    """50 Adam steps fitting 4096 rows to a fixed target, next to the same loop in torch-eager fp32 on the GPU from the
    same initial weights: both losses fall by 10x or more and end within 1 % of each other."""
    dims3 = DIMS[0]
    net, params, dims = _net(idn, dev, dims3)
    x, (aud, expr, lat), _ = _inputs(dims3, 4096, seed=9)
    x, aud, expr, lat = (t.to(dev) for t in (x, aud, expr, lat))
    tgt = torch.tensor([0.5, -0.3, 0.2, 1.0], device=dev) + 0.1 * torch.sin(3 * x[:, :4])
    p_eager = {k: v.to(dev).requires_grad_(True) for k, v in params.items() if not k.startswith("feature_linear")}
    opt_h = torch.optim.Adam([p for k, p in net.named_parameters() if not k.startswith("feature_linear")], lr=1e-3)
    opt_e = torch.optim.Adam(list(p_eager.values()), lr=1e-3)
    lh, le = [], []
    for _ in range(50):
        loss = ((net(x, aud, expr, lat) - tgt) ** 2).mean()
        opt_h.zero_grad()
        loss.backward()
        opt_h.step()
        lh.append(float(loss.detach()))
        loss = ((oracle.facenerf_forward(p_eager, x, aud, expr, lat, dims=dims) - tgt) ** 2).mean()
        opt_e.zero_grad()
        loss.backward()
        opt_e.step()
        le.append(float(loss.detach()))
    print(f"\nAdam x 50: HIP {lh[0]:.4e} -> {lh[-1]:.4e}, torch eager {le[0]:.4e} -> {le[-1]:.4e}")
    assert lh[0] / lh[-1] >= 10 and le[0] / le[-1] >= 10
    assert abs(lh[-1] - le[-1]) <= 0.01 * le[-1]


def test_errors(idn, dev):
    from idealnerf_amd import ops
    net, _, _ = _net(idn, dev, DIMS[0])
    x, cond, _ = _inputs(DIMS[0], 16)
    cd = [c.to(dev) for c in cond]
    with pytest.raises(idn._lib.IdealNerfError):     # rows on the CPU: no fallback
        net(x.requires_grad_(True), *cd)
    with pytest.raises(idn._lib.IdealNerfError):
        ops.facenerf_train_fwd(net.packed_weights("bf16x6"), net.folded_bias(*cd), x.detach(), idn._lib.IDN_PREC_BF16X6)
    with pytest.raises(idn._lib.IdealNerfError):
        ops.facenerf_train_fwd(net.packed_weights("bf16x3"), net.folded_bias(*cd), x.detach().to(dev), idn._lib.IDN_PREC_BF16X3)
    out = net(x.detach().to(dev).requires_grad_(True), *cd)
    with pytest.raises(idn._lib.IdealNerfError):     # once differentiable
        torch.autograd.grad(out.sum(), list(net.parameters())[:1], create_graph=True)
