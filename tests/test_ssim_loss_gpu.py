"""The patch SSIM loss on the GPU: the forward and the backward against an fp64 reference (ssim_loss_common.reference: torch
conv2d and autograd in float64 on the CPU), the same index as the scorer, determinism and independence of the patches,
``patch_pixels`` against its numpy restatement, the loader's patch rows, the gradient that reaches the render output in a
train step, and the trainers with the option off (the parent's bytes) and on (finite, resumable bit for bit).

Measured on an MI355X (profiles/ssim_loss_parity.json; $IDN_SSIM_LOSS_RECORD rewrites it), maxima over all shapes: forward
|out - out64| 1.1e-15 (uniform), 1.2e-13 (flat truth + noise), 0 (pred == truth), bound 1e-10; against the scorer 1.1e-16;
backward 0.49 of its per-element bound (the half ulp of the one fp32 rounding), 3.7e-17 at pred == truth (bound 1e-9); the
gradient at the render output 0.26 of its bound."""
import os

import numpy as np
import pytest
import torch

from idealnerf_amd.synthetic import write_clip_directory
from ssim_loss_common import CASES, SHAPES, inputs, patch_pixels_reference, record, reference
from train_loop_common import train_flags

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    return idealnerf_amd


@pytest.fixture(scope="module")
def refs():
    """(case, k, p) -> (pred, truth, out64, d64) on the CPU: computed once, shared, never written."""
    cache = {}

    def get(case, k, p):
        key = (case, k, p)
        if key not in cache:
            pred, truth = inputs(case, k, p)
            cache[key] = (pred, truth, *reference(pred, truth, k, p))
        return cache[key]
    return get


# ------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("k,p", SHAPES)
def test_forward_against_fp64(idn, dev, refs, k, p):
    """Every element of out within 1e-10 of the reference: fp64 moment sums carry about 121 * 2^-53, and the variance
    difference is divided by at least C2 = 9e-4, twice.  pred == truth gives SSIM 1 (and loss 0) within the same bound."""
    for case in CASES:
        pred, truth, out64, _ = refs(case, k, p)
        out = idn.ops.ssim_patch_fwd(pred.to(dev), truth.to(dev), k, p)
        assert out.shape == (k + 1,) and out.dtype == torch.float64
        err = float((out.cpu() - out64).abs().max())
        print(f"forward {case} k={k} p={p}: max |out - out64| = {err:.3e}")
        record(f"forward_max_abs_err_{case}", err)
        assert err <= 1e-10, (case, err)
        if case == "equal":
            assert float((out[:k].cpu() - 1.0).abs().max()) <= 1e-10 and abs(float(out[k])) <= 1e-10
    # the rows a render returns, [k p p, 3], are the same memory
    pred, truth, _, _ = refs("uniform", k, p)
    a = idn.ops.ssim_patch_fwd(pred.to(dev), truth.to(dev), k, p)
    b = idn.ops.ssim_patch_fwd(pred.reshape(-1, 3).to(dev), truth.reshape(-1, 3).to(dev), k, p)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 2. the scorer's index
@pytest.mark.parametrize("p", [32, 48])
def test_same_index_as_the_scorer(idn, dev, p):
    """A p x p "frame" with byte truth: frame_scores' ssim_sum / (3 n_windows) equals ssim_patch_fwd on truth_u8 / 255 within
    1e-10 (the two kernels add the same window values in another order).  The quotient is formed on the HOST, where it is the
    correctly rounded fp32 division the scorer's own `(float) byte / 255.0f` is: the same expression on a device tensor is
    evaluated as a product with fp32(1 / 255) and differs from it by an ulp at some bytes, which moves the index by 4e-9 -- a
    difference of the inputs, not of the kernels."""
    gen = torch.Generator().manual_seed(p)
    truth_host = torch.randint(0, 256, (p, p, 3), generator=gen, dtype=torch.uint8)
    unit = truth_host.float() / 255.0
    assert np.array_equal(unit.numpy(), truth_host.numpy().astype(np.float32) / np.float32(255.0))
    truth_u8, unit = truth_host.to(dev), unit.to(dev)
    pred = (unit + 0.1 * torch.randn((p, p, 3), generator=gen).to(dev)).contiguous()
    table = idn.ops.frame_scores(pred, truth_u8)
    n_win = float(table[0, 2])
    assert n_win == (p - 10) ** 2
    scorer = float(table[0, 3]) / (3.0 * n_win)
    out = idn.ops.ssim_patch_fwd(pred, unit.contiguous(), 1, p)
    err = abs(float(out[0]) - scorer)
    print(f"scorer p={p}: |patch - scorer| = {err:.3e}")
    record("scorer_max_abs_diff", err)
    assert err <= 1e-10 and abs(float(out[1]) - (1.0 - scorer)) <= 1e-10


# ------------------------------------------------------------------------------------------------ 3. backward
@pytest.mark.parametrize("k,p", SHAPES)
def test_backward_against_fp64(idn, dev, refs, k, p):
    """g = 1: per element |d - d64| <= 2^-23 |d64| + 1e-9 max|d64| (one fp32 rounding of an fp64 value, plus fp64 noise);
    pred == truth: max|d| <= 1e-9; g = 0.25 scales the uniform case within one more fp32 rounding."""
    for case in CASES:
        pred, truth, _, d64 = refs(case, k, p)
        d = idn.ops.ssim_patch_bwd(pred.to(dev), truth.to(dev), k, p, 1.0)
        assert d.shape == pred.shape and d.dtype == torch.float32
        d = d.cpu().double()
        if case == "equal":
            worst = float(d.abs().max())
            print(f"backward equal k={k} p={p}: max |d| = {worst:.3e}")
            record("backward_equal_max_abs", worst)
            assert worst <= 1e-9
            continue
        top = float(d64.abs().max())
        excess = ((d - d64).abs() - (EPS32 * d64.abs() + 1e-9 * top)).max()
        ratio = float(((d - d64).abs() / (EPS32 * d64.abs() + 1e-9 * top)).max())
        print(f"backward {case} k={k} p={p}: max |d - d64| / bound = {ratio:.3f}, max |d64| = {top:.3e}")
        record(f"backward_max_err_over_bound_{case}", ratio)
        assert float(excess) <= 0.0, (case, ratio)
    pred, truth, _, d64 = refs("uniform", k, p)
    q = idn.ops.ssim_patch_bwd(pred.to(dev), truth.to(dev), k, p, 0.25).cpu().double()
    want, top = 0.25 * d64, 0.25 * float(d64.abs().max())
    assert float(((q - want).abs() - (2 * EPS32 * want.abs() + 1e-9 * top)).max()) <= 0.0


# ------------------------------------------------------------------------------------------------ 4. determinism, independence
@pytest.mark.parametrize("p", [11, 12, 32, 48])
def test_deterministic_and_patches_independent(idn, dev, refs, p):
    """Two calls give the same bytes; patch 1 of a k = 3 call equals the k = 1 call on that patch bit for bit, forward and
    backward.  (The backward's factor is (g / k) / (3 (p - 10)^2) with g / k formed first: g = 3 on three patches and g = 1 on
    one give exactly the same factor, and so the same bytes; g = 1 on both differs by the division by 3 alone.)"""
    ops = idn.ops
    pred, truth = (t.to(dev) for t in refs("uniform", 3, p)[:2])
    f1, f2 = ops.ssim_patch_fwd(pred, truth, 3, p), ops.ssim_patch_fwd(pred, truth, 3, p)
    b1, b2 = ops.ssim_patch_bwd(pred, truth, 3, p, 1.0), ops.ssim_patch_bwd(pred, truth, 3, p, 1.0)
    assert torch.equal(f1, f2) and torch.equal(b1, b2)
    one_p, one_t = pred[1:2].contiguous(), truth[1:2].contiguous()
    f = ops.ssim_patch_fwd(one_p, one_t, 1, p)
    assert torch.equal(f[0], f1[1])
    assert torch.equal(ops.ssim_patch_bwd(one_p, one_t, 1, p, 1.0), ops.ssim_patch_bwd(pred, truth, 3, p, 3.0)[1:2])
    # and the other patches' VALUES do not enter: garbage around patch 1 leaves it alone
    noisy_p, noisy_t = pred.clone(), truth.clone()
    noisy_p[0], noisy_p[2], noisy_t[0], noisy_t[2] = 7.0, -3.0, 0.0, 1e3
    assert torch.equal(ops.ssim_patch_fwd(noisy_p, noisy_t, 3, p)[1], f1[1])
    assert torch.equal(ops.ssim_patch_bwd(noisy_p, noisy_t, 3, p, 1.0)[1], b1[1])


# ------------------------------------------------------------------------------------------------ 5. patch_pixels
@pytest.mark.parametrize("p", [11, 48])
def test_patch_pixels_equals_restatement(idn, dev, p):
    ops, H, W = idn.ops, 450, 450
    origins = [(0, 0), (H - p, W - p), (0, W - p)]       # the frame's corners
    sel = ops.patch_pixels(origins, p, W, device=dev)
    assert sel.dtype == torch.int64 and sel.shape == (3 * p * p,)
    assert np.array_equal(sel.cpu().numpy(), patch_pixels_reference(origins, p, W))
    assert int(sel.max()) == H * W - 1 and int(sel.min()) == 0
    buf = torch.full((3 * p * p + 7,), -5, dtype=torch.int64, device=dev)
    out = ops.patch_pixels([(H - p, 0), (17, 23), (3, 5)], p, W, out=buf[5:5 + 3 * p * p])   # a tail that starts anywhere
    assert out.data_ptr() == buf[5:].data_ptr()
    assert np.array_equal(out.cpu().numpy(), patch_pixels_reference([(H - p, 0), (17, 23), (3, 5)], p, W))
    assert (buf[:5] == -5).all() and (buf[5 + 3 * p * p:] == -5).all()


def test_patch_pixels_limits_raise(idn, dev):
    E = idn._lib.IdealNerfError
    for origins, p in (([(0, 0)], 10), ([(0, 0)], 49), ([(0, 0)] * 17, 11), ([(0, 440)], 11), ([(-1, 0)], 11)):
        with pytest.raises(E):
            idn.ops.patch_pixels(origins, p, 450, device=dev)
    x = torch.rand(1, 12, 12, 3, device=dev)
    for k, p in ((1, 10), (1, 49), (17, 12)):
        with pytest.raises(E):
            idn.ops.ssim_patch_fwd(x, x, k, p)
        with pytest.raises(E):
            idn.ops.ssim_patch_bwd(x, x, k, p)


# ------------------------------------------------------------------------------------------------ the generated clip
@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """64 x 64, 3 frames, N_rand 512: the rect region's share is int(500 * 0.95) = 475 >= 256."""
    tmp = tmp_path_factory.mktemp("ssim_loss")
    d = str(tmp / "clip")
    os.makedirs(d)
    flags, meta = write_clip_directory(d, 64, 3, seed=2, N_rand=512, mouth_rays=8, torso_rays=4)
    return tmp, d, flags, meta


# ------------------------------------------------------------------------------------------------ 6. loader
@pytest.mark.parametrize("patches", [(1, 16), (2, 11)])
def test_loader_puts_patches_in_the_tail(idn, dev, clip, patches):
    from idealnerf_amd import dataset
    ops = idn.ops
    _, d, flags, meta = clip
    k, p = patches
    plain = dataset.ResidentFrames(d, "aud.npy", "train", flags, device=dev, seed=3)
    frames = dataset.ResidentFrames(d, "aud.npy", "train", flags, device=dev, seed=3, patches=patches)
    n_s = 512 - k * p * p
    assert plain.patch_rows() == slice(512, 512) and plain.counts == ops.sample_counts(512, 8, 4, 0.95)
    assert frames.patch_rows() == slice(n_s, 512)
    assert frames.counts == (plain.counts[0] - k * p * p, *plain.counts[1:]) and sum(frames.counts) == n_s
    index, draw = 1, 7
    batch = frames.batch(index, draw)
    rays, target, bc = (t.clone() for t in batch[:3])
    sel = frames.selection().clone()
    assert rays.shape == (2, 512, 3) and target.shape == (512, 3) and bc.shape == (512, 3) and sel.shape == (512,)
    origins = frames.patch_origins_of(index, draw)
    assert len(origins) == k
    # the tail: the patches' pixels, targets bit for bit, rays as the gather makes them
    tail = torch.cat([(torch.arange(oy, oy + p)[:, None] * 64 + torch.arange(ox, ox + p)[None]).reshape(-1) for oy, ox in origins])
    assert torch.equal(sel[n_s:].cpu(), tail)
    want_t = torch.cat([(frames.imgs[index][oy:oy + p, ox:ox + p].float() / 255.0).reshape(-1, 3) for oy, ox in origins])
    assert torch.equal(target[n_s:], want_t)
    g_rays, g_target, g_bc = ops.gather_rays(tail.to(dev), frames._cams[index], 64, 64, frames.focal, frames.imgs[index],
                                             frames.background, frames.cx, frames.cy)
    assert torch.equal(rays[:, n_s:], g_rays) and torch.equal(target[n_s:], g_target) and torch.equal(bc[n_s:], g_bc)
    # the prefix: the sampler with the reduced counts
    want_sel = ops.sample_pixels(frames.maps[index], frames.counts, 3, draw)
    assert torch.equal(sel[:n_s], want_sel)
    p_rays, p_target, p_bc = ops.gather_rays(want_sel, frames._cams[index], 64, 64, frames.focal, frames.imgs[index],
                                             frames.background, frames.cx, frames.cy)
    assert torch.equal(rays[:, :n_s], p_rays) and torch.equal(target[:n_s], p_target) and torch.equal(bc[:n_s], p_bc)
    # the same (index, draw) gives the same batch, whatever was drawn in between
    frames.batch(2, 99)
    again = frames.batch(index, draw)
    assert all(torch.equal(a, b) for a, b in zip(again[:3], (rays, target, bc))) and torch.equal(frames.selection(), sel)
    # without patches the loader is what it was
    a, b = plain.batch(index, draw), dataset.ResidentFrames(d, "aud.npy", "train", flags, device=dev, seed=3, patches=None).batch(index, draw)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert torch.equal(plain.selection(), ops.sample_pixels(plain.maps[index], plain.counts, 3, draw))
    # 50 draws: every patch inside the face rect clipped to the frame (pixel rows and columns 4 .. 54), several origins
    rect = meta["frames"][index]["face_rect"]
    seen = set()
    for dr in range(50):
        for oy, ox in frames.patch_origins_of(index, dr):
            assert rect[0] <= oy and oy + p - 1 <= min(rect[0] + rect[2], 63) and rect[1] <= ox and ox + p - 1 <= min(rect[1] + rect[3], 63)
            seen.add((oy, ox))
    assert len(seen) >= 2
    whole = dataset.ResidentFrames(d, "aud.npy", "train", flags, device=dev, seed=3, patches=patches, patch_region="frame")
    spots = [o for dr in range(50) for o in whole.patch_origins_of(index, dr)]
    assert all(0 <= oy <= 64 - p and 0 <= ox <= 64 - p for oy, ox in spots) and len(set(spots)) >= 2


# ------------------------------------------------------------------------------------------------ 7. gradient at the render output
class _Tapped:
    """The network as train_step calls it, with the gradient that arrives at the fine image kept."""

    def __init__(self, network):
        self.network, self.args, self.rgb, self.grad = network, network.args, None, None

    def __call__(self, x):
        out = self.network(x)
        self.rgb = out[0].detach().clone()
        out[0].register_hook(lambda g: setattr(self, "grad", g.detach().clone()))
        return out


def test_gradient_at_the_render_output(idn, dev, clip):
    """One train_step with ssim_weight = 0.5: the gradient at rgb against the fp64 gradient of mse + 0.5 (1 - ssim) from the
    same rgb values, |g - g64| <= 2^-21 (|g_mse64| + |g_ssim64|) + 1e-9 max|g64| (four fp32 roundings: the subtract, the scale,
    the SSIM rounding and the add); rows outside the patches carry the MSE gradient alone; info["ssim_loss"] is out[k] of a
    direct call within one fp32 rounding."""
    from idealnerf_amd import dataset, train as T_
    from idealnerf_amd.audio_exp_nerf import Network, init_weights
    from idealnerf_amd.config import to_render_config
    tmp, d, flags, _ = clip
    k, p = 1, 16
    args = train_flags(d, tmp / "logs", "grad", flags, perturb=0.0, chunk=8192)
    frames = dataset.ResidentFrames(d, "aud.npy", "train", flags, device=dev, seed=3, patches=(k, p))
    torch.manual_seed(11)
    net = Network(64, 64, frames.focal, near=args.near, far=args.far, chunk=args.chunk, intrinsic=None, N_samlpes=args.N_samples,
                  N_importance=args.N_importance, args=to_render_config(args)).to(dev)
    lat = torch.ones(len(frames), 32, dtype=torch.float32, device=dev)
    net.apply(init_weights)
    lat.requires_grad = True
    opt = T_.make_optimizer(net, lat, args.lrate)
    net.train()
    tap = _Tapped(net)
    data = frames.batch(0, 0)
    target = data[1].clone()
    rows = frames.patch_rows()
    info = T_.train_step(tap, opt, data, lat, 0, len(frames), lrate=args.lrate, lrate_decay=args.lrate_decay, ssim=(0.5, rows, k, p))
    assert tap.grad is not None and tap.grad.shape == (512, 3) and torch.isfinite(info["loss"])
    rgb64, t64 = tap.rgb.cpu().double(), target.cpu().double()
    g_mse = 2.0 * (rgb64 - t64) / rgb64.numel()
    out64, d64 = reference(tap.rgb[rows].cpu(), target[rows].cpu(), k, p)
    g_ssim = torch.zeros_like(g_mse)
    g_ssim[rows] = 0.5 * d64.reshape(-1, 3)
    g64 = g_mse + g_ssim
    g = tap.grad.cpu().double()
    bound = 2.0 ** -21 * (g_mse.abs() + g_ssim.abs()) + 1e-9 * float(g64.abs().max())
    ratio = float(((g - g64).abs() / bound).max())
    print(f"render-output gradient: max |g - g64| / bound = {ratio:.3f}; max |g_mse64| = {float(g_mse.abs().max()):.3e}, "
          f"max |g_ssim64| = {float(g_ssim.abs().max()):.3e}")
    record("render_output_grad_max_err_over_bound", ratio)
    assert float(((g - g64).abs() - bound).max()) <= 0.0, ratio
    assert float(g_ssim[rows].abs().max()) > 0 and float(g_ssim[:rows.start].abs().max()) == 0.0
    outside = (g[:rows.start] - g_mse[:rows.start]).abs() - (2.0 ** -21 * g_mse[:rows.start].abs() + 1e-9 * float(g64.abs().max()))
    assert float(outside.max()) <= 0.0
    direct = idn.ops.ssim_patch_fwd(tap.rgb[rows].contiguous(), target[rows].contiguous(), k, p)
    assert info["ssim_loss"].dtype == torch.float32
    assert abs(float(info["ssim_loss"]) - float(direct[k])) <= 2.0 ** -24 * abs(float(direct[k]))
    assert abs(float(direct[k]) - float(out64[k])) <= 1e-10
    # and the plain step's dict is what it was
    plain = T_.train_step(net, opt, frames.batch(1, 1), lat, 1, len(frames), lrate=args.lrate, lrate_decay=args.lrate_decay)
    assert set(plain) == {"loss", "psnr", "latent_code_loss", "lr"} and set(info) == set(plain) | {"ssim_loss"}


# ------------------------------------------------------------------------------------------------ 8, 9. the trainers
def _state(run):
    st = {"w." + k: v.detach().clone() for k, v in run["network"].state_dict().items()}
    if run["latent_codes"] is not None:
        st["latent"] = run["latent_codes"].detach().clone()
    osd = run["optimizer"].state_dict()
    for i, s in osd["state"].items():
        for k, v in s.items():
            st[f"opt.{i}.{k}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    st["opt.lr"] = torch.tensor([g["lr"] for g in osd["param_groups"]], dtype=torch.float64)
    return st


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k


def test_off_is_the_parent(idn, dev, clip):
    """Two steps with ssim_weight = 0, patches = None and two steps with no new argument: equal state, the same head.tar keys."""
    from idealnerf_amd import train as T_
    tmp, d, flags, _ = clip
    mk = lambda name: train_flags(d, tmp / "logs", name, flags, perturb=0.0, i_print=1, i_weights=1, N_iters=10, chunk=8192)
    logs = {}

    def run(name, **kw):
        torch.manual_seed(11)
        return T_.train(mk(name), loader="resident", sample_seed=3, device=dev, steps=2,
                        on_log=lambda kind, step, payload: logs.setdefault(name, []).append((kind, payload)), **kw)
    a, b = run("off_named", ssim_weight=0.0, patches=None, patch_region="rect"), run("off_plain")
    _same(_state(a), _state(b))
    ka, kb = (torch.load(str(tmp / "logs" / n / "head.tar"), weights_only=False) for n in ("off_named", "off_plain"))
    assert set(ka) == set(kb) == {"global_step", "model_state_dict", "optimizer", "latent_codes"}
    assert all(set(pl) == {"loss", "psnr", "learning_rate", "latent_code_loss"} for name in logs for kind, pl in logs[name] if kind == "train")


@pytest.mark.parametrize("model", ["head", "agg", "baseline"])
def test_on_runs_and_resumes(idn, dev, clip, tmp_path, model):
    """train(steps=3, ssim_weight=0.2, patches=(1, 16)): finite losses, ssim_loss in info and in the log, no new checkpoint
    key; 2 steps + 1 resumed step (perturb = 0) reproduce the 3-step run's state bit for bit."""
    from idealnerf_amd import train as T_, train_agg, train_baseline
    tmp, d, flags, _ = clip
    over = dict(perturb=0.0, i_print=1, i_weights=1, N_iters=10, chunk=8192)
    if model == "agg":                                   # its expressions are 79 wide
        d = str(tmp_path / "agg")
        os.makedirs(d)
        flags, _ = write_clip_directory(d, 64, 3, seed=2, N_rand=512, dim_expr=79)
        flags.use_highlight = False
    train = {"head": T_.train, "agg": train_agg.train, "baseline": train_baseline.train}[model]
    name = {"head": "head.tar", "agg": "000000_head.tar", "baseline": "000000_head.tar"}[model]
    infos, logs = {}, []

    def run(tag, steps, seed):
        ns = train_flags(d, tmp_path / "logs", tag, flags, **over)
        ns.use_highlight = False
        torch.manual_seed(seed)
        return train(ns, loader="resident", sample_seed=3, device=dev, steps=steps, ssim_weight=0.2, patches=(1, 16),
                     on_step=lambda step, info: infos.setdefault(tag, []).append({k: v.clone() if torch.is_tensor(v) else v for k, v in info.items()}),
                     on_log=lambda kind, step, payload: logs.append((tag, kind, payload)))
    whole = run("whole", 3, 11)
    assert whole["global_step"] == 3 and len(infos["whole"]) == 3
    for info in infos["whole"]:
        assert torch.isfinite(info["loss"]) and torch.isfinite(info["ssim_loss"]) and 0.0 < float(info["ssim_loss"]) < 2.0
    train_logs = [pl for tag, kind, pl in logs if tag == "whole" and kind == "train"]
    assert len(train_logs) == 3 and all("ssim_loss" in pl and np.isfinite(pl["ssim_loss"]) for pl in train_logs)
    ck = torch.load(str(tmp_path / "logs" / "whole" / name), weights_only=False)
    assert set(ck) == ({"global_step", "model_state_dict", "optimizer"} | ({"latent_codes"} if model != "baseline" else set()))
    run("parts", 2, 11)
    assert torch.load(str(tmp_path / "logs" / "parts" / name), weights_only=False)["global_step"] == 2
    second = run("parts", 1, 999)                        # nothing of the last step may come from anywhere but the checkpoint
    assert second["global_step"] == 3
    _same(_state(whole), _state(second))
    assert all(torch.equal(x["loss"], y["loss"]) and torch.equal(x["ssim_loss"], y["ssim_loss"])
               for x, y in zip(infos["whole"], infos["parts"]))
