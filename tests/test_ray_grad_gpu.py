"""The render backward's gradient with respect to the ray records, and pose refinement end to end (run with ``-m gpu``).

Case 1 -- d rays of ``Network.render_rays`` against the CPU oracle's float64 autograd, evaluated at the sample depths the HIP
forward used (so an importance-index flip cannot pass for a gradient error).  The loss is a fixed random linear functional of
rgb_map, rgb0, acc_map (and rgb_map_fg in the torso variant).  Yardstick: e32 = oracle.fp32_noise_floor of the fp32 oracle's
d rays against the fp64 oracle's on the same inputs -- the reference against itself.  Bound: per column block (o, d, viewdirs),
max |HIP - fp64| / max |fp64| <= 4 e32 (the HIP path differs from the fp32 oracle in summation order in three places: the MFMA
accumulate, the six-piece split and the per-ray tree).  Shapes, the smallest at which the kernels can still go wrong:
  3 x (64 + 128)     the fine pass has 576 points: 4.5 tiles of 128
  37 x (64 + 128)    both passes end inside a tile
  26 x 5, Ni = 0     130 points: rays straddle the tile boundary, fewer samples than lanes
  2 x (256 + 256)    512 fine samples: 8 per lane
  37 x (64 + 128) fg train_torso.Network's unfrozen pair, with rgb_map_fg
Every case runs under both training precisions: the process's own (IDN_TRAIN_PRECISION, default bf16x6) here, the other one in a
fresh child process (the constant is read at import).  With the ORACLE's depths, on the CPU, the scenes of ray_grad_common.py
measured: e32 = 2.5e-7, 2.6e-4, 6.8e-6, 8.0e-7, 9.0e-5 in the order above (all below 1e-3: none is too sharp to test a gradient
on), and detaching rays_d inside the oracle's composite moves d rays_d by 5.4e-4, 3.4e-2, 7.7e-3, 1.4e-2, 1.5e-2 of its largest
entry -- each more than 10 x the case's bound (1.0e-5, 1.0e-2, 2.7e-4, 3.2e-5, 3.6e-3), so a build that drops the |rays_d| term
fails; the test re-checks both conditions at the HIP depths.  Measured on an MI355X (profiles/ray_grad_parity.json), bf16x6:
e32 2.5e-7, 2.6e-4, 6.8e-6, 6.3e-7, 9.0e-5; the HIP gradient's largest block error 4.8e-7, 3.3e-4, 7.1e-6, 6.0e-7, 9.6e-5 -- at
the fp32 oracle's own distance from fp64, a quarter of the bound.  $IDN_RAY_GRAD_RECORD names a JSON file the figures are merged
into.

Case 2 -- determinism (twice the same bits; the same bits with 128 other rays in front) and the no-op paths.
Case 3 -- d loss / d (omega, tau) of one ``train_step`` against the oracle through ``camera_rays`` of the refined camera, and
``train(refine_poses=True)``: visited rows, the checkpoint, resume bit for bit.
"""
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
import ray_grad_common as rg
from idealnerf_amd.synthetic import write_clip_directory
from train_loop_common import train_flags

pytestmark = pytest.mark.gpu

FACTOR = 4.0   # the issue's: three places where the HIP path's summation order differs from the fp32 oracle's


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
    path = os.environ.get("IDN_RAY_GRAD_RECORD")
    if not path:
        return
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(old, open(path, "w"), indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------ the HIP side of a case
_NETS = {}


def _network(idn, dev, sc):
    """The case's Network in train mode with the scene's weights -> (network, coarse module, fine module)."""
    key = sc["name"]
    if key in _NETS:
        return _NETS[key]
    torch.manual_seed(77)   # the audio nets are torch-initialised (and unused here)
    from idealnerf_amd.helper import RenderConfig
    S, Ni = sc["S"], sc["Ni"]
    if sc["fg"]:
        from idealnerf_amd.train_torso import Network
        cfg = RenderConfig(perturb=0.0, chunk=512, near=rg.NEAR, far=rg.FAR, dim_expr=79, N_samples=S, N_importance=Ni)
        net = Network(32, 32, 50.0, rg.NEAR, rg.FAR, 512, S, Ni, args=cfg).to(dev)
        coarse, fine = net.torso_coarse_nerf, net.torso_fine_nerf
    else:
        from idealnerf_amd.audio_exp_nerf import Network
        cfg = RenderConfig(perturb=0.0, chunk=512, near=rg.NEAR, far=rg.FAR, N_samples=S, N_importance=Ni)
        net = Network(32, 32, 50.0, rg.NEAR, rg.FAR, 512, None, S, Ni, args=cfg).to(dev)
        coarse, fine = net.face_nerf_coarse, net.face_nerf_fine
    coarse.load_state_dict(sc["coarse"])
    fine.load_state_dict(sc["fine"])
    net.train()
    _NETS[key] = (net, coarse, fine)
    return _NETS[key]


def _hip_d_rays(idn, dev, sc, front=None, rays_grad=True, entry_calls=None):
    """One render of the case's rays with gradients and the backward of its loss -> dict(d_rays, z_c, z_f, outputs, param
    gradients).  The depths are the ones the forward handed to its two network passes (autograd._train_query).
    front: other rays put in front of the scene's (with loss weights and background of their own; the scene's rows keep
    theirs); entry_calls: a list that counts calls of ops.pass_bwd_rays."""
    from idealnerf_amd import autograd as ag
    ops = idn.ops
    net, coarse, fine = _network(idn, dev, sc)
    g = lambda t: None if t is None else t.to(dev)
    k = 0 if front is None else front.shape[0]
    pad = lambda t: t if k == 0 else torch.cat([t.repeat(-(-k // t.shape[0]), *([1] * (t.dim() - 1)))[:k], t], 0)
    rays = (sc["rays"] if front is None else torch.cat([front, sc["rays"]], 0)).to(dev).clone().requires_grad_(rays_grad)
    weights = {key: pad(w) for key, w in sc["weights"].items()}
    bc = g(pad(sc["bc"])).contiguous()
    zs = []
    real_query, real_entry = ag._train_query, ops.pass_bwd_rays
    ag._train_query = lambda net_, folded, r, z: (zs.append(z.detach().clone()), real_query(net_, folded, r, z))[1]
    if entry_calls is not None:
        ops.pass_bwd_rays = lambda *a: (entry_calls.append(1), real_entry(*a))[1]
    try:
        for p in net.parameters():
            p.grad = None
        ret = net._render(rays, bc, g(sc["aud"]), g(sc["latent"]), g(sc["expr"]), coarse, fine, sc["fg"])
        loss = rg.loss_of(ret, weights)
        loss.backward()
    finally:
        ag._train_query, ops.pass_bwd_rays = real_query, real_entry
    grads = {f"{tag}.{k}": p.grad.clone() for tag, m in (("c", coarse), ("f", fine)) for k, p in m.named_parameters()
             if p.grad is not None}
    return dict(d_rays=None if rays.grad is None else rays.grad.clone(), z_c=zs[0], z_f=zs[1] if len(zs) > 1 else None,
                out={k: v.detach().clone() for k, v in ret.items()}, grads=grads)


# ------------------------------------------------------------------------------------------------ case 1
@pytest.mark.parametrize("name", list(rg.CASES))
def test_d_rays_vs_fp64_oracle(idn, dev, name):
    from idealnerf_amd import autograd as ag
    sc = rg.scene(name)
    hip = _hip_d_rays(idn, dev, sc)
    d_rays = hip["d_rays"]
    assert d_rays is not None and d_rays.shape == (sc["n"], 11) and torch.isfinite(d_rays).all()
    assert float(d_rays[:, 6:8].abs().max()) == 0.0                                  # near / far: written as 0
    assert hip["z_c"].shape == (sc["n"], sc["S"]) and (hip["z_f"] is None) == (sc["Ni"] == 0)
    g64 = rg.oracle_d_rays(sc, hip["z_c"], hip["z_f"], torch.float64)
    g32 = rg.oracle_d_rays(sc, hip["z_c"], hip["z_f"], torch.float32)
    e32 = oracle.fp32_noise_floor(g32, g64)
    bound = FACTOR * e32
    errs = rg.block_errors(d_rays, g64)
    no_norm = rg.block_errors(rg.oracle_d_rays(sc, hip["z_c"], hip["z_f"], torch.float64, detach_norm=True), g64)["d"]
    print(f"\n{name} [{ag.TRAIN_PRECISION}]: e32 {e32:.2e}  bound {bound:.2e}  HIP " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
          f"  (fp32 oracle per block: " + "  ".join(f"{k} {v:.2e}" for k, v in rg.block_errors(g32, g64).items()) +
          f"; without the |rays_d| term d moves {no_norm:.2e})")
    _record(f"{name}/{ag.TRAIN_PRECISION}", dict(e32=e32, bound=bound, hip=errs, fp32_oracle=rg.block_errors(g32, g64),
                                                 norm_term_share_of_d=no_norm, n=sc["n"], S=sc["S"], Ni=sc["Ni"]))
    assert e32 <= 1e-3, "the scene is too sharp to test a gradient on"
    assert no_norm > 10 * bound, "the |rays_d| term does not carry enough of d rays_d on this scene"
    for k, v in errs.items():
        assert v <= bound, (name, k, v, bound)


def test_d_rays_cases_on_the_other_training_precision(idn, dev):
    """IDN_TRAIN_PRECISION is read once at import: the five cases again in a fresh process on the other arithmetic."""
    from idealnerf_amd import autograd as ag
    other = "f32" if ag.TRAIN_PRECISION == "bf16x6" else "bf16x6"
    env = dict(os.environ, IDN_TRAIN_PRECISION=other)
    child = subprocess.Popen([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-k",
                              "test_d_rays_vs_fp64_oracle"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                             start_new_session=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        out, err = child.communicate(timeout=180)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.wait()
        pytest.fail("the child run did not finish within 180 s")
    print(out[-4000:])
    assert child.returncode == 0 and f"{len(rg.CASES)} passed" in out, out[-4000:] + err[-2000:]


# ------------------------------------------------------------------------------------------------ case 2
@pytest.mark.parametrize("name", ["37x64+128", "26x5", "2x256+256"])
def test_d_rays_is_deterministic_and_independent_of_the_rays_position(idn, dev, name):
    """The same call twice gives d rays bit for bit; so does a call with the batch preceded by 128 other rays, on the shared
    rows: no summation order depends on where a ray stands in the grid."""
    sc = rg.scene(name)
    a = _hip_d_rays(idn, dev, sc)
    b = _hip_d_rays(idn, dev, sc)
    assert torch.equal(a["d_rays"], b["d_rays"])
    other = rg.scene("37x64+128fg")["rays"]
    front = other.repeat(4, 1)[:128]
    assert front.shape[0] == 128
    c = _hip_d_rays(idn, dev, sc, front=front)
    n = sc["n"]
    assert torch.equal(c["z_c"][128:], a["z_c"]) and (a["z_f"] is None or torch.equal(c["z_f"][128:], a["z_f"]))
    assert torch.equal(c["d_rays"][128:128 + n], a["d_rays"])


def test_rays_without_grad_never_reach_the_new_entry(idn, dev):
    """With rays not requiring grad the outputs and every parameter gradient are bit-identical to the call with rays that do,
    and ops.pass_bwd_rays is never called (with: once per pass)."""
    from idealnerf_amd import autograd as ag
    sc = rg.scene("37x64+128")
    calls_on, calls_off = [], []
    on = _hip_d_rays(idn, dev, sc, entry_calls=calls_on)
    off = _hip_d_rays(idn, dev, sc, rays_grad=False, entry_calls=calls_off)
    assert len(calls_on) == 2 and calls_off == []
    assert off["d_rays"] is None and on["d_rays"] is not None
    assert on["out"].keys() == off["out"].keys() and on["grads"].keys() == off["grads"].keys() and len(on["grads"]) == 2 * len(ag.PARAM_KEYS)
    for k in on["out"]:
        assert torch.equal(on["out"][k], off["out"][k]), k
    for k in on["grads"]:
        assert torch.equal(on["grads"][k], off["grads"][k]), k


def test_pass_bwd_rays_with_null_d_rays_is_pass_bwd(idn, dev):
    """idealnerf_pass_bwd_rays(d_rays = NULL) fills the same gradient tensors as idealnerf_pass_bwd, bit for bit -- and with
    d_rays given, still the same (the ray gradient is computed after, and beside, everything else)."""
    from idealnerf_amd import autograd as ag
    from idealnerf_amd.helper import linspace01
    ops = idn.ops
    sc = rg.scene("26x5")
    net, coarse, _ = _network(idn, dev, sc)
    g = lambda t: t.to(dev)
    rays, bc = g(sc["rays"]).contiguous(), g(sc["bc"]).contiguous()
    aud, expr, lat = g(sc["aud"]), g(sc["expr"]), g(sc["latent"])
    for S in (5, 192):
        z = ops.coarse_depths(rays, linspace01(S, dev))
        raw, acts = ag._train_query(coarse, coarse.folded_bias(aud, expr, lat), rays, z)
        rs = np.random.RandomState(S)
        g_rgb = torch.from_numpy(rs.standard_normal((sc["n"], 3)).astype(np.float32)).to(dev)
        g_acc = torch.from_numpy(rs.standard_normal(sc["n"]).astype(np.float32)).to(dev)
        sd = coarse.kernel_tensors()

        def run(fn, *extra):
            grads = {k: torch.full_like(sd[k], float("nan")) for k in ag.PARAM_KEYS}
            d_aud, d_lat = torch.zeros_like(aud), torch.zeros_like(lat)
            fn(coarse.kernel_params(), grads, aud, expr, lat, acts, raw, z, rays, bc, g_rgb, None, None, g_acc, d_aud, d_lat, *extra)
            return dict(grads, d_aud=d_aud, d_lat=d_lat)
        base = run(ops.pass_bwd)
        null = run(ops.pass_bwd_rays, None)
        d_rays = torch.full((sc["n"], 11), float("nan"), device=dev)
        full = run(ops.pass_bwd_rays, d_rays)
        for k in base:
            assert torch.isfinite(base[k]).all(), k
            assert torch.equal(base[k], null[k]) and torch.equal(base[k], full[k]), (S, k)
        assert torch.isfinite(d_rays).all() and float(d_rays[:, 6:8].abs().max()) == 0.0 and float(d_rays.abs().max()) > 0


def test_rays_with_grad_and_a_frozen_network_raise(idn, dev):
    sc = rg.scene("26x5")
    net, coarse, fine = _network(idn, dev, sc)
    coarse.requires_grad_(False)
    try:
        with pytest.raises(idn._lib.IdealNerfError, match="frozen"):
            _hip_d_rays(idn, dev, sc)
    finally:
        coarse.requires_grad_(True)


# ------------------------------------------------------------------------------------------------ case 3
def _clip(tmp_path, name="clip"):
    d = str(tmp_path / name)
    os.makedirs(d)
    flags, meta = write_clip_directory(d, 64, 6, seed=2, N_rand=48, mouth_rays=8, torso_rays=4)
    return d, flags, meta


def test_train_step_gradient_of_the_pose_delta_vs_fp64_oracle(idn, dev, tmp_path):
    """One train_step (the reference's loss, 48 rays of the resident loader on a 6-frame directory) with the frame's rays
    refined by a non-zero delta: d loss / d (omega, tau) against the oracle's float64 autograd of the same loss through
    camera_rays of c2w' at the batch's pixels, at the HIP forward's depths.  Bound as in case 1: 4 x the fp32 oracle's own
    distance from the fp64 oracle, relative to the largest entry of the omega and of the tau block."""
    from idealnerf_amd import autograd as ag, dataset, train as T_
    from idealnerf_amd.audio_exp_nerf import Network, init_weights
    from idealnerf_amd.config import to_render_config
    from idealnerf_amd.pose_refine import PoseRefiner, refined_c2w
    d, flags, _ = _clip(tmp_path)
    args = train_flags(d, tmp_path / "logs", "grad", flags, perturb=0.0, chunk=8192)
    torch.manual_seed(5)
    frames = dataset.ResidentFrames(d, "aud.npy", "train", args, device=dev, seed=3)
    net = Network(64, 64, frames.focal, near=args.near, far=args.far, chunk=args.chunk, intrinsic=None, N_samlpes=args.N_samples,
                  N_importance=args.N_importance, args=to_render_config(args)).to(dev)
    net.apply(init_weights)
    net.train()
    lat = torch.ones(len(frames), 32, dtype=torch.float32, device=dev, requires_grad=True)
    ref = PoseRefiner(len(frames)).to(dev)
    frame, draw = 4, 9
    delta = torch.tensor([0.011, -0.007, 0.004, 0.003, -0.002, 0.005])
    with torch.no_grad():
        ref.deltas[frame] = delta.to(dev)
    opt = T_.make_optimizer(net, lat, args.lrate)
    opt.add_param_group({"params": [ref.deltas], "lr": 0.0, "lr_scale": 0.0})
    pix = frames.select(frame, draw).clone().cpu()
    data = frames.batch(frame, draw)
    assert data[0].shape == (2, 48, 3)
    with torch.no_grad():   # what the step is about to see: the oracle's constants, taken before Adam moves them
        aud = net.audio_feature(data[3].to(dev, torch.float32), frame, 0, len(frames)).reshape(-1).cpu()
    pc = {k: v.detach().cpu().clone() for k, v in net.face_nerf_coarse.state_dict().items()}
    pf = {k: v.detach().cpu().clone() for k, v in net.face_nerf_fine.state_dict().items()}
    zs = []
    real_query = ag._train_query
    ag._train_query = lambda net_, folded, r, z: (zs.append(z.detach().clone()), real_query(net_, folded, r, z))[1]
    try:
        info = T_.train_step(net, opt, (ref(frame, data[0]), *data[1:]), lat, 0, len(frames), lrate=args.lrate,
                             lrate_decay=args.lrate_decay)
    finally:
        ag._train_query = real_query
    got = ref.deltas.grad[frame].detach().double().cpu()
    assert float(ref.deltas.grad[[0, 1, 2, 3, 5]].abs().max()) == 0.0 and torch.isfinite(got).all()
    expr, target, bc = data[6].float().cpu(), data[1].float().cpu(), data[2].float().cpu()
    sc = dict(dims=oracle.facenerf_dims(), fg=False, coarse=pc, fine=pf, aud=aud, expr=expr, latent=torch.ones(32), bc=bc)
    c2w = torch.as_tensor(np.asarray(frames.all_poses[frame]), dtype=torch.float64)[:3, :4]

    def oracle_grad(dtype):
        old = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            dl = delta.to(dtype).clone().requires_grad_(True)
            ro, rd = oracle.camera_rays(frames.H, frames.W, frames.focal, refined_c2w(dl, c2w.to(dtype)), cx=frames.cx, cy=frames.cy)
            o, dd = ro.reshape(-1, 3)[pix], rd.reshape(-1, 3)[pix]
            one = torch.ones_like(dd[:, :1])
            rays = torch.cat([o, dd, args.near * one, args.far * one, dd / torch.norm(dd, dim=-1, keepdim=True)], -1)
            out = rg.oracle_outputs(sc, rays, zs[0].cpu().to(dtype), zs[1].cpu().to(dtype))
            loss, _ = oracle.train_loss(out, target.to(dtype), torch.ones(32, dtype=dtype), lc_weight=args.lc_weight)
            g, = torch.autograd.grad(loss, dl)
            return g.double(), float(loss.detach())
        finally:
            torch.set_default_dtype(old)
    g64, loss64 = oracle_grad(torch.float64)
    g32, _ = oracle_grad(torch.float32)
    assert abs(float(info["loss"]) - loss64) < 1e-5 * abs(loss64)
    e32 = oracle.fp32_noise_floor(g32, g64)
    bound = FACTOR * e32
    blocks = {"omega": slice(0, 3), "tau": slice(3, 6)}
    errs = {k: float((got[s] - g64[s]).abs().max() / g64[s].abs().max()) for k, s in blocks.items()}
    print(f"\nd loss / d (omega, tau): e32 {e32:.2e}  bound {bound:.2e}  HIP {errs}  d = {got.tolist()}")
    _record(f"train_step_pose_delta/{ag.TRAIN_PRECISION}", dict(e32=e32, bound=bound, hip=errs))
    assert e32 <= 1e-3
    for k, v in errs.items():
        assert v <= bound, (k, v, bound)


def _refine_state(run):
    st = {"w." + k: v.detach().clone() for k, v in run["network"].state_dict().items()}
    st["latent"] = run["latent_codes"].detach().clone()
    st["deltas"] = run["pose_refiner"].deltas.detach().clone()
    osd = run["optimizer"].state_dict()
    for i, s in osd["state"].items():
        for k, v in s.items():
            st[f"opt.{i}.{k}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    st["opt.lr"] = torch.tensor([g["lr"] for g in osd["param_groups"]], dtype=torch.float64)
    return st


def test_train_with_pose_refinement_moves_visited_rows_checkpoints_and_resumes(idn, dev, tmp_path):
    """train(steps=4, refine_poses=True) on 6 frames: only the rows of frames 0..3 have moved; head.tar carries pose_deltas;
    2 steps + 2 resumed steps reproduce the 4-step run's deltas, weights, optimizer state and losses bit for bit; with the
    option off the file's keys and the optimizer's groups are what they were."""
    from idealnerf_amd import train as T_
    d, flags, _ = _clip(tmp_path)
    mk = lambda name: train_flags(d, tmp_path / "logs", name, flags, perturb=0.0, i_print=1, i_weights=1, N_iters=10, chunk=8192)
    losses = {}

    def run(name, steps, seed, **kw):
        torch.manual_seed(seed)
        return T_.train(mk(name), loader="resident", sample_seed=3, device=dev, steps=steps, val="reference",
                        on_step=lambda step, info: losses.setdefault(name, []).append(info["loss"].clone()), **kw)
    whole = run("whole", 4, 11, refine_poses=True)
    deltas = whole["pose_refiner"].deltas.detach()
    assert whole["global_step"] == 4 and deltas.shape == (6, 6)
    assert all(float(deltas[i].abs().max()) > 0 for i in range(4)) and float(deltas[4:].abs().max()) == 0.0
    groups = whole["optimizer"].param_groups
    assert len(groups) == 2 and groups[1]["params"][0] is whole["pose_refiner"].deltas
    assert groups[1]["lr"] == pytest.approx(0.1 * groups[0]["lr"], rel=1e-12)      # default pose_lrate = 0.1 lrate, same decay
    ck = torch.load(str(tmp_path / "logs" / "whole" / "head.tar"), weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer", "latent_codes", "pose_deltas"} and ck["global_step"] == 4
    assert torch.equal(ck["pose_deltas"].to(dev), deltas)

    run("parts", 2, 11, refine_poses=True)
    second = run("parts", 2, 999, refine_poses=True)        # nothing of the second half may come from anywhere but head.tar
    assert second["global_step"] == 4
    a, b = _refine_state(whole), _refine_state(second)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    assert len(losses["parts"]) == 4 and all(torch.equal(x, y) for x, y in zip(losses["whole"], losses["parts"]))

    plain = run("plain", 2, 11)
    assert "pose_refiner" not in plain and len(plain["optimizer"].param_groups) == 1
    assert "lr_scale" not in plain["optimizer"].param_groups[0]
    ck = torch.load(str(tmp_path / "logs" / "plain" / "head.tar"), weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer", "latent_codes"}
    # the first step of both runs sees the same rays (zero deltas are the identity, exactly): the same loss
    assert torch.equal(losses["plain"][0], losses["whole"][0])
