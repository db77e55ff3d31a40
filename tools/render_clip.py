#!/usr/bin/env python3
"""Render a whole clip to an AVI and print one JSON line: the command line over idealnerf_amd.clip.

    python tools/render_clip.py --flow torso --frames 25 --out clip.avi             # head + torso, synthetic scene
    python tools/render_clip.py --flow torso --frames 64 --gpus 8 --out clip.avi    # frame-parallel, one rank per GPU
    python tools/render_clip.py --flow head --datadir dataset/May --aud-file aud.npy --ckpt run/head.tar --out clip.avi
    python tools/render_clip.py --tail-timing                                        # the fused tail against the eager ops

--flow torso is `clip.render_torso_clip` on the scene bench.py's torso measurement builds (synthetic.frame, xavier seeds
2..5 with density gains 300 / 4, plain bf16, perturb 0, 512 x 512, 64 + 128 samples) with a seeded pose and audio track of
--frames entries.  --flow head is `clip.render_head_clip` on a dataset directory in the reference's format, weights from a
reference checkpoint (--ckpt) or xavier.  --gpus N starts N ranks as fresh child processes (`python -m
torch.distributed.run`, rendezvous on 127.0.0.1); this parent never opens the GPU.  IDN_DIST_BACKEND=gloo
IDN_FORCE_DEVICE=0 rehearses N > 1 on one GPU (the ranks share it: that proves the path, it is not a scaling number).

The line: {"metric": "frames/s (...)", "value", "n_frames", "nonfinite_frames", "seconds", "frames_per_s", "world", ...}.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--flow", choices=("torso", "head"), default="torso")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--frames", type=int, default=25, help="clip length (torso: at least the smoothing window, 8)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--perturb", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=None, help="per-frame draws seeded with seed + frame (perturb > 0)")
    ap.add_argument("--warmup", type=int, default=1, help="frames rendered and thrown away before the clip is timed")
    ap.add_argument("--out", default="clip.avi")
    ap.add_argument("--codec", choices=("MJPG", "raw"), default="MJPG")
    ap.add_argument("--swap-rb", action="store_true")
    ap.add_argument("--still-every", type=int, default=0)
    ap.add_argument("--still-path", default=None, help="torso: a directory; head: a template such as out/frame_{i}.jpg")
    ap.add_argument("--datadir", default=None)
    ap.add_argument("--aud-file", default="aud.npy")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--global-step", type=int, default=None, help="head: default is the checkpoint's, else nosmo_iters")
    ap.add_argument("--tail-timing", action="store_true", help="HIP-event time of ops.compose_to8b against multiply + add + to8b")
    ap.add_argument("--scene", choices=("xavier", "box"), default="xavier",
                    help="torso: box = the analytic scene of synthetic.box_density_state_dict (a head box and a lower torso box in empty "
                         "space; xavier density is positive in about half the volume and nothing culls there)")
    ap.add_argument("--timing-json", default=None, help="torso: measure --cull 0 against --cull G (default 128) -- and, with --cull-samples, "
                                                        "against --cull G --cull-samples -- in this process, alternating, three rounds of "
                                                        "warmed windows, and write the figures there")
    cull_arguments(ap)
    return ap.parse_args()


def cull_arguments(ap):
    """--cull G and its options, shared by the clip tools."""
    ap.add_argument("--cull", type=int, default=0, metavar="G",
                    help="skip empty rays with a per-clip occupancy grid of G^3 cells (a multiple of 32, e.g. 128); 0: off")
    ap.add_argument("--cull-dilate", type=int, default=None, help="cells of dilation (default 1)")
    ap.add_argument("--cull-sigma-min", type=float, default=None, help="a corner is occupied above this sigma_raw (default 0.0)")
    ap.add_argument("--cull-stride", type=int, default=None,
                    help="mark every k-th frame's conditioning only (default 1; k > 1 gives up the bit-exact guarantee)")
    ap.add_argument("--cull-samples", action="store_true",
                    help="with --cull G: the live rays' network passes skip the samples in empty cells too (same bytes)")


def cull_option(args):
    """The flows' cull= argument from the command line: None when --cull is 0."""
    if not args.cull:
        if args.cull_samples:
            sys.exit("--cull-samples culls the samples of the rays the grid leaves live: it needs --cull G")
        return None
    return dict(G=args.cull, dilate=args.cull_dilate, sigma_min=args.cull_sigma_min, frame_stride=args.cull_stride,
                samples=True if args.cull_samples else None)


def launch(n, argv, script=None):
    """N ranks as children of this process, which has not touched the GPU; rank 0's JSON line is relayed.
    script: the file the ranks run (default: this one; tools/score_clip.py starts its ranks through here)."""
    script = os.path.abspath(script or __file__)
    name = os.path.basename(script)
    import signal
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), script] + list(argv)
    child = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, _ = child.communicate(timeout=float(os.environ.get("IDN_LAUNCH_TIMEOUT_S", "1500")))
    except subprocess.TimeoutExpired:
        for sig in (signal.SIGTERM, signal.SIGKILL):     # the whole group, by its id
            try:
                os.killpg(child.pid, sig)
                child.wait(timeout=15)
                break
            except ProcessLookupError:
                break
            except subprocess.TimeoutExpired:
                continue
        sys.stderr.write(f"{name}: the {n}-rank run did not finish in time\n")
        return 124
    line = None
    for ln in out.splitlines():
        try:
            obj = json.loads(ln)
        except ValueError:
            obj = None
        if isinstance(obj, dict) and "metric" in obj:
            line = ln
        else:
            sys.stderr.write(ln + "\n")
    if child.returncode != 0 or line is None:
        sys.stderr.write(f"{name}: the ranks failed (exit code {child.returncode}) or printed no result line\n")
        return child.returncode or 1
    print(line, flush=True)
    return 0


def init_ranks():
    import datetime
    import torch
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("IDN_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    backend = os.environ.get("IDN_DIST_BACKEND", "nccl") if world > 1 else None
    have = torch.cuda.device_count()
    if "IDN_FORCE_DEVICE" not in os.environ and (local >= have or (backend == "nccl" and world > have)):
        sys.exit(f"render_clip.py: rank {rank} of {world} needs GPU {local}, but this node exposes {have}: use --gpus <= {have}, "
                 "or rehearse with IDN_DIST_BACKEND=gloo IDN_FORCE_DEVICE=0")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if backend is not None:
        limit = datetime.timedelta(seconds=int(os.environ.get("IDN_DIST_TIMEOUT_S", "300")))
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=limit)
        else:
            dist.init_process_group(backend, timeout=limit)
    return world, rank, dev, backend


def torso_scene(args, dev):
    import numpy as np
    import torch
    import idealnerf_amd
    from idealnerf_amd import synthetic
    from idealnerf_amd.helper import RenderConfig
    from idealnerf_amd.train_torso import Network
    H = W = args.size
    syn = synthetic.frame(H, W, seed=0)
    cfg = RenderConfig(perturb=args.perturb, chunk=32768, near=syn["near"], far=syn["far"], dim_expr=76)
    torch.manual_seed(0)   # the audio nets: every rank builds the same network
    net = Network(H, W, syn["focal"], syn["near"], syn["far"], 32768, 64, 128, args=cfg, dim_expr_head=76).to(dev).eval()
    for i, m in enumerate((net.face_nerf_coarse, net.face_nerf_fine, net.torso_coarse_nerf, net.torso_fine_nerf)):
        if args.scene == "box":   # a head box whose half-width follows the audio a little, and a torso box below it
            synthetic.box_density_state_dict(m, 2 + i, (0.0, 0.0, 0.0) if i < 2 else (0.0, -0.17, 0.0), 0.08 if i < 2 else 0.06, 200.0,
                                             0.002 if i < 2 else 0.0)
        else:
            synthetic.xavier_state_dict(m, 2 + i, 300.0 if i < 2 else 4.0, 0.3 if i < 2 else -0.2)
    idealnerf_amd.set_render_precision(net, args.precision)
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]])
    poses = torch.stack([torch.cat([synthetic.frame(H, W, seed=j)["c2w"], bottom], 0) for j in range(args.frames)])
    auds = torch.from_numpy(np.random.RandomState(11).standard_normal((args.frames, 16, 29)).astype(np.float32))
    return net, dict(poses=poses, auds=auds, bc_img=syn["bc"]), dict(expr=syn["expr"], latent_code=syn["latent"], torso_pose=poses[0])


def run_torso(args, dev):
    from idealnerf_amd import clip
    net, track, cond = torso_scene(args, dev)
    common = dict(cond, seed=args.seed, swap_rb=args.swap_rb, cull=cull_option(args))
    if args.timing_json:
        return cull_timing(args, dev, net, track, common)
    if args.warmup:   # first-launch costs (code objects, weight packing, pinned buffers) stay out of the clip's time
        clip.render_torso_clip(net, track["poses"], track["auds"], track["bc_img"], None, frames=range(args.warmup), codec="raw", **common)
    if args.still_every and args.still_path:
        os.makedirs(args.still_path, exist_ok=True)
    return clip.render_torso_clip(net, track["poses"], track["auds"], track["bc_img"], args.out, codec=args.codec,
                                  still_every=args.still_every, still_path=args.still_path, **common)


def run_head(args, dev):
    import torch
    import idealnerf_amd
    from types import SimpleNamespace
    from idealnerf_amd import checkpoint, clip, dataset, synthetic
    from idealnerf_amd.audio_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    if not args.datadir:
        sys.exit("render_clip.py: --flow head needs --datadir (a dataset directory in the reference's format)")
    flags = SimpleNamespace(gt_dirs="head_imgs", testskip=1, N_rand=64, sample_rate=0.95, mouth_rays=8, torso_rays=4)
    ds = dataset.GetData(args.datadir, args.aud_file, "val", flags, skip=1, device=dev)
    cfg = RenderConfig(perturb=args.perturb)
    net = Network(ds.H, ds.W, ds.focal, cfg.near, cfg.far, cfg.chunk, None, cfg.N_samples, cfg.N_importance, args=cfg)
    step, latent = cfg.nosmo_iters, torch.zeros(32)
    if args.ckpt:
        step, codes = checkpoint.load_checkpoint(args.ckpt, net, map_location="cpu")
        latent = codes[0]
    else:
        synthetic.xavier_state_dict(net.face_nerf_coarse, 2, 300.0, 0.3)
        synthetic.xavier_state_dict(net.face_nerf_fine, 3, 300.0, 0.3)
    net = net.to(dev).eval()
    idealnerf_amd.set_render_precision(net, args.precision)
    frames = range(min(args.frames, ds.data_size))
    return clip.render_head_clip(net, ds, args.out, step if args.global_step is None else args.global_step, latent_code=latent,
                                 frames=frames, seed=args.seed, codec=args.codec, swap_rb=args.swap_rb,
                                 still_every=args.still_every, still_path=args.still_path, cull=cull_option(args))


def cull_timing(args, dev, net, track, common, rounds=3):
    """--cull 0 against --cull G on one scene in one process: per round one window of --frames frames per arm, alternating,
    each window warmed by --warmup frames and ended by the clip's own end (the last frame's bytes on the host).  The grid is
    built inside each culled window (its time is reported apart and is NOT in the arm's frames/s: a clip pays it once).
    Then, on the head pair's frame 0: the HIP-event times of classify, gather and fill + scatter, and the host cost of the
    one n_live read.  With --cull-samples a third arm renders with the sample cull on as well (the grids' `samples`), its
    `evaluated_share` is reported per pair, and the pieces gain the sample cull's three kernels and its read on the coarse and
    on the fine pass of one 32 768-ray chunk of that frame's live rays."""
    import time
    import torch
    from idealnerf_amd import clip, cull, ops
    opts = cull.options(dict(cull_option(args) or {}, G=args.cull or 128, samples=None))
    poses, auds, bc = track["poses"], track["auds"], track["bc_img"]
    base = {k: v for k, v in common.items() if k != "cull"}
    n = args.frames
    frames = list(range(n))
    arms = {"cull_0": [], f"cull_{opts['G']}": []}
    if args.cull_samples:
        arms[f"cull_{opts['G']}_samples"] = []
    info, shares = {}, None
    for r in range(rounds):
        for name in arms:
            on = name != "cull_0"
            arm_opts = dict(opts, samples=name.endswith("_samples"))
            grids = clip._torso_grids(net, poses, auds, bc, base["expr"], base["latent_code"], base["torso_pose"], frames, arm_opts) if on else {}
            net.set_cull(**grids)
            try:
                clip.render_torso_clip(net, poses, auds, bc, None, frames=range(args.warmup or 1), codec="raw", **base)
                torch.cuda.synchronize(dev)
                res = clip.render_torso_clip(net, poses, auds, bc, None, frames=frames, codec="raw", **base)
            finally:
                net.set_cull()
            arms[name].append(res["frames_per_s"])
            if name.endswith("_samples"):
                shares = cull.summary(grids)["evaluated_share"]
            elif on:
                info = cull.summary(grids)
                info["frames_marked"] = {k: g.stats["frames_marked"] for k, g in grids.items()}
                info["torso_classifications"] = grids["torso"].classify_calls
    if shares is not None:
        info["evaluated_share"] = shares
    # the pieces, on the head pair at frame 0
    grid = clip._torso_grids(net, poses, auds, bc, base["expr"], base["latent_code"], base["torso_pose"], frames, opts)["head"]
    H, W = int(bc.shape[0]), int(bc.shape[1])
    frame = ops.make_frame(poses[0][:3, :4], H, W, net.focal, net.near, net.far)
    bc_flat = bc.to(dev).reshape(-1, 3).contiguous()
    dz, K = grid.steps(frame)

    def timed(fn, reps=50):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / reps

    sel, n_dev = ops.cull_classify(grid.bits, grid.G, grid.lo, grid.cell, frame, dz, K)
    n_live = int(n_dev.item())
    rays, bc_live = ops.cull_gather(sel[:n_live], frame, bc_flat)
    live3, live1 = torch.rand(n_live, 3, device=dev), torch.rand(n_live, device=dev)
    fills = cull._fills(frame.far_)
    outs = {k: ((live3 if fills[k][0] == 3 else live1), *fills[k]) for k in fills}
    pieces = dict(classify_us=timed(lambda: ops.cull_classify(grid.bits, grid.G, grid.lo, grid.cell, frame, dz, K, sel, n_dev)),
                  gather_us=timed(lambda: ops.cull_gather(sel[:n_live], frame, bc_flat)),
                  fill_scatter_11_outputs_us=timed(lambda: ops.cull_scatter(sel, n_live, bc_flat, outs)), march_steps=K, n_live=n_live)
    reads = []
    for _ in range(20):   # the read alone: the classification has finished before the clock starts
        ops.cull_classify(grid.bits, grid.G, grid.lo, grid.cell, frame, dz, K, sel, n_dev)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        n_dev.item()
        reads.append((time.perf_counter() - t0) * 1e6)
    pieces["n_live_read_idle_queue_us"] = sorted(reads)[len(reads) // 2]
    if args.cull_samples:
        pieces["samples"] = sample_pieces(dev, net, grid, rays[:32768].contiguous(), bc_live[:32768].contiguous(), base, timed)
    out = dict(scene=args.scene, size=args.size, dtype=args.precision, frames_per_window=n, rounds=rounds, warmup=args.warmup or 1,
               frames_per_s={k: dict(rounds=v, median=sorted(v)[len(v) // 2]) for k, v in arms.items()}, cull=info, pieces=pieces,
               options=opts, device=torch.cuda.get_device_name(dev))
    with open(args.timing_json, "w") as f:
        json.dump(out, f, indent=1)
    return dict(n_frames=n, nonfinite_frames=[], seconds=0.0, frames_per_s=out["frames_per_s"][f"cull_{opts['G']}"]["median"], world=1,
                timing=out)


def sample_pieces(dev, net, grid, rays, bc_live, base, timed):
    """The sample cull's own kernels and its read, per network pass, on one chunk of live rays of the head pair."""
    import time
    import torch
    from idealnerf_amd import ops
    from idealnerf_amd.helper import linspace01
    S, Ni = net.args.N_samples, net.args.N_importance
    coarse = net.face_nerf_coarse
    with torch.no_grad():   # (a zero audio feature: the depths only have to be representative of a frame's)
        folded = coarse.folded_bias(torch.zeros(coarse.dim_aud, device=dev), base["expr"].to(dev), base["latent_code"].to(dev))
        z_c = ops.coarse_depths(rays, linspace01(S, dev))
        raw = ops.query_rays_fwd(coarse.packed_weights(), folded, rays, z_c, coarse.prec_code)
        z_f = ops.march_fwd(raw, z_c, rays, bc_live, linspace01(Ni, dev), Ni)["z_fine"]
    out = dict(n_rays=int(rays.shape[0]))
    for name, z in (("coarse", z_c), ("fine", z_f)):
        n, Sz = z.shape
        sel, n_dev = ops.cull_sample_classify(grid.bits, grid.G, grid.lo, grid.cell, rays, z)
        m = int(n_dev.item())
        pts, dirs = ops.cull_sample_gather(sel[:m], rays, z)
        raw_live = torch.rand(m, 4, device=dev)
        reads = []
        for _ in range(20):
            ops.cull_sample_classify(grid.bits, grid.G, grid.lo, grid.cell, rays, z, sel, n_dev)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            n_dev.item()
            reads.append((time.perf_counter() - t0) * 1e6)
        out[name] = dict(points=n * Sz, live=m,
                         classify_us=timed(lambda: ops.cull_sample_classify(grid.bits, grid.G, grid.lo, grid.cell, rays, z, sel, n_dev)),
                         gather_us=timed(lambda: ops.cull_sample_gather(sel[:m], rays, z)),
                         fill_scatter_us=timed(lambda: ops.cull_sample_scatter(sel, m, raw_live, n, Sz)),
                         count_read_idle_queue_us=sorted(reads)[len(reads) // 2])
    return out


def tail_timing(dev, sizes=(450, 512), reps=200):
    """HIP-event time per call of the fused tail and of the three eager launches it replaces."""
    import torch
    from idealnerf_amd import ops
    out = {}
    for size in sizes:
        g = torch.Generator(device=dev).manual_seed(size)
        rgb = torch.rand((size, size, 3), device=dev, generator=g)
        lw = torch.rand((size, size), device=dev, generator=g)
        fg = torch.rand((size, size, 3), device=dev, generator=g) * 0.5
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        ways = {"compose_to8b_us": lambda: ops.compose_to8b(rgb, lw, fg, False, flag),
                "compose_to8b_with_fg_us": lambda: ops.compose_to8b(rgb, lw, fg, False, flag, want_fg=True),
                "eager_mul_add_to8b_us": lambda: ops.to8b(rgb * lw[..., None] + fg, False, flag)}
        assert torch.equal(ways["compose_to8b_us"](), ways["eager_mul_add_to8b_us"]())
        res = {}
        for name, fn in ways.items():
            for _ in range(20):
                fn()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(reps):
                fn()
            stop.record()
            stop.synchronize()
            res[name] = start.elapsed_time(stop) * 1e3 / reps
        res["note"] = f"back-to-back calls, {reps} per figure, each including its output allocation; host launch cost bounds the small sizes"
        out[f"{size}x{size}"] = res
    return out


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        return launch(args.gpus, sys.argv[1:])
    import torch
    import torch.distributed as dist
    world, rank, dev, backend = init_ranks()
    try:
        if args.tail_timing:
            print(json.dumps({"metric": "fused clip tail, microseconds per call", "device": torch.cuda.get_device_name(dev),
                              "tail": tail_timing(dev)}), flush=True)
            return 0
        res = (run_torso if args.flow == "torso" else run_head)(args, dev)
        if res is not None:
            what = "head + torso composite" if args.flow == "torso" else "head only"
            print(json.dumps(dict(res, metric=f"frames/s ({what} clip, render + convert + copy + file, whole job)",
                                  value=res["frames_per_s"], unit="frames/s", higher_is_better=True, n_gpus=world, backend=backend,
                                  shared_device="IDN_FORCE_DEVICE" in os.environ and world > 1, flow=args.flow, size=args.size,
                                  dtype=args.precision, perturb=args.perturb, codec=args.codec, warmup=args.warmup,
                                  device=torch.cuda.get_device_name(dev))), flush=True)
    finally:
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
