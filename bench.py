#!/usr/bin/env python3
"""Headline benchmark: BASELINE.json configs[1] -- May HeadNeRF 512x512 full-frame
render, N_sample=64 + N_importance=128, synthetic inputs.

    python bench.py --gpus N --steps K --warmup W           (N > 1: starts its own N ranks)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
    python bench.py --full                                  (+ the side measurements, see --full)
    python bench.py --dump-outputs DIR                      (+ the last timed step's outputs as DIR/<name>.npy)

A step = one full frame through the hot path (ray generation -> coarse PE+MLP ->
compositing -> inverse-CDF sampling -> fine PE+MLP -> compositing).  With N ranks the
frame is split into N row bands (one per GPU) and the rendered tiles are all-gathered
over RCCL, so total work is fixed: "strong" scaling.  Inputs are resident in HBM before
the timed region.  value = ray-samples (MLP point evaluations, 256 per ray) per second,
whole job.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_SAMPLE = 1_114_368      # algorithmic, SURVEY.md section 8(d)
PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2516.6   # dense bf16 MFMA: 16x the fp32 rate (1024 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz)
# training step, per ray-sample: forward (as above) + dX (the transposed products of every layer that has a
# hidden input: 7 x 256x256 + 256x129 + 2 x 128x128 + 128x3 MAC) + dW (every forward product once more)
FLOP_PER_SAMPLE_DX = 2 * (7 * 65536 + 256 * 129 + 2 * 16384 + 384)     # 1 049 856
# dW products that run on the bf16 pipe (six piece products each): pts_linears.1..7 (the 256-wide part of .5), views_linears.0's
# 128 units + alpha_linear against a8 (one 256 x 256 launch), views_linears.1 / .2 (the diagonal blocks of one 256 x 256 launch):
# 1 049 088 of the 1 114 368; the rest (pts_linears.0, pts_linears.5's encoding columns, rgb_linear) stays on the fp32 MFMA kernel
FLOP_PER_SAMPLE_DW_X6 = 2 * (7 * 256 * 256 + 256 + 256 * 128 + 2 * 128 * 128)
FLOP_PER_SAMPLE_STEP = FLOP_PER_SAMPLE + FLOP_PER_SAMPLE_DX + FLOP_PER_SAMPLE   # 3 278 592 (SURVEY's 3x rounds up by 2 %)


def mode_peaks():
    # a bf16x3 kernel issues three bf16 MFMAs per algorithmic product: it is priced against peak / 3
    # mixed = two kernels with two peaks (1/4 of the samples on the fp32 path, 3/4 on bf16x3): the blended
    # peak is total FLOP / (coarse FLOP / fp32 peak + fine FLOP / (bf16 peak / 3)), so frac = ideal time / actual
    mixed_peak = 1.0 / (0.25 / PEAK_F32_MFMA_TFLOPS + 0.75 / (PEAK_BF16_MFMA_TFLOPS / 3.0))
    return {"f32": PEAK_F32_MFMA_TFLOPS, "bf16x3": PEAK_BF16_MFMA_TFLOPS / 3.0, "fp16x3": PEAK_BF16_MFMA_TFLOPS / 3.0,
            "bf16": PEAK_BF16_MFMA_TFLOPS, "mixed": mixed_peak,   # the dense fp16 and bf16 MFMA peaks are equal on gfx950
            "mixed6": 1.0 / (0.25 / (PEAK_BF16_MFMA_TFLOPS / 6.0) + 0.75 / (PEAK_BF16_MFMA_TFLOPS / 3.0)),   # bf16x6 coarse + bf16x3 fine
            "bf16x6": PEAK_BF16_MFMA_TFLOPS / 6.0}                # six bf16 piece products per algorithmic product


def profile_kinds(lib):
    """{kind: (ms, launches, points)} from the library's HIP-event profiler (idealnerf_profile_end_kinds)."""
    import ctypes as C
    import idealnerf_amd
    n = len(idealnerf_amd._lib.PROF_KINDS)
    ms, cnt, pts = (C.c_double * n)(), (C.c_int64 * n)(), (C.c_int64 * n)()
    lib.idealnerf_profile_end_kinds(ms, cnt, pts)
    return {k: (ms[i], cnt[i], pts[i]) for i, k in enumerate(idealnerf_amd._lib.PROF_KINDS)}


def launch_ranks(n, argv, script=None, timeout=None):
    """`python bench.py --gpus N` started as ONE plain process: start the N ranks as fresh children
    (`python -m torch.distributed.run`, one rank per GPU, rendezvous on 127.0.0.1), relay rank 0's
    JSON line, and return non-zero when any rank failed or no line came back.  Takes the place of the
    reference's single-process nn.DataParallel start (NeRFs/HeadNeRF/train/distribute_nerf.py:457-466).
    This parent never touches the GPU (no torch.cuda / HIP call precedes this function) and never
    re-execs itself: the ranks are children, so no process that has initialised the GPU is replaced."""
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
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), script or os.path.abspath(__file__)] + list(argv)
    if timeout is None:   # ranks that hang (a peer that never joined a collective) end the run instead of outliving it
        timeout = float(os.environ.get("IDN_LAUNCH_TIMEOUT_S", "1500"))
    import signal
    child = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, start_new_session=True)   # its own process group
    try:
        out, _ = child.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        # the whole group -- the launcher AND its ranks -- by its exact id (never by name): first politely, then not
        for sig in (signal.SIGTERM, signal.SIGKILL):
            try:
                os.killpg(child.pid, sig)
            except ProcessLookupError:
                break
            try:
                child.wait(timeout=15)
                break
            except subprocess.TimeoutExpired:
                continue
        sys.stderr.write(f"bench.py: the {n}-rank run did not finish within {timeout} s\n")
        return 124
    proc = subprocess.CompletedProcess(cmd, child.returncode, out, None)
    line = None
    for ln in proc.stdout.splitlines():
        try:
            obj = json.loads(ln)
        except ValueError:
            obj = None
        if isinstance(obj, dict) and "metric" in obj:   # (a stray "1" from a rank's log is valid JSON too)
            line = ln
            continue
        sys.stderr.write(ln + "\n")      # anything else the ranks printed is diagnostics
    if proc.returncode != 0:
        sys.stderr.write(f"bench.py: a rank failed (torch.distributed.run exit code {proc.returncode})\n")
        return proc.returncode
    if line is None:
        sys.stderr.write("bench.py: the ranks finished without printing a result line\n")
        return 1
    print(line, flush=True)
    return 0


def cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


# the three arrangements of the fp32 64 + 128 per-ray path (idn_render_args::fused_march, IDN_FUSED_MARCH)
KNAME = {0: "idn::mlp_f32_kernel<kModeRays> (fused PE + FaceNeRF MLP, fp32 MFMA)",
         1: ("idn::render_fused_kernel<whole> (ONE launch per chunk: PE + coarse FaceNeRF, march, PE + fine FaceNeRF, compositing; fp32 MFMA; "
             "a ray's depths, raw outputs, weights and cdf stay in LDS)"),
         2: ("idn::render_fused_kernel<coarse> + <fine> (two launches per chunk: PE + coarse FaceNeRF + march | PE + fine FaceNeRF + "
             "compositing; fp32 MFMA; raw outputs, weights and cdf stay in LDS, the fine depths cross HBM)")}
ARRANGEMENT_BLOCK = {0: "kernel_sequence_mode", 1: "fused_march", 2: "fused_split"}
ARRANGEMENT_PMC = {0: "mlp_f32", 1: "render_fused", 2: "render_split"}
ARRANGEMENT_NOTE = ("the arrangements: (0) the kernel sequence mlp_f32_kernel -> march_kernel -> mlp_f32_kernel -> composite_kernel (raw network "
                    "outputs and fine depths cross HBM: 40 B per sample, 0.2 % of the frame time); (1) render_fused_kernel<whole> (fused=True / "
                    "IDN_FUSED_MARCH=1): one launch per 32768-ray chunk, nothing per-sample crosses HBM -- but every change of network re-fetches a "
                    "2.4 MB weight stream into each XCD's L2 (the two streams are 4.7 MB against 4 MiB), more HBM traffic than (0) moves; (2) the same "
                    "kernel as two launches, one network each (fused='split' / IDN_FUSED_MARCH=2): the stream stays in L2 and only the 768 B of fine "
                    "depths per ray cross HBM.  DESIGN.md section 3")


def kernel_source_sha16():
    """Identity of the kernel sources a PMC summary belongs to (tools/pmc_summary.py stores the same hash)."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "ideal-nerf_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            h.update(name.encode())
            h.update(open(os.path.join(csrc, name), "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(precision, fused=0):
    """HBM bytes per launch of the dominant kernel.  PMC counters cannot be read from inside the process, so the
    figure comes from the newest committed rocprofv3 --pmc summary of this same command for this arithmetic
    (profiles/rNN_pmc_mlp_<prec>_final.json; tools/profile_round.sh: FETCH_SIZE x2 gfx950 correction + WRITE_SIZE,
    separate passes) -- and only if that summary was taken from the kernel sources that are running now.
    Returns (bytes or None, traffic_source dict)."""
    import glob
    stem = f"pmc_{ARRANGEMENT_PMC[int(fused)]}_final.json" if fused else f"pmc_mlp_{precision}_final.json"   # (fused: the fp32 64 + 128 arrangements 1 / 2)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_" + stem)))
    if not files:
        return None, {"file": None, "reason": "no PMC summary committed for this arithmetic"}
    path = files[-1]
    try:
        pmc = json.load(open(path))
        src = {"file": os.path.relpath(path, ROOT), "kernel_source_sha16": pmc.get("kernel_source_sha16"),
               "commit": pmc.get("commit"), "current_kernel_source_sha16": kernel_source_sha16()}
        if pmc.get("kernel_source_sha16") != src["current_kernel_source_sha16"]:
            src["reason"] = "summary was taken from different kernel sources: not reported"
            return None, src
        return pmc["hbm_traffic_bytes_per_launch"], src
    except (OSError, KeyError, ValueError) as e:
        return None, {"file": os.path.relpath(path, ROOT), "reason": f"unreadable: {e}"}


def host_cpu_share():
    """CPUs this process may actually use: the cgroup quota if there is one, else the
    affinity mask (the GPU box exposes 256 hardware threads but grants a 16-CPU share)."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return min(n, int(os.environ.get("IDN_CPU_THREADS", "16")))


def cpu_baseline(syn, pc, pf, gpu_rgb_band, band_row0, n_rays=4096, runs=3):
    """The CPU oracle (a port of the reference's path, pinned to it by tests/golden) timed on this host on a
    bounded sample: the first `n_rays` rays of the frame, one warm-up on that same
    tile, then the median of `runs` timed runs."""
    import statistics
    import oracle
    W = syn["W"]
    nrows = (n_rays + W - 1) // W
    threads = host_cpu_share()
    torch.set_num_threads(threads)
    kw = dict(chunk=1024)
    run = lambda: oracle.render_frame(syn["H"], W, syn["focal"], syn["c2w"], syn["near"], syn["far"], syn["bc"], pc, pf,
                                      syn["aud"], syn["expr"], syn["latent"], rows=(0, nrows), **kw)
    times = []
    with torch.no_grad():
        ref = run()   # warm-up on the timed tile
        for _ in range(runs):
            t0 = time.perf_counter()
            ref = run()
            times.append(time.perf_counter() - t0)
    dt = statistics.median(times)
    rays = nrows * W
    out = {"value": rays * 256 / dt, "unit": "ray-samples/s", "cores": torch.get_num_threads(), "kind": "port",
           "cpu": cpu_model(), "s_per_frame_extrapolated": dt * (syn["H"] * W) / rays,
           "sample": f"first {rays} rays ({nrows} rows) of the same {syn['H']}x{W} frame, 64+128 samples, "
                     f"PyTorch-CPU oracle, 1 warm-up on that tile + median of {runs} timed runs "
                     f"({', '.join(f'{t:.2f}' for t in times)} s)"}
    psnr = None
    if gpu_rgb_band is not None and band_row0 == 0 and gpu_rgb_band.shape[0] >= nrows:
        mse = float(((gpu_rgb_band[:nrows].cpu() - ref["rgb_map"]) ** 2).mean())
        psnr = 10.0 * torch.log10(torch.tensor(1.0 / max(mse, 1e-20))).item()
    return out, psnr


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays, limit=DUMP_LIMIT_BYTES):
    """`--dump-outputs`: each tensor of `arrays` as path/<name>.npy in float32, at most `limit` bytes in all.  Every
    array is per pixel ([..., pixels] or [..., pixels, 3]); past the limit each keeps every k-th pixel (the same fixed
    k for all of them, flattened to [pixels / k] or [pixels / k, 3]), so runs with the same arguments stay comparable.
    Returns k."""
    import numpy as np
    host = {k: v.detach().to(torch.float32).cpu().numpy() for k, v in arrays.items()}
    pixels = {k: a.reshape(-1, 3) if a.ndim > 1 and a.shape[-1] == 3 else a.reshape(-1) for k, a in host.items()}
    nbytes = lambda k: sum(-(-p.shape[0] // k) * p[:1].nbytes for p in pixels.values())
    stride = 1
    while nbytes(stride) > limit:
        stride += 1
    os.makedirs(path, exist_ok=True)
    for name, a in host.items():
        np.save(os.path.join(path, name + ".npy"), a if stride == 1 else np.ascontiguousarray(pixels[name][::stride]))
    return stride


def init_ranks(need_gpu=True):
    """(world, rank, device, backend) of this rank.  One process per GPU over RCCL ("nccl" on ROCm);
    IDN_FORCE_DEVICE / IDN_DIST_BACKEND=gloo exist only to rehearse the N>1 path on a one-GPU box
    (ranks sharing device 0) or without a GPU at all (--workload rendezvous)."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("IDN_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    dev = None
    backend = os.environ.get("IDN_DIST_BACKEND", "nccl") if (world > 1 or os.environ.get("IDN_DIST_INIT_WORLD1") == "1") else None
    if need_gpu:
        # one process per GPU: say so before a communicator is built on a device that does not exist
        # (device_count() does not initialise the GPU on this image; ranks sharing a device is the gloo rehearsal only)
        have = torch.cuda.device_count()
        if "IDN_FORCE_DEVICE" not in os.environ and (local >= have or (backend == "nccl" and world > have)):
            sys.exit(f"bench.py: rank {rank} of {world} needs GPU {local}, but this node exposes {have} GPU(s): run with --gpus <= {have} "
                     "(one process per GPU over RCCL), or rehearse with IDN_DIST_BACKEND=gloo IDN_FORCE_DEVICE=0")
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
    if backend is not None:
        import datetime
        limit = datetime.timedelta(seconds=int(os.environ.get("IDN_DIST_TIMEOUT_S", "300")))   # a rank that never shows up is an error, not a 30-minute wait
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=limit)
        else:
            dist.init_process_group(backend, timeout=limit)
        assert dist.get_world_size() == world
    return world, rank, dev, backend


def dist_on():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


def bench_rendezvous(args):
    """No compute: the ranks meet, exchange their row bands and rank 0 prints a line.  It is what the
    CPU test of the launcher runs (tests/test_boundary_cpu.py), and a quick check of a node's
    rendezvous before a real run."""
    import torch.distributed as dist
    from idealnerf_amd import parallel
    world, rank, _, backend = init_ranks(need_gpu=False)
    r0, r1 = parallel.row_band(args.size, rank, world)
    mine = torch.tensor([r0, r1], dtype=torch.int64)
    bands = [torch.zeros(2, dtype=torch.int64) for _ in range(world)]
    if world > 1:
        dist.all_gather(bands, mine)
    else:
        bands = [mine]
    if rank == 0:
        print(json.dumps({"metric": "rendezvous", "value": float(world), "unit": "ranks", "n_gpus": args.gpus,
                          "ranks": world, "backend": backend, "steps": args.steps, "warmup": args.warmup,
                          "bands": [[int(b[0]), int(b[1])] for b in bands]}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def bench_train(args):
    """BASELINE configs[2] as its own line (`--workload train`); the default line carries the same measurement as `train_step`.
    With N ranks: data-parallel training -- every rank draws its own N_rand rays (weak scaling), the gradients are averaged by
    ONE bucketed all-reduce per step (parallel.average_gradients, called by train.train_step) and every replica takes the same
    Adam step.  The reference's counterpart is nn.DataParallel around the Network (distribute_nerf.py:423,457-466)."""
    world, rank, dev, backend = init_ranks()
    res = train_measurement(dev, args.steps, args.warmup, world, rank, backend)
    if rank == 0:
        print(json.dumps(res))
    if dist_on():
        import torch.distributed as dist
        dist.destroy_process_group()


def train_measurement(dev, steps, warmup, world=1, rank=0, backend=None):
    """BASELINE configs[2]: May HeadNeRF train step, N_rand=3072 (2432 uniform + 512 mouth box + 128
    outside the face rect), fwd + bwd + Adam, per GPU.  Secondary measurement; not the headline."""
    import idealnerf_amd
    from idealnerf_amd import synthetic, train as T_
    from idealnerf_amd.audio_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    import numpy as np
    import types
    import torch.distributed as dist
    args = types.SimpleNamespace(steps=steps, warmup=warmup)
    torch.manual_seed(0)      # the audio nets' initialisation: the SAME model on every rank
    H = W = 450
    syn = synthetic.frame(H, W, seed=0)
    cfg = RenderConfig(perturb=1.0, chunk=8192, near=syn["near"], far=syn["far"])
    net = Network(H, W, syn["focal"], syn["near"], syn["far"], 8192, None, 64, 128, args=cfg).to(dev).train()
    synthetic.xavier_state_dict(net.face_nerf_coarse, 2, 300.0, 0.3)
    synthetic.xavier_state_dict(net.face_nerf_fine, 3, 300.0, 0.3)
    torch.manual_seed(rank)   # perturb=1 draws the stratified offsets from torch's generator: same run, same loss; each rank its own draws
    rs = np.random.RandomState(rank)     # every rank samples its own rays of the frame; the weights above are the same everywhere
    uni = rs.choice(H * W, 2432, replace=False)
    yy, xx = np.meshgrid(np.arange(250, 310), np.arange(175, 275), indexing="ij")
    mouth = rs.choice((yy * W + xx).reshape(-1), 512, replace=False)
    border = rs.choice(np.arange(0, 60 * W), 128, replace=False)
    sel = torch.from_numpy(np.concatenate([uni, mouth, border]))
    from idealnerf_amd import ops
    rec = ops.frame_rays(syn["c2w"], H, W, syn["focal"], syn["near"], syn["far"], device=dev)  # [H*W, 11]: o, d, ...
    batch_rays = torch.stack([rec[sel.to(dev), 0:3], rec[sel.to(dev), 3:6]], 0).contiguous()
    bg = syn["bc"].reshape(-1, 3)[sel].contiguous().to(dev)
    tgt = torch.from_numpy(rs.uniform(0, 1, size=(len(sel), 3)).astype(np.float32)).to(dev)
    auds = torch.from_numpy(rs.standard_normal((8, 16, 29)).astype(np.float32)).to(dev)
    pose = torch.cat([syn["c2w"], torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0).to(dev)
    latent_codes = torch.ones(8, 32, device=dev, requires_grad=True)
    opt = T_.make_optimizer(net, latent_codes)
    data = (batch_rays[None], tgt, bg, auds[None], torch.zeros(1, H, W, 3), pose, syn["expr"][None].to(dev), torch.tensor([3]))
    lib = idealnerf_amd._lib.load()

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        T_.train_step(net, opt, data, latent_codes, i, 8)
    fence()
    lib.idealnerf_profile_begin()
    t0 = time.perf_counter()
    for i in range(args.steps):
        info = T_.train_step(net, opt, data, latent_codes, args.warmup + i, 8)
    fence()
    dt = time.perf_counter() - t0
    kinds = profile_kinds(lib)
    in_sync = None
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        # the replicas must still be ONE model: the same gradients and the same Adam step everywhere, bit for bit
        flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()] + [latent_codes.detach().reshape(-1)])
        lo, hi = flat.clone(), flat.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        in_sync = bool(torch.equal(lo, hi))
    samples = len(sel) * 256 * args.steps
    # the MFMA kernel families of a step; forward and delta chain count the points they were launched on, the dW
    # GEMMs the step's points (one launch per layer contracts over all of them).  Families on the bf16 pipe compute
    # six piece products per fp32 product (fp32-grade result): priced against bf16 peak / 6; the others against fp32 MFMA.
    X6 = PEAK_BF16_MFMA_TFLOPS / 6.0
    fl, peaks = {}, {}
    for k, flop, pk in (("mlp_fwd_save", FLOP_PER_SAMPLE, PEAK_F32_MFMA_TFLOPS), ("mlp_fwd_save_x6", FLOP_PER_SAMPLE, X6),
                        ("delta_chain", FLOP_PER_SAMPLE_DX, PEAK_F32_MFMA_TFLOPS), ("delta_chain_x6", FLOP_PER_SAMPLE_DX, X6),
                        ("dw_gemm_x6", FLOP_PER_SAMPLE_DW_X6, X6), ("dw_gemm", FLOP_PER_SAMPLE - FLOP_PER_SAMPLE_DW_X6, PEAK_F32_MFMA_TFLOPS)):
        if kinds[k][1] > 0:      # the families this build / IDN_TRAIN_PRECISION actually launched
            fl[k], peaks[k] = samples * flop, pk
    if "dw_gemm_x6" not in fl:   # a build with -DIDN_DW_X6=0: every dW GEMM on the fp32 pipe
        fl["dw_gemm"] = samples * FLOP_PER_SAMPLE
    split = {k: {"ms_per_step": kinds[k][0] / args.steps, "launches_per_step": kinds[k][1] / args.steps,
                 "algorithmic_tflops": fl[k] / (kinds[k][0] * 1e-3) / 1e12 if kinds[k][0] > 0 else None,
                 "peak_tflops": peaks[k],
                 "frac_of_peak": fl[k] / (kinds[k][0] * 1e-3) / 1e12 / peaks[k] if kinds[k][0] > 0 else None}
             for k in fl}
    k_ms = sum(kinds[k][0] for k in fl)
    ach = sum(fl.values()) / (k_ms * 1e-3) / 1e12 if k_ms > 0 else None
    # blended peak of families with different peaks: total FLOP / (sum of each family's ideal time), so frac = ideal / actual
    peak = sum(fl.values()) / sum(fl[k] / peaks[k] for k in fl)
    return ({"metric": "train ray-samples/sec (N_rand=3072 per GPU, 64+128, fwd+bwd+Adam)", "value": world * samples / dt,
                      "unit": "ray-samples/s", "n_gpus": world, "ranks": world, "backend": backend,
                      **({"replicas_in_sync": in_sync, "parallelism": f"dp{world}: one bucketed gradient all-reduce per step"} if world > 1 else {}),
                      "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                      "dtype": "f32", "data": "synthetic",
                      "arithmetic": "families named `_x6`: every fp32 operand as the exact sum of three bf16 pieces, six piece products per "
                                    "product on the bf16 MFMA pipe, fp32 accumulate (error <= 2^-23 per product, as an fp32 fma chain; "
                                    "gradient parity tests unchanged); the others fp32 MFMA / VALU.  IDN_TRAIN_PRECISION=f32 IDN_BACKWARD_PIPE=f32 "
                                    "put everything on the fp32 pipe",
                      "config": {"workload": "BASELINE configs[2]: May HeadNeRF train step, N_rand=3072 mouth_rays=512 "
                                             "dim_aud=64 dim_expr=76, perturb=1"},
                      "roofline": {"bound": "mfma", "kernel": "the step's MFMA kernel families (see `kernels`): forward with saved activations, delta chain, "
                                                             "256x256 dW GEMMs -- `_x6` = bf16 MFMA, six piece products per fp32 product -- and the "
                                                             "64/128-wide dW GEMMs (fp32 MFMA)",
                                   "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                                   "frac": ach / peak if ach else None, "traffic": None,
                                   "flop_per_sample": FLOP_PER_SAMPLE_STEP, "kernels": split,
                                   "frac_of_fp32_mfma_peak": ach / PEAK_F32_MFMA_TFLOPS if ach else None,
                                   "kernel_time_share": (k_ms * 1e-3) / dt,
                                   "whole_step_algorithmic_tflops": samples * FLOP_PER_SAMPLE_STEP / dt / 1e12,
                                   "note": "achieved = algorithmic FLOP of the families / their summed HIP-event time; peak = the "
                                           "families' blended peak (fp32 MFMA 157.3; the x6 GEMMs bf16 peak / 6 = 419.4); "
                                           "the rest of a step is compositing fwd/bwd, sampling, partial-slab reductions, "
                                           "audio net, Adam"},
                      "final_loss": float(info["loss"])})


def bench_torso(args):
    """BASELINE configs[4]: HeadNeRF + TorsoNeRF two-stage composite, plain-bf16 MFMA MLP, frame-parallel
    (rank r renders its own frames, no collective on the data path: weak scaling).  A step = one
    composited 512x512 frame = two full renders (head C=235, torso C=169).  Secondary measurement."""
    import idealnerf_amd
    from idealnerf_amd import synthetic
    from idealnerf_amd.helper import RenderConfig
    from idealnerf_amd.train_torso import Network
    import torch.distributed as dist
    world, rank, dev, backend = init_ranks()
    res = torso_measurement(dev, args.size, args.precision if args.precision_given else "bf16", args.steps, args.warmup, world, rank, backend)
    if rank == 0:
        print(json.dumps(res))
    if dist_on():
        dist.destroy_process_group()


def torso_measurement(dev, size, prec, steps, warmup, world=1, rank=0, backend=None):
    """The measurement behind `--workload torso` and behind the default line's `torso_composite` block (world = 1)."""
    import idealnerf_amd
    from idealnerf_amd import synthetic
    from idealnerf_amd.helper import RenderConfig
    from idealnerf_amd.train_torso import Network
    import torch.distributed as dist
    import types
    args = types.SimpleNamespace(steps=steps, warmup=warmup)
    H = W = size
    syn = synthetic.frame(H, W, seed=rank)   # every rank renders a different frame of the clip
    cfg = RenderConfig(perturb=0.0, chunk=32768, near=syn["near"], far=syn["far"], dim_expr=76)
    net = Network(H, W, syn["focal"], syn["near"], syn["far"], 32768, 64, 128, args=cfg, dim_expr_head=76).to(dev).eval()
    for i, m in enumerate((net.face_nerf_coarse, net.face_nerf_fine, net.torso_coarse_nerf, net.torso_fine_nerf)):
        synthetic.xavier_state_dict(m, 2 + i, 300.0 if i < 2 else 4.0, 0.3 if i < 2 else -0.2)
    idealnerf_amd.set_render_precision(net, prec)   # "mixed" = fp32 coarse + bf16x3 fine network of each pair
    g = lambda t: t.to(dev)
    aud, expr, latent, bc = g(syn["aud"]), g(syn["expr"]), g(syn["latent"]), g(syn["bc"])
    pose = g(torch.cat([syn["c2w"], torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0))
    kw = dict(H=H, W=W, focal=syn["focal"], render_poses=pose[:3, :4], chunk=32768, near=syn["near"], far=syn["far"], bc_rgb=bc)

    def step():
        aud_torso = net.torso_signal(aud, pose)
        rgb, _, _, _, _, _ = net.render_pair(expr=expr, latent_code=latent, aud_para=aud,
                                             network_nerf={"coarse": net.face_nerf_coarse, "fine": net.face_nerf_fine}, **kw)
        _, _, _, lw_t, fg_t, _ = net.render_pair(expr=None, latent_code=None, aud_para=aud_torso,
                                                 network_nerf={"coarse": net.torso_coarse_nerf, "fine": net.torso_fine_nerf}, **kw)
        return rgb * lw_t[..., None] + fg_t   # train_torso.py:269

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    lib = idealnerf_amd._lib.load()
    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        fence()
        lib.idealnerf_profile_begin()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            frame = step()
        fence()
        dt = time.perf_counter() - t0
    k_ms, k_n, k_pts = profile_kinds(lib)["mlp_fwd"]
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    psnr = None
    if prec != "f32":   # config 5 is judged by PSNR: the same composited frame in exact fp32, after the timed region
        with torch.no_grad():
            idealnerf_amd.set_render_precision(net, "f32")
            ref = step()
            idealnerf_amd.set_render_precision(net, prec)
        psnr = float(-10.0 * torch.log10(((frame.double() - ref.double()) ** 2).mean().clamp_min(1e-30)))
    samples = world * args.steps * H * W * 2 * 256
    return ({"metric": "ray-samples/sec (head + torso composite, 64+128 pts each, whole job)", "value": samples / dt,
                          "unit": "ray-samples/s", "n_gpus": world, "ranks": world, "backend": backend,
                          "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": prec, "data": "synthetic",
                          "frames_per_s": world * args.steps / dt,
                          "config": {"workload": f"BASELINE configs[4]: HeadNeRF+TorsoNeRF composite, {H}x{W}, frame-parallel",
                                     "nets": "head C=235 (aud 64, expr 76, latent 32) + torso C=169 (aud 64 + pose PE 42)"},
                          "roofline": {"bound": "mfma", "kernel": f"fused PE + FaceNeRF MLP forward, {prec} arithmetic (rank 0's launches)",
                                       "achieved": k_pts * FLOP_PER_SAMPLE / (k_ms * 1e-3) / 1e12 if k_ms > 0 else None,
                                       "peak": mode_peaks()[prec], "unit": "TFLOP/s",
                                       "frac": k_pts * FLOP_PER_SAMPLE / (k_ms * 1e-3) / 1e12 / mode_peaks()[prec] if k_ms > 0 else None,
                                       "traffic": None, "launches": k_n, "avg_launch_ms": k_ms / k_n if k_n else None,
                                       "flop_per_sample": FLOP_PER_SAMPLE, "kernel_time_share": (k_ms * 1e-3) / dt},
                          "finite": bool(torch.isfinite(frame).all()), "psnr_vs_fp32_frame_db": psnr})


def network_api_measurement(args, syn, coarse, fine, c_abi_value, c_abi_tile, frames=3, perturb=0.0):
    """The same frame through the drop-in surface a reference caller uses: ``Network.forward([data, global_step,
    dataset_size])`` in eval mode with the reference's default ``chunk = 8192`` (helper.py:54), audio net and
    conditioning fold included, against the number measured on ``ops.render_rays_fwd`` above."""
    from idealnerf_amd.audio_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    dev = c_abi_tile.device
    H, W = syn["H"], syn["W"]
    cfg = RenderConfig(perturb=perturb, chunk=8192, near=syn["near"], far=syn["far"])
    torch.manual_seed(0)
    net = Network(H, W, syn["focal"], syn["near"], syn["far"], 8192, None, 64, 128, args=cfg).to(dev).eval()
    net.face_nerf_coarse.load_state_dict(coarse.state_dict())
    net.face_nerf_fine.load_state_dict(fine.state_dict())
    net.face_nerf_coarse.precision, net.face_nerf_fine.precision = coarse.precision, fine.precision
    auds = torch.randn(8, 16, 29, device=dev)
    pose = torch.cat([syn["c2w"], torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
    data = (torch.zeros(1, 2, 1, 3), torch.zeros(1, 3), syn["bc"].to(dev)[None], auds[None], torch.zeros(1, H, W, 3), pose[None],
            syn["expr"].to(dev)[None], syn["latent"].to(dev), torch.tensor([3]))
    with torch.no_grad():
        net([data, 0, 8])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            rgb, disp, acc, last_w, extras = net([data, 0, 8])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / frames
        # same pixels as the C-ABI frame when the audio feature is the bench's: re-render with it for the check
        net_rgb = net.render_dynamic_face(H, W, syn["focal"], expr=syn["expr"].to(dev), poses=pose, latent_code=syn["latent"].to(dev),
                                          render_poses=pose[:3, :4], chunk=8192, near=syn["near"], far=syn["far"],
                                          bc_rgb=syn["bc"].to(dev), aud_para=syn["aud"].to(dev))[0]
    v = H * W * 256 / dt
    in_kernel = None
    if perturb > 0.:   # the same call with the draws made inside the kernels (idn_render_args.rng_mode; opt-in: net.in_kernel_draws)
        net.in_kernel_draws = True
        with torch.no_grad():
            net([data, 0, 8])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(frames):
                rgb_k = net([data, 0, 8])[0]
            torch.cuda.synchronize()
        dt_k = (time.perf_counter() - t0) / frames
        net.in_kernel_draws = False
        in_kernel = {"value": H * W * 256 / dt_k, "ms_per_frame": dt_k * 1e3, "ratio_to_c_abi": H * W * 256 / dt_k / c_abi_value,
                     "finite": bool(torch.isfinite(rgb_k).all()),
                     "psnr_vs_deterministic_frame_db": float(-10.0 * torch.log10(((rgb_k.reshape(-1, 3).double() - c_abi_tile.reshape(-1, 3).double()) ** 2).mean().clamp_min(1e-30))),
                     "note": "net.in_kernel_draws = True: stratified offsets and importance draws from Philox4x32-10 inside the coarse-depth "
                             "and march kernels (one seed per call from torch's CPU generator); no [n, S] / [n, Ni] random tensors"}
    if perturb > 0.:
        # the reference's DEFAULT eval mode (helper.py:70: --perturb 1.0): stratified depths and random u, drawn for the whole
        # frame at once (round 3 drew them chunk by chunk: 32 C calls, 64 folds and 64 torch.rand draws per frame)
        return {"value": v, "unit": "ray-samples/s", "ms_per_frame": dt * 1e3, "ratio_to_c_abi": v / c_abi_value, "perturb": perturb,
                "finite": bool(torch.isfinite(rgb).all()),
                "psnr_vs_deterministic_frame_db": float(-10.0 * torch.log10(((rgb.reshape(-1, 3).double() - c_abi_tile.reshape(-1, 3).double()) ** 2).mean().clamp_min(1e-30))),
                "call": "Network.forward([data, global_step, dataset_size]) in eval mode with the reference's default perturb = 1.0: "
                        "t_rand and u of the whole frame drawn at once (torch.rand on the device), one C call per frame",
                "in_kernel_draws": in_kernel}
    return {"value": v, "unit": "ray-samples/s", "ms_per_frame": dt * 1e3, "ratio_to_c_abi": v / c_abi_value,
            "identical_to_c_abi_frame": bool(torch.equal(net_rgb.reshape(-1, 3), c_abi_tile.reshape(-1, 3))),
            "call": "Network.forward([data, global_step, dataset_size]) in eval mode, chunk=8192, AudioNet + both folds per "
                    "frame; batchify_rays issues one C call per frame when perturb == 0"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the side measurements of a one-rank frame run: the other arithmetic "
                         "modes and kernel arrangements, Network.forward, the train step, the head+torso composite and the "
                         "CPU-oracle baseline (off by default: a plain run times only the headline)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="frame workload: write what the last timed step computed as DIR/<name>.npy (float32, <= 64 MB in all): "
                         "frame_rgb = the gathered [H, W, 3] frame, the others = render_rays_fwd's per-ray outputs of rank 0's band")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU-oracle baseline")
    ap.add_argument("--no-f32-mode", "--no-side-mode", dest="no_f32_mode", action="store_true",
                    help="with --full: skip the side measurements of the other modes, Network.forward, train and torso (profiling runs)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--soak", action="store_true",
                    help="compare every timed frame with the first one bit for bit (the path is deterministic: a mismatch is "
                         "a race); reported as `soak_mismatched_frames`")
    ap.add_argument("--precision", choices=["f32", "mixed", "mixed6", "fp16x3", "bf16x3", "bf16", "bf16x6"], default=os.environ.get("IDN_PRECISION", "f32"),
                    help="arithmetic of the MLP contraction.  f32 (default, the headline line): exact fp32 MFMA chains, "
                         "RGB within 1e-6..1e-5 of the reference.  bf16x3: three bf16 MFMAs per product, 3.4x faster, "
                         "within the 1e-4 RGB budget on the reference's golden frame and this scene, but sharp scenes "
                         "amplify its 1.5e-5 through the importance sampling (DESIGN.md section 3) -- measured beside "
                         "the headline as `bf16x3_mode`.  mixed: fp32 coarse network (it drives the sampling) + bf16x3 fine "
                         "network, ~2x the fp32 speed inside the 1e-4 budget, measured as `mixed_mode`.  bf16 (plain, ~1e-2): "
                         "BASELINE config 5's PSNR criterion only.  bf16x6: weights and activations as three bf16 pieces each, six "
                         "MFMAs per product: the fp32 kernel's parity on the bf16 pipe, measured as `bf16x6_mode`")
    ap.add_argument("--workload", choices=["frame", "train", "torso", "rendezvous"], default="frame",
                    help="frame = BASELINE configs[1] (default, the headline metric); train = configs[2] train step; "
                         "torso = configs[4] head+torso composite frames, plain bf16, frame-parallel")
    args = ap.parse_args()
    args.precision_given = any(a.startswith("--precision") for a in sys.argv[1:]) or "IDN_PRECISION" in os.environ
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and args.workload != "frame":
        ap.error("--dump-outputs is implemented for the frame workload")
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            # plain `python bench.py --gpus N`: this process only starts the ranks (no GPU call before here)
            sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}")
    if args.workload == "train":
        return bench_train(args)
    if args.workload == "torso":
        return bench_torso(args)
    if args.workload == "rendezvous":
        return bench_rendezvous(args)

    import torch.distributed as dist
    world, rank, dev, backend = init_ranks()

    import idealnerf_amd
    from idealnerf_amd import ops, parallel, synthetic
    from idealnerf_amd.helper import linspace01
    lib = idealnerf_amd._lib.load()

    H = W = args.size
    S, Ni = 64, 128
    syn = synthetic.frame(H, W, seed=0)
    coarse = synthetic.xavier_state_dict(idealnerf_amd.FaceNeRF(dim_aud=64, dim_latent=32, dim_expr=76), 2, 300.0, 0.3).to(dev)
    fine = synthetic.xavier_state_dict(idealnerf_amd.FaceNeRF(dim_aud=64, dim_latent=32, dim_expr=76), 3, 300.0, 0.3).to(dev)
    g = lambda t: t.to(dev)
    aud, expr, latent = g(syn["aud"]), g(syn["expr"]), g(syn["latent"])
    r0, r1 = parallel.row_band(H, rank, world)
    bc = syn["bc"][r0:r1].reshape(-1, 3).contiguous().to(dev)
    t_vals, u = linspace01(S, dev), linspace01(Ni, dev)
    def set_mode(mode):
        coarse.precision, fine.precision = {"mixed": ("f32", "bf16x3"), "mixed6": ("bf16x6", "bf16x3")}.get(mode, (mode, mode))
    set_mode(args.precision)
    pk_c, pk_f = coarse.packed_weights(), fine.packed_weights()
    prec, prec_f = coarse.prec_code, fine.prec_code

    fused_headline = ops.FUSED_MARCH_DEFAULT if (args.precision == "f32" and S == 64 and Ni == 128) else 0   # what fused=None resolves to below (0 / 1 / 2)
    collective = dist_on()   # world > 1, or the one-rank RCCL communicator of IDN_DIST_INIT_WORLD1=1 (the collective then runs at world size 1)
    marks = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]

    def step(i=None):
        # per frame: pose -> rays, conditioning -> biases, then the per-ray path, then the tile exchange
        if i is not None:
            marks[i][0].record()
        # (frame mode: the rays of this rank's row band are derived on the device inside the render call, pass by pass)
        frame = ops.make_frame(syn["c2w"], H, W, syn["focal"], syn["near"], syn["far"], r0, r1 - r0)
        fc = coarse.folded_bias(aud, expr, latent)
        ff = fine.folded_bias(aud, expr, latent)
        out = ops.render_rays_fwd(None, bc, pk_c, fc, pk_f, ff, t_vals, u, Ni, precision=prec, precision_fine=prec_f, frame=frame)
        tile = out["rgb_map"].reshape(r1 - r0, W, 3)
        if i is not None:
            marks[i][1].record()
        frame = parallel.gather_rows(tile, H, force=collective)
        if i is not None:
            marks[i][2].record()   # the collective is ordered into this stream: the event fires when the gathered frame is usable
        return frame, tile, out

    def fence():
        if collective:
            dist.barrier()
        torch.cuda.synchronize()

    if collective:   # communicator set-up and the first all-gather of this size are not part of any step (--warmup 0 is legal)
        parallel.gather_rows(torch.zeros((r1 - r0, W, 3), device=dev), H, force=True)
    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        fence()
        lib.idealnerf_profile_begin()
        first, mismatched = None, torch.zeros((), dtype=torch.int64, device=dev)
        t0 = time.perf_counter()
        for i_step in range(args.steps):
            frame, tile, out = step(i_step)
            if args.soak:
                if first is None:
                    first = tile.clone()
                else:
                    mismatched += (tile != first).any().to(torch.int64)
        fence()
        dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:   # what the last timed step computed, after the clock stopped
        dump_outputs(args.dump_outputs, {"frame_rgb": frame, **out})
    import ctypes as C
    k_ms, k_n, k_pts = C.c_double(), C.c_int64(), C.c_int64()
    lib.idealnerf_profile_end(C.byref(k_ms), C.byref(k_n), C.byref(k_pts))

    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    # what each rank's GPU did with a step, by HIP events on the launch stream: render (rays + folds + the per-ray path) and
    # the tile all-gather (which includes waiting for the slowest rank's tile); mean over the timed steps, gathered to rank 0
    mine = torch.tensor([sum(m[0].elapsed_time(m[1]) for m in marks) / args.steps, sum(m[1].elapsed_time(m[2]) for m in marks) / args.steps,
                         k_ms.value / args.steps], dtype=torch.float64, device=dev)
    per_rank = [mine]
    if world > 1:
        per_rank = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(per_rank, mine)
    per_rank = [[float(v) for v in t.tolist()] for t in per_rank]

    if rank == 0:
        traffic, traffic_source = pmc_traffic(args.precision, fused=fused_headline)
        if not (H == 512 and world == 1):
            traffic, traffic_source = None, {"file": None, "reason": "PMC summaries exist for the 512x512 single-GPU run only"}
        samples = H * W * (S + S + Ni) * args.steps
        value = samples / dt
        ach = (k_pts.value * FLOP_PER_SAMPLE) / (k_ms.value * 1e-3) / 1e12 if k_ms.value > 0 else None
        peaks = mode_peaks()
        peak = peaks[args.precision]
        kname = {"f32": KNAME[fused_headline],
                 "bf16x3": "idn::mlp_bf16x3_kernel<kModeRays> (fused PE + FaceNeRF MLP, 3 bf16 MFMAs per product)",
                 "bf16": "idn::mlp_bf16_kernel<kModeRays> (fused PE + FaceNeRF MLP, plain bf16 MFMA)",
                 "fp16x3": "idn::mlp_fp16x3_kernel<kModeRays> (fused PE + FaceNeRF MLP, 3 fp16 MFMAs per product)",
                 "mixed": "idn::mlp_f32_kernel (coarse network) + idn::mlp_bf16x3_kernel (fine network); blended peak",
                 "mixed6": "idn::x6::mlp_bf16x6_kernel (coarse network) + idn::mlp_bf16x3_kernel (fine network); blended peak",
                 "bf16x6": "idn::x6::mlp_bf16x6_kernel<kModeRays> (fused PE + FaceNeRF MLP, 6 bf16 piece products per fp32 product)"}[args.precision]
        res = {
            "metric": "ray-samples/sec (64+128 pts, 512x512), whole job", "value": value, "unit": "ray-samples/s",
            "n_gpus": world, "ranks": world, "backend": backend,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": {"f32": "f32", "bf16x3": "bf16x3 (fp32 in/out, fp32 accumulate)", "bf16": "bf16 (fp32 in/out, fp32 accumulate; PSNR-only parity)", "mixed": "f32 coarse network + bf16x3 fine network", "mixed6": "bf16x6 (fp32-grade) coarse network + bf16x3 fine network", "fp16x3": "fp16x3 (fp32 in/out, fp32 accumulate)", "bf16x6": "bf16x6 (operands as three bf16 pieces = 24 significand bits, fp32 accumulate: fp32-grade)"}[args.precision], "data": "synthetic",
            "per_gpu": value / world, "rays_per_s": value / (S + S + Ni),
            "per_rank": {"render_ms": [r[0] for r in per_rank], "all_gather_ms": [r[1] for r in per_rank], "mlp_kernel_ms": [r[2] for r in per_rank],
                         "step_ms_min": min(r[0] + r[1] for r in per_rank), "step_ms_max": max(r[0] + r[1] for r in per_rank),
                         "note": "HIP events on each rank's launch stream, mean per timed step: render = rays + conditioning folds + the per-ray path; "
                                 "all_gather = the RCCL tile exchange as this rank sees it (includes waiting for the slowest band)"},
            **({"soak_mismatched_frames": int(mismatched.item())} if args.soak else {}),
            "config": {"workload": f"BASELINE configs[1]: May HeadNeRF {H}x{W} full-frame render, N_sample=64 "
                                   "N_importance=128, dim_aud=64 dim_expr=76 latent=32, perturb=0",
                       "rays_per_step": H * W, "samples_per_ray": S + S + Ni,
                       "partition": f"{world} row band(s) + {backend} all_gather of rgb tiles" if world > 1 else "single GPU",
                       "band_rows": [b - a for a, b in parallel.all_bands(H, world)]},
            "roofline": {"bound": "mfma", "kernel": kname,
                         "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                         "frac": (ach / peak) if ach else None, "traffic": traffic, "traffic_source": traffic_source,
                         "launches": k_n.value, "avg_launch_ms": (k_ms.value / k_n.value) if k_n.value else None,
                         "flop_per_sample": FLOP_PER_SAMPLE, "samples_per_launch": (k_pts.value / k_n.value) if k_n.value else None,
                         "kernel_time_share": (k_ms.value * 1e-3) / dt if dt > 0 else None,
                         "note": "peak = dense MFMA peak at 2.4 GHz (guide).  Under sustained load the chip holds "
                                 "1.8-2.0 GHz; an LDS-fed bf16 MFMA loop on random data tops out at 1.3-1.5 PFLOP/s of "
                                 "issued MFMAs (tools/mfma_shape_ubench.hip, DESIGN.md section 3)"},
        }
        if world == 1 and args.full and not args.no_f32_mode:
            # the other arithmetic modes of the same kernel family on the same box and scene, measured after the
            # timed region (2 frames each): mixed and bf16x3 beside the fp32 headline, fp32 beside anything else
            notes = {"f32": "IDN_PREC_F32: v_mfma_f32_32x32x2_f32, exact fp32 fma chains",
                     "bf16x3": "IDN_PREC_BF16X3: 3 x v_mfma_f32_32x32x16_bf16 per product, fp32 accumulate; priced against bf16 peak / 3",
                     "mixed": "coarse network (drives the importance sampling) in exact fp32, fine network (3/4 of the samples) in "
                              "bf16x3; priced against the blended peak of the two kernels"}
            notes["fp16x3"] = ("IDN_PREC_FP16X3: 3 x v_mfma_f32_32x32x16_f16 per product (11+11 significand bits per operand), "
                               "fp32 accumulate; priced against the fp16 (= bf16) peak / 3")
            notes["bf16x6"] = ("IDN_PREC_BF16X6: weights and activations as the exact sum of three bf16 pieces, 6 x v_mfma_f32_32x32x16_bf16 per "
                               "product, fp32 accumulate: fp32-grade (<= 2^-23 per product), fp32's range; priced against bf16 peak / 6")
            notes["mixed6"] = ("coarse network (drives the importance sampling) in bf16x6 -- fp32-grade on the bf16 pipe --, fine network in "
                               "bf16x3; priced against the blended peak of the two kernels")
            # (fp16x3 / bf16x3 are narrower than the reference's arithmetic: `--precision fp16x3|bf16x3` measures them, the default line no longer does)
            for other in (["bf16x6", "mixed6", "mixed"] if args.precision == "f32" else ["f32"]):
                set_mode(other)
                pko_c, pko_f = coarse.packed_weights(), fine.packed_weights()
                code_c, code_f = coarse.prec_code, fine.prec_code
                def step_other():
                    frame = ops.make_frame(syn["c2w"], H, W, syn["focal"], syn["near"], syn["far"], r0, r1 - r0)
                    return ops.render_rays_fwd(None, bc, pko_c, coarse.folded_bias(aud, expr, latent), pko_f,
                                               fine.folded_bias(aud, expr, latent), t_vals, u, Ni, precision=code_c, precision_fine=code_f, frame=frame)
                with torch.no_grad():
                    step_other()
                    torch.cuda.synchronize()
                    lib.idealnerf_profile_begin()
                    t1 = time.perf_counter()
                    for _ in range(2):
                        o_out = step_other()
                    torch.cuda.synchronize()
                    d_o = time.perf_counter() - t1
                lib.idealnerf_profile_end(C.byref(k_ms), C.byref(k_n), C.byref(k_pts))
                a_o = (k_pts.value * FLOP_PER_SAMPLE) / (k_ms.value * 1e-3) / 1e12
                diff = (o_out["rgb_map"].reshape(-1, 3).double() - tile.reshape(-1, 3).double())
                res[other + "_mode"] = {
                    "value": H * W * (S + S + Ni) * 2 / d_o, "unit": "ray-samples/s", "ms_per_step": d_o / 2 * 1e3,
                    "roofline": {"bound": "mfma", "achieved": a_o, "peak": peaks[other], "unit": "TFLOP/s", "frac": a_o / peaks[other]},
                    "rgb_vs_headline_frame": {"max_abs": float(diff.abs().max()),
                                              "psnr_db": float(-10.0 * torch.log10((diff ** 2).mean().clamp_min(1e-30)))},
                    "note": notes[other]}
            set_mode(args.precision)
            if args.precision == "f32" and S == 64 and Ni == 128:
                # the OTHER arrangements of the same arithmetic on the same frame, after the timed region (same pixels, bit for bit):
                # 0 the kernel sequence; 1 north_star's fused ray-march kernel (csrc/render_fused.hip: both networks, the march and
                # the final compositing as ONE launch, a ray's depths / raw outputs / weights / cdf in LDS); 2 the same kernel as two
                # launches (coarse network + march | fine network + compositing), only the fine depths crossing HBM
                for arr in (0, 1, 2):
                    if arr == fused_headline:
                        continue
                    def step_alt():
                        frame = ops.make_frame(syn["c2w"], H, W, syn["focal"], syn["near"], syn["far"], r0, r1 - r0)
                        return ops.render_rays_fwd(None, bc, pk_c, coarse.folded_bias(aud, expr, latent), pk_f, fine.folded_bias(aud, expr, latent),
                                                   t_vals, u, Ni, precision=prec, precision_fine=prec_f, fused=arr, frame=frame)
                    with torch.no_grad():
                        step_alt()
                        torch.cuda.synchronize()
                        lib.idealnerf_profile_begin()
                        t1 = time.perf_counter()
                        for _ in range(2):
                            q_out = step_alt()
                        torch.cuda.synchronize()
                        d_q = time.perf_counter() - t1
                    lib.idealnerf_profile_end(C.byref(k_ms), C.byref(k_n), C.byref(k_pts))
                    a_q = (k_pts.value * FLOP_PER_SAMPLE) / (k_ms.value * 1e-3) / 1e12
                    res[ARRANGEMENT_BLOCK[arr]] = {
                        "value": H * W * (S + S + Ni) * 2 / d_q, "unit": "ray-samples/s", "ms_per_step": d_q / 2 * 1e3,
                        "ratio_to_headline": (H * W * (S + S + Ni) * 2 / d_q) / value,
                        "identical_to_headline_frame": bool(torch.equal(q_out["rgb_map"].reshape(-1, 3), tile.reshape(-1, 3))),
                        "roofline": {"bound": "mfma", "kernel": KNAME[arr],
                                     "achieved": a_q, "peak": peaks["f32"], "unit": "TFLOP/s", "frac": a_q / peaks["f32"],
                                     "launches": k_n.value, "avg_launch_ms": (k_ms.value / k_n.value) if k_n.value else None,
                                     "traffic": pmc_traffic("f32", fused=arr)[0]},
                        "note": ARRANGEMENT_NOTE}
        if world == 1 and args.full and not args.no_f32_mode:
            res["network_api"] = network_api_measurement(args, syn, coarse, fine, value, tile)
            res["network_api_perturb1"] = network_api_measurement(args, syn, coarse, fine, value, tile, frames=2, perturb=1.0)
            # BASELINE configs[2] and configs[4] beside the headline, each with its own roofline block, after the timed region
            t_side = time.perf_counter()
            tr = train_measurement(dev, steps=8, warmup=4)
            res["train_step"] = {k: tr[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "dtype", "config", "roofline", "final_loss")}
            to = torso_measurement(dev, H, "bf16", steps=3, warmup=1)
            res["torso_composite"] = {k: to[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "dtype", "frames_per_s", "config",
                                                         "roofline", "finite", "psnr_vs_fp32_frame_db")}
            res["side_blocks_s"] = time.perf_counter() - t_side
        if world == 1 and args.full and not args.no_cpu_baseline:
            pc = {k: v.detach().cpu() for k, v in coarse.state_dict().items()}
            pf = {k: v.detach().cpu() for k, v in fine.state_dict().items()}
            res["cpu_baseline"], psnr = cpu_baseline(syn, pc, pf, tile, r0)
            res["psnr_vs_cpu_oracle_db"] = psnr
        print(json.dumps(res))
    if dist_on():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
