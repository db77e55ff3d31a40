"""Forward + backward of FaceNeRF.forward with gradients (autograd.FaceNeRFFn) at 2^16 and 2^19 rows, next to the same
loss in torch-eager fp32 on the GPU; and, from a `rocprofv3 --kernel-trace --stats` run of this script, the share of the
input-gradient kernel (dx_kernel) in the backward.  Report only: nothing here passes or fails.

    python tools/facenerf_train_timing.py [--sizes 65536 524288] [--iters 10] [--no-eager] [--out profiles/x.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/facenerf_train_timing.py --sizes 524288 --iters 3 --no-eager
    python tools/facenerf_train_timing.py --summarize DIR/.../run_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarize(path):
    rows = list(csv.DictReader(open(path)))
    tot = {}
    for r in rows:
        tot[r["Name"]] = tot.get(r["Name"], 0.0) + float(r["TotalDurationNs"])
    fwd = {k: v for k, v in tot.items() if "mlp_" in k}     # the activation-saving forward
    bwd = {k: v for k, v in tot.items() if k not in fwd}
    dx = sum(v for k, v in bwd.items() if "dx_kernel" in k)
    out = {"backward_ns": sum(bwd.values()), "forward_ns": sum(fwd.values()), "dx_kernel_ns": dx,
           "dx_share_of_backward": dx / max(sum(bwd.values()), 1.0),
           "kernels_ns": dict(sorted(tot.items(), key=lambda kv: -kv[1]))}
    print(json.dumps(out, indent=1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 19])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarize", default=None, help="kernel_stats.csv of a rocprofv3 run of this script")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
        return
    import torch
    import oracle
    import idealnerf_amd as idn
    from idealnerf_amd import autograd

    dev = torch.device("cuda:0")
    dims = oracle.facenerf_dims()
    params = oracle.xavier_facenerf_params(5, dims)
    net = idn.FaceNeRF(dim_aud=64, dim_latent=32, dim_expr=76)
    net.load_state_dict(params)
    net = net.to(dev)
    p_eager = {k: v.to(dev).requires_grad_(True) for k, v in params.items() if not k.startswith("feature_linear")}
    g = torch.Generator().manual_seed(0)
    cond = [(torch.randn(d, generator=g) * 0.3).to(dev).requires_grad_(True) for d in (64, 76, 32)]
    results = []

    def timed(step):
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            step()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.iters

    for n in a.sizes:
        x = (torch.rand(n, 90, generator=g) * 2 - 1).to(dev).requires_grad_(True)
        w = torch.randn(n, 4, generator=g).to(dev)

        def hip_step():
            net.zero_grad(set_to_none=True)
            (net(x, *cond) * w).sum().backward()

        def eager_step():
            for t in p_eager.values():
                t.grad = None
            (oracle.facenerf_forward(p_eager, x, *cond, dims=dims) * w).sum().backward()

        r = {"rows": n, "train_precision": autograd.TRAIN_PRECISION,
             "backward_pipe": os.environ.get("IDN_BACKWARD_PIPE", "bf16x6"), "hip_fwd_bwd_ms": timed(hip_step)}
        if not a.no_eager:
            r["torch_eager_fp32_fwd_bwd_ms"] = timed(eager_step)
            r["speedup"] = r["torch_eager_fp32_fwd_bwd_ms"] / r["hip_fwd_bwd_ms"]
        print(json.dumps(r), flush=True)
        results.append(r)
        del x, w
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
