"""Worker of tests/test_clip_cpu.py and tests/test_clip_gpu.py (not collected by pytest).

    python -m torch.distributed.run --nproc-per-node N tests/clip_worker.py assemble OUT.avi
        no GPU: N ranks over gloo push the frames `assembly_frame(j)` through parallel.ClipAssembler into a host sink.
    python [-m torch.distributed.run --nproc-per-node 2] tests/clip_worker.py torso OUT.avi PERTURB SEED DRAWS
        the head + torso scene of `torso_scene()` through clip.render_torso_clip, alone or as two ranks sharing GPU 0 over
        gloo (IDN_DIST_BACKEND=gloo IDN_FORCE_DEVICE=0: the one-GPU rehearsal of the RCCL path).

Every rank prints one JSON line {"rank": r, "result": <what the call returned>}.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ASM_FRAMES, ASM_H, ASM_W, ASM_BAD = 10, 6, 8, 5     # frame ASM_BAD is marked non-finite by the rank that owns it


def assembly_frame(j):
    """Frame j, every byte a function of j and of its position: order, loss and duplication all show."""
    return ((np.arange(ASM_H * ASM_W * 3, dtype=np.int64) * 7 + 31 * j + j * j) % 251).astype(np.uint8).reshape(ASM_H, ASM_W, 3)


class HostSink:
    """submit_u8 / release over RawAviWriter: what ClipAssembler needs of a sink, without FrameSink's GPU."""

    def __init__(self, path, width, height):
        from idealnerf_amd.frame_io import RawAviWriter
        self.writer, self.count, self.nonfinite_frames = RawAviWriter(path, width, height, fps=25.0), 0, []

    def submit_u8(self, u8, nonfinite=False):
        if nonfinite:
            self.nonfinite_frames.append(self.count)
        self.writer.write(u8.numpy() if torch.is_tensor(u8) else u8)
        self.count += 1

    def release(self):
        self.writer.release()


def assemble(path, rank, world):
    from idealnerf_amd.parallel import ClipAssembler, frames_of
    asm = ClipAssembler(HostSink(path, ASM_W, ASM_H) if rank == 0 else None, ASM_FRAMES, None)
    mine = list(frames_of(rank, world, ASM_FRAMES))
    for k in range(-(-ASM_FRAMES // world)):
        if k < len(mine):
            asm.push(torch.from_numpy(assembly_frame(mine[k])), mine[k] == ASM_BAD)
        else:
            asm.push(None)
    return asm.close()


HEAD_SIZE, HEAD_FRAMES, HEAD_SEED = 64, 6, 0


def head_dataset(d, seed=HEAD_SEED):
    """A HEAD_FRAMES-frame dataset directory in the reference's on-disk format (data_util/process_data.py:250-288), 64 x 64:
    seeded poses, expressions, DeepSpeech windows, a random background; returns the loader flags GetData needs."""
    import json
    from types import SimpleNamespace
    from PIL import Image
    from idealnerf_amd import synthetic
    rs = np.random.RandomState(seed)
    H = W = HEAD_SIZE
    for sub in ("head_imgs", "ori_imgs", "parsing"):
        os.makedirs(os.path.join(d, sub))
    frames = []
    for i in range(HEAD_FRAMES):
        Image.fromarray(rs.randint(0, 255, (H, W, 3), dtype=np.uint8)).save(os.path.join(d, "head_imgs", f"{i}.jpg"))
        par = np.zeros((H, W, 3), np.uint8)
        par[50:, 4:60] = (255, 0, 0)
        Image.fromarray(par).save(os.path.join(d, "parsing", f"{i}.png"))
        lms = rs.uniform(6, 58, (68, 2))
        lms[48:] = rs.uniform(28, 36, (20, 2))
        np.savetxt(os.path.join(d, "ori_imgs", f"{i}.lms"), lms)
        c2w = torch.cat([synthetic.frame(H, W, seed=seed + 20 + i)["c2w"], torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
        frames.append({"img_id": i, "aud_id": HEAD_FRAMES - 1 - i, "transform_matrix": c2w.double().tolist(),
                       "face_rect": [4, 4, 50, 50], "exp": rs.standard_normal(76).tolist()})
    Image.fromarray(rs.randint(0, 255, (H, W, 3), dtype=np.uint8)).save(os.path.join(d, "bc.jpg"))
    np.save(os.path.join(d, "aud.npy"), rs.standard_normal((HEAD_FRAMES, 16, 29)).astype(np.float32))
    meta = {"focal_len": 1200.0 * W / 450.0, "cx": W / 2, "cy": H / 2, "frames": frames}
    for mode in ("train", "val"):
        with open(os.path.join(d, f"transforms_exp_{mode}.json"), "w") as f:
            json.dump(meta, f)
    return SimpleNamespace(gt_dirs="head_imgs", testskip=1, N_rand=64, sample_rate=0.95, mouth_rays=8, torso_rays=4)


def head_network(dev, focal):
    """Head-only Network, xavier weights at the sharp-scene gain, 64 + 128 samples, perturb = 0."""
    from idealnerf_amd import synthetic
    from idealnerf_amd.audio_exp_nerf import Network
    from idealnerf_amd.helper import RenderConfig
    cfg = RenderConfig(perturb=0.0, chunk=8192, near=synthetic.NEAR, far=synthetic.FAR)
    torch.manual_seed(0)   # the audio nets
    net = Network(HEAD_SIZE, HEAD_SIZE, focal, synthetic.NEAR, synthetic.FAR, 8192, None, 64, 128, args=cfg)
    synthetic.xavier_state_dict(net.face_nerf_coarse, 2, 300.0, 0.3)
    synthetic.xavier_state_dict(net.face_nerf_fine, 3, 300.0, 0.3)
    return net.to(dev).eval()


def head_expected_inputs(d, net):
    """Per frame of the dataset at `d`, what the oracle needs: (c2w, expression, smoothed audio feature), and the decoded
    background -- read from the files, the audio feature by the audio modules' eager CPU path with the reference's window
    logic (audio_exp_nerf.py:246-262: eight frames around the index, zero-padded RAW windows at the clip's ends)."""
    import copy
    import json
    from PIL import Image
    meta = json.load(open(os.path.join(d, "transforms_exp_val.json")))
    table = np.load(os.path.join(d, "aud.npy"))
    auds = torch.from_numpy(np.stack([table[min(f["aud_id"], table.shape[0] - 1)] for f in meta["frames"]]))
    aud_net, att_net = copy.deepcopy(net.aud_net).cpu().eval(), copy.deepcopy(net.aud_att_net).cpu().eval()
    n, half, out = len(meta["frames"]), int(net.args.smo_size / 2), []
    for i, f in enumerate(meta["frames"]):
        left, right = max(i - half, 0), min(i + half, n)
        win = torch.cat([torch.zeros(half - i if i < half else 0, 16, 29), auds[left:right],
                         torch.zeros(max(i + half - n, 0), 16, 29)], 0)
        with torch.no_grad():
            aud = att_net(aud_net(win))
        c2w = torch.tensor(f["transform_matrix"], dtype=torch.float64)[:3, :4].to(torch.float32)
        out.append((c2w, torch.tensor(f["exp"], dtype=torch.float32), aud))
    bc = torch.tensor(np.asarray(Image.open(os.path.join(d, "bc.jpg"))) / 255.0).to(torch.float32)
    return out, bc, float(meta["focal_len"])


TORSO_SIZE, TORSO_CLIP, TORSO_FRAMES = 64, 8, 5    # an 8-entry track (the smoothing window), the first 5 frames rendered


def torso_scene(dev, size=TORSO_SIZE, n_clip=TORSO_CLIP, perturb=0.0, precision=None):
    """The sharp head + torso scene of bench.py's torso measurement (xavier seeds 2..5, density gains 300 / 4) with a
    pose and audio track of n_clip entries."""
    import idealnerf_amd
    from idealnerf_amd import synthetic
    from idealnerf_amd.helper import RenderConfig
    from idealnerf_amd.train_torso import Network
    syn = synthetic.frame(size, size, seed=0)
    cfg = RenderConfig(perturb=perturb, chunk=32768, near=syn["near"], far=syn["far"], dim_expr=76)
    torch.manual_seed(0)   # the audio nets
    net = Network(size, size, syn["focal"], syn["near"], syn["far"], 32768, 64, 128, args=cfg, dim_expr_head=76).to(dev).eval()
    for i, m in enumerate((net.face_nerf_coarse, net.face_nerf_fine, net.torso_coarse_nerf, net.torso_fine_nerf)):
        synthetic.xavier_state_dict(m, 2 + i, 300.0 if i < 2 else 4.0, 0.3 if i < 2 else -0.2)
    if precision is not None:
        idealnerf_amd.set_render_precision(net, precision)
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]])
    poses = torch.stack([torch.cat([synthetic.frame(size, size, seed=10 + j)["c2w"], bottom], 0) for j in range(n_clip)])
    auds = torch.from_numpy(np.random.RandomState(11).standard_normal((n_clip, 16, 29)).astype(np.float32))
    return dict(net=net, poses=poses, auds=auds, bc=syn["bc"], expr=syn["expr"], latent=syn["latent"],
                torso_pose=torch.cat([syn["c2w"], bottom], 0))


def torso(path, rank, perturb, seed, in_kernel_draws):
    from idealnerf_amd import clip
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    s = torso_scene(dev, perturb=perturb)
    s["net"].in_kernel_draws = in_kernel_draws
    return clip.render_torso_clip(s["net"], s["poses"], s["auds"], s["bc"], path if rank == 0 else None, expr=s["expr"],
                                  latent_code=s["latent"], torso_pose=s["torso_pose"], frames=range(TORSO_FRAMES), seed=seed,
                                  codec="raw")


def main():
    import torch.distributed as dist
    mode, path = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import datetime
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=int(os.environ.get("IDN_DIST_TIMEOUT_S", "120"))))
    try:
        if mode == "assemble":
            res = assemble(path, rank, world)
        else:
            perturb, seed, draws = float(sys.argv[3]), sys.argv[4], sys.argv[5] == "1"
            res = torso(path, rank, perturb, None if seed == "none" else int(seed), draws)
        if res is not None:
            res = {k: v for k, v in res.items() if k not in ("seconds", "frames_per_s")}
        # line and newline in ONE write: the ranks share a pipe, and on an unbuffered stdout print() writes the two apart
        sys.stdout.write(json.dumps({"rank": rank, "result": res}) + "\n")
        sys.stdout.flush()
    finally:
        if world > 1:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
