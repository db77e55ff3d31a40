"""What tests/test_drive_cpu.py, tests/test_drive_gpu.py and tests/golden/make_golden_drive.py share (not collected by pytest):
the tiny dataset directory the driving loaders are tested on, rebuilt from a seed wherever it is needed, and the networks,
checkpoints and config files of the GPU tests.

The directory (``build_directory``): an identity of IDENTITY_FRAMES frames (``transforms_exp_val.json``), a driving
performance of DRIVING_FRAMES frames with ANOTHER focal length, other poses and other expressions
(``transforms_exp_drive.json``), a SHORT_AUDIO-row and a LONG_AUDIO-row DeepSpeech file and a SIZE x SIZE ``bc.jpg``.  There
is no ``head_imgs/``, ``ori_imgs/`` or ``parsing/``: the driving loaders open none of them.
"""
import json
import os

import numpy as np
import torch

SEED = 31
SIZE = 40                     # 1 600 rays: the last 128-point tile of a frame is ragged
IDENTITY_FRAMES, DRIVING_FRAMES = 9, 11
SHORT_AUDIO, LONG_AUDIO = 6, 12
DIM_EXPR = 76
IDENTITY_FILE, DRIVING_FILE = "transforms_exp_val.json", "transforms_exp_drive.json"
SHORT_FILE, LONG_FILE = "aud_short.npy", "aud_long.npy"
N_SAMPLES, N_IMPORTANCE = 16, 32


def _frames(rs, n, pose_seed):
    from idealnerf_amd import synthetic
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]])
    out = []
    for i in range(n):
        c2w = torch.cat([synthetic.frame(SIZE, SIZE, seed=pose_seed + i)["c2w"], bottom], 0)
        out.append({"img_id": i, "aud_id": n - 1 - i, "transform_matrix": c2w.double().tolist(), "face_rect": [3, 3, 30, 30],
                    "exp": rs.standard_normal(DIM_EXPR).tolist()})
    return out


def build_directory(d, seed=SEED):
    """Write the directory at `d` (created) -> dict of the paths in it."""
    from PIL import Image
    os.makedirs(d)
    rs = np.random.RandomState(seed)
    focal = 1200.0 * SIZE / 450.0
    identity = {"focal_len": focal, "cx": SIZE / 2, "cy": SIZE / 2, "frames": _frames(rs, IDENTITY_FRAMES, seed + 20)}
    driving = {"focal_len": focal * 1.25, "cx": SIZE / 2 + 1.0, "cy": SIZE / 2 - 1.0, "frames": _frames(rs, DRIVING_FRAMES, seed + 60)}
    paths = {"dir": d}
    for key, name, meta in (("identity", IDENTITY_FILE, identity), ("driving", DRIVING_FILE, driving)):
        paths[key] = os.path.join(d, name)
        with open(paths[key], "w") as f:
            json.dump(meta, f)
    for key, name, rows in (("short", SHORT_FILE, SHORT_AUDIO), ("long", LONG_FILE, LONG_AUDIO)):
        paths[key] = os.path.join(d, name)
        np.save(paths[key], rs.standard_normal((rows, 16, 29)).astype(np.float32))
    yy, xx = np.meshgrid(np.arange(SIZE), np.arange(SIZE), indexing="ij")
    bc = np.stack([40 + 4 * yy, 30 + 5 * xx, 220 - 2 * yy - 2 * xx], -1).astype(np.uint8)     # smooth: JPEG keeps its shape
    Image.fromarray(bc).save(os.path.join(d, "bc.jpg"), quality=95)
    paths["bc"] = os.path.join(d, "bc.jpg")
    return paths


def metas(paths):
    with open(paths["identity"]) as f:
        identity = json.load(f)
    with open(paths["driving"]) as f:
        driving = json.load(f)
    return identity, driving


# ---- the GPU tests' networks, checkpoints and config files ------------------------------------------------------------------

def render_config():
    from idealnerf_amd import synthetic
    from idealnerf_amd.helper import RenderConfig
    return RenderConfig(perturb=0.0, chunk=8192, near=synthetic.NEAR, far=synthetic.FAR, dim_aud=64, dim_expr=DIM_EXPR,
                        N_samples=N_SAMPLES, N_importance=N_IMPORTANCE)


def _latent_codes(seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((IDENTITY_FRAMES, 32)).astype(np.float32))


def head_network(dev, focal):
    """-> (head-only Network with Xavier weights at the sharp-scene gain, in eval mode on `dev`; random latent codes)."""
    from idealnerf_amd import synthetic
    from idealnerf_amd.audio_exp_nerf import Network, init_weights
    cfg = render_config()
    torch.manual_seed(5)
    net = Network(SIZE, SIZE, focal, cfg.near, cfg.far, cfg.chunk, None, N_SAMPLES, N_IMPORTANCE, args=cfg)
    net.apply(init_weights)
    synthetic.xavier_state_dict(net.face_nerf_coarse, 2, 300.0, 0.3)
    synthetic.xavier_state_dict(net.face_nerf_fine, 3, 300.0, 0.3)
    return net.to(dev).eval(), _latent_codes(7)


def torso_network(dev, focal):
    """-> (head + torso Network, Xavier weights with the density gains of the sharp head + torso scene; random latent codes)."""
    from idealnerf_amd import synthetic
    from idealnerf_amd.audio_exp_nerf import init_weights
    from idealnerf_amd.train_torso import Network
    cfg = render_config()
    torch.manual_seed(6)
    net = Network(SIZE, SIZE, focal, cfg.near, cfg.far, cfg.chunk, N_SAMPLES, N_IMPORTANCE, args=cfg, dim_aud_body=64,
                  dim_expr_head=DIM_EXPR)
    net.apply(init_weights)
    for i, m in enumerate((net.face_nerf_coarse, net.face_nerf_fine, net.torso_coarse_nerf, net.torso_fine_nerf)):
        synthetic.xavier_state_dict(m, 12 + i, 300.0 if i < 2 else 4.0, 0.3 if i < 2 else -0.2)
    return net.to(dev).eval(), _latent_codes(8)


def config_text(paths, run_root, save_path, flow):
    """The `key = value` config file of a flow: datadir, the run directory `run_root`/run, the driving files, the tests' sample
    counts, perturb 0."""
    from idealnerf_amd import synthetic
    lines = [f"expname = run", f"basedir = {run_root}", f"datadir = {paths['dir']}", f"save_path = {save_path}",
             f"evalExpr_path = {paths['driving']}", "testskip = 1", f"N_samples = {N_SAMPLES}", f"N_importance = {N_IMPORTANCE}",
             "perturb = 0", "chunk = 8192", f"near = {synthetic.NEAR!r}", f"far = {synthetic.FAR!r}", "dim_aud = 64"]
    if flow == "head":
        lines += [f"aud_file = {LONG_FILE}", f"dim_expr = {DIM_EXPR}"]
    else:
        lines += [f"aud_file = {paths['long']}", f"test_pose_file = {paths['identity']}", "test_size = 9", "aud_start = 2",
                  "dim_aud_body = 64"]
    return "\n".join(lines) + "\n"


def flags(paths, run_root, save_path, flow):
    """The flags namespace of `config_text` (without making it the process's flags) and the config file's path."""
    from idealnerf_amd import config
    os.makedirs(run_root, exist_ok=True)
    path = os.path.join(run_root, f"{flow}_{os.path.basename(save_path)}.txt")
    with open(path, "w") as f:
        f.write(config_text(paths, run_root, save_path, flow))
    return config.load_config(path, kind=flow), path


def decode_raw(path, H=SIZE, W=SIZE):
    """The frames of a raw AVI as written (uint8 [H, W, 3] each; bottom-up rows padded to 4 bytes in the file)."""
    from idealnerf_amd.frame_io import read_avi_chunks
    info, chunks = read_avi_chunks(path)
    row = (W * 3 + 3) & ~3
    return info, [np.frombuffer(c, dtype=np.uint8).reshape(H, row)[::-1, :W * 3].reshape(H, W, 3).copy() for c in chunks]
