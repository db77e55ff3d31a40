"""Seeded synthetic workload of the shape BASELINE.json names:
there is no dataset or checkpoint to load, so benchmarks and smoke tests render a
512x512 frame from a seeded pose with May near/far (configs/audio_expr_nerf/may/
paper_model/torso_bg.txt), uniform background, Gaussian audio/expression latents, the
trainer's ones latent code (audio_exp_nerf.py:482) and Xavier-uniform weights with bias
0.01 (audio_exp_nerf.py:442-448).  Pure numpy/torch data generation; no rendering here.
"""
import math

import numpy as np
import torch

NEAR, FAR = 0.5772005200386048, 1.1772005200386046


def frame(H=512, W=512, seed=0, dim_aud=64, dim_expr=76, dim_latent=32):
    rs = np.random.RandomState(seed)
    ang = rs.uniform(-0.08, 0.08, size=3)
    c, s = np.cos(ang), np.sin(ang)
    Rx = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
    Ry = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
    Rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
    c2w = np.concatenate([Rz @ Ry @ Rx, np.array([[0.0], [0.0], [0.877]])], axis=1).astype(np.float32)
    bc = np.random.RandomState(seed + 1).uniform(0, 1, size=(H, W, 3)).astype(np.float32)
    rs2 = np.random.RandomState(seed + 100)
    t = lambda a: None if a is None else torch.from_numpy(a)
    aud = rs2.standard_normal(dim_aud).astype(np.float32) if dim_aud else None
    expr = rs2.standard_normal(dim_expr).astype(np.float32) if dim_expr else None
    latent = np.ones(dim_latent, dtype=np.float32) if dim_latent else None
    return dict(H=H, W=W, focal=1200.0 * W / 450.0, c2w=torch.from_numpy(c2w), near=NEAR, far=FAR,
                bc=torch.from_numpy(bc), aud=t(aud), expr=t(expr), latent=t(latent))


def xavier_state_dict(module, seed, sigma_gain=None, sigma_bias=None):
    """Fill a FaceNeRF's parameters from numpy RandomState(seed) in state_dict order
    (Xavier-uniform weights, bias 0.01).  ``sigma_gain`` scales the density head so the
    volume is not empty (Xavier-initialised sigma is ~0 everywhere)."""
    rs = np.random.RandomState(seed)
    sd = {}
    for k, v in module.state_dict().items():
        if k.endswith(".weight"):
            bound = math.sqrt(6.0 / (v.shape[0] + v.shape[1]))
            sd[k] = torch.from_numpy(rs.uniform(-bound, bound, size=tuple(v.shape)).astype(np.float32))
        else:
            sd[k] = torch.full(tuple(v.shape), 0.01, dtype=torch.float32)
    if sigma_gain is not None:
        sd["alpha_linear.weight"] = sd["alpha_linear.weight"] * sigma_gain
    if sigma_bias is not None:
        sd["alpha_linear.bias"] = torch.full_like(sd["alpha_linear.bias"], sigma_bias)
    module.load_state_dict(sd)
    return module


def box_density_state_dict(module, seed, centre=(0.0, 0.0, 0.0), half=0.08, slope=200.0, aud_gain=0.0):
    """Fill a FaceNeRF with an ANALYTIC density: an axis-aligned box with empty space around it (Xavier sigma is positive in
    about half the volume; nothing can be culled there).  The first three input channels of the point encoding are the
    coordinates themselves, so with half_eff = half + aud_gain * aud[0]:
      pts_linears.0      six live units relu(+-slope (x_i - c_i) - slope half_eff), i = 0..2 (coordinate weights on columns
                         0..2, the audio weight on the first conditioning column); every other row and bias zero
      pts_linears.1..7   carry those six channels through unchanged (pts_linears.5 takes [input | h]: column c_all + j)
      alpha_linear       1 - the sum of the six
    so sigma_raw = 1 inside |x_i - c_i| <= half_eff, falls with slope times the L1 excess outside, and is <= 0 from 1 / slope
    outward.  The colour branch (views_linears.*, rgb_linear) keeps the seeded Xavier weights of `xavier_state_dict`."""
    xavier_state_dict(module, seed)
    sd = {k: v.clone() for k, v in module.state_dict().items()}
    if aud_gain and not module.dim_aud:
        raise ValueError("aud_gain needs a network with audio conditioning columns (dim_aud > 0)")
    c_in, c_all = module.input_xyz_ch, module.pts_linears[0].in_features
    for i in range(8):
        sd[f"pts_linears.{i}.weight"].zero_()
        sd[f"pts_linears.{i}.bias"].zero_()
    for i in range(3):
        for j, sign in ((2 * i, 1.0), (2 * i + 1, -1.0)):
            sd["pts_linears.0.weight"][j, i] = sign * slope
            sd["pts_linears.0.bias"][j] = -sign * slope * centre[i] - slope * half
            if module.dim_aud:
                sd["pts_linears.0.weight"][j, c_in] = -slope * aud_gain
    for i in range(1, 8):
        for j in range(6):
            sd[f"pts_linears.{i}.weight"][j, (c_all if i == 5 else 0) + j] = 1.0
    sd["alpha_linear.weight"].zero_()
    sd["alpha_linear.weight"][0, :6] = -1.0
    sd["alpha_linear.bias"].fill_(1.0)
    module.load_state_dict(sd)
    return module


def write_clip_directory(d, size, n_frames, seed=0, flat=False, N_rand=64, mouth_rays=8, torso_rays=4, sample_rate=0.95,
                         dim_expr=76, face_rect=None, mouth_range=None):
    """An n_frames-frame directory in the reference's on-disk format (data_util/process_data.py:250-288), size x size: seeded
    poses, expressions, DeepSpeech windows and landmarks; face rect, mouth landmarks and torso rows at fixed fractions of the
    frame.  flat: every frame is one colour inside the face rect over the (other) background colour, instead of noise.
    dim_expr: the length of the frames' `exp` vectors (the torso network's head pair takes 79); face_rect: [x, y, w, h] instead
    of the fixed fraction; mouth_range: (lo, hi) the mouth landmarks are drawn from, on both axes, instead of the fixed fraction.
    For tests and for tools/train_head.py's and tools/train_torso.py's timing runs.  -> (loader flags as a namespace, the
    transforms metadata)."""
    import json
    import os
    from types import SimpleNamespace
    from PIL import Image
    rs = np.random.RandomState(seed)
    H = W = size
    k = size / 64.0
    for sub in ("head_imgs", "ori_imgs", "parsing"):
        os.makedirs(os.path.join(d, sub))
    rect = [int(4 * k), int(4 * k), int(50 * k), int(50 * k)] if face_rect is None else [int(v) for v in face_rect]
    mouth_lo, mouth_hi = (28 * k, 36 * k) if mouth_range is None else mouth_range
    face, back = np.array([40, 90, 200], np.uint8), np.array([200, 160, 30], np.uint8)
    bc = np.broadcast_to(back, (H, W, 3)).copy() if flat else rs.randint(0, 255, (H, W, 3), dtype=np.uint8)
    frames = []
    for i in range(n_frames):
        if flat:
            img = bc.copy()
            img[rect[0]:rect[0] + rect[2] + 1, rect[1]:rect[1] + rect[3] + 1] = face   # rows against the rect's x bounds, as the loader
        else:
            img = rs.randint(0, 255, (H, W, 3), dtype=np.uint8)
        Image.fromarray(img).save(os.path.join(d, "head_imgs", f"{i}.jpg"), quality=95)
        par = np.zeros((H, W, 3), np.uint8)
        par[int(50 * k):, int(4 * k):int(60 * k)] = (255, 0, 0)
        Image.fromarray(par).save(os.path.join(d, "parsing", f"{i}.png"))
        lms = rs.uniform(6 * k, 58 * k, (68, 2))
        lms[48:] = rs.uniform(mouth_lo, mouth_hi, (20, 2))
        np.savetxt(os.path.join(d, "ori_imgs", f"{i}.lms"), lms)
        c2w = torch.cat([frame(H, W, seed=seed + 20 + (0 if flat else i))["c2w"], torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
        frames.append({"img_id": i, "aud_id": n_frames - 1 - i, "transform_matrix": c2w.double().tolist(),
                       "face_rect": rect, "exp": rs.standard_normal(dim_expr).tolist()})
    Image.fromarray(bc).save(os.path.join(d, "bc.jpg"), quality=95)
    np.save(os.path.join(d, "aud.npy"), rs.standard_normal((n_frames, 16, 29)).astype(np.float32))
    meta = {"focal_len": 1200.0 * W / 450.0, "cx": W / 2, "cy": H / 2, "frames": frames}
    for mode in ("train", "val"):
        with open(os.path.join(d, f"transforms_exp_{mode}.json"), "w") as f:
            json.dump(meta, f)
    return SimpleNamespace(gt_dirs="head_imgs", testskip=1, N_rand=N_rand, sample_rate=sample_rate, mouth_rays=mouth_rays,
                           torso_rays=torso_rays), meta


def perturb_train_poses(d, degrees, length, seed=0):
    """Seeded noise on the TRAINING cameras of a generated directory (tools/train_head.py --pose_noise): each frame's c2w becomes
    [R(w) R | t + e] with w uniform on the sphere of radius ``degrees`` (as an angle) and e on the sphere of radius ``length``.
    The clean file is kept beside it as transforms_exp_train_clean.json: the ground truth a pose-refinement run is scored
    against.  Validation poses stay clean.  -> (noisy c2w [n, 4, 4], clean c2w [n, 4, 4])."""
    import json
    import os
    from .pose_refine import rotation
    path = os.path.join(d, "transforms_exp_train.json")
    with open(path) as f:
        meta = json.load(f)
    with open(os.path.join(d, "transforms_exp_train_clean.json"), "w") as f:
        json.dump(meta, f)
    rs = np.random.RandomState(seed + 4242)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    n = len(meta["frames"])
    w = torch.from_numpy(unit(rs.standard_normal((n, 3))) * math.radians(degrees))
    e = torch.from_numpy(unit(rs.standard_normal((n, 3))) * length)
    clean = torch.tensor([fr["transform_matrix"] for fr in meta["frames"]], dtype=torch.float64)
    noisy = clean.clone()
    noisy[:, :3, :3] = rotation(w) @ clean[:, :3, :3]
    noisy[:, :3, 3] = clean[:, :3, 3] + e
    for fr, m in zip(meta["frames"], noisy):
        fr["transform_matrix"] = m.tolist()
    with open(path, "w") as f:
        json.dump(meta, f)
    return noisy, clean
