"""Reader for the reference's on-disk dataset and its region-weighted ray sampler
(``GetData``, NeRFs/HeadNeRF/train/audio_exp_nerf.py:45-195; format written by
data_util/process_data.py:250-288):

    <dir>/transforms_exp_{train,val}.json   focal_len, cx, cy, frames[{img_id, aud_id,
                                            transform_matrix[4][4], face_rect[4], exp[...]}]
    <dir>/<aud_file>.npy  [F, 16, 29]       DeepSpeech windows
    <dir>/bc.jpg                            background
    <dir>/<gt_dirs>/<id>.jpg, ori_imgs/<id>.lms [68,2], parsing/<id>.png

``__getitem__`` returns the reference's 8-tuple.  Pixel selection reproduces upstream's numpy
RNG call sequence (mouth, torso, face rect, outside rect -- each ``np.random.choice`` without
replacement), including its row/column convention (pixel rows are compared against the
landmark / rect *x* bounds, :150-155); rays come from the device-side pinhole kernel with the
dataset's principal point and are gathered on the device.
"""
import json
import os

import numpy as np
import torch

from . import ops


def _imread(path):
    try:
        from PIL import Image
    except ImportError as e:  # pragma: no cover
        raise RuntimeError("reading dataset images needs Pillow") from e
    return np.asarray(Image.open(path))


def region_masks(H, W, face_rect, landmark, parse_img):
    """The pixel regions the sampler draws from (audio_exp_nerf.py:143-175) -> (coords [H W, 2] float32 (row, col), mouth [H W],
    rect [H W], torso [H, W]) as boolean masks.  Upstream's row/column convention is kept: pixel ROWS are compared against the
    landmark / rect *x* bounds (:150-155).  The one definition of the regions: `select_pixels` draws from these masks and
    `region_byte_map` packs them for the device-side sampler."""
    mouth = landmark[48:]
    max_x, min_x = np.max(mouth[:, 0]) + 20, np.min(mouth[:, 0]) - 20
    max_y, min_y = np.max(mouth[:, 1]) + 20, np.min(mouth[:, 1]) - 20
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    coords = np.stack([rows, cols], -1).reshape(-1, 2)
    mouth_w = (coords[:, 0] >= min_x) & (coords[:, 0] <= max_x) & (coords[:, 1] >= min_y) & (coords[:, 1] <= max_y)
    rect_w = ((coords[:, 0] >= face_rect[0]) & (coords[:, 0] <= face_rect[0] + face_rect[2]) &
              (coords[:, 1] >= face_rect[1]) & (coords[:, 1] <= face_rect[1] + face_rect[3]))
    torso = (parse_img[:, :, 0] == 255) & (parse_img[:, :, 1] == 0) & (parse_img[:, :, 2] == 0)
    return coords, mouth_w, rect_w, torso


REGION_NAMES = ("rect", "outside", "mouth", "torso")   # bit g of the byte map, row block g of a batch


def region_byte_map(H, W, face_rect, landmark, parse_img):
    """uint8 [H, W]: bit 0 = face rect minus mouth box, bit 1 = outside the face rect, bit 2 = mouth box, bit 3 = torso
    (parsing == (255, 0, 0)) -- the four populations `select_pixels` draws from, for ops.sample_pixels."""
    _, mouth_w, rect_w, torso = region_masks(H, W, face_rect, landmark, parse_img)
    m = ((rect_w & ~mouth_w).astype(np.uint8) | ((~rect_w).astype(np.uint8) << 1) | (mouth_w.astype(np.uint8) << 2)).reshape(H, W)
    return m | (torso.astype(np.uint8) << 3)


def select_pixels(H, W, face_rect, landmark, parse_img, n_rand, mouth_rays, torso_rays, sample_rate):
    """-> int64 [n_rand, 2] (row, col) in the reference's order: face rect, outside rect, mouth,
    torso (audio_exp_nerf.py:143-187).  Draws from the global numpy RNG exactly like upstream."""
    coords, mouth_w, rect_w, torso = region_masks(H, W, face_rect, landmark, parse_img)
    c_mouth, c_rect, c_norect = coords[mouth_w], coords[rect_w & ~mouth_w], coords[~rect_w]
    c_torso = coords.reshape(H, W, 2)[torso].reshape(-1, 2)
    sample_num = n_rand - mouth_rays - torso_rays
    rect_num = int(sample_num * sample_rate)
    norect_num = sample_num - rect_num
    pick = lambda c, k: c[np.random.choice(c.shape[0], size=[k], replace=False)].astype(np.int64)
    s_mouth = pick(c_mouth, mouth_rays)
    s_torso = pick(c_torso, torso_rays)
    s_rect = pick(c_rect, rect_num)
    s_norect = pick(c_norect, norect_num)
    return np.concatenate([s_rect, s_norect, s_mouth, s_torso], 0)


def sample_rays(pose, face_rect, target, bc_img, landmark, parse_img, H, W, focal, cx, cy, n_rand, mouth_rays,
                torso_rays, sample_rate, device):
    """audio_exp_nerf.py:134-195 -> (batch_rays [2, n, 3], target_s [n, 3], bc_rgb [n, 3]) on `device`."""
    sel = torch.from_numpy(select_pixels(H, W, face_rect, landmark, parse_img, n_rand, mouth_rays, torso_rays, sample_rate))
    flat = (sel[:, 0] * W + sel[:, 1]).to(device)
    rec = ops.frame_rays(torch.as_tensor(pose, dtype=torch.float32), H, W, focal, 0.0, 1.0, cx=cx, cy=cy, device=device)
    batch_rays = torch.stack([rec[flat, 0:3], rec[flat, 3:6]], 0)
    target_s = target.reshape(-1, 3)[flat]
    bc_rgb = bc_img.reshape(-1, 3)[flat]
    return batch_rays, target_s, bc_rgb


class GetData(torch.utils.data.Dataset):
    """mode in {train, val, test}; ``args`` needs gt_dirs, testskip, N_rand, sample_rate, mouth_rays, torso_rays."""

    def __init__(self, data_dir, aud_file, mode, args, skip=1, device="cuda"):
        self.data_dir, self.aud_file, self.mode, self.args, self.device = data_dir, aud_file, mode, args, device
        with open(os.path.join(data_dir, f"transforms_exp_{mode}.json")) as fp:
            self.meta = json.load(fp)
        self.aud_features = np.load(os.path.join(data_dir, aud_file))
        self.background_img = torch.tensor(_imread(os.path.join(data_dir, "bc.jpg")) / 255.0).to(device)
        self.focal, self.cx, self.cy = float(self.meta["focal_len"]), float(self.meta["cx"]), float(self.meta["cy"])
        self.H, self.W = int(self.cy * 2), int(self.cx * 2)
        self.skip = 1 if mode == "train" else args.testskip
        self.all_imgs, self.all_parse_imgs, self.all_landmarks = [], [], []
        self.all_poses, self.all_face_rects, self.all_exprs, auds = [], [], [], []
        for frame in self.meta["frames"][::skip]:
            fid = str(frame["img_id"])
            self.all_imgs.append(os.path.join(data_dir, args.gt_dirs, fid + ".jpg"))
            self.all_landmarks.append(os.path.join(data_dir, "ori_imgs", fid + ".lms"))
            self.all_parse_imgs.append(os.path.join(data_dir, "parsing", fid + ".png"))
            self.all_poses.append(np.array(frame["transform_matrix"]))
            auds.append(self.aud_features[min(frame["aud_id"], self.aud_features.shape[0] - 1)])
            self.all_face_rects.append(np.array(frame["face_rect"], dtype=np.int32))
            self.all_exprs.append(frame["exp"])
        self.data_size = len(self.all_imgs)
        self.auds = torch.tensor(np.asarray(auds), dtype=torch.float)

    def __len__(self):
        return self.data_size

    def __getitem__(self, index):
        if index is None:
            index = np.random.choice(self.data_size)
        raw = _imread(self.all_imgs[index])[..., ::-1].copy()  # upstream reads with cv2: BGR
        raw_img = torch.tensor(raw)
        self.H, self.W = raw_img.shape[0], raw_img.shape[1]
        target = raw_img.to(self.device).float() / 255.0
        parse = _imread(self.all_parse_imgs[index])
        pose = self.all_poses[index][:3, :4]
        landmark = np.loadtxt(self.all_landmarks[index])
        a = self.args
        batch_rays, target_s, bc_rgb = sample_rays(pose, self.all_face_rects[index], target, self.background_img,
                                                   landmark, parse, self.H, self.W, self.focal, self.cx, self.cy,
                                                   a.N_rand, a.mouth_rays, a.torso_rays, a.sample_rate, self.device)
        bc_rgb = bc_rgb if self.mode == "train" else self.background_img
        exp = torch.tensor(self.all_exprs[index], dtype=torch.float32)
        return batch_rays, target_s, bc_rgb, self.auds, raw_img, pose, exp, index


class ResidentFrames:
    """The training clip resident on the device, drawn from by the device-side sampler: the opt-in second data path beside
    ``GetData`` (which stays the reference's host-side loader, numpy draw sequence included).

    Same constructor arguments as ``GetData(mode="train")``.  The directory is read ONCE: per frame the ground-truth image
    (uint8 [H, W, 3], BGR as ``GetData.__getitem__`` produces it) and the region byte map (``region_byte_map``) go to the device
    -- 4 bytes per pixel and frame, 4.9 GB for 6 000 frames at 450 x 450 -- with the background (uint8), the clip's audio
    windows, the expressions and the poses; the poses also stay on the host (they travel as kernel arguments, like
    ``ops.frame_rays``'), as do the four region populations of every frame.

    ``batch(index, draw)`` returns the reference's 8-tuple for frame ``index`` with the pixels of draw number ``draw``
    (``ops.sample_pixels``: a function of (frame, seed, draw) alone): two kernel launches, no host synchronisation, no
    device-to-host copy, no allocation beyond the three output tensors; no [H W, 11] ray tensor exists.

    ``frame(index)`` is the validation side of the same object (``mode="val"``, ``skip=args.testskip``): the whole frame as the
    8-tuple the eval forward takes, for ``clip.score_head_clip`` and ``train.train(val="resident")``.

    Raises ``ValueError`` at construction -- from the host-side populations, before anything is uploaded -- if the clip needs
    more than ``max_bytes`` of device memory or if a region of a frame holds fewer pixels than its share of ``N_rand`` (the step
    at which upstream's ``np.random.choice`` raises)."""

    def __init__(self, data_dir, aud_file, mode, args, skip=1, device="cuda", max_bytes=8 << 30, seed=0):
        self.data_dir, self.aud_file, self.mode, self.args, self.device, self.seed = data_dir, aud_file, mode, args, device, int(seed)
        with open(os.path.join(data_dir, f"transforms_exp_{mode}.json")) as fp:
            self.meta = json.load(fp)
        frames = self.meta["frames"][::skip]
        self.focal, self.cx, self.cy = float(self.meta["focal_len"]), float(self.meta["cx"]), float(self.meta["cy"])
        self.H, self.W = int(self.cy * 2), int(self.cx * 2)
        self.data_size = n = len(frames)
        need = (n + 1) * self.H * self.W * 4
        if max_bytes is not None and need > max_bytes:
            raise ValueError(f"{n} frames of {self.H} x {self.W} need {need} bytes of device memory (4 per pixel and frame), more "
                             f"than max_bytes = {max_bytes}: raise max_bytes, take fewer frames (skip=), or use GetData")
        self.counts = ops.sample_counts(args.N_rand, args.mouth_rays, args.torso_rays, args.sample_rate)
        if min(self.counts) < 0:
            raise ValueError(f"N_rand {args.N_rand} is smaller than mouth_rays + torso_rays")
        from ._lib import SAMPLE_MAX_REGION
        if max(self.counts) > SAMPLE_MAX_REGION:
            raise ValueError(f"the split {dict(zip(REGION_NAMES, self.counts))} asks a region for more than the sampler's "
                             f"{SAMPLE_MAX_REGION} picks")
        aud_features = np.load(os.path.join(data_dir, aud_file))
        img_paths, maps, poses, exprs, auds = [], [], [], [], []
        self.populations = np.zeros((n, 4), np.int64)
        for i, frame in enumerate(frames):
            fid = str(frame["img_id"])
            img_paths.append(os.path.join(data_dir, args.gt_dirs, fid + ".jpg"))
            parse = _imread(os.path.join(data_dir, "parsing", fid + ".png"))
            if parse.shape[:2] != (self.H, self.W):
                raise ValueError(f"frame {fid}: parsing image is {parse.shape[:2]}, the clip's cx / cy say {(self.H, self.W)}")
            landmark = np.loadtxt(os.path.join(data_dir, "ori_imgs", fid + ".lms"))
            m = region_byte_map(self.H, self.W, np.array(frame["face_rect"], dtype=np.int32), landmark, parse)
            self.populations[i] = [int(((m >> g) & 1).sum()) for g in range(4)]
            for g in range(4):
                if self.populations[i, g] < self.counts[g]:
                    raise ValueError(f"frame {fid} (index {i}): region '{REGION_NAMES[g]}' holds {self.populations[i, g]} pixels, "
                                     f"fewer than the {self.counts[g]} the batch draws from it without replacement")
            maps.append(m)
            poses.append(np.array(frame["transform_matrix"])[:3, :4])
            auds.append(aud_features[min(frame["aud_id"], aud_features.shape[0] - 1)])
            exprs.append(frame["exp"])
        self.all_poses = poses                                   # float64 [3, 4] each, as GetData keeps them
        self._cams = [ops.camera_floats(p) for p in poses]       # the same matrices as the 12 floats the kernels take
        # ---- upload
        self.maps = torch.empty((n, self.H, self.W), dtype=torch.uint8, device=device)
        self.imgs = torch.empty((n, self.H, self.W, 3), dtype=torch.uint8, device=device)
        for i in range(n):
            self.maps[i].copy_(torch.from_numpy(maps[i]))
            raw = _imread(img_paths[i])[..., ::-1].copy()        # upstream reads with cv2: BGR
            if raw.shape != (self.H, self.W, 3):
                raise ValueError(f"{img_paths[i]} is {raw.shape}, the clip's cx / cy say {(self.H, self.W, 3)}")
            self.imgs[i].copy_(torch.from_numpy(raw))
        del maps
        background = np.array(_imread(os.path.join(data_dir, "bc.jpg")))
        self.background = torch.from_numpy(background).to(device)
        self.background_unit = torch.tensor(background / 255.0).to(device)   # float64, GetData's background_img: what frame() hands over
        self._poses_host = [torch.from_numpy(np.ascontiguousarray(p)) for p in poses]   # float64 [3, 4] each, on the host
        self._no_rays = torch.empty(0, dtype=torch.float32, device=device)
        self.auds = torch.tensor(np.asarray(auds), dtype=torch.float).to(device)
        self.poses = torch.tensor(np.asarray(poses), dtype=torch.float32).to(device)
        self.exprs = torch.tensor(np.asarray(exprs), dtype=torch.float32).to(device)
        self._sel = torch.empty(sum(self.counts), dtype=torch.int64, device=device)
        self._ws = torch.zeros(4, dtype=torch.int32, device=device)
        if torch.device(device).type == "cuda":
            ops.byte_tables(device)                              # built here, so that batch() allocates nothing but its outputs

    def __len__(self):
        return self.data_size

    def frame(self, index):
        """The resident validation loader: frame ``index`` as the 8-tuple ``Network.forward`` takes in eval mode -- (batch_rays,
        target_s, bg_img, auds, raw_img, pose, expr, index) with GetData(val)'s values in the fields the full-frame render reads:
        the whole background as GetData keeps it (float64 ``uint8 / 255.0``, uploaded once), the clip's audio windows, the
        ground-truth image (uint8, BGR), the expression and the index on the device, and the pose on the HOST (float64 [3, 4]:
        the camera travels as kernel arguments, so the forward must not have to fetch it from the device).  batch_rays and
        target_s, which the eval forward never reads, are empty.  No file is read, no host meshgrid is built, nothing is copied
        from the device, nothing is allocated."""
        index = int(index)
        return (self._no_rays, self._no_rays, self.background_unit, self.auds, self.imgs[index], self._poses_host[index],
                self.exprs[index], index)

    def select(self, index, draw):
        """The flat pixel indices of draw `draw` on frame `index` (int64 [N_rand]; the loader's own buffer, overwritten by
        the next call in stream order)."""
        return ops.sample_pixels(self.maps[index], self.counts, self.seed, draw, out=self._sel, workspace=self._ws)

    def batch(self, index, draw):
        """-> (batch_rays [2, n, 3], target_s [n, 3], bc_rgb [n, 3], auds, raw_img, pose, expr, index), every tensor on the device."""
        index = int(index)
        sel = self.select(index, draw)
        batch_rays, target_s, bc_rgb = ops.gather_rays(sel, self._cams[index], self.H, self.W, self.focal, self.imgs[index],
                                                       self.background, self.cx, self.cy)
        return batch_rays, target_s, bc_rgb, self.auds, self.imgs[index], self.poses[index], self.exprs[index], index
