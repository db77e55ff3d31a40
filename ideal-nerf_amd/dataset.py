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


def _box_masks(H, W, face_rect, landmark):
    """-> (coords [H W, 2] float32 (row, col), mouth box [H W], face rect [H W]); upstream's row/column convention is kept:
    pixel ROWS are compared against the landmark / rect *x* bounds (audio_exp_nerf.py:150-155, train_torso.py:145-149)."""
    mouth = landmark[48:]
    max_x, min_x = np.max(mouth[:, 0]) + 20, np.min(mouth[:, 0]) - 20
    max_y, min_y = np.max(mouth[:, 1]) + 20, np.min(mouth[:, 1]) - 20
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    coords = np.stack([rows, cols], -1).reshape(-1, 2)
    mouth_w = (coords[:, 0] >= min_x) & (coords[:, 0] <= max_x) & (coords[:, 1] >= min_y) & (coords[:, 1] <= max_y)
    rect_w = ((coords[:, 0] >= face_rect[0]) & (coords[:, 0] <= face_rect[0] + face_rect[2]) &
              (coords[:, 1] >= face_rect[1]) & (coords[:, 1] <= face_rect[1] + face_rect[3]))
    return coords, mouth_w, rect_w


def region_masks(H, W, face_rect, landmark, parse_img):
    """The pixel regions the sampler draws from (audio_exp_nerf.py:143-175) -> (coords [H W, 2] float32 (row, col), mouth [H W],
    rect [H W], torso [H, W]) as boolean masks.  Upstream's row/column convention is kept: pixel ROWS are compared against the
    landmark / rect *x* bounds (:150-155).  The one definition of the regions: `select_pixels` draws from these masks and
    `region_byte_map` packs them for the device-side sampler."""
    coords, mouth_w, rect_w = _box_masks(H, W, face_rect, landmark)
    torso = (parse_img[:, :, 0] == 255) & (parse_img[:, :, 1] == 0) & (parse_img[:, :, 2] == 0)
    return coords, mouth_w, rect_w, torso


def torso_region_masks(H, W, face_rect, landmark):
    """The torso stage's regions (train_torso.py:136-153) -> (coords, mouth box [H W], rect [H W], drawn [H W], M).  M is the
    mouth box's population; `drawn` marks the first M outside-rect pixels in row-major order -- the population upstream's mouth
    block REALLY draws from: it indexes `coords_norect` with indices drawn from the mouth box's population (:168-169).  (All of
    the outside pixels where M exceeds their number: there upstream raises IndexError.)  The one definition of the torso
    regions: `torso_select_pixels` draws from them, `torso_region_byte_map` packs them."""
    coords, mouth_w, rect_w = _box_masks(H, W, face_rect, landmark)
    M = int(mouth_w.sum())
    outside = ~rect_w
    drawn = outside & (np.cumsum(outside) <= M)
    return coords, mouth_w, rect_w, drawn, M


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


def torso_region_byte_map(H, W, face_rect, landmark):
    """uint8 [H, W] for the torso stage: bit 0 = face rect minus mouth box, bit 1 = outside the face rect, bit 2 = the first M
    outside-rect pixels in row-major order (`torso_region_masks`), bit 3 clear."""
    _, mouth_w, rect_w, drawn, _ = torso_region_masks(H, W, face_rect, landmark)
    return ((rect_w & ~mouth_w).astype(np.uint8) | ((~rect_w).astype(np.uint8) << 1) | (drawn.astype(np.uint8) << 2)).reshape(H, W)


def torso_mouth_num(n_rand, use_highlight):
    """train_torso.py:157: a quarter of the batch goes to the mouth block under `use_highlight`."""
    return n_rand // 4 if use_highlight else 0


def torso_select_pixels(H, W, face_rect, landmark, n_rand, use_highlight, sample_rate):
    """-> int64 [n_rand, 2] (row, col), train_torso.py:136-170: draws AND rows in the order rect, outside, mouth, from the global
    numpy RNG exactly like upstream -- the mouth block's indices are drawn from the mouth box's population and index
    `coords_norect` (an index past its end raises IndexError, as upstream)."""
    coords, mouth_w, rect_w, _, M = torso_region_masks(H, W, face_rect, landmark)
    c_rect, c_norect = coords[rect_w & ~mouth_w], coords[~rect_w]
    mouth_num = torso_mouth_num(n_rand, use_highlight)
    sample_num = n_rand - mouth_num
    rect_num = int(sample_num * sample_rate)
    norect_num = sample_num - rect_num
    s_rect = c_rect[np.random.choice(c_rect.shape[0], size=[rect_num], replace=False)]
    s_norect = c_norect[np.random.choice(c_norect.shape[0], size=[norect_num], replace=False)]
    s_mouth = c_norect[np.random.choice(M, size=[mouth_num], replace=False)]
    return np.concatenate([s_rect, s_norect, s_mouth], 0).astype(np.int64)


def baseline_select_pixels(H, W, face_rect, landmark, n_rand, sample_rate):
    """-> int64 [n_rand, 2] (row, col), head_baseline.py:124-160: ``int(n_rand * sample_rate)`` picks from the face rect minus
    the mouth box, the rest from outside the rect, rows in that order, from the global numpy RNG exactly like upstream --
    including its third draw (:158): ZERO picks over the mouth box's population.  It selects nothing, but a draw without
    replacement permutes its whole population whatever its size, so it advances the generator and decides every later batch."""
    coords, mouth_w, rect_w = _box_masks(H, W, face_rect, landmark)
    c_rect, c_norect = coords[rect_w & ~mouth_w], coords[~rect_w]
    rect_num = int(n_rand * sample_rate)
    norect_num = n_rand - rect_num
    s_rect = c_rect[np.random.choice(c_rect.shape[0], size=[rect_num], replace=False)]
    s_norect = c_norect[np.random.choice(c_norect.shape[0], size=[norect_num], replace=False)]
    np.random.choice(int(mouth_w.sum()), size=[0], replace=False)
    return np.concatenate([s_rect, s_norect], 0).astype(np.int64)


def baseline_region_byte_map(H, W, face_rect, landmark):
    """uint8 [H, W] for the baseline: bits 0 and 1 as ``torso_region_byte_map`` (face rect minus mouth box; outside the face
    rect) -- the two populations ``baseline_select_pixels`` picks from --, bit 2 the mouth box itself (nothing is drawn from it:
    it is there for the per-region scores), bit 3 clear (an AD-NeRF dataset has no parsing)."""
    _, mouth_w, rect_w = _box_masks(H, W, face_rect, landmark)
    return ((rect_w & ~mouth_w).astype(np.uint8) | ((~rect_w).astype(np.uint8) << 1) | (mouth_w.astype(np.uint8) << 2)).reshape(H, W)


def gather_selected(sel, poses, target, bc_img, H, W, focal, cx, cy, device):
    """Rays of the pixels `sel` (int64 [n, 2] (row, col), numpy) from each camera of `poses`, and their colours ->
    ([batch_rays [2, n, 3] per pose], target_s [n, 3], bc_rgb [n, 3]) on `device`: the device-side pinhole kernel on the whole
    frame, gathered there."""
    sel = torch.from_numpy(sel)
    flat = (sel[:, 0] * W + sel[:, 1]).to(device)
    rays = []
    for pose in poses:
        rec = ops.frame_rays(torch.as_tensor(pose, dtype=torch.float32), H, W, focal, 0.0, 1.0, cx=cx, cy=cy, device=device)
        rays.append(torch.stack([rec[flat, 0:3], rec[flat, 3:6]], 0))
    return rays, target.reshape(-1, 3)[flat], bc_img.reshape(-1, 3)[flat]


def sample_rays(pose, face_rect, target, bc_img, landmark, parse_img, H, W, focal, cx, cy, n_rand, mouth_rays,
                torso_rays, sample_rate, device):
    """audio_exp_nerf.py:134-195 -> (batch_rays [2, n, 3], target_s [n, 3], bc_rgb [n, 3]) on `device`."""
    sel = select_pixels(H, W, face_rect, landmark, parse_img, n_rand, mouth_rays, torso_rays, sample_rate)
    (batch_rays,), target_s, bc_rgb = gather_selected(sel, [pose], target, bc_img, H, W, focal, cx, cy, device)
    return batch_rays, target_s, bc_rgb


def torso_sample_rays(pose, pose_torso, face_rect, target, bc_img, landmark, H, W, focal, cx, cy, n_rand, use_highlight,
                      sample_rate, device):
    """train_torso.py:130-183 -> (batch_rays, batch_rays_torso [2, n, 3] each, target_s [n, 3], bc_rgb [n, 3]) on `device`;
    batch_rays_torso: the same pixels seen from `pose_torso` (the clip's frame-0 pose)."""
    sel = torso_select_pixels(H, W, face_rect, landmark, n_rand, use_highlight, sample_rate)
    (batch_rays, batch_rays_torso), target_s, bc_rgb = gather_selected(sel, [pose, pose_torso], target, bc_img, H, W, focal, cx,
                                                                        cy, device)
    return batch_rays, batch_rays_torso, target_s, bc_rgb


def baseline_sample_rays(pose, face_rect, target, bc_img, landmark, H, W, focal, cx, cy, n_rand, sample_rate, device):
    """head_baseline.py:124-168 -> (batch_rays [2, n, 3], target_s [n, 3], bc_rgb [n, 3]) on `device`."""
    sel = baseline_select_pixels(H, W, face_rect, landmark, n_rand, sample_rate)
    (batch_rays,), target_s, bc_rgb = gather_selected(sel, [pose], target, bc_img, H, W, focal, cx, cy, device)
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
            self.all_imgs.append(os.path.join(data_dir, self._image_dir(args), fid + ".jpg"))
            self.all_landmarks.append(os.path.join(data_dir, "ori_imgs", fid + ".lms"))
            self.all_parse_imgs.append(os.path.join(data_dir, "parsing", fid + ".png"))
            self.all_poses.append(np.array(frame["transform_matrix"]))
            auds.append(self.aud_features[min(frame["aud_id"], self.aud_features.shape[0] - 1)])
            self.all_face_rects.append(np.array(frame["face_rect"], dtype=np.int32))
            self.all_exprs.append(self._frame_expr(frame))
        self.data_size = len(self.all_imgs)
        self.auds = torch.tensor(np.asarray(auds), dtype=torch.float)

    def __len__(self):
        return self.data_size

    # ---- what the baseline's loader (BaselineGetData) replaces
    def _image_dir(self, args):
        return args.gt_dirs

    def _frame_expr(self, frame):
        return frame["exp"]

    def _read_image(self, index):
        return _imread(self.all_imgs[index])[..., ::-1].copy()  # upstream reads with cv2: BGR

    def _sample(self, index, target, pose):
        """-> (the frame's ray sets ..., target_s, bc_rgb) of one draw."""
        a = self.args
        parse = _imread(self.all_parse_imgs[index])
        landmark = np.loadtxt(self.all_landmarks[index])
        return sample_rays(pose, self.all_face_rects[index], target, self.background_img, landmark, parse, self.H, self.W,
                           self.focal, self.cx, self.cy, a.N_rand, a.mouth_rays, a.torso_rays, a.sample_rate, self.device)

    def __getitem__(self, index):
        if index is None:
            index = np.random.choice(self.data_size)
        raw_img = torch.tensor(self._read_image(index))
        self.H, self.W = raw_img.shape[0], raw_img.shape[1]
        target = raw_img.to(self.device).float() / 255.0
        pose = self.all_poses[index][:3, :4]
        *rays, target_s, bc_rgb = self._sample(index, target, pose)
        bc_rgb = bc_rgb if self.mode == "train" else self.background_img
        exp = torch.tensor(self.all_exprs[index], dtype=torch.float32)
        return (*rays, target_s, bc_rgb, self.auds, raw_img, pose, exp, index)


class TorsoGetData(GetData):
    """The torso stage's host-side loader (``GetData`` of NeRFs/TorsoNeRF/train_torso.py:46-183): ``__getitem__`` returns the
    9-tuple (batch_rays, batch_rays_torso, target_s, bc_rgb, auds, raw_img, pose, exp, index).  ``batch_rays_torso`` are the same
    pixels seen from the clip's frame-0 pose; the images are RGB (upstream reads them with imageio here); no parsing image is
    read; the pixel selection is ``torso_select_pixels``.  ``args`` needs gt_dirs, testskip, N_rand, sample_rate, use_highlight.
    As upstream (:82), a non-train clip's ``data_size`` is its frame count divided by ``testskip`` once more."""

    def __init__(self, data_dir, aud_file, mode, args, skip=1, device="cuda"):
        super().__init__(data_dir, aud_file, mode, args, skip=skip, device=device)
        if mode != "train":
            self.data_size = len(self.all_imgs) // args.testskip

    def _read_image(self, index):
        return _imread(self.all_imgs[index])

    def _sample(self, index, target, pose):
        a = self.args
        landmark = np.loadtxt(self.all_landmarks[index])
        return torso_sample_rays(pose, self.all_poses[0][:3, :4], self.all_face_rects[index], target, self.background_img, landmark,
                                 self.H, self.W, self.focal, self.cx, self.cy, a.N_rand, a.use_highlight, a.sample_rate, self.device)


class AggGetData(TorsoGetData):
    """The feature-aggregation trainer's host-side loader (``GetData`` of NeRFs/HeadNeRF/train/agg_aud_exp_nerf.py:43-172): the
    torso stage's pixel recipe (``torso_select_pixels``: ``N_rand // 4`` mouth picks under ``use_highlight``, draws and rows in
    the order rect, outside, mouth, the mouth block indexing ``coords_norect``), RGB images, no parsing read and
    ``data_size = len // testskip`` outside train mode -- on ONE camera: ``__getitem__`` returns the reference's 8-tuple
    (batch_rays, target_s, bc_rgb, auds, raw_img, pose, exp, index).  ``args`` as ``TorsoGetData``'s."""

    def _sample(self, index, target, pose):
        a = self.args
        landmark = np.loadtxt(self.all_landmarks[index])
        sel = torso_select_pixels(self.H, self.W, self.all_face_rects[index], landmark, a.N_rand, a.use_highlight, a.sample_rate)
        (batch_rays,), target_s, bc_rgb = gather_selected(sel, [pose], target, self.background_img, self.H, self.W, self.focal,
                                                          self.cx, self.cy, self.device)
        return batch_rays, target_s, bc_rgb


class BaselineGetData(GetData):
    """The AD-NeRF baseline's host-side loader (``GetData`` of NeRFs/HeadNeRF/train/head_baseline.py:47-168): the images come
    from ``head_imgs/`` whatever ``gt_dirs`` says and are RGB (upstream reads them with imageio), the landmarks from
    ``ori_imgs/<id>.lms``; neither ``exp`` nor ``parsing/`` is read -- an AD-NeRF dataset has neither --; the pixel selection is
    ``baseline_select_pixels`` (upstream's numpy draw sequence, its zero-size third draw included).  ``__getitem__`` returns the
    reference's 7-tuple (batch_rays, target_s, bc_rgb, auds, raw_img, pose, index); outside train mode ``bc_rgb`` is the whole
    background.  ``args`` needs testskip, N_rand, sample_rate."""

    def _image_dir(self, args):
        return "head_imgs"

    def _frame_expr(self, frame):
        return None

    def _read_image(self, index):
        return _imread(self.all_imgs[index])

    def _sample(self, index, target, pose):
        a = self.args
        landmark = np.loadtxt(self.all_landmarks[index])
        return baseline_sample_rays(pose, self.all_face_rects[index], target, self.background_img, landmark, self.H, self.W,
                                    self.focal, self.cx, self.cy, a.N_rand, a.sample_rate, self.device)

    def __getitem__(self, index):
        if index is None:
            index = np.random.choice(self.data_size)
        raw_img = torch.tensor(np.array(self._read_image(index)))
        self.H, self.W = raw_img.shape[0], raw_img.shape[1]
        target = raw_img.to(self.device).float() / 255.0
        pose = self.all_poses[index][:3, :4]
        batch_rays, target_s, bc_rgb = self._sample(index, target, pose)
        bc_rgb = bc_rgb if self.mode == "train" else self.background_img
        return batch_rays, target_s, bc_rgb, self.auds, raw_img, pose, index


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
    at which upstream's ``np.random.choice`` raises).

    ``patches=(k, p)`` (no counterpart upstream; None: nothing below exists and the draw, both launches and every byte are what
    they were): k contiguous p x p patches ride in every batch, for ``ssim_loss.ssim_patch_loss``.  The batch KEEPS its
    ``N_rand`` rows: the k p^2 patch rays come out of the rect region's share -- ``counts = (rect - k p^2, outside, mouth,
    torso)``, ValueError at construction if that goes negative -- so a step's network shapes do not change.  ``batch`` puts the
    sampler's rows first and the patches' pixel indices (``ops.patch_pixels``) in the tail of the same selection buffer, and
    ONE gather covers all rows: three launches, still no host synchronisation, no device-to-host copy, no allocation beyond the
    outputs.  ``patch_rows()`` is the tail as a slice; ``selection()`` stays the whole buffer.  The patches' top-left corners
    are ``ssim_loss.patch_origins(seed, index, draw, ...)``: computed on the HOST from a counter-based generator, a function
    of (seed, frame index, draw) alone, from the frames' ``face_rect`` kept on the host.  ``patch_region`` = "rect" (default):
    uniform over the origins for which the patch lies inside the face rect clipped to the frame (centred on the rect and
    clamped to the frame where the rect is narrower than p); "frame": uniform over the frame.  ``patch_origins_of(index,
    draw)`` returns them.  A patch pixel may also be one of the sampler's picks: the two draws are independent."""

    _takes_patches = True

    def __init__(self, data_dir, aud_file, mode, args, skip=1, device="cuda", max_bytes=8 << 30, seed=0, patches=None,
                 patch_region="rect"):
        self.data_dir, self.aud_file, self.mode, self.args, self.device, self.seed = data_dir, aud_file, mode, args, device, int(seed)
        self.patches = None
        if patches is not None:
            from .ssim_loss import PATCH_REGIONS, check_patches
            if not self._takes_patches:
                raise ValueError(f"{type(self).__name__} takes no patches: the torso stage has no SSIM term")
            self.patches = check_patches(patches)
            if patch_region not in PATCH_REGIONS:
                raise ValueError(f"patch_region must be one of {PATCH_REGIONS}, got {patch_region!r}")
        self.patch_region = patch_region
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
        self.counts = self._counts(args)
        if min(self.counts) < 0:
            raise ValueError(f"N_rand {args.N_rand} is smaller than mouth_rays + torso_rays")
        self._patch_rows = slice(sum(self.counts), sum(self.counts))
        if self.patches is not None:
            k, p = self.patches
            rect = self.counts[0]
            if k * p * p > rect:
                raise ValueError(f"patches = ({k}, {p}) take {k} * {p}^2 = {k * p * p} rays out of the rect region's share of the "
                                 f"batch, which is {rect} of N_rand = {args.N_rand}: fewer or smaller patches, or a larger N_rand")
            if p > self.H or p > self.W:
                raise ValueError(f"a patch of {p} x {p} does not fit a {self.H} x {self.W} frame")
            self._patch_rows = slice(sum(self.counts) - k * p * p, sum(self.counts))
            self.counts = (rect - k * p * p, *self.counts[1:])
        self.face_rects = [np.array(f["face_rect"], dtype=np.int32) for f in frames]   # on the host: the patch origins need them
        from ._lib import SAMPLE_MAX_REGION
        if max(self.counts) > SAMPLE_MAX_REGION:
            raise ValueError(f"the split {dict(zip(REGION_NAMES, self.counts))} asks a region for more than the sampler's "
                             f"{SAMPLE_MAX_REGION} picks")
        aud_features = np.load(os.path.join(data_dir, aud_file))
        img_paths, maps, poses, exprs, auds = [], [], [], [], []
        self.populations = np.zeros((n, 4), np.int64)
        for i, frame in enumerate(frames):
            fid = str(frame["img_id"])
            img_paths.append(os.path.join(data_dir, self._image_dir(args), fid + ".jpg"))
            m = self._region_map(fid, np.array(frame["face_rect"], dtype=np.int32))
            self.populations[i] = [int(((m >> g) & 1).sum()) for g in range(4)]
            for g in range(4):
                if self.populations[i, g] < self.counts[g]:
                    raise ValueError(f"frame {fid} (index {i}): region '{REGION_NAMES[g]}' holds {self.populations[i, g]} pixels, "
                                     f"fewer than the {self.counts[g]} the batch draws from it without replacement")
            maps.append(m)
            poses.append(np.array(frame["transform_matrix"])[:3, :4])
            auds.append(aud_features[min(frame["aud_id"], aud_features.shape[0] - 1)])
            exprs.append(self._frame_expr(frame))
        self.all_poses = poses                                   # float64 [3, 4] each, as GetData keeps them
        self._cams = [ops.camera_floats(p) for p in poses]       # the same matrices as the 12 floats the kernels take
        # ---- upload
        self.maps = torch.empty((n, self.H, self.W), dtype=torch.uint8, device=device)
        self.imgs = torch.empty((n, self.H, self.W, 3), dtype=torch.uint8, device=device)
        for i in range(n):
            self.maps[i].copy_(torch.from_numpy(maps[i]))
            raw = self._read_image(img_paths[i])
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
        self.exprs = None if exprs and exprs[0] is None else torch.tensor(np.asarray(exprs), dtype=torch.float32).to(device)
        self._sel = torch.empty(self._patch_rows.stop, dtype=torch.int64, device=device)
        # (without patches the views below are the buffer itself and an empty tail)
        self._sel_sampled, self._sel_patches = self._sel[:self._patch_rows.start], self._sel[self._patch_rows]
        self._ws = torch.zeros(4, dtype=torch.int32, device=device)
        if torch.device(device).type == "cuda":
            ops.byte_tables(device)                              # built here, so that batch() allocates nothing but its outputs

    # ---- what the other stages' loaders (ResidentTorsoFrames, ResidentBaselineFrames) replace
    _image_dir, _frame_expr = GetData._image_dir, GetData._frame_expr

    def _counts(self, args):
        """(rect, outside, mouth, torso) picks of one batch."""
        return ops.sample_counts(args.N_rand, args.mouth_rays, args.torso_rays, args.sample_rate)

    def _region_map(self, fid, face_rect):
        """The region byte map of frame `fid` (raises ValueError for a frame the sampler cannot serve)."""
        parse = _imread(os.path.join(self.data_dir, "parsing", fid + ".png"))
        if parse.shape[:2] != (self.H, self.W):
            raise ValueError(f"frame {fid}: parsing image is {parse.shape[:2]}, the clip's cx / cy say {(self.H, self.W)}")
        landmark = np.loadtxt(os.path.join(self.data_dir, "ori_imgs", fid + ".lms"))
        return region_byte_map(self.H, self.W, face_rect, landmark, parse)

    def _read_image(self, path):
        return _imread(path)[..., ::-1].copy()                   # upstream reads with cv2: BGR

    def _gather(self, index, sel):
        """-> the sampled tensors of a batch, in the tuple's order."""
        return ops.gather_rays(sel, self._cams[index], self.H, self.W, self.focal, self.imgs[index], self.background, self.cx, self.cy)

    _no_sets = 2   # empty fields at the head of frame()'s tuple: batch_rays, target_s

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
        return (*(self._no_rays,) * self._no_sets, self.background_unit, self.auds, self.imgs[index], self._poses_host[index],
                self.exprs[index], index)

    def select(self, index, draw):
        """The flat pixel indices of draw `draw` on frame `index` (int64 [N_rand]; the loader's own buffer, overwritten by
        the next call in stream order)."""
        if self.patches is None:
            return ops.sample_pixels(self.maps[index], self.counts, self.seed, draw, out=self._sel, workspace=self._ws)
        ops.sample_pixels(self.maps[index], self.counts, self.seed, draw, out=self._sel_sampled, workspace=self._ws)
        ops.patch_pixels(self.patch_origins_of(index, draw), self.patches[1], self.W, out=self._sel_patches)
        return self._sel

    def patch_origins_of(self, index, draw):
        """[(oy, ox)] * k: the top-left corners of the patches of draw `draw` on frame `index` (host numbers, no device read)."""
        from .ssim_loss import patch_origins
        k, p = self.patches
        return patch_origins(self.seed, int(index), draw, k, p, self.H, self.W, self.face_rects[int(index)], self.patch_region)

    def patch_rows(self):
        """The rows of a batch (and of ``selection()``) that hold the patches, k p^2 of them, patch by patch and row-major inside
        a patch: the tail of the batch.  An empty slice at its end without ``patches``."""
        return self._patch_rows

    def selection(self):
        """The flat pixel indices of the latest ``select`` / ``batch`` (int64 [N_rand], row-major over H x W): row i of that
        batch's rays, targets and background rows belongs to pixel ``selection()[i]``.  The loader's own buffer, as ``select``
        returns it: the next draw overwrites it in stream order."""
        return self._sel

    def batch(self, index, draw):
        """-> (batch_rays [2, n, 3], target_s [n, 3], bc_rgb [n, 3], auds, raw_img, pose, expr, index), every tensor on the device."""
        index = int(index)
        return (*self._gather(index, self.select(index, draw)), self.auds, self.imgs[index], self.poses[index], self.exprs[index],
                index)


class ResidentTorsoFrames(ResidentFrames):
    """``ResidentFrames`` for the torso stage: the resident counterpart of ``TorsoGetData``.  Same constructor arguments
    (``args`` needs gt_dirs, N_rand, sample_rate, use_highlight); what differs from the head stage's loader:

    - the byte map is ``torso_region_byte_map`` (no parsing image is read): bit 0 rect minus mouth box, bit 1 outside the rect,
      bit 2 the first M outside-rect pixels in row-major order (M = the mouth box's population: what upstream's mouth block
      really draws from), bit 3 clear; counts ``ops.sample_counts(N_rand, N_rand // 4 if use_highlight else 0, 0, sample_rate)``.
      The sampler is the head stage's, unchanged: regions may overlap, and are drawn independently, as upstream's;
    - the images are RGB;
    - ``batch`` returns the 9-tuple (batch_rays, batch_rays_torso, target_s, bc_rgb, auds, raw_img, pose, expr, index), both ray
      sets from one launch (``ops.gather_ray_pairs``; the second camera is the clip's frame-0 pose); ``frame`` the eval 9-tuple.

    Beside ``ResidentFrames``' construction errors, ``ValueError`` where ``use_highlight`` is set and a frame's M exceeds its
    outside population -- the frames on which upstream's mouth block can raise IndexError.  ``patches`` is not for this stage
    (its step has no SSIM term): anything but None raises ValueError."""

    _no_sets = 3
    _takes_patches = False

    def _counts(self, args):
        return ops.sample_counts(args.N_rand, torso_mouth_num(args.N_rand, args.use_highlight), 0, args.sample_rate)

    def _region_map(self, fid, face_rect):
        landmark = np.loadtxt(os.path.join(self.data_dir, "ori_imgs", fid + ".lms"))
        *_, M = torso_region_masks(self.H, self.W, face_rect, landmark)
        m = torso_region_byte_map(self.H, self.W, face_rect, landmark)
        outside = int(((m >> 1) & 1).sum())
        if self.args.use_highlight and M > outside:
            raise ValueError(f"frame {fid}: the mouth box holds {M} pixels, more than the {outside} outside the face rect that "
                             "the mouth block indexes with them (train_torso.py:168-169 raises IndexError there)")
        return m

    def _read_image(self, path):
        return np.array(_imread(path))

    def _gather(self, index, sel):
        return ops.gather_ray_pairs(sel, self._cams[index], self._cams[0], self.H, self.W, self.focal, self.imgs[index],
                                    self.background, self.cx, self.cy)


class ResidentAggFrames(ResidentTorsoFrames):
    """``ResidentFrames`` for the feature-aggregation trainer: the resident counterpart of ``AggGetData``.  The torso stage's
    byte map, counts, construction errors and RGB images (``ResidentTorsoFrames``) with the head stage's single camera:
    ``batch`` returns the 8-tuple (batch_rays, target_s, bc_rgb, auds, raw_img, pose, expr, index) from ``ops.gather_rays``,
    ``frame`` the eval 8-tuple (``mode="val"``).  ``patches`` / ``patch_region``: as ``ResidentFrames``."""

    _no_sets = 2
    _takes_patches = True
    _gather = ResidentFrames._gather


class ResidentBaselineFrames(ResidentFrames):
    """``ResidentFrames`` for the AD-NeRF baseline: the resident counterpart of ``BaselineGetData``.  Same constructor arguments
    (``args`` needs N_rand, sample_rate); what differs from the head stage's loader:

    - the byte map is ``baseline_region_byte_map`` (no parsing image is read); counts ``ops.sample_counts(N_rand, 0, 0,
      sample_rate)``: nothing is drawn from the mouth box, so a box of any size -- empty, or the whole rect -- leaves
      construction alone (a rect it swallows still fails it, as upstream's first draw does).  The sampler and the gather are the
      head stage's, unchanged;
    - the images are RGB and come from ``head_imgs/``; no ``exp`` is read;
    - ``batch`` returns the 7-tuple (batch_rays, target_s, bc_rgb, auds, raw_img, pose, index), ``frame`` the eval 7-tuple."""

    _image_dir, _frame_expr = BaselineGetData._image_dir, BaselineGetData._frame_expr

    def _counts(self, args):
        return ops.sample_counts(args.N_rand, 0, 0, args.sample_rate)

    def _region_map(self, fid, face_rect):
        landmark = np.loadtxt(os.path.join(self.data_dir, "ori_imgs", fid + ".lms"))
        return baseline_region_byte_map(self.H, self.W, face_rect, landmark)

    def _read_image(self, path):
        return np.array(_imread(path))

    def frame(self, index):
        index = int(index)
        return (self._no_rays, self._no_rays, self.background_unit, self.auds, self.imgs[index], self._poses_host[index], index)

    def batch(self, index, draw):
        index = int(index)
        return (*self._gather(index, self.select(index, draw)), self.auds, self.imgs[index], self.poses[index], index)


# ---- test-time loaders: a trained model on a track that is not its training clip -----------------------------------------

def load_test_data(datadir, aud_file, test_pose_file, testskip=1, test_size=-1, aud_start=0):
    """The torso test's track (``load_test_data``, NeRFs/TorsoNeRF/load_audface.py:87-114) -> (poses [F, 4, 4] float32,
    auds [F, 16, 29] float32, bc_img uint8 [H, W, 3], [H, W, focal, cx, cy], aud_ids, torso_pose [4, 4] float64).

    ``test_pose_file`` and ``aud_file`` are opened as given (not joined to ``datadir``, which only supplies ``bc.jpg`` and with
    it H and W); focal, cx, cy are the pose file's.  Frame i of ``frames[::testskip]`` takes audio row
    ``min(aud_start + i, n_aud - 1)`` and ``aud_ids[i] = aud_start + i`` (the row is clamped, the id is not).  The track ends
    after the frame that makes its length ``test_size`` or ``n_aud`` -- tested after the frame is taken, so ``test_size <= 0``
    never ends it.  ``torso_pose`` is frame 0 of the unskipped pose file."""
    with open(test_pose_file) as fp:
        meta = json.load(fp)
    aud_features = np.load(aud_file)
    n_aud = aud_features.shape[0]
    poses, auds, aud_ids = [], [], []
    for frame in meta["frames"][::testskip]:
        i = len(poses)
        poses.append(np.array(frame["transform_matrix"]))
        auds.append(aud_features[min(aud_start + i, n_aud - 1)])
        aud_ids.append(aud_start + i)
        if len(poses) == test_size or len(poses) == n_aud:
            break
    bc_img = np.array(_imread(os.path.join(datadir, "bc.jpg")))
    hwfcxy = [bc_img.shape[0], bc_img.shape[1], float(meta["focal_len"]), float(meta["cx"]), float(meta["cy"])]
    torso_pose = np.array(meta["frames"][0]["transform_matrix"])
    return np.array(poses).astype(np.float32), np.array(auds).astype(np.float32), bc_img, hwfcxy, aud_ids, torso_pose


def load_test_exprs(path, testskip, n):
    """-> float32 [n, E]: the ``exp`` vectors of ``frames[::testskip][:n]`` of a ``transforms_exp_*.json``-style file.
    ValueError if the file holds fewer than ``n``."""
    with open(path) as fp:
        frames = json.load(fp)["frames"][::testskip]
    if len(frames) < n:
        raise ValueError(f"{path} holds {len(frames)} expression vectors at testskip {testskip}, the track needs {n}")
    return np.asarray([f["exp"] for f in frames[:n]], dtype=np.float32).reshape(n, -1)


class DrivingFrames(torch.utils.data.Dataset):
    """The eval script's loader (``GetData``, NeRFs/HeadNeRF/test/eval_aud_exp_nerf.py:46-124): an identity driven by another
    performance.  Poses and cx, cy come from ``<data_dir>/transforms_exp_{mode}.json`` (``frames[::skip]``; H, W =
    int(2 cy), int(2 cx)), the audio rows are 0 .. n-1 from the START of the audio file (not the frames' ``aud_id``;
    ``aud_file`` as given if it exists, else under ``data_dir``), and the expressions (``frames[::skip]``, as many as there are
    identity frames) and the focal length (``focal_len``) come from ``args.evalExpr_path``.

    ``__getitem__(j)`` is the 8-tuple ``Network.forward`` reads in eval mode, in ``GetData``'s field positions: (empty
    batch_rays, empty target_s, the background in [0, 1], the whole audio track, a zero uint8 image of the frame's shape -- only
    its shape is read --, the pose [3, 4], expression j, j).  No image, landmark or parsing file is opened: the identity's
    ``head_imgs/`` need not exist.  ``clip.render_head_clip`` takes it as it takes ``GetData``.

    Where upstream fails at the first missing frame, this raises ``ValueError`` at construction: fewer expressions than
    frames, fewer audio rows than frames, ``evalExpr_path`` unset, a ``bc.jpg`` of another shape than (H, W)."""

    def __init__(self, data_dir, aud_file, mode, args, skip=1, device="cuda"):
        self.data_dir, self.aud_file, self.mode, self.args, self.device = data_dir, aud_file, mode, args, device
        expr_path = getattr(args, "evalExpr_path", None)
        if expr_path is None or expr_path == "None":
            raise ValueError("DrivingFrames needs args.evalExpr_path: the transforms_exp_*.json of the driving performance")
        with open(os.path.join(data_dir, f"transforms_exp_{mode}.json")) as fp:
            self.meta_identity = json.load(fp)
        with open(expr_path) as fp:
            self.meta_expr = json.load(fp)
        self.focal = float(self.meta_expr["focal_len"])
        self.cx, self.cy = float(self.meta_identity["cx"]), float(self.meta_identity["cy"])
        self.H, self.W = int(self.cy * 2), int(self.cx * 2)
        self.skip = skip
        self.all_poses = [np.array(f["transform_matrix"]) for f in self.meta_identity["frames"][::skip]]
        self.data_size = n = len(self.all_poses)
        exprs = [f["exp"] for f in self.meta_expr["frames"][::skip][:n]]
        if len(exprs) < n:
            raise ValueError(f"{expr_path} holds {len(exprs)} expression vectors at skip {skip}, the identity has {n} frames")
        self.all_exprs = exprs
        aud_path = aud_file if os.path.exists(aud_file) else os.path.join(data_dir, aud_file)
        self.aud_features = np.load(aud_path)
        if self.aud_features.shape[0] < n:
            raise ValueError(f"{aud_path} holds {self.aud_features.shape[0]} audio rows, the identity has {n} frames")
        background = np.array(_imread(os.path.join(data_dir, "bc.jpg")))
        if background.shape != (self.H, self.W, 3):
            raise ValueError(f"{os.path.join(data_dir, 'bc.jpg')} is {background.shape}, the identity's cx / cy say "
                             f"{(self.H, self.W, 3)}")
        self.background_img = torch.tensor(background / 255.0).to(device)
        self.auds = torch.tensor(np.asarray(self.aud_features[:n]), dtype=torch.float)
        self._exprs = torch.tensor(np.asarray(exprs), dtype=torch.float32)
        self._raw_img = torch.zeros((self.H, self.W, 3), dtype=torch.uint8)
        self._no_rays = torch.empty(0, dtype=torch.float32)

    def __len__(self):
        return self.data_size

    def __getitem__(self, index):
        index = int(index)
        return (self._no_rays, self._no_rays, self.background_img, self.auds, self._raw_img, self.all_poses[index][:3, :4],
                self._exprs[index], index)


class BaselineTestFrames(torch.utils.data.Dataset):
    """The baseline tester's loader (``GetData``, NeRFs/HeadNeRF/test/test_nerf.py:27-82): the poses and the intrinsics of
    ``<data_dir>/transforms_exp_{mode}.json`` (``frames[::skip]``; H, W = int(2 cy), int(2 cx)) with the audio rows taken BY
    POSITION -- frame i of the loader gets ``aud_features[i]``, whatever its ``aud_id`` says (:51-53).

    ``__getitem__(j)`` is the 7-tuple ``head_baseline.Network.forward`` reads in eval mode: (empty batch_rays, empty target_s,
    the background in [0, 1], the audio rows 0 .. n-1, a zero uint8 image of the frame's shape -- only its shape is read --,
    the pose [3, 4], j).  No image or landmark file is opened.  ``clip.render_head_clip(model="baseline")`` takes it.

    Where upstream fails at the first missing row, this raises ``ValueError`` at construction: fewer audio rows than frames, a
    ``bc.jpg`` of another shape than (H, W)."""

    def __init__(self, data_dir, aud_file, mode, args, skip=1, device="cuda"):
        self.data_dir, self.aud_file, self.mode, self.args, self.device = data_dir, aud_file, mode, args, device
        with open(os.path.join(data_dir, f"transforms_exp_{mode}.json")) as fp:
            self.meta = json.load(fp)
        self.focal, self.cx, self.cy = float(self.meta["focal_len"]), float(self.meta["cx"]), float(self.meta["cy"])
        self.H, self.W = int(self.cy * 2), int(self.cx * 2)
        self.skip = skip
        self.all_poses = [np.array(f["transform_matrix"]) for f in self.meta["frames"][::skip]]
        self.data_size = n = len(self.all_poses)
        self.aud_features = np.load(os.path.join(data_dir, aud_file))
        if self.aud_features.shape[0] < n:
            raise ValueError(f"{os.path.join(data_dir, aud_file)} holds {self.aud_features.shape[0]} audio rows, the clip has {n} "
                             "frames and takes them by position")
        background = np.array(_imread(os.path.join(data_dir, "bc.jpg")))
        if background.shape != (self.H, self.W, 3):
            raise ValueError(f"{os.path.join(data_dir, 'bc.jpg')} is {background.shape}, the clip's cx / cy say {(self.H, self.W, 3)}")
        self.background_img = torch.tensor(background / 255.0).to(device)
        self.auds = torch.tensor(np.asarray(self.aud_features[:n]), dtype=torch.float)
        self._raw_img = torch.zeros((self.H, self.W, 3), dtype=torch.uint8)
        self._no_rays = torch.empty(0, dtype=torch.float32)

    def __len__(self):
        return self.data_size

    def __getitem__(self, index):
        index = int(index)
        return (self._no_rays, self._no_rays, self.background_img, self.auds, self._raw_img, self.all_poses[index][:3, :4], index)
