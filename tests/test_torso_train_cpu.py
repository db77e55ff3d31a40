"""Host side of the torso stage's training loop (no GPU): ``TorsoGetData``'s pixel selection against the reference's own
``sample_rays`` (tests/golden/torso_sample_rays.npz), the torso byte map against a numpy restatement, ``ResidentTorsoFrames``'
refusals and ``latest_checkpoint(contains=)``."""
import os

import numpy as np
import pytest

from idealnerf_amd.synthetic import write_clip_directory


def _restated_map(H, W, rect, lms):
    """The torso byte map written out once more, pixel loops instead of masks: bit 0 rect minus mouth box, bit 1 outside the
    rect, bit 2 the first M outside pixels in row-major order (M = the mouth box's population)."""
    mouth = lms[48:]
    lo_r, hi_r = mouth[:, 0].min() - 20, mouth[:, 0].max() + 20      # pixel ROWS against the landmarks' x, as upstream
    lo_c, hi_c = mouth[:, 1].min() - 20, mouth[:, 1].max() + 20
    m = np.zeros((H, W), np.uint8)
    box = np.zeros((H, W), bool)
    for r in range(H):
        for c in range(W):
            box[r, c] = lo_r <= r <= hi_r and lo_c <= c <= hi_c
            in_rect = rect[0] <= r <= rect[0] + rect[2] and rect[1] <= c <= rect[1] + rect[3]
            m[r, c] = (1 if in_rect and not box[r, c] else 0) | (0 if in_rect else 2)
    M, rank = int(box.sum()), 0
    for r in range(H):
        for c in range(W):
            if m[r, c] & 2:
                if rank < M:
                    m[r, c] |= 4
                rank += 1
    return m, M


@pytest.mark.parametrize("case", ["off", "on"])
def test_torso_selection_equals_the_reference(golden, case):
    """``torso_select_pixels`` (what ``TorsoGetData`` draws with) under the golden's numpy seed: the reference's coordinates in
    the reference's order -- rect, outside, mouth, the mouth block indexing ``coords_norect``."""
    from idealnerf_amd import dataset
    g = golden("torso_sample_rays")
    H, W = g["image"].shape[:2]
    np.random.seed(int(g["seed"]))
    sel = dataset.torso_select_pixels(H, W, g["rect"], g["landmark"], int(g["N_rand"]), case == "on", float(g["sample_rate"]))
    assert sel.dtype == np.int64
    np.testing.assert_array_equal(sel, g[f"coords_{case}"])
    # the reference's colours follow from its coordinates (the images are RGB, read as they are)
    np.testing.assert_array_equal((g["image"][sel[:, 0], sel[:, 1]].astype(np.float32) / np.float32(255.0)), g[f"target_s_{case}"])
    n_mouth = dataset.torso_mouth_num(int(g["N_rand"]), case == "on")
    assert n_mouth == (16 if case == "on" else 0)
    m = dataset.torso_region_byte_map(H, W, g["rect"], g["landmark"])
    n_rect = int((int(g["N_rand"]) - n_mouth) * float(g["sample_rate"]))
    bits = m[sel[:, 0], sel[:, 1]]
    assert ((bits[:n_rect] & 1) == 1).all() and ((bits[n_rect:] & 2) == 2).all()
    assert ((bits[len(sel) - n_mouth:] & 4) == 4).all()               # the mouth block: among the first M outside pixels


def test_torso_byte_map_and_populations(golden, tmp_path):
    from idealnerf_amd import dataset
    g = golden("torso_sample_rays")
    frames = [(g["image"].shape[0], g["image"].shape[1], g["rect"], g["landmark"])]
    rs = np.random.RandomState(3)
    lms = rs.uniform(2, 38, (68, 2))
    lms[48:] = rs.uniform(25, 27, (20, 2))
    frames.append((40, 48, np.array([3, 5, 20, 24], np.int32), lms))
    for H, W, rect, lm in frames:
        want, M = _restated_map(H, W, rect, lm)
        m = dataset.torso_region_byte_map(H, W, rect, lm)
        assert m.dtype == np.uint8 and m.shape == (H, W) and int(m.max()) < 8          # bit 3 clear
        np.testing.assert_array_equal(m, want)
        _, mouth_w, rect_w, drawn, M2 = dataset.torso_region_masks(H, W, rect, lm)
        assert M2 == M == int(mouth_w.sum()) and int(drawn.sum()) == min(M, int((~rect_w).sum()))
        # bit 2 in row-major rank order: exactly the first M entries of coords_norect
        outside = np.nonzero((m.reshape(-1) >> 1) & 1)[0]
        np.testing.assert_array_equal(np.nonzero((m.reshape(-1) >> 2) & 1)[0], outside[:M])
    # the loader's populations are the map's
    d = str(tmp_path / "clip")
    os.makedirs(d)
    flags, meta = write_clip_directory(d, 128, 2, dim_expr=79, face_rect=[8, 8, 60, 60], mouth_range=(30, 38))
    flags.use_highlight = True
    fr = dataset.ResidentTorsoFrames(d, "aud.npy", "train", flags, device="cpu")
    assert fr.counts == (45, 3, 16, 0) and fr.exprs.shape == (2, 79) and fr.imgs.shape == (2, 128, 128, 3)
    for i in range(2):
        want, M = _restated_map(128, 128, meta["frames"][i]["face_rect"], np.loadtxt(os.path.join(d, "ori_imgs", f"{i}.lms")))
        np.testing.assert_array_equal(fr.maps[i].numpy(), want)
        assert fr.populations[i].tolist() == [int(((want >> b) & 1).sum()) for b in range(4)] and fr.populations[i, 2] == M
    # RGB, as the file holds them (the head stage's loader flips to BGR)
    from PIL import Image
    np.testing.assert_array_equal(fr.imgs[1].numpy(), np.asarray(Image.open(os.path.join(d, "head_imgs", "1.jpg"))))
    assert len(fr.frame(1)) == 9 and fr.frame(1)[6].dtype.is_floating_point and fr.frame(1)[6].device.type == "cpu"


def test_resident_torso_frames_refusals(tmp_path):
    """ValueError at construction: where use_highlight's mouth block can index past the outside pixels (upstream: IndexError),
    and where a region is smaller than its count."""
    from idealnerf_amd import dataset
    d = str(tmp_path / "clip")
    os.makedirs(d)
    flags, _ = write_clip_directory(d, 64, 3, dim_expr=79)
    flags.use_highlight = True                      # the box (about 47 x 47) exceeds the 64 * 64 - 51 * 51 = 1495 outside pixels
    with pytest.raises(ValueError, match=r"mouth box holds \d+ pixels, more than the 1495 outside"):
        dataset.ResidentTorsoFrames(d, "aud.npy", "train", flags, device="cpu")
    np.random.seed(0)
    ds = dataset.TorsoGetData(d, "aud.npy", "train", flags, device="cpu")
    assert ds.data_size == 3 and not hasattr(flags, "dim_expr")
    flags.use_highlight = False
    assert len(dataset.ResidentTorsoFrames(d, "aud.npy", "train", flags, device="cpu")) == 3
    flags.N_rand, flags.sample_rate = 3200, 0.5     # 1600 from each of rect-minus-box (about 51 * 51 - 47 * 47) and outside (1495)
    with pytest.raises(ValueError, match=r"frame 0 .*region 'rect' holds \d+ pixels, fewer than the 1600"):
        dataset.ResidentTorsoFrames(d, "aud.npy", "train", flags, device="cpu")


def test_latest_checkpoint_contains(tmp_path):
    from idealnerf_amd.checkpoint import latest_checkpoint
    d = str(tmp_path)
    assert latest_checkpoint(d, contains="torso.tar") is None
    for name in ("head.tar", "000000_torso.tar", "000010_torso.tar", "args.txt"):
        open(os.path.join(d, name), "w").close()
    assert latest_checkpoint(d, contains="head.tar") == os.path.join(d, "head.tar")
    assert latest_checkpoint(d, contains="torso.tar") == os.path.join(d, "000010_torso.tar")
    assert latest_checkpoint(d) == os.path.join(d, "head.tar")           # the head stage's rule is unchanged: natsorted, '.tar'
    assert latest_checkpoint(os.path.join(d, "missing"), contains="head.tar") is None
