"""The two test-time loaders against the reference's own, on the directory of tests/drive_common.py: ``dataset.load_test_data``
against ``load_test_data`` of NeRFs/TorsoNeRF/load_audface.py and ``dataset.DrivingFrames`` against the constructor of the eval
script's ``GetData`` -- both recorded by tests/golden/make_golden_drive.py into tests/golden/drive_loaders.npz, array for
array (audio and expression rows as the index of the table row they copy) --, and the errors the loaders raise by name.  No GPU."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import drive_common as dc

# name -> (audio file key, testskip, test_size, aud_start, frames, audio rows, aud_ids): make_golden_drive.LOAD_CASES and what
# the rules give on it (the fixture must say the same)
LOAD_CASES = {"short": ("short", 1, -1, 0, 6, [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]),
              "clamped": ("short", 2, 3, 4, 3, [4, 5, 5], [4, 5, 6]),
              "long": ("long", 1, -1, 0, 9, list(range(9)), list(range(9)))}


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return dc.build_directory(str(tmp_path_factory.mktemp("drive") / "May"))


@pytest.fixture(scope="module")
def fx(golden):
    return golden("drive_loaders")


def flags(paths, **kw):
    return SimpleNamespace(**dict(dict(evalExpr_path=paths["driving"], testskip=1, gt_dirs="head_imgs"), **kw))


@pytest.mark.parametrize("case", sorted(LOAD_CASES))
def test_load_test_data_equals_the_reference(paths, fx, case):
    from idealnerf_amd import dataset
    aud, skip, size, start, n, rows, ids = LOAD_CASES[case]
    poses, auds, bc_img, hwfcxy, aud_ids, torso_pose = dataset.load_test_data(paths["dir"], paths[aud], paths["identity"], skip, size, start)
    table = np.load(paths[aud])
    assert fx[f"ltd_{case}_aud_rows"].tolist() == rows and fx[f"ltd_{case}_aud_ids"].tolist() == ids      # the issue's figures
    assert poses.dtype == np.float32 and poses.shape == (n, 4, 4)
    np.testing.assert_array_equal(poses, fx[f"ltd_{case}_poses"])
    assert auds.dtype == np.float32 and auds.shape == (n, 16, 29)
    np.testing.assert_array_equal(auds, table[fx[f"ltd_{case}_aud_rows"]])
    assert bc_img.dtype == np.uint8
    np.testing.assert_array_equal(bc_img, fx["bc"])
    assert [type(v) for v in hwfcxy] == [int, int, float, float, float]
    np.testing.assert_array_equal(np.asarray(hwfcxy, dtype=np.float64), fx[f"ltd_{case}_hwfcxy"])
    assert list(aud_ids) == ids
    assert torso_pose.dtype == np.float64
    np.testing.assert_array_equal(torso_pose, fx[f"ltd_{case}_torso_pose"])
    identity, _ = dc.metas(paths)
    np.testing.assert_array_equal(torso_pose, np.array(identity["frames"][0]["transform_matrix"]))


def test_load_test_data_opens_its_files_as_given(paths, tmp_path):
    """The pose file and the audio file are not joined to datadir, which supplies bc.jpg alone; focal, cx, cy are the pose
    file's; test_size 0 never ends the track."""
    from idealnerf_amd import dataset
    away = tmp_path / "elsewhere"
    away.mkdir()
    pose_file, aud_file = str(away / "poses.json"), str(away / "a.npy")
    with open(paths["driving"]) as f:
        meta = json.load(f)
    with open(pose_file, "w") as f:
        json.dump(meta, f)
    np.save(aud_file, np.load(paths["long"]))
    poses, auds, bc_img, hwfcxy, aud_ids, torso_pose = dataset.load_test_data(paths["dir"], aud_file, pose_file, 1, 0, 3)
    assert poses.shape[0] == dc.DRIVING_FRAMES and aud_ids == list(range(3, 3 + dc.DRIVING_FRAMES))
    assert hwfcxy == [dc.SIZE, dc.SIZE, float(meta["focal_len"]), float(meta["cx"]), float(meta["cy"])]
    np.testing.assert_array_equal(auds, np.load(aud_file)[np.minimum(np.arange(3, 3 + dc.DRIVING_FRAMES), dc.LONG_AUDIO - 1)])
    with pytest.raises(FileNotFoundError):
        dataset.load_test_data(paths["dir"], dc.LONG_FILE, pose_file)


@pytest.mark.parametrize("skip", [1, 2])
def test_driving_frames_equal_the_reference(paths, fx, skip):
    from idealnerf_amd import dataset
    ds = dataset.DrivingFrames(paths["dir"], paths["long"], "val", flags(paths), skip=skip, device="cpu")
    identity, driving = dc.metas(paths)
    focal, cx, cy, H, W, n = fx[f"gd_skip{skip}_scalars"]
    assert (ds.focal, ds.cx, ds.cy, ds.H, ds.W, ds.data_size, len(ds)) == (focal, cx, cy, H, W, n, n)
    assert ds.focal == float(driving["focal_len"]) != float(identity["focal_len"])         # the driving file's
    assert (ds.cx, ds.cy) == (float(identity["cx"]), float(identity["cy"])) != (float(driving["cx"]), float(driving["cy"]))
    np.testing.assert_array_equal(np.asarray(ds.all_poses), fx[f"gd_skip{skip}_poses"])                     # the identity's
    np.testing.assert_array_equal(np.asarray(ds.all_poses), np.asarray([f["transform_matrix"] for f in identity["frames"][::skip]]))
    table = np.asarray([f["exp"] for f in driving["frames"]])
    np.testing.assert_array_equal(np.asarray(ds.all_exprs, dtype=np.float64), table[fx[f"gd_skip{skip}_expr_rows"]])
    assert fx[f"gd_skip{skip}_expr_rows"].tolist() == list(range(0, skip * int(n), skip))
    assert ds.auds.dtype == torch.float32
    np.testing.assert_array_equal(ds.auds.numpy(), np.load(paths["long"])[fx[f"gd_skip{skip}_aud_rows"]])
    assert fx[f"gd_skip{skip}_aud_rows"].tolist() == list(range(int(n)))                                   # from the file's start
    assert ds.background_img.dtype == torch.float64
    np.testing.assert_array_equal(ds.background_img.numpy(), fx["bc"] / 255.0)


def test_driving_frames_item_is_the_eval_tuple(paths):
    """GetData's field positions, with what the eval forward reads; no image, landmark or parsing file exists in the directory."""
    from idealnerf_amd import dataset
    assert not any(os.path.exists(os.path.join(paths["dir"], sub)) for sub in ("head_imgs", "ori_imgs", "parsing"))
    ds = dataset.DrivingFrames(paths["dir"], dc.LONG_FILE, "val", flags(paths), skip=2, device="cpu")      # the name joined to data_dir
    _, driving = dc.metas(paths)
    for j in range(ds.data_size):
        item = ds[j]
        assert len(item) == 8
        batch_rays, target_s, bg, auds, raw_img, pose, expr, index = item
        assert batch_rays.numel() == 0 and target_s.numel() == 0 and index == j
        assert bg is ds.background_img and float(bg.min()) >= 0.0 and float(bg.max()) <= 1.0
        assert auds is ds.auds and tuple(auds.shape) == (ds.data_size, 16, 29)
        assert raw_img.dtype == torch.uint8 and tuple(raw_img.shape) == (ds.H, ds.W, 3) and int(raw_img.max()) == 0
        assert pose.shape == (3, 4)
        np.testing.assert_array_equal(pose, ds.all_poses[j][:3, :4])
        assert expr.dtype == torch.float32
        np.testing.assert_array_equal(expr.numpy(), np.asarray(driving["frames"][2 * j]["exp"], dtype=np.float32))
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)))       # collates like GetData's
    assert tuple(batch[5].shape) == (1, 3, 4) and tuple(batch[4].shape) == (1, ds.H, ds.W, 3) and int(batch[7]) == 0


def test_driving_frames_errors(paths, tmp_path):
    from idealnerf_amd import dataset
    make = lambda aud=paths["long"], skip=1, d=paths["dir"], **kw: dataset.DrivingFrames(d, aud, "val", flags(paths, **kw), skip=skip,
                                                                                        device="cpu")
    with pytest.raises(ValueError, match="evalExpr_path"):
        make(evalExpr_path=None)
    with pytest.raises(ValueError, match=rf"{dc.SHORT_AUDIO} audio rows.*{dc.IDENTITY_FRAMES} frames"):
        make(aud=paths["short"])
    with open(paths["driving"]) as f:
        meta = json.load(f)
    meta["frames"] = meta["frames"][:dc.IDENTITY_FRAMES - 2]
    few = str(tmp_path / "few.json")
    with open(few, "w") as f:
        json.dump(meta, f)
    with pytest.raises(ValueError, match=rf"{dc.IDENTITY_FRAMES - 2} expression vectors.*{dc.IDENTITY_FRAMES} frames"):
        make(evalExpr_path=few)
    with pytest.raises(ValueError, match=r"4 expression vectors at skip 2.*5 frames"):
        make(evalExpr_path=few, skip=2)
    # a bc.jpg of another shape than the identity's cx / cy
    from PIL import Image
    other = dc.build_directory(str(tmp_path / "Other"))
    Image.fromarray(np.zeros((dc.SIZE, dc.SIZE + 8, 3), np.uint8)).save(other["bc"])
    with pytest.raises(ValueError, match="bc.jpg"):
        dataset.DrivingFrames(other["dir"], other["long"], "val", flags(other), device="cpu")


def test_load_test_exprs(paths):
    from idealnerf_amd import dataset
    _, driving = dc.metas(paths)
    table = np.asarray([f["exp"] for f in driving["frames"]], dtype=np.float32)
    got = dataset.load_test_exprs(paths["driving"], 1, dc.IDENTITY_FRAMES)
    assert got.dtype == np.float32 and got.shape == (dc.IDENTITY_FRAMES, dc.DIM_EXPR)
    np.testing.assert_array_equal(got, table[:dc.IDENTITY_FRAMES])
    np.testing.assert_array_equal(dataset.load_test_exprs(paths["driving"], 3, 4), table[::3][:4])
    with pytest.raises(ValueError, match=r"holds 4 .*needs 5"):
        dataset.load_test_exprs(paths["driving"], 3, 5)
    with pytest.raises(ValueError, match=rf"holds {dc.DRIVING_FRAMES} .*needs {dc.DRIVING_FRAMES + 1}"):
        dataset.load_test_exprs(paths["driving"], 1, dc.DRIVING_FRAMES + 1)


def test_load_stage_checkpoints(tmp_path):
    """What train_torso.train and drive.drive_torso both load through: the newest *head.tar* with strict=False, then the
    newest *torso.tar* strictly -> (the torso file's step, the latent codes of the last file loaded)."""
    from idealnerf_amd import checkpoint
    from idealnerf_amd.audio_exp_nerf import Network as HeadNetwork
    from idealnerf_amd.train_torso import Network, load_stage_checkpoints
    cfg = dc.render_config()
    head_net = lambda: HeadNetwork(dc.SIZE, dc.SIZE, 100.0, cfg.near, cfg.far, cfg.chunk, None, dc.N_SAMPLES, dc.N_IMPORTANCE, args=cfg)
    torso_net = lambda: Network(dc.SIZE, dc.SIZE, 100.0, cfg.near, cfg.far, cfg.chunk, dc.N_SAMPLES, dc.N_IMPORTANCE, args=cfg,
                                dim_aud_body=64, dim_expr_head=dc.DIM_EXPR)
    run = str(tmp_path / "run")
    assert load_stage_checkpoints(run, torso_net()) == (0, None)
    torch.manual_seed(1)
    head, old, new = head_net(), torso_net(), torso_net()
    codes = [torch.full((3, 32), float(i)) for i in range(3)]
    checkpoint.save_checkpoint(os.path.join(run, "head.tar"), head, None, codes[0], 5)       # holds ds_aud_net, no torso pair
    net = torso_net()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    step, got = load_stage_checkpoints(run, net)
    assert step == 0 and torch.equal(got, codes[0])
    sd = net.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in head.state_dict().items() if k in sd)
    assert all(torch.equal(sd[k], before[k]) for k in sd if k.startswith("torso_"))
    checkpoint.save_checkpoint(os.path.join(run, "000002_torso.tar"), old, None, codes[1], 7)
    checkpoint.save_checkpoint(os.path.join(run, "000010_torso.tar"), new, None, codes[2], 9)    # newest in natural order
    step, got = load_stage_checkpoints(run, net)
    assert step == 9 and torch.equal(got, codes[2])
    assert all(torch.equal(v, new.state_dict()[k]) for k, v in net.state_dict().items())
