"""Driving trained models on the device: ``drive.drive_head`` and ``drive.drive_torso`` against the loops they stand for, written
out by hand; a per-frame expression track through ``clip.render_torso_clip``; and ``tools/drive_clip.py`` as two ranks against
one.  Every comparison is byte equality of decoded raw frames: the driven clip makes the same deterministic render calls
(perturb 0) on the same tensors as the hand-written loop, so there is no tolerance.

Shapes (tests/drive_common.py): 40 x 40 frames -- 1 600 rays, the last 128-point tile ragged --, 16 + 32 samples, 9 frames (at
least the smoothing window of 8, an uneven tail for two ranks), Xavier weights, random latent codes, checkpoints written by
``checkpoint.save_checkpoint``.  The one child process runs under its own timeout; nothing is retried."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import drive_common as dc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = dc.IDENTITY_FRAMES


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()  # fail loudly if the HIP library is missing
    return idealnerf_amd


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return dc.build_directory(str(tmp_path_factory.mktemp("drive") / "May"))


@pytest.fixture(scope="module")
def torso(idn, dev, paths, tmp_path_factory):
    """The head + torso network, its checkpoint pair in a run directory (``head.tar`` from a head-only network with the same
    head pair and audio nets, ``000000_torso.tar`` the whole network: other latent codes than the head file's), the loader's
    track, and -- rendered once -- the driven clip of ``drive_torso``."""
    from idealnerf_amd import checkpoint, dataset, drive
    root = tmp_path_factory.mktemp("torso")
    run_root, save = str(root / "logs"), str(root / "out")
    args, config = dc.flags(paths, run_root, save, "torso")
    track = dataset.load_test_data(args.datadir, args.aud_file, args.test_pose_file, args.testskip, args.test_size, args.aud_start)
    net, codes = dc.torso_network(dev, track[3][2])
    head_net, head_codes = dc.head_network(dev, track[3][2])
    head_net.load_state_dict({k: v for k, v in net.state_dict().items() if k in head_net.state_dict()}, strict=False)
    run = os.path.join(run_root, "run")
    checkpoint.save_checkpoint(os.path.join(run, "head.tar"), head_net, None, head_codes, 11)
    checkpoint.save_checkpoint(os.path.join(run, "000000_torso.tar"), net, None, codes, 3)
    exprs = dataset.load_test_exprs(paths["driving"], 1, F)
    res = drive.drive_torso(args, device=dev, codec="raw")
    return dict(net=net, codes=codes, args=args, config=config, track=track, exprs=exprs, res=res, save=save, root=root,
                run_root=run_root)


def _hand_torso(net, s, path, expr, **kw):
    from idealnerf_amd import clip
    poses, auds, bc_img, _, aud_ids, torso_pose = s["track"]
    return clip.render_torso_clip(net, poses, auds, bc_img / 255, path, expr=expr, latent_code=s["codes"][0], torso_pose=torso_pose,
                                  aud_ids=aud_ids, swap_rb=True, codec="raw", **kw)


def test_drive_head_equals_the_hand_fed_forward(idn, dev, paths, tmp_path):
    """Frame j of drive_head's clip == ops.to8b(network([...])) fed by hand: identity pose j, driving expression j, audio row j
    from the start of the file, latent row 0 of the checkpoint, step 0, the driving file's focal length.  And the clip is not
    the one the identity's own expressions give."""
    from idealnerf_amd import checkpoint, drive
    identity, driving = dc.metas(paths)
    args, _ = dc.flags(paths, str(tmp_path / "logs"), str(tmp_path / "out"), "head")
    net, codes = dc.head_network(dev, float(driving["focal_len"]))
    checkpoint.save_checkpoint(os.path.join(args.basedir, args.expname, "head.tar"), net, None, codes, 40000)
    out = str(tmp_path / "driven.avi")
    res = drive.drive_head(args, out=out, device=dev, codec="raw")
    assert res["path"] == out and res["n_frames"] == F and res["nonfinite_frames"] == [] and res["world"] == 1
    name = f"{args.datadir[8:].lstrip(os.sep)}_{args.aud_file[-9:-4]}_ExpPose_0.jpg"
    assert os.path.exists(os.path.join(args.save_path, name))                                   # the reference's still of frame 0
    info, frames = dc.decode_raw(out)
    assert info["frames"] == F == len(frames)

    from PIL import Image
    bg = torch.tensor(np.asarray(Image.open(paths["bc"])) / 255.0)
    auds = torch.from_numpy(np.load(paths["long"])[:F])
    raw_img = torch.zeros(1, dc.SIZE, dc.SIZE, 3, dtype=torch.uint8)
    none = torch.empty(0)

    def by_hand(j, exp):
        pose = torch.tensor(identity["frames"][j]["transform_matrix"], dtype=torch.float64)[:3, :4]
        data = (none, none, bg, auds, raw_img, pose, torch.tensor(exp, dtype=torch.float32), codes[0], j)
        with torch.no_grad():
            return idn.ops.to8b(net([data, 0, F])[0]).cpu().numpy()

    assert net.focal == float(driving["focal_len"]) != float(identity["focal_len"])
    differ = 0
    for j in range(F):
        want = by_hand(j, driving["frames"][j]["exp"])
        np.testing.assert_array_equal(frames[j], want, err_msg=f"frame {j}")
        assert want.std() > 1                                                                   # not a flat frame
        differ += int(not np.array_equal(frames[j], by_hand(j, identity["frames"][j]["exp"])))
    assert differ >= 1 and len({f.tobytes() for f in frames}) == F

    args.dim_expr = dc.DIM_EXPR + 3
    with pytest.raises(ValueError, match="dim_expr"):
        drive.drive_head(args, out=out, device=dev, codec="raw")
    assert len(dc.decode_raw(out)[1]) == F                                                      # raised before anything was written


def test_expression_track_through_the_torso_clip(idn, dev, torso, tmp_path):
    """render_torso_clip(expr=track[F, E]): frame j takes row j -- by the clip's frame number, whatever `frames` selects --, a
    track of equal rows is the 1-D call's file, a track of F - 1 rows is refused before anything is rendered."""
    net, track = torso["net"], torso["exprs"]
    ids = [0, 4, 8]
    p = lambda name: str(tmp_path / name)
    res = _hand_torso(net, torso, p("track.avi"), track, frames=ids)
    assert res["n_frames"] == len(ids) and res["nonfinite_frames"] == []
    _, got = dc.decode_raw(p("track.avi"))
    for pos, j in enumerate(ids):
        _hand_torso(net, torso, p(f"one{j}.avi"), track[j], frames=[j])
        np.testing.assert_array_equal(got[pos], dc.decode_raw(p(f"one{j}.avi"))[1][0], err_msg=f"frame {j}")
    assert len({g.tobytes() for g in got}) == len(ids)
    # the expression shows: frame 4 under row 0 is another picture
    _hand_torso(net, torso, p("other.avi"), track[0], frames=[4])
    assert not np.array_equal(got[1], dc.decode_raw(p("other.avi"))[1][0])
    _hand_torso(net, torso, p("same_rows.avi"), np.repeat(track[4:5], F, 0), frames=ids)
    _hand_torso(net, torso, p("vector.avi"), track[4], frames=ids)
    assert open(p("same_rows.avi"), "rb").read() == open(p("vector.avi"), "rb").read()
    with pytest.raises(ValueError, match=rf"{F - 1} rows.*{F} frames"):
        _hand_torso(net, torso, p("short.avi"), track[:F - 1], frames=ids)
    assert not os.path.exists(p("short.avi"))
    # the scoring loop takes the same track: its file is the render loop's
    from idealnerf_amd import clip
    poses, auds, bc_img, _, _, torso_pose = torso["track"]
    truth = torch.zeros((F, dc.SIZE, dc.SIZE, 3), dtype=torch.uint8, device=dev)
    clip.score_torso_clip(net, poses, auds, bc_img / 255, truth, expr=track, latent_code=torso["codes"][0], torso_pose=torso_pose,
                          frames=ids, path=p("scored.avi"), swap_rb=True, codec="raw")
    assert open(p("scored.avi"), "rb").read() == open(p("track.avi"), "rb").read()
    with pytest.raises(ValueError, match=rf"{F - 1} rows.*{F} frames"):
        clip.score_torso_clip(net, poses, auds, bc_img / 255, truth, expr=track[:F - 1], latent_code=torso["codes"][0],
                              torso_pose=torso_pose, frames=ids)


def test_drive_torso_equals_the_hand_called_clip(idn, dev, torso, tmp_path):
    """result.avi of drive_torso (head.tar + 000000_torso.tar, testskip 1, test_size 9, aud_start 2, the driving file's
    expressions) == render_torso_clip called by hand with the loader's arrays, the torso file's latent row 0 and the network
    the checkpoints were written from; stills under the audio ids' names."""
    res, save = torso["res"], torso["save"]
    assert res["path"] == os.path.join(save, "result.avi") and res["n_frames"] == F and res["nonfinite_frames"] == []
    assert torso["track"][4] == list(range(2, 2 + F))
    assert sorted(n for n in os.listdir(save) if n.endswith(".jpg")) == ["2.jpg", "2_torso.jpg"]
    _, driven = dc.decode_raw(res["path"])
    assert len(driven) == F and len({f.tobytes() for f in driven}) == F
    ids = [0, 5]
    hand = str(tmp_path / "hand.avi")
    _hand_torso(torso["net"], torso, hand, torso["exprs"], frames=ids)
    _, want = dc.decode_raw(hand)
    for pos, j in enumerate(ids):
        np.testing.assert_array_equal(driven[j], want[pos], err_msg=f"frame {j}")
        assert want[pos].std() > 1


def test_drive_torso_refuses_a_track_of_another_width(idn, dev, torso, paths, tmp_path):
    from idealnerf_amd import drive
    with open(paths["driving"]) as f:
        meta = json.load(f)
    for fr in meta["frames"]:
        fr["exp"] = fr["exp"][:-3]
    narrow = str(tmp_path / "narrow.json")
    with open(narrow, "w") as f:
        json.dump(meta, f)
    args, _ = dc.flags(paths, torso["run_root"], str(tmp_path / "out"), "torso")
    args.evalExpr_path = narrow
    with pytest.raises(ValueError, match=rf"{dc.DIM_EXPR} expression columns.*{dc.DIM_EXPR - 3} wide"):
        drive.drive_torso(args, device=dev, codec="raw")
    assert not os.path.exists(os.path.join(args.save_path, "result.avi"))


def test_drive_clip_two_ranks_write_the_single_rank_clip(dev, torso, paths):
    """tools/drive_clip.py --flow torso --gpus 2: two ranks as fresh child processes sharing the device over gloo (9 frames:
    5 + 4) write, byte for byte, the file one rank wrote in this process, and the tool prints one JSON line."""
    out = str(torso["root"] / "two.avi")
    _, config = dc.flags(paths, torso["run_root"], str(torso["root"] / "out2"), "torso")
    env = dict(os.environ, IDN_DIST_BACKEND="gloo", IDN_FORCE_DEVICE="0", IDN_LAUNCH_TIMEOUT_S="120", IDN_DIST_TIMEOUT_S="90",
               OMP_NUM_THREADS="4")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "drive_clip.py"), "--flow", "torso", "--config", config, "--gpus", "2",
                        "--codec", "raw", "--out", out], env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["world"] == 2 and line["nonfinite_frames"] == [] and line["n_frames"] == F and line["path"] == out
    assert line["flow"] == "torso" and line["shared_device"] is True
    assert open(out, "rb").read() == open(torso["res"]["path"], "rb").read()
    assert sorted(n for n in os.listdir(str(torso["root"] / "out2")) if n.endswith(".jpg")) == ["2.jpg", "2_torso.jpg"]
