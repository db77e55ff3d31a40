"""Frame scores, the parts that need no GPU: the fp64 reference against a brute-force evaluation of single windows, the host-side
summary, the C entry's argument errors, the resident validation loader against GetData(val), and the one collective of a
scored clip (child ranks over gloo, worker tests/score_worker.py)."""
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import score_worker as sw
import scores_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_separable_reference_equals_brute_force_windows():
    """Two fp64 evaluation orders of the same definition -- row filter then column filter, and the 121 products of a window
    directly -- agree within 1e-11 on EVERY window: a 13 x 12 noise image, and a 12 x 13 image with uniform truth (200) under
    sigma-0.02 noise, where E[x^2] - mu^2 cancels against C2.  (Observed: at most 7e-13.)"""
    rs = np.random.RandomState(0)
    cases = [(rs.uniform(-0.1, 1.1, (13, 12, 3)).astype(np.float32), rs.randint(0, 256, (13, 12, 3)).astype(np.uint8))]
    flat = np.full((12, 13, 3), 200, np.uint8)
    cases.append(((sc.unit_truth(flat) + rs.normal(0, 0.02, flat.shape)).astype(np.float32), flat))
    for pred, truth in cases:
        a, b = sc.ssim_map(pred, truth), sc.ssim_map_brute(pred, truth)
        assert a.shape == b.shape == (pred.shape[0] - 10, pred.shape[1] - 10, 3) and a.size > 0
        print(f"\n  {pred.shape[:2]}: separable vs brute force, largest difference {np.abs(a - b).max():.2e}")
        assert np.abs(a - b).max() <= 1e-11
    w = sc.window_weights()
    assert w.shape == (11,) and np.array_equal(w, w[::-1]) and abs(w.sum() - 1) < 1e-7 and np.array_equal(w, w.astype(np.float32))


def test_summarise_scores_on_a_hand_built_table():
    from idealnerf_amd import ops
    from idealnerf_amd.helper import mse2psnr
    table = np.zeros((2, 5, 4))
    table[0, 0] = [100, 3.0, 40, 90.0]        # ordinary
    table[0, 1] = [10, 0.0, 4, 12.0]          # sse == 0: psnr inf, ssim 1
    table[0, 2] = [0, 0.0, 0, 0.0]            # empty group
    table[0, 3] = [7, 2.1, 0, 0.0]            # pixels but no window centre
    table[0, 4] = [50, 1e-3, 20, 59.4]
    table[1] = table[0] * 2
    got = ops.summarise_scores(table)
    assert set(got) == {"mse", "psnr", "ssim"} and all(v.shape == (2, 5) and v.dtype == np.float64 for v in got.values())
    assert got["mse"][0, 0] == 3.0 / 300 and got["ssim"][0, 0] == 90.0 / 120 and got["ssim"][0, 4] == 59.4 / 60
    assert got["mse"][0, 1] == 0.0 and got["psnr"][0, 1] == np.inf and got["ssim"][0, 1] == 1.0
    assert np.isnan(got["mse"][0, 2]) and np.isnan(got["psnr"][0, 2]) and np.isnan(got["ssim"][0, 2])
    assert got["mse"][0, 3] == 2.1 / 21 and np.isnan(got["ssim"][0, 3])
    for g in (0, 3, 4):
        want = float(mse2psnr(torch.tensor(got["mse"][0, g], dtype=torch.float64)))
        # mse2psnr divides by log(10) held as an fp32 tensor: that constant is within 2^-24 of log(10), nothing else rounds in fp32
        assert abs(got["psnr"][0, g] - want) <= 2.0 ** -23 * abs(want), (g, got["psnr"][0, g], want)
    assert np.array_equal(got["psnr"][1], got["psnr"][0], equal_nan=True)      # sums scale, ratios do not
    one = ops.summarise_scores(torch.from_numpy(table[0]))
    assert np.array_equal(one["psnr"], got["psnr"][0], equal_nan=True)
    with pytest.raises(ValueError):
        ops.summarise_scores(np.zeros((5, 3)))


def test_frame_scores_is_exported_and_refuses_bad_arguments_without_a_gpu():
    import idealnerf_amd
    lib = idealnerf_amd._lib.load()
    assert hasattr(lib, "idealnerf_frame_scores") and hasattr(lib, "idealnerf_frame_scores_workspace_bytes")
    assert len(idealnerf_amd._lib.PROTOTYPES["idealnerf_frame_scores"][1]) == 9
    assert lib.idealnerf_version() == 4
    T = idealnerf_amd._lib.SCORE_TILE
    assert idealnerf_amd.ops.SCORE_TILE == T
    assert lib.idealnerf_frame_scores_workspace_bytes(1, 1) == 160
    assert lib.idealnerf_frame_scores_workspace_bytes(T, T + 1) == 2 * 160
    assert lib.idealnerf_frame_scores_workspace_bytes(0, 5) == 0
    ok = 4096                                     # any non-null address: nothing is dereferenced before the checks
    assert lib.idealnerf_frame_scores(ok, ok, None, 0, 5, ok, ok, 1 << 20, None) < 0 and b"0 x 5" in lib.idealnerf_last_error()
    assert lib.idealnerf_frame_scores(ok, ok, None, 4, 4, None, ok, 1 << 20, None) < 0 and b"NULL" in lib.idealnerf_last_error()
    assert lib.idealnerf_frame_scores(None, ok, None, 4, 4, ok, ok, 1 << 20, None) < 0 and b"NULL" in lib.idealnerf_last_error()
    assert lib.idealnerf_frame_scores(ok, ok, None, 4, 4, ok, ok, 159, None) < 0 and b"workspace" in lib.idealnerf_last_error()
    assert lib.idealnerf_frame_scores(ok, ok, None, 4, 4, ok, None, 0, None) < 0 and b"workspace" in lib.idealnerf_last_error()
    with pytest.raises(idealnerf_amd._lib.IdealNerfError):
        idealnerf_amd.ops.frame_scores(torch.zeros(4, 4, 3), torch.zeros(4, 4, 3, dtype=torch.uint8))    # CPU tensors: no fallback


def test_resident_frame_equals_getdata_val(tmp_path, monkeypatch):
    """ResidentFrames(mode="val").frame(i) hands Network.forward the values GetData(val)[i] does -- background (float64
    uint8 / 255.0), audio windows, ground-truth image, pose, expression, index: exactly -- with the pose on the host.
    (GetData's ray sampling needs the device; its three outputs are the fields the eval forward does not read, so it is
    stubbed out here.  tests/test_scores_gpu.py pins the same fields through the rendered bytes.)"""
    from idealnerf_amd import dataset
    from idealnerf_amd.synthetic import write_clip_directory
    d = str(tmp_path / "clip")
    os.makedirs(d)
    flags, _ = write_clip_directory(d, 64, 3, seed=4)
    nothing = torch.empty(0)
    monkeypatch.setattr(dataset, "sample_rays", lambda *a, **k: (nothing, nothing, nothing))
    gd = dataset.GetData(d, "aud.npy", "val", flags, skip=flags.testskip, device="cpu")
    fr = dataset.ResidentFrames(d, "aud.npy", "val", flags, skip=flags.testskip, device="cpu")
    assert len(fr) == len(gd) == 3
    for i in range(3):
        np.random.seed(i)
        _, _, bg, auds, raw, pose, expr, index = gd[i]
        r = fr.frame(i)
        assert len(r) == 8
        assert r[2].dtype == bg.dtype == torch.float64 and torch.equal(r[2], bg)
        assert r[3].dtype == auds.dtype and torch.equal(r[3], auds)
        assert r[4].dtype == raw.dtype == torch.uint8 and torch.equal(r[4], raw)
        assert isinstance(r[5], torch.Tensor) and r[5].device.type == "cpu" and np.array_equal(r[5].numpy(), pose)
        assert r[6].dtype == expr.dtype and torch.equal(r[6], expr)
        assert r[7] == index == i and isinstance(r[7], int)
        assert r[0].numel() == 0 and r[1].numel() == 0
    assert not torch.equal(fr.frame(0)[4], fr.frame(1)[4])


def test_gather_frame_rows_gloo_three_ranks(tmp_path):
    """10 frames over 3 ranks (shares of 4, 3, 3: an uneven tail), one gather: rank 0 holds every frame's row once, in frame
    order; the other ranks get None; without a process group the rows pass through."""
    from idealnerf_amd.parallel import gather_frame_rows
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, OMP_NUM_THREADS="1", IDN_DIST_TIMEOUT_S="90")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = str(tmp_path / "rows.npy")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "tests", "score_worker.py"), "gather", out],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = sorted((json.loads(m) for m in re.findall(r'\{"rank"[^{}]*\}', p.stdout)), key=lambda d: d["rank"])   # the ranks share one pipe
    assert [(d["rank"], d["got"]) for d in lines] == [(0, "rows"), (1, "none"), (2, "none")]
    want = np.stack([sw.gather_row(j) for j in range(sw.GATHER_FRAMES)])
    got = np.load(out)
    assert got.dtype == np.float64 and got.shape == (sw.GATHER_FRAMES, sw.GATHER_K) and np.array_equal(got, want)
    assert len({r.tobytes() for r in want}) == sw.GATHER_FRAMES
    assert not torch.distributed.is_initialized()
    t = torch.from_numpy(want)
    assert gather_frame_rows(t, sw.GATHER_FRAMES) is t
    with pytest.raises(ValueError):
        gather_frame_rows(t[:4], sw.GATHER_FRAMES)
