"""Frame scores on the device: idealnerf_frame_scores against its fp64 definition (tests/scores_common.py) at the shapes where
the tiling can go wrong, its exact and its hard cases, determinism and host-sync behaviour; clip.score_head_clip and
clip.score_torso_clip against their own per-frame calls bit for bit; two frame-parallel ranks against one (worker
tests/score_worker.py, own timeout, nothing retried); and train.train(val="resident")."""
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import clip_worker as cw
import score_worker as sw
import scores_common as sc
from train_loop_common import train_flags

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()  # fail loudly if the HIP library is missing
    return idealnerf_amd


def _tile():
    import idealnerf_amd
    return idealnerf_amd.ops.SCORE_TILE


def _shapes():
    T = _tile()
    return [(11, 11), (11, 40), (40, 11), (10, 23), (1, 1), (97, 61), (T + 9, T + 10), (T + 10, T + 11), (2 * T + 13, T + 21)]


def _images(H, W, seed):
    rs = np.random.RandomState(seed)
    truth = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    pred = (sc.unit_truth(truth) + rs.normal(0, 0.1, truth.shape)).astype(np.float32)
    regions = rs.randint(0, 16, (H, W)).astype(np.uint8)
    return pred, truth, regions


def _gpu(dev, *arrays):
    return [None if a is None else torch.from_numpy(a).to(dev) for a in arrays]


@pytest.mark.parametrize("H,W", _shapes(), ids=lambda v: str(v))
def test_frame_scores_against_the_fp64_reference(idn, dev, H, W):
    """Every shape with: a random region map over bits 0-3, the same map with bit 2 never set, and no map (rows 1-4 zero).
    Bounds as derived in scores_common.check_against_reference; every group of every shape is checked."""
    pred, truth, regions = _images(H, W, 1000 * H + W)
    no_mouth = regions & np.uint8(0b1011)
    for label, m in (("random", regions), ("bit 2 never set", no_mouth), ("no map", None)):
        got = idn.ops.frame_scores(*_gpu(dev, pred, truth, m))
        assert got.dtype == torch.float64 and tuple(got.shape) == (5, 4) and got.is_cuda
        got, want = got.cpu().numpy(), sc.reference_scores(pred, truth, m)
        windows = max(H - 10, 0) * max(W - 10, 0)
        assert want[0, 0] == H * W and want[0, 2] == windows and want[0, 1] > 0
        if windows:
            print(f"\n  {H} x {W} {label}: sse relative error {abs(got[0, 1] - want[0, 1]) / want[0, 1]:.1e}, "
                  f"mean SSIM error {abs(got[0, 3] - want[0, 3]) / (3 * windows):.1e}")
        sc.check_against_reference(got, want, f"{H} x {W} {label}")
        if m is None:
            assert not got[1:].any()
        elif label != "random":
            assert not got[3].any()
        if H < 11 or W < 11:
            assert not got[:, 2:].any()


def test_identical_images_score_exactly(idn, dev):
    """pred = float(truth) / 255.0f: the squared error is 0.0 exactly and every group's mean SSIM is 1 within 1e-12."""
    _, truth, regions = _images(97, 61, 5)
    got = idn.ops.frame_scores(*_gpu(dev, sc.unit_truth(truth), truth, regions)).cpu().numpy()
    assert (got[:, 0] > 0).all() and (got[:, 2] > 0).all()
    assert (got[:, 1] == 0.0).all()
    assert np.abs(got[:, 3] / (3 * got[:, 2]) - 1.0).max() <= 1e-12
    s = idn.ops.summarise_scores(got)
    assert np.isinf(s["psnr"]).all() and (s["psnr"] > 0).all()


def test_flat_truth_under_small_noise(idn, dev):
    """Truth uniform at 200, sigma-0.02 noise on the prediction: E[x^2] - mu^2 is 4e-4 against mu^2 = 0.6 and C2 = 9e-4, the
    case fp32 window sums get wrong by 3e-4 per window.  The fp64 bounds hold unchanged."""
    rs = np.random.RandomState(9)
    truth = np.full((97, 61, 3), 200, np.uint8)
    pred = (sc.unit_truth(truth) + rs.normal(0, 0.02, truth.shape)).astype(np.float32)
    regions = rs.randint(0, 16, (97, 61)).astype(np.uint8)
    got = idn.ops.frame_scores(*_gpu(dev, pred, truth, regions)).cpu().numpy()
    want = sc.reference_scores(pred, truth, regions)
    print(f"\n  flat truth: mean SSIM {want[0, 3] / (3 * want[0, 2]):.6f}, error {abs(got[0, 3] - want[0, 3]) / (3 * want[0, 2]):.1e}")
    sc.check_against_reference(got, want, "flat truth")


def test_frame_scores_is_deterministic_and_refuses_cpu_tensors(idn, dev):
    pred, truth, regions = _gpu(dev, *_images(97, 61, 6))
    a = idn.ops.frame_scores(pred, truth, regions)
    b = idn.ops.frame_scores(pred, truth, regions)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    table = torch.full((3, 5, 4), -1.0, dtype=torch.float64, device=dev)
    ws = torch.empty(idn.ops.frame_scores_workspace_doubles(97, 61), dtype=torch.float64, device=dev)
    r = idn.ops.frame_scores(pred, truth, regions, out=table[1], workspace=ws)
    assert r.data_ptr() == table[1].data_ptr()
    assert table[1].cpu().numpy().tobytes() == a.cpu().numpy().tobytes()
    assert (table[0] == -1).all() and (table[2] == -1).all()
    with pytest.raises(idn._lib.IdealNerfError):
        idn.ops.frame_scores(pred.cpu(), truth.cpu(), regions.cpu())
    with pytest.raises(idn._lib.IdealNerfError):
        idn.ops.frame_scores(pred, truth, regions, workspace=ws[:3])
    with pytest.raises(idn._lib.IdealNerfError):
        idn.ops.frame_scores(pred, truth[:, :-1], regions)
    with pytest.raises(idn._lib.IdealNerfError):
        idn.ops.frame_scores(pred, truth.float(), regions)


@pytest.fixture(scope="module")
def head_clip(idn, dev, tmp_path_factory):
    """clip_worker's 64 x 64, 6-frame head dataset, resident as a validation clip, and its network."""
    from idealnerf_amd import dataset
    d = str(tmp_path_factory.mktemp("head") / "May")
    args = cw.head_dataset(d)
    fr = dataset.ResidentFrames(d, "aud.npy", "val", args, skip=1, device=dev)
    assert fr.data_size == cw.HEAD_FRAMES
    return d, args, fr, cw.head_network(dev, fr.focal)


def test_scoring_and_the_resident_frame_do_not_synchronise(idn, dev, head_clip):
    """ops.frame_scores with the caller's out / workspace, and ResidentFrames.frame, under torch's sync debug mode "error"."""
    _, _, fr, _ = head_clip
    pred = torch.rand((fr.H, fr.W, 3), device=dev)
    out = torch.empty((5, 4), dtype=torch.float64, device=dev)
    ws = torch.empty(idn.ops.frame_scores_workspace_doubles(fr.H, fr.W), dtype=torch.float64, device=dev)
    want = idn.ops.frame_scores(pred, fr.imgs[2], fr.maps[2]).clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            torch.ones(1, device=dev).item()
        except RuntimeError:
            honoured = True
        data = fr.frame(2)
        idn.ops.frame_scores(pred, data[4], fr.maps[2], out=out, workspace=ws)     # raises here if anything inside waits
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print(f"sync debug mode honoured by this build: {honoured}")
    assert torch.equal(out, want)
    assert not data[5].is_cuda and data[2].is_cuda and data[2].dtype == torch.float64


def test_score_head_clip_end_to_end(idn, dev, head_clip, tmp_path):
    from idealnerf_amd import clip, dataset
    d, args, fr, net = head_clip
    step, latent, n = net.args.nosmo_iters, torch.ones(32), cw.HEAD_FRAMES
    before = sorted(os.listdir(tmp_path))
    net.train()
    try:
        res = clip.score_head_clip(net, fr, step, latent_code=latent)
        assert net.training is True        # the caller's mode is restored
    finally:
        net.eval()
    assert sorted(os.listdir(tmp_path)) == before     # path=None: no file appears
    assert res["frames"] == list(range(n)) and res["n_frames"] == n and res["nonfinite_frames"] == [] and res["world"] == 1
    assert res["seconds"] > 0 and res["frames_per_s"] > 0
    table = res["table"]
    assert table.dtype == torch.float64 and tuple(table.shape) == (n, 5, 4) and not table.is_cuda
    for j in range(n):
        data = fr.frame(j)
        with torch.no_grad():
            rgb = net([(*data[:7], latent, data[7]), step, fr.data_size])[0]
            want = idn.ops.frame_scores(rgb, fr.imgs[j], fr.maps[j])
        assert torch.equal(table[j], want.cpu()), j
        ref = sc.reference_scores(rgb.cpu().numpy(), fr.imgs[j].cpu().numpy(), fr.maps[j].cpu().numpy())
        assert (ref[:, 0] > 0).all() and (ref[:, 2] > 0).all()         # every region is present in these frames
        sc.check_against_reference(table[j].numpy(), ref, f"frame {j}")
    assert len({table[j].numpy().tobytes() for j in range(n)}) == n

    # the summaries are functions of the table
    s = idn.ops.summarise_scores(table)
    for k in ("mse", "psnr", "ssim"):
        assert np.array_equal(res["per_frame"][k], s[k], equal_nan=True)
        # six positive fp64 terms per sum: any order of adding them agrees within 6 x 2^-53 relative, and so do the ratios
        np.testing.assert_allclose(res["pooled"][k], idn.ops.summarise_scores(table.sum(0))[k], rtol=1e-14, atol=0)
    for k in ("psnr", "ssim"):
        assert np.isfinite(s[k]).all() and (res["mean"]["n_excluded"][k] == 0).all()
        np.testing.assert_allclose(res["mean"][k], s[k].mean(0), rtol=1e-13)
    assert (s["psnr"] > 0).all() and (np.abs(s["ssim"]) <= 1).all()
    # ... and frames that have no finite value are counted, not dropped
    holed = table.clone()
    holed[1, 0, 1] = 0.0          # a perfect frame: psnr inf
    holed[2, 3] = 0.0             # a frame without the mouth region
    m = clip.summarise_clip(holed)["mean"]
    assert m["n_excluded"]["psnr"].tolist() == [1, 0, 0, 1, 0] and m["n_excluded"]["ssim"].tolist() == [0, 0, 0, 1, 0]
    np.testing.assert_allclose(m["psnr"][0], np.delete(s["psnr"][:, 0], 1).mean(), rtol=1e-13)

    # with path=: the same table, and the file render_head_clip writes from GetData(val), byte for byte
    scored, rendered = str(tmp_path / "scored.avi"), str(tmp_path / "rendered.avi")
    res2 = clip.score_head_clip(net, fr, step, latent_code=latent, path=scored, codec="raw")
    assert torch.equal(res2["table"], table) and res2["nonfinite_frames"] == []
    ds = dataset.GetData(d, "aud.npy", "val", args, skip=1, device=dev)
    clip.render_head_clip(net, ds, rendered, step, latent_code=latent, codec="raw")
    assert open(scored, "rb").read() == open(rendered, "rb").read()
    # a subset, in the caller's order
    res3 = clip.score_head_clip(net, fr, step, latent_code=latent, frame_ids=[4, 1])
    assert res3["frames"] == [4, 1] and torch.equal(res3["table"], table[[4, 1]])


def test_score_torso_clip_equals_the_per_frame_calls(idn, dev):
    from idealnerf_amd import clip
    from idealnerf_amd.models.audio_net import clip_audio_features
    s = cw.torso_scene(dev)
    net, S, n = s["net"], cw.TORSO_SIZE, 4
    rs = np.random.RandomState(3)
    truth = torch.from_numpy(rs.randint(0, 256, (cw.TORSO_CLIP, S, S, 3)).astype(np.uint8)).to(dev)
    regions = torch.from_numpy(rs.randint(0, 16, (cw.TORSO_CLIP, S, S)).astype(np.uint8)).to(dev)
    res = clip.score_torso_clip(net, s["poses"], s["auds"], s["bc"], truth, regions=regions, expr=s["expr"], latent_code=s["latent"],
                                torso_pose=s["torso_pose"], frames=range(n))
    assert res["n_frames"] == n and res["nonfinite_frames"] == [] and tuple(res["table"].shape) == (n, 5, 4)
    g = lambda t: t.to(dev)
    with torch.no_grad():
        aud_smo = clip_audio_features(net.aud_net, net.aud_att_net, g(s["auds"]), net.args.smo_size)
        kw = dict(H=S, W=S, focal=net.focal, chunk=net.args.chunk, near=net.near, far=net.far, bc_rgb=g(s["bc"]))
        for j in range(n):
            rgb, _, _, _, _, _ = net.render_pair(expr=g(s["expr"]), latent_code=g(s["latent"]), aud_para=aud_smo[j],
                                                 render_poses=s["poses"][j][:3, :4],
                                                 network_nerf={"coarse": net.face_nerf_coarse, "fine": net.face_nerf_fine}, **kw)
            _, _, _, lw_t, fg_t, _ = net.render_pair(expr=None, latent_code=None, aud_para=net.torso_signal(aud_smo[j], g(s["poses"])[j]),
                                                     render_poses=s["torso_pose"][:3, :4],
                                                     network_nerf={"coarse": net.torso_coarse_nerf, "fine": net.torso_fine_nerf}, **kw)
            want = idn.ops.frame_scores(rgb * lw_t[..., None] + fg_t, truth[j], regions[j])
            assert torch.equal(res["table"][j], want.cpu()), j
    assert len({res["table"][j].numpy().tobytes() for j in range(n)}) == n
    plain = clip.score_torso_clip(net, s["poses"], s["auds"], s["bc"], truth, expr=s["expr"], latent_code=s["latent"],
                                  torso_pose=s["torso_pose"], frames=range(2))
    assert torch.equal(plain["table"][:, 0], res["table"][:2, 0]) and not plain["table"][:, 1:].any()


def _run_score_worker(tmp_path, name, ranks, datadir):
    out = str(tmp_path / f"{name}.npy")
    env = dict(os.environ, OMP_NUM_THREADS="4", IDN_DIST_TIMEOUT_S="90")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "IDN_IN_KERNEL_DRAWS"):
        env.pop(k, None)
    tail = [os.path.join(ROOT, "tests", "score_worker.py"), "head", out, datadir]
    if ranks == 1:
        cmd = [sys.executable] + tail
    else:
        env.update(IDN_DIST_BACKEND="gloo", IDN_FORCE_DEVICE="0")
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1",
               "--master-port", str(port)] + tail
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = sorted((json.loads(m) for m in re.findall(r'\{"rank"[^{}]*\}', p.stdout)), key=lambda r: r["rank"])   # the ranks share one pipe
    assert [r["rank"] for r in lines] == list(range(ranks))
    assert lines[0] == {"rank": 0, "got": "rows", "frames": list(range(sw.SCORE_FRAMES)), "n_frames": sw.SCORE_FRAMES,
                        "nonfinite_frames": [], "world": ranks}
    assert all(r == {"rank": r["rank"], "got": "none"} for r in lines[1:])
    return np.load(out)


def test_two_ranks_score_the_single_rank_table(dev, head_clip, tmp_path):
    """5 frames over 2 ranks (3 + 2: an uneven tail), the ranks sharing the device over gloo as fresh child processes,
    perturb = 0: rank 0's table is the single-rank table bit for bit."""
    d = head_clip[0]
    one = _run_score_worker(tmp_path, "one", 1, d)
    two = _run_score_worker(tmp_path, "two", 2, d)
    assert one.dtype == np.float64 and one.shape == (sw.SCORE_FRAMES, 5, 4)
    assert one.tobytes() == two.tobytes()
    assert len({r.tobytes() for r in one}) == sw.SCORE_FRAMES and (one[:, 0, 1] > 0).all()


def test_train_with_resident_validation(idn, dev, tmp_path):
    """64 x 64, 3 frames, 2 steps: step 0 is a validation moment.  val="resident" hands on_log "val_scores" whose whole-frame
    PSNR is the reference's mse2psnr(img2mse(rgb, raw / 255)) of the image logged beside it (1e-5 dB), renders the image the
    default path renders, and leaves the training sequence alone; two default runs log the same sequence."""
    from idealnerf_amd import train as T_
    from idealnerf_amd.helper import img2mse, mse2psnr
    from idealnerf_amd.synthetic import write_clip_directory
    d = str(tmp_path / "clip")
    os.makedirs(d)
    flags, _ = write_clip_directory(d, 64, 3, seed=2)
    mk = lambda name: train_flags(d, tmp_path / "logs", name, flags, perturb=0.0, i_print=1, i_weights=1000, N_iters=10, chunk=8192)

    def run(name, **kw):
        events = []
        torch.manual_seed(11)
        out = T_.train(mk(name), loader="resident", sample_seed=3, device=dev, steps=2,
                       on_log=lambda kind, step, payload: events.append((kind, step, payload)), **kw)
        assert out["global_step"] == 2
        return events

    a, b, r = run("a"), run("b"), run("r", val="resident")
    assert [(k, s) for k, s, _ in a] == [("train", 0), ("val", 0), ("train", 1)] == [(k, s) for k, s, _ in b]
    for (_, _, pa), (_, _, pb) in zip(a, b):
        assert torch.equal(pa, pb) if torch.is_tensor(pa) else pa == pb
    assert [(k, s) for k, s, _ in r] == [("train", 0), ("val", 0), ("val_scores", 0), ("train", 1)]
    assert [p for k, _, p in r if k == "train"] == [p for k, _, p in a if k == "train"]
    image, scores = r[1][2], r[2][2]
    assert torch.equal(image, a[1][2])
    assert scores["groups"] == list(idn.ops.SCORE_GROUPS) and 0 <= scores["frame"] < 3
    assert all(len(scores[k]) == 5 and np.isfinite(scores[k]).all() for k in ("mse", "psnr", "ssim"))
    H = image.shape[1] // 2
    want = float(mse2psnr(img2mse(image[:, :H], image[:, H:])))
    print(f"\n  val/psnr {scores['psnr'][0]:.6f} dB, mse2psnr(img2mse(.)) of the logged image {want:.6f} dB; val/ssim {scores['ssim'][0]:.4f}")
    assert abs(scores["psnr"][0] - want) <= 1e-5
    with pytest.raises(ValueError):
        T_.train(mk("a"), val="nope", device=dev, steps=1)
