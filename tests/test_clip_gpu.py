"""Whole-clip rendering on the device, through the C ABI: the fused clip tail against numpy, the head-only eval flow
against the CPU oracle frame by frame, the head + torso flow against its own per-frame calls byte for byte, and
frame-parallel ranks against one rank.  Scenes and the rank worker: tests/clip_worker.py.  Child processes run under their
own timeouts; nothing is retried."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
import clip_worker as cw
from parity_proof import BEYOND_SHARE, E2E_CAP

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


def np_to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)      # NeRFs/HeadNeRF/helper.py:154


def np_compose(head, lw, fg):
    """to8b(rgb * lw[:, None] + fg) in fp32 on the host, one rounding per operation."""
    prod = (head.astype(np.float32) * lw.astype(np.float32)[:, None]).astype(np.float32)
    return np_to8b((prod + fg.astype(np.float32)).astype(np.float32))


def decode_raw(path, H, W):
    from idealnerf_amd.frame_io import read_avi_chunks
    info, chunks = read_avi_chunks(path)
    row = (W * 3 + 3) & ~3
    return info, [np.frombuffer(c, dtype=np.uint8).reshape(H, row)[::-1, :W * 3].reshape(H, W, 3).copy() for c in chunks]


def compose_inputs(n, seed):
    """Values straddling 0, 1 and the k/255 steps: the composite lands on, just below and just above byte boundaries."""
    rs = np.random.RandomState(seed)
    head = rs.uniform(-0.2, 1.2, (n, 3)).astype(np.float32)
    lw = rs.uniform(0.0, 1.0, n).astype(np.float32)
    lw[rs.rand(n) < 0.2] = 0.0
    lw[rs.rand(n) < 0.2] = 1.0
    k = rs.randint(0, 256, (n, 3)).astype(np.float32)
    target = (k / np.float32(255.0)).astype(np.float32)
    step = rs.choice([-1, 0, 1], (n, 3)).astype(np.float32)
    target = np.where(step == 0, target, np.nextafter(target, np.float32(2) * step)).astype(np.float32)
    fg = (target - (head * lw[:, None]).astype(np.float32)).astype(np.float32)     # composite ~ k/255 +- an ulp
    plain = rs.rand(n) < 0.3
    fg[plain] = rs.uniform(-0.3, 1.3, (int(plain.sum()), 3)).astype(np.float32)
    return head, lw, fg


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 450 * 450])
def test_compose_to8b_bit_exact(idn, dev, n):
    """idealnerf_compose_to8b == numpy's to8b(rgb * lw[:, None] + fg), bit for bit, with and without the channel swap, on the
    vector path (aligned) and the scalar path (n % 4 tail; views that start at an odd float offset); fg_out == to8b(rgb_fg);
    == ops.to8b of the eager device expression."""
    head, lw, fg = compose_inputs(n, n)
    ref = np_compose(head, lw, fg)
    if n >= 1023:
        assert len(np.unique(ref)) == 256       # every byte value occurs
    d = lambda a: torch.from_numpy(a).to(dev)
    for swap in (False, True):
        want = ref[:, ::-1] if swap else ref
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        out, fgo = idn.ops.compose_to8b(d(head), d(lw), d(fg), swap, flag, want_fg=True)
        assert out.dtype == torch.uint8 and out.shape == (n, 3) and int(flag.item()) == 0
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        assert torch.equal(fgo, idn.ops.to8b(d(fg), swap))
        np.testing.assert_array_equal(fgo.cpu().numpy(), np_to8b(fg)[:, ::-1] if swap else np_to8b(fg))
        assert torch.equal(idn.ops.compose_to8b(d(head), d(lw), d(fg), swap), out)          # without fg_out, without a flag
        assert torch.equal(out, idn.ops.to8b(d(head) * d(lw)[:, None] + d(fg), swap))       # the eager expression it replaces
        # unaligned: every input a view one float into a larger buffer (4 bytes off 16-byte alignment), outputs as allocated
        off = lambda a: torch.cat([torch.zeros(1, device=dev), d(a).reshape(-1)])[1:].reshape(a.shape)
        h1, w1, f1 = off(head), off(lw), off(fg)
        assert h1.data_ptr() % 16 == 4 and h1.is_contiguous()
        np.testing.assert_array_equal(idn.ops.compose_to8b(h1, w1, f1, swap).cpu().numpy(), want)
        np.testing.assert_array_equal(idn.ops.compose_to8b(d(head), w1, d(fg), swap).cpu().numpy(), want)
    # image-shaped arguments
    if n == 450 * 450:
        out = idn.ops.compose_to8b(d(head).reshape(450, 450, 3), d(lw).reshape(450, 450), d(fg).reshape(450, 450, 3))
        np.testing.assert_array_equal(out.cpu().numpy(), ref.reshape(450, 450, 3))


def test_compose_to8b_nonfinite_and_argument_errors(idn, dev):
    """A NaN / Inf in any of the three inputs sets the flag and that value is written as 0; everything else is untouched.
    Shape / device errors are raised before the C call; n == 0 launches nothing."""
    n = 1023
    head, lw, fg = compose_inputs(n, 5)
    ref = np_compose(head, lw, fg)
    d = lambda a: torch.from_numpy(a).to(dev)
    cases = [("head", 17, 1, np.nan), ("head", 600, 0, np.inf), ("head", 1022, 2, -np.inf), ("lw", 40, None, np.nan),
             ("lw", 1020, None, np.inf), ("fg", 3, 2, np.nan), ("fg", 513, 0, np.inf), ("fg", 1021, 1, -np.inf)]
    for which, px, ch, bad in cases:
        h, w, f = head.copy(), lw.copy(), fg.copy()
        if which == "lw":
            w[px] = bad
            if bad == np.inf:
                h[px] = [0.5, 0.0, -0.25]        # inf * 0 = NaN, inf * negative = -inf: all three non-finite
        else:
            (h if which == "head" else f)[px, ch] = bad
            if which == "head" and not np.isnan(bad):
                w[px] = 0.5                      # (inf * 0 would be the NaN case again)
        with np.errstate(invalid="ignore"):
            x = ((h * w[:, None]).astype(np.float32) + f).astype(np.float32)
            want = np.where(np.isfinite(x), np_to8b(np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)), 0).astype(np.uint8)
        hit = ~np.isfinite(x)
        assert hit[px].all() if which == "lw" else (hit[px, ch] and hit.sum() == 1), (which, px, bad)
        rest = np.arange(n) != px
        np.testing.assert_array_equal(want[rest], ref[rest])
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        out, fgo = idn.ops.compose_to8b(d(h), d(w), d(f), False, flag, want_fg=True)
        assert int(flag.item()) == 1, (which, px, bad)
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{which} {px} {bad}")
        assert (out.cpu().numpy()[hit] == 0).all()
        assert torch.equal(fgo, idn.ops.to8b(d(f)))          # the torso-only still keeps to8b's own convention
    E = idn._lib.IdealNerfError
    with pytest.raises(E):
        idn.ops.compose_to8b(d(head), d(lw)[:-1], d(fg))
    with pytest.raises(E):
        idn.ops.compose_to8b(d(head), d(lw), d(fg)[:, :2])
    with pytest.raises(E):
        idn.ops.compose_to8b(d(head), d(lw).cpu(), d(fg))
    with pytest.raises(E):
        idn.ops.compose_to8b(d(head).double(), d(lw), d(fg))
    assert idn.ops.compose_to8b(d(head)[:0], d(lw)[:0], d(fg)[:0]).shape == (0, 3)
    lib = idn._lib.load()
    assert lib.idealnerf_compose_to8b(None, None, None, 8, 0, None, None, None, None) != 0          # IDN_EINVAL before any launch


def test_frame_sink_submit_u8_and_submit_composite(idn, dev, tmp_path):
    """Ready uint8 frames (device and host, interleaved) and composite frames enter the same ordered writer as submit();
    the composite still's torso-only image comes out of the same launch."""
    from PIL import Image
    from idealnerf_amd.frame_io import FrameSink
    H, W, N = 12, 16, 7
    rs = np.random.RandomState(0)
    rgb = [rs.uniform(-0.1, 1.1, (H, W, 3)).astype(np.float32) for _ in range(N)]
    lw = [rs.uniform(0, 1, (H, W)).astype(np.float32) for _ in range(N)]
    fg = [rs.uniform(0, 0.6, (H, W, 3)).astype(np.float32) for _ in range(N)]
    rgb[4][2, 3, 1] = np.nan
    yy, xx = np.meshgrid(np.linspace(0, 1, H, dtype=np.float32), np.linspace(0, 1, W, dtype=np.float32), indexing="ij")
    ramp = (0.3 * (yy + xx)).astype(np.float32)
    fg[3] = np.stack([ramp, 0.9 * ramp, 0.8 * ramp], -1)      # a smooth still: JPEG keeps it to about a level
    d = lambda a: torch.from_numpy(a).to(dev)
    sink = FrameSink(str(tmp_path / "c.avi"), W, H, device=dev, keep_frames=True, codec="raw", still_every=3,
                     still_path=str(tmp_path / "s_{i}.jpg"), still_ids=[10 * i for i in range(N)])
    want, kinds = [], ["submit", "u8_dev", "u8_host", "composite", "composite", "u8_host", "composite"]
    for i, kind in enumerate(kinds):
        if kind == "submit":
            sink.submit(d(rgb[i]))
            want.append(np_to8b(rgb[i]))
        elif kind == "composite":
            sink.submit_composite(d(rgb[i]), d(lw[i]), d(fg[i]))
            with np.errstate(invalid="ignore"):
                want.append(np_compose(rgb[i].reshape(-1, 3), lw[i].reshape(-1), fg[i].reshape(-1, 3)).reshape(H, W, 3))
        else:
            u8 = np_to8b(rgb[i])
            flag = torch.ones(1, dtype=torch.int32, device=dev) if i == 1 else False
            sink.submit_u8(torch.from_numpy(u8).to(dev) if kind == "u8_dev" else u8, flag if kind == "u8_dev" else (i == 5))
            want.append(u8)
    sink.release()
    assert sink.nonfinite_frames == [1, 4, 5]
    want[4][2, 3, 1] = 0
    _, frames = decode_raw(str(tmp_path / "c.avi"), H, W)
    assert len(frames) == N == len(sink.frames)
    for i in range(N):
        np.testing.assert_array_equal(frames[i], want[i], err_msg=f"frame {i} ({kinds[i]})")
        np.testing.assert_array_equal(sink.frames[i], want[i])
    names = [str(tmp_path / n) for n in ("s_0.jpg", "s_30.jpg", "s_30_torso.jpg", "s_60.jpg", "s_60_torso.jpg")]
    assert sorted(sink.stills) == sorted(names)
    torso = np.asarray(Image.open(names[2]).convert("RGB"))[..., ::-1]
    err = lambda a, b: np.abs(a.astype(np.int32) - b.astype(np.int32)).mean()
    # quality-95 JPEG of a smooth image: the bound of test_frame_sink_mjpg_and_stills (2 levels on average); the composite
    # frame of the same index is a different picture
    assert torso.shape == (H, W, 3) and err(torso, np_to8b(fg[3])) < 2.0 and err(torso, want[3]) > 20.0
    with pytest.raises(ValueError):
        FrameSink(None, W, H, device=dev).submit_u8(np.zeros((H, W + 1, 3), np.uint8))


def test_head_clip_matches_the_oracle(idn, dev, tmp_path):
    """The head-only eval flow end to end (NeRFs/HeadNeRF/test/eval_aud_exp_nerf.py:435-496): a 6-frame dataset directory
    in the reference's on-disk format -> GetData(val) -> clip.render_head_clip (loader, Network.forward behind nosmo_iters:
    smoothing window + AudioAttNet, render, to8b, ordered writer) -> raw AVI.  Frame j must be to8b of the CPU oracle's
    frame from the dataset's pose, expression and decoded bc.jpg and the audio feature of the audio modules' eager CPU path.

    Bounds (derived, not measured): the project's end-to-end cap is E2E_CAP = 1e-3 per ray (tests/parity_proof.py), 255e-3 < 1
    and astype(uint8) truncates, so NO byte may differ by more than one 8-bit step; and the share of bytes that differ at
    all is at most BEYOND_SHARE (3 %, rays beyond 1e-4) + 255 x 1e-4 (values within the fixed 1e-4 RGB budget of a step
    boundary).  tools/clip_seed_check.py shows that on this scene the oracle's own response to 1e-7 on its coarse weights
    stays inside both.  No frame and no pixel is left out."""
    from idealnerf_amd import clip, dataset
    d = str(tmp_path / "May")
    args = cw.head_dataset(d)
    ds = dataset.GetData(d, "aud.npy", "val", args, skip=1, device=dev)
    assert ds.data_size == cw.HEAD_FRAMES
    net = cw.head_network(dev, ds.focal)
    latent = torch.ones(32)
    path = str(tmp_path / "head.avi")
    net.train()
    res = clip.render_head_clip(net, ds, path, net.args.nosmo_iters, latent_code=latent, codec="raw")
    assert net.training is True        # the caller's mode is restored
    net.eval()
    assert res["n_frames"] == cw.HEAD_FRAMES and res["nonfinite_frames"] == [] and res["world"] == 1
    assert res["seconds"] > 0 and res["frames_per_s"] > 0
    S = cw.HEAD_SIZE
    info, frames = decode_raw(path, S, S)
    assert info["frames"] == cw.HEAD_FRAMES == len(frames) and (info["width"], info["height"]) == (S, S)
    inputs, bc, focal = cw.head_expected_inputs(d, net)
    assert focal == ds.focal
    pc = {k: v.detach().cpu() for k, v in net.face_nerf_coarse.state_dict().items()}
    pf = {k: v.detach().cpu() for k, v in net.face_nerf_fine.state_dict().items()}
    limit = BEYOND_SHARE + 255 * 1e-4
    assert 255 * E2E_CAP < 1
    worst = []
    for j, (c2w, expr, aud) in enumerate(inputs):
        with torch.no_grad():
            ref = oracle.render_frame(S, S, focal, c2w, net.near, net.far, bc, pc, pf, aud, expr, latent)["rgb_map"]
        want = np_to8b(ref.numpy()).astype(np.int32)
        diff = np.abs(frames[j].astype(np.int32) - want)
        print(f"\n  head clip frame {j}: largest byte difference {diff.max()}, bytes that differ {(diff > 0).mean():.4%} "
              f"(limit {limit:.2%}); frame differs from the background by {np.abs(want / 255.0 - bc.numpy()).mean():.3f}")
        worst.append((int(diff.max()), float((diff > 0).mean())))
        assert np.abs(want / 255.0 - bc.numpy()).mean() > 0.02          # there is a volume in front of the background
    assert len({f.tobytes() for f in frames}) == cw.HEAD_FRAMES          # six different frames, in dataset order (above)
    assert all(m <= 1 for m, _ in worst), worst
    assert all(s <= limit for _, s in worst), worst


def test_torso_clip_equals_the_per_frame_calls(idn, dev, tmp_path):
    """NeRFs/TorsoNeRF/test_torso.py:474-535 as clip.render_torso_clip, 4 frames of the sharp head + torso scene: every
    decoded frame equals, byte for byte, ops.to8b(rgb * last_w_t[..., None] + rgb_fg_t) from two plain render_pair calls
    (head pair at poses[j] with the smoothed feature, torso pair at torso_pose with the torso signal).  The clip-level
    audio features equal the per-frame sliding-window loop's (2e-6 of the largest value, as
    test_clip_audio_features_match_reference_loop); the stills of frames 0 and 2 exist and decode to the frame size."""
    from PIL import Image
    from idealnerf_amd import clip
    from idealnerf_amd.models.audio_net import clip_audio_features
    s = cw.torso_scene(dev)
    net, S, n = s["net"], cw.TORSO_SIZE, 4
    path, stills = str(tmp_path / "torso.avi"), tmp_path / "stills"
    stills.mkdir()
    aud_ids = [100 + 3 * j for j in range(cw.TORSO_CLIP)]
    res = clip.render_torso_clip(net, s["poses"], s["auds"], s["bc"], path, expr=s["expr"], latent_code=s["latent"],
                                 torso_pose=s["torso_pose"], aud_ids=aud_ids, frames=range(n), codec="raw", still_every=2,
                                 still_path=str(stills))
    assert res["n_frames"] == n and res["nonfinite_frames"] == [] and res["world"] == 1
    info, frames = decode_raw(path, S, S)
    assert info["frames"] == n == len(frames)
    g = lambda t: t.to(dev)
    auds, poses = g(s["auds"]), g(s["poses"])
    half, F = int(net.args.smo_size / 2), cw.TORSO_CLIP
    with torch.no_grad():
        aud_smo = clip_audio_features(net.aud_net, net.aud_att_net, auds, net.args.smo_size)
        loop = []
        for i in range(F):       # test_torso.py:480-497
            left, right = max(i - half, 0), min(i + half, F)
            win = auds[left:right]
            if i - half < 0:
                win = torch.cat((torch.zeros_like(win)[:half - i], win), 0)
            if i + half > F:
                win = torch.cat((win, torch.zeros_like(win)[:i + half - F]), 0)
            loop.append(net.aud_att_net(net.aud_net(win)))
        loop = torch.stack(loop, 0)
        assert float((aud_smo - loop).abs().max()) < 2e-6 * max(1.0, float(loop.abs().max()))
        kw = dict(H=S, W=S, focal=net.focal, chunk=net.args.chunk, near=net.near, far=net.far, bc_rgb=g(s["bc"]))
        for j in range(n):
            rgb, _, _, _, _, _ = net.render_pair(expr=g(s["expr"]), latent_code=g(s["latent"]), aud_para=aud_smo[j],
                                                 render_poses=s["poses"][j][:3, :4],
                                                 network_nerf={"coarse": net.face_nerf_coarse, "fine": net.face_nerf_fine}, **kw)
            _, _, _, lw_t, fg_t, _ = net.render_pair(expr=None, latent_code=None, aud_para=net.torso_signal(aud_smo[j], poses[j]),
                                                     render_poses=s["torso_pose"][:3, :4],
                                                     network_nerf={"coarse": net.torso_coarse_nerf, "fine": net.torso_fine_nerf}, **kw)
            want = idn.ops.to8b(rgb * lw_t[..., None] + fg_t).cpu().numpy()
            np.testing.assert_array_equal(frames[j], want, err_msg=f"frame {j}")
            assert want.std() > 1 and float(lw_t.max()) > 0.05 and float(fg_t.max()) > 0.05    # not a flat frame; both pairs show in it
    assert len({f.tobytes() for f in frames}) == n
    assert sorted(os.listdir(stills)) == sorted(f"{aud_ids[j]}{sfx}.jpg" for j in (0, 2) for sfx in ("", "_torso"))
    for name in os.listdir(stills):
        assert np.asarray(Image.open(stills / name)).shape == (S, S, 3)


def _run_worker(tmp_path, name, ranks, perturb, seed, draws):
    out = str(tmp_path / f"{name}.avi")
    env = dict(os.environ, OMP_NUM_THREADS="4", IDN_DIST_TIMEOUT_S="90")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "IDN_IN_KERNEL_DRAWS"):
        env.pop(k, None)
    tail = [os.path.join(ROOT, "tests", "clip_worker.py"), "torso", out, str(perturb), str(seed), "1" if draws else "0"]
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
    lines = sorted((json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith('{"rank"')), key=lambda r: r["rank"])
    assert [r["rank"] for r in lines] == list(range(ranks))
    assert lines[0]["result"] == {"n_frames": cw.TORSO_FRAMES, "nonfinite_frames": [], "world": ranks}
    assert all(r["result"] is None for r in lines[1:])
    return open(out, "rb").read()


@pytest.mark.parametrize("perturb,seed,draws", [(0.0, "none", False), (1.0, 7, False), (1.0, 7, True)],
                         ids=["perturb0", "perturb1-torch-rand", "perturb1-in-kernel-draws"])
def test_two_ranks_write_the_single_rank_clip(dev, tmp_path, perturb, seed, draws):
    """5 frames over 2 ranks (3 + 2: an uneven last round), the ranks sharing the device over gloo as fresh child
    processes: rank 0's raw AVI is the single-rank file byte for byte -- also with perturb = 1, where `seed` ties a
    frame's draws to the frame and not to the rank that renders it, in both draw modes."""
    one = _run_worker(tmp_path, "one", 1, perturb, seed, draws)
    two = _run_worker(tmp_path, "two", 2, perturb, seed, draws)
    assert one == two
    _, frames = decode_raw(str(tmp_path / "two.avi"), cw.TORSO_SIZE, cw.TORSO_SIZE)
    assert len(frames) == cw.TORSO_FRAMES and len({f.tobytes() for f in frames}) == cw.TORSO_FRAMES
