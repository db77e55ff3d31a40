"""The training loop's resident data path on the GPU: the sampler kernels against their numpy definition and against the
reference loader's own values, ``ResidentFrames`` against ``GetData`` on one generated directory, and ``train.train``
(resume, checkpoint keys, validation, the hand-written loop, and that it learns as well as the reference loader)."""
import json
import os

import numpy as np
import pytest
import torch

from idealnerf_amd.synthetic import write_clip_directory
from train_loop_common import random_region_map, sampler_reference, train_flags

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    return idealnerf_amd


def _pops(m):
    return [int(((m >> g) & 1).sum()) for g in range(4)]


# ------------------------------------------------------------------------------------------------ sample_pixels
@pytest.mark.parametrize("H,W", [(450, 450), (64, 64), (48, 80)])
def test_sample_pixels_equals_definition(idn, dev, H, W):
    """sel equals the numpy restatement element for element: several seeds and draws (one above 2^32), a region whose count is
    0, a region drawn whole, the default 3072 / 256 / 0 / 0.95 split at 450 x 450, and maps that start at any byte address."""
    ops = idn.ops
    m = random_region_map(H, W, seed=H + W)
    pops = _pops(m)
    small = (min(37, pops[0]), min(11, pops[1]), min(5, pops[2]), min(9, pops[3]))
    cases = [(small, 0, 0), (small, 0x0123456789ABCDEF, 1), (small, 7, (1 << 32) + 5), (small, (1 << 63) + 11, (1 << 40) + 3),
             ((small[0], 0, small[2], small[3]), 3, 2),                                # a region whose count is 0
             ((5, 3, min(pops[2], 4096), 0), 5, 9)]                                    # a region drawn whole (or to the maximum)
    if (H, W) == (450, 450):
        cases += [(ops.sample_counts(3072, 256, 0, 0.95), 0, 0), (ops.sample_counts(3072, 256, 0, 0.95), 99, 123456789),
                  (ops.sample_counts(3072, 256, 64, 0.95), 1, (1 << 33))]
    else:
        whole = min(pops, key=lambda p: p if p > 0 else 1 << 30)
        g = pops.index(whole)
        c = [2, 2, 2, 2]
        c[g] = whole
        assert whole <= 4096
        cases.append((tuple(c), 13, 4))                                                # count == population
    # the map at offsets 0 .. 3 of a larger buffer: 16-byte aligned, and three ragged starts
    pad = torch.zeros(H * W + 64, dtype=torch.uint8, device=dev)
    ws = torch.zeros(4, dtype=torch.int32, device=dev)
    for k, (counts, seed, draw) in enumerate(cases):
        off = (0, 1, 7, 12)[k % 4]
        view = pad[off:off + H * W].view(H, W)
        view.copy_(torch.from_numpy(m))
        sel = ops.sample_pixels(view, counts, seed, draw, workspace=ws)
        want = sampler_reference(m, counts, seed, draw)
        assert sel.dtype == torch.int64 and sel.shape == (sum(counts),)
        got = sel.cpu().numpy()
        assert np.array_equal(got, want), (counts, seed, draw, off, int((got != want).sum()))
        assert ws.cpu().tolist() == [p if c > 0 else -1 for p, c in zip(pops, counts)]   # the populations, as counted


def test_sample_pixels_when_the_boundary_bin_is_shared(idn, dev):
    """The select usually ends after two 11-bit passes, when the bin that holds the c-th smallest composite holds nothing else.
    Draws are searched (in numpy, deterministically) for which another pixel of the region shares the top 22 key bits of the
    c-th smallest, so that a third pass has to separate them; the kernel must still equal the definition."""
    from oracle.philox import philox4x32_10
    ops = idn.ops
    m = random_region_map(450, 450, seed=900)
    counts = ops.sample_counts(3072, 256, 0, 0.95)
    p = np.nonzero(m.reshape(-1) & 1)[0].astype(np.uint64)
    md = torch.from_numpy(m).to(dev)
    found = []
    for draw in range(600):
        key = philox4x32_10((p, np.zeros_like(p), np.full_like(p, draw), np.zeros_like(p)), (77, 0))[0]
        comp = np.sort((key << np.uint64(32)) | p)
        if int((comp >> np.uint64(42) == comp[counts[0] - 1] >> np.uint64(42)).sum()) > 1:
            found.append(draw)
            if len(found) == 3:
                break
    assert len(found) == 3, found          # about one draw in forty at this population
    for draw in found:
        sel = ops.sample_pixels(md, counts, 77, draw).cpu().numpy()
        assert np.array_equal(sel, sampler_reference(m, counts, 77, draw)), draw


def test_sample_pixels_refuses_what_it_cannot_do(idn, dev):
    ops = idn.ops
    m = torch.from_numpy(random_region_map(450, 450, seed=3)).to(dev)
    with pytest.raises(idn._lib.IdealNerfError, match="4096"):
        ops.sample_pixels(m, (4097, 0, 0, 0), 0, 0)
    ws = torch.zeros(4, dtype=torch.int32, device=dev)
    out = torch.empty(4097, dtype=torch.int64, device=dev)
    rc = idn._lib.load().idealnerf_sample_pixels(m.data_ptr(), 450, 450, 0, 4097, 0, 0, 0, 0, ws.data_ptr(), 16, out.data_ptr(), None)
    assert rc == -2                                                                    # IDN_EUNSUPPORTED, nothing launched
    with pytest.raises(idn._lib.IdealNerfError):
        ops.sample_pixels(m.cpu(), (1, 1, 1, 1), 0, 0)
    with pytest.raises(idn._lib.IdealNerfError):
        ops.sample_pixels(m.to(torch.int32), (1, 1, 1, 1), 0, 0)
    # a count above the POPULATION (which only the loader can know) never yields a partial or repeated pick: the rows say -1
    tiny = np.zeros((64, 64), np.uint8)
    tiny[:2, :3] = 1 << 2
    tiny[10:, :] |= 1
    sel = ops.sample_pixels(torch.from_numpy(tiny).to(dev), (4, 0, 7, 0), 1, 1).cpu().numpy()
    assert np.array_equal(sel[:4], sampler_reference(tiny, (4, 0, 0, 0), 1, 1)) and (sel[4:] == -1).all()


def test_sample_pixels_is_reproducible(idn, dev):
    ops = idn.ops
    m = torch.from_numpy(random_region_map(450, 450, seed=8)).to(dev)
    counts = ops.sample_counts(3072, 256, 0, 0.95)
    a = ops.sample_pixels(m, counts, 4, 17)
    b = ops.sample_pixels(m, counts, 4, 17)
    c = ops.sample_pixels(m, counts, 4, 18)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert len(set(a[:counts[0]].tolist())) == counts[0]


# ------------------------------------------------------------------------------------------------ gather_rays
@pytest.mark.parametrize("cxcy", [None, (30.25, 41.5)])
def test_gather_rays_bit_identical_to_loader(idn, dev, cxcy, monkeypatch):
    """Ray rows equal ops.frame_rays(...)[sel] bit for bit (frame centre and an off-centre principal point); target_s and
    bc_rgb equal dataset.sample_rays' for the same sel on images that hold all 256 byte values."""
    from idealnerf_amd import dataset, synthetic
    ops = idn.ops
    H, W = 48, 80
    rs = np.random.RandomState(2)
    pose = synthetic.frame(H, W, seed=4)["c2w"][:3, :4]
    img = ((np.arange(H * W * 3) * 37 + 11) % 256).astype(np.uint8).reshape(H, W, 3)
    bg = ((np.arange(H * W * 3) * 101 + 5) % 256).astype(np.uint8).reshape(H, W, 3)
    assert len(np.unique(img)) == 256 and len(np.unique(bg)) == 256
    sel_rc = np.stack([rs.randint(0, H, 500), rs.randint(0, W, 500)], 1).astype(np.int64)
    sel_rc[:4] = [[0, 0], [H - 1, W - 1], [0, W - 1], [H - 1, 0]]
    flat = torch.from_numpy(sel_rc[:, 0] * W + sel_rc[:, 1]).to(dev)
    cx, cy = (None, None) if cxcy is None else cxcy
    focal = 173.5
    rays, tgt, bc = ops.gather_rays(flat, pose, H, W, focal, torch.from_numpy(img).to(dev), torch.from_numpy(bg).to(dev), cx, cy)
    rec = ops.frame_rays(pose, H, W, focal, 0.0, 1.0, cx=cx, cy=cy, device=dev)
    assert torch.equal(rays[0], rec[flat, 0:3]) and torch.equal(rays[1], rec[flat, 3:6])
    # the loader's own arithmetic for the colours: GetData.__getitem__ / __init__ and dataset.sample_rays with this very sel
    monkeypatch.setattr(dataset, "select_pixels", lambda *a, **k: sel_rc)
    target = torch.tensor(img).to(dev).float() / 255.0
    bc_img = torch.tensor(bg / 255.0).to(dev)
    r2, t2, b2 = dataset.sample_rays(pose.numpy(), None, target, bc_img, None, None, H, W, focal, W / 2 if cx is None else cx,
                                     H / 2 if cy is None else cy, 500, 0, 0, 0.95, dev)
    assert torch.equal(rays, r2) and torch.equal(tgt, t2) and torch.equal(bc, b2.to(torch.float32))
    assert tgt.dtype == torch.float32 and bc.dtype == torch.float32
    # rows outside the frame read nothing and give zeros
    bad = torch.tensor([-1, H * W, 5], dtype=torch.int64, device=dev)
    r3, t3, b3 = ops.gather_rays(bad, pose, H, W, focal, torch.from_numpy(img).to(dev), torch.from_numpy(bg).to(dev), cx, cy)
    assert float(r3[:, :2].abs().max()) == 0.0 and float(t3[:2].abs().max()) == 0.0 and float(b3[:2].abs().max()) == 0.0
    assert torch.equal(r3[0, 2], rec[5, 0:3]) and torch.equal(r3[1, 2], rec[5, 3:6])


# ------------------------------------------------------------------------------------------------ ResidentFrames
@pytest.fixture(scope="module")
def clip450(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("clip450"))
    flags, meta = write_clip_directory(d, 450, 3, seed=1, N_rand=3072, mouth_rays=256, torso_rays=32)
    return d, flags, meta


def test_resident_frames_against_getdata(idn, dev, clip450, monkeypatch):
    """One generated 450 x 450 directory through both loaders: audio windows, pose, expression and index agree, and GetData's
    own select_pixels output fed through gather_rays reproduces GetData's (batch_rays, target_s, bc_rgb) bit for bit."""
    from idealnerf_amd import dataset
    d, flags, meta = clip450
    ds = dataset.GetData(d, "aud.npy", "train", flags, device=dev)
    fr = dataset.ResidentFrames(d, "aud.npy", "train", flags, device=dev, seed=5)
    assert len(fr) == len(ds) == 3 and (fr.H, fr.W, fr.focal, fr.cx, fr.cy) == (ds.H, ds.W, ds.focal, ds.cx, ds.cy)
    assert fr.maps.dtype == torch.uint8 and fr.imgs.shape == (3, 450, 450, 3) and fr.background.dtype == torch.uint8
    picked = []
    real = dataset.select_pixels
    monkeypatch.setattr(dataset, "select_pixels", lambda *a, **k: (picked.append(real(*a, **k)), picked[-1])[1])
    for i in (0, 2):
        np.random.seed(40 + i)
        g_rays, g_tgt, g_bc, g_auds, g_raw, g_pose, g_expr, g_index = ds[i]
        r_rays, r_tgt, r_bc, r_auds, r_raw, r_pose, r_expr, r_index = fr.batch(i, 3 + i)
        assert torch.equal(r_auds.cpu(), g_auds) and r_auds.is_cuda and r_index == g_index == i
        assert torch.equal(r_pose.cpu(), torch.as_tensor(g_pose, dtype=torch.float32)) and torch.equal(r_expr.cpu(), g_expr)
        assert torch.equal(r_raw.cpu(), g_raw) and r_raw.shape[1] == g_raw.shape[1]        # BGR bytes, and the shape forward reads
        for t in (r_rays, r_tgt, r_bc, r_pose, r_expr, r_raw):
            assert t.is_cuda
        assert r_rays.shape == (2, 3072, 3) and r_tgt.shape == (3072, 3) and r_bc.shape == (3072, 3)
        sel = picked[-1]
        flat = torch.from_numpy(sel[:, 0] * fr.W + sel[:, 1]).to(dev)
        rays, tgt, bc = idn.ops.gather_rays(flat, fr.all_poses[i], fr.H, fr.W, fr.focal, fr.imgs[i], fr.background, fr.cx, fr.cy)
        assert torch.equal(rays, g_rays) and torch.equal(tgt, g_tgt) and torch.equal(bc, g_bc.to(torch.float32))
        # the resident draw is the definition's on the frame's own byte map, and gathers the frame's own pixels
        lm = np.loadtxt(ds.all_landmarks[i])
        from PIL import Image
        m = dataset.region_byte_map(fr.H, fr.W, ds.all_face_rects[i], lm, np.asarray(Image.open(ds.all_parse_imgs[i])))
        assert np.array_equal(fr.maps[i].cpu().numpy(), m) and fr.populations[i].tolist() == _pops(m)
        want = torch.from_numpy(sampler_reference(m, fr.counts, 5, 3 + i)).to(dev)
        assert torch.equal(fr.select(i, 3 + i), want)
        w_rays, w_tgt, w_bc = idn.ops.gather_rays(want, fr.all_poses[i], fr.H, fr.W, fr.focal, fr.imgs[i], fr.background, fr.cx, fr.cy)
        assert torch.equal(r_rays, w_rays) and torch.equal(r_tgt, w_tgt) and torch.equal(r_bc, w_bc)


def test_batch_is_reproducible_and_does_not_synchronise(idn, dev, clip450):
    """Two calls with one (seed, draw) give identical bytes, consecutive draws differ; and the call neither synchronises
    nor copies to the host: it runs under torch's sync debug mode "error" (where the build honours that mode)."""
    from idealnerf_amd import dataset
    d, flags, _ = clip450
    fr = dataset.ResidentFrames(d, "aud.npy", "train", flags, device=dev, seed=9)
    a = fr.batch(1, 70)
    b = fr.batch(1, 70)
    c = fr.batch(1, 71)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            torch.ones(1, device=dev).item()
        except RuntimeError:
            honoured = True
        out = fr.batch(2, 5)            # raises here if anything inside waits for the device
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print(f"sync debug mode honoured by this build: {honoured}")
    assert torch.equal(out[0], fr.batch(2, 5)[0])


# ------------------------------------------------------------------------------------------------ the loop
def _state(run):
    net, opt, lat = run["network"], run["optimizer"], run["latent_codes"]
    st = {"w." + k: v.detach().clone() for k, v in net.state_dict().items()}
    st["latent"] = lat.detach().clone()
    osd = opt.state_dict()
    for i, s in osd["state"].items():
        for k, v in s.items():
            st[f"opt.{i}.{k}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    st["opt.lr"] = torch.tensor([g["lr"] for g in osd["param_groups"]], dtype=torch.float64)
    return st


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k


def test_train_loop_resume_checkpoint_validation_and_hand_loop(idn, dev, tmp_path):
    """64 x 64, N_rand 64, perturb 0, K = 4.  train() for 2 K steps == K steps, then new objects under another torch seed,
    then K resumed steps from head.tar, bit for bit (weights, latent codes, optimizer state); head.tar has the reference's four
    keys; the validation frame was rendered at step 0 (the one multiple of 100 * i_print in range) and only there; the loop's
    result equals a hand-written loop of train_step over frames.batch(i, step)."""
    from idealnerf_amd import dataset, train as T_
    from idealnerf_amd.audio_exp_nerf import Network, init_weights
    from idealnerf_amd.config import to_render_config
    d = str(tmp_path / "clip")
    os.makedirs(d)
    flags, _ = write_clip_directory(d, 64, 3, seed=2)
    K = 4
    mk = lambda name: train_flags(d, tmp_path / "logs", name, flags, perturb=0.0, i_print=2, i_weights=K - 1, N_iters=10, chunk=8192)

    events = []
    torch.manual_seed(11)
    whole = T_.train(mk("whole"), loader="resident", sample_seed=3, device=dev, steps=2 * K,
                     on_log=lambda kind, step, payload: events.append((kind, step, payload)))
    assert whole["global_step"] == 2 * K and whole["data_size"] == 3
    assert [s for k, s, _ in events if k == "train"] == [0, 2, 4, 6]
    assert [s for k, s, _ in events if k == "val"] == [0]
    val = [p for k, _, p in events if k == "val"][0]
    assert val.shape == (3, 128, 64) and torch.isfinite(val).all() and not val.is_cuda
    assert all(np.isfinite(list(p.values())).all() for k, _, p in events if k == "train")
    ck = torch.load(str(tmp_path / "logs" / "whole" / "head.tar"), weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer", "latent_codes"} and ck["global_step"] == 7
    assert os.path.exists(str(tmp_path / "logs" / "whole" / "args.txt"))

    torch.manual_seed(11)
    first = T_.train(mk("parts"), loader="resident", sample_seed=3, device=dev, steps=K)
    assert first["global_step"] == K
    assert torch.load(str(tmp_path / "logs" / "parts" / "head.tar"), weights_only=False)["global_step"] == K
    del first
    torch.manual_seed(999)                       # nothing of the second half may come from anywhere but head.tar
    events2 = []
    second = T_.train(mk("parts"), loader="resident", sample_seed=3, device=dev, steps=K,
                      on_log=lambda kind, step, payload: events2.append((kind, step)))
    assert second["global_step"] == 2 * K and events2 == [("train", 4), ("train", 6)]
    _assert_same_state(_state(whole), _state(second))

    # the same 2 K steps written by hand
    args = mk("hand")
    torch.manual_seed(11)
    frames = dataset.ResidentFrames(d, "aud.npy", "train", args, device=dev, seed=3)
    net = Network(64, 64, frames.focal, near=args.near, far=args.far, chunk=args.chunk, intrinsic=None, N_samlpes=args.N_samples,
                  N_importance=args.N_importance, args=to_render_config(args)).to(dev)
    lat = torch.ones(len(frames), 32, dtype=torch.float32, device=dev)
    net.apply(init_weights)
    lat.requires_grad = True
    opt = T_.make_optimizer(net, lat, args.lrate)
    net.train()
    for step in range(2 * K):
        T_.train_step(net, opt, frames.batch(step % len(frames), step), lat, step, len(frames), lrate=args.lrate,
                      lrate_decay=args.lrate_decay)
    _assert_same_state(_state(whole), _state(dict(network=net, optimizer=opt, latent_codes=lat)))

    # the reference loader drives the same loop (upstream's numpy draw sequence): it runs, and draws other pixels
    np.random.seed(0)
    torch.manual_seed(11)
    ref = T_.train(mk("ref"), loader="reference", device=dev, steps=2)
    assert ref["global_step"] == 2
    with pytest.raises(ValueError):
        T_.train(mk("ref"), loader="nope", device=dev, steps=1)


LEARN_STEPS, LEARN_SEEDS, LEARN_FACTOR = 240, (0, 1, 2), 2.0


def test_resident_loader_learns_as_well_as_the_reference_loader(idn, dev, tmp_path):
    """Frames of one flat colour inside the face rect over another background; three frames train, two more are held out.
    From the same initial weights, LEARN_STEPS steps with each loader over three sampling seeds; PSNR of the held-out full
    frame.  The resident loader's mean PSNR must not be below the reference loader's mean by more than the margin:
    LEARN_FACTOR = 2 times the spread (max - min) of the reference loader's own three results -- the loaders differ in which
    pixels a step sees, exactly as two sampling seeds of one loader do, so the reference's seed-to-seed spread is the scale of
    that difference; 2 because the range of three results underestimates the range of six about that often.
    All six numbers are printed, and written to $IDN_TRAIN_LOOP_RECORD when that is set (profiles/train_loop.json)."""
    from idealnerf_amd import train as T_
    d = str(tmp_path / "flat")
    os.makedirs(d)
    flags, meta = write_clip_directory(d, 64, 5, seed=6, flat=True, N_rand=256, mouth_rays=16, torso_rays=0)
    held = dict(meta, frames=meta["frames"][3:])
    json.dump(dict(meta, frames=meta["frames"][:3]), open(os.path.join(d, "transforms_exp_train.json"), "w"))
    json.dump(held, open(os.path.join(d, "transforms_exp_val.json"), "w"))

    def run(loader, seed):
        args = train_flags(d, tmp_path / "logs", f"{loader}{seed}", flags, perturb=0.0, i_print=10 ** 6, i_weights=10 ** 6, N_iters=10 ** 4,
                           chunk=8192)
        np.random.seed(seed)                     # the reference loader's sampling seed
        torch.manual_seed(0)                     # the same initial weights everywhere
        out = T_.train(args, loader=loader, sample_seed=seed, device=dev, steps=LEARN_STEPS)
        from idealnerf_amd import dataset
        val = dataset.GetData(d, "aud.npy", "val", args, skip=1, device=dev)
        img = T_.validation_frame(out["network"], val, out["latent_codes"], 0)
        pred, label = img[:, :64], img[:, 64:]
        flat_guess = float(-10.0 * torch.log10(torch.mean((label - label.mean(dim=(1, 2), keepdim=True)) ** 2)))
        return float(-10.0 * torch.log10(torch.mean((pred - label) ** 2))), flat_guess

    ref, res, floor = [], [], None
    for loader, into in (("reference", ref), ("resident", res)):
        for s in LEARN_SEEDS:
            psnr, floor = run(loader, s)
            into.append(psnr)
    margin = LEARN_FACTOR * (max(ref) - min(ref))
    record = dict(steps=LEARN_STEPS, seeds=list(LEARN_SEEDS), psnr_reference=ref, psnr_resident=res, factor=LEARN_FACTOR, margin=margin,
                  psnr_best_single_colour=floor)
    print("held-out PSNR:", json.dumps(record))
    if os.environ.get("IDN_TRAIN_LOOP_RECORD"):
        json.dump(record, open(os.environ["IDN_TRAIN_LOOP_RECORD"], "w"))
    # learning at all: better than the best image of ONE colour (the frame's mean), which knows nothing of the two regions
    assert min(ref + res) > floor, record
    assert np.mean(res) >= np.mean(ref) - margin, record
