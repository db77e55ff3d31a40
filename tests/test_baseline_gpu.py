"""The AD-NeRF baseline model (head_baseline.Network: audio only, C = 127, no expression and no latent code) on the GPU:
gradients through ``Network.render_rays`` against one training step of the reference itself and against the oracle's autograd,
the eval forward in both audio branches against the reference's, the resident loader, the training loop, an AD-NeRF checkpoint
rendered as what it is, and whole clips."""
import json
import os

import numpy as np
import pytest
import torch

import oracle
import baseline_common as bc_
import test_hip_parity as hp
from idealnerf_amd.synthetic import write_clip_directory
from train_loop_common import sampler_reference, train_flags

pytestmark = pytest.mark.gpu

NEAR, FAR = bc_.NEAR, bc_.FAR
PAIR = ("face_nerf_coarse", "face_nerf_fine")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()
    return idealnerf_amd


# ------------------------------------------------------------------------------------------------ gradients
def test_baseline_train_step_gradients_golden(idn, dev, golden):
    """One training step of the reference's own baseline Network (tests/golden/baseline_train_step.npz,
    make_golden_baseline.py) at exactly test_agg_train_step_gradients_golden's bounds: RGB hp.RGB_TOL (1e-4), loss 1e-5
    relative, every gradient 2e-3 of its tensor's largest entry -- g_aud and agg_train_step.npz's tensor selection without
    the agg_linears (every second row of the weight gradients with 128 rows or more, as the fixture stores them)."""
    from idealnerf_amd.helper import img2mse
    g, f = golden("baseline_train_step"), golden("frame32")
    net, syn = bc_.baseline_network(dev, seeds=(int(g["seed_coarse"]), int(g["seed_fine"])))
    sel = hp.T(g["sel"])
    rays = hp.T(f["rays"])[sel].contiguous().to(dev)
    bc = syn["bc"].reshape(-1, 3)[sel].contiguous().to(dev)
    aud = syn["aud"].to(dev).requires_grad_(True)
    tgt = hp.T(g["target"]).to(dev)
    ret = net.render_rays(rays, bc, aud)
    e_rgb, e_rgb0 = hp.rel_err(ret["rgb_map"], g["rgb_map"]), hp.rel_err(ret["rgb0"], g["rgb0"])
    loss = img2mse(ret["rgb_map"], tgt) + img2mse(ret["rgb0"], tgt)
    loss.backward()
    e_loss = abs(float(loss.detach()) - float(g["loss"])) / abs(float(g["loss"]))
    errs = {"aud": hp.rel_err(aud.grad, g["g_aud"])}
    for tag, m in (("c", net.face_nerf_coarse), ("f", net.face_nerf_fine)):
        named = dict(m.named_parameters())
        for key in g:
            if key.startswith(f"g_{tag}_"):
                grad = named[key[4:]].grad
                rows = grad[::int(g["row_step"])] if grad.dim() == 2 and grad.shape[0] >= 128 else grad   # as the fixture stores them
                errs[f"{tag}.{key[4:]}"] = hp.rel_err(rows, g[key])
        assert named["feature_linear.weight"].grad is None
    assert len(errs) == 21
    print(f"\nrgb {e_rgb:.1e} rgb0 {e_rgb0:.1e} loss {e_loss:.1e}; gradient errors (max abs / max |ref|):",
          {k: f"{v:.1e}" for k, v in errs.items()})
    assert e_rgb < hp.RGB_TOL and e_rgb0 < hp.RGB_TOL and e_loss < 1e-5
    bad = {k: v for k, v in errs.items() if not v < 2e-3}
    assert not bad, bad


@pytest.mark.parametrize("n_rays,ni", [(64, 128), (37, 128), (64, 0), (37, 0)])
def test_baseline_render_step_gradients_match_oracle_autograd(idn, dev, n_rays, ni):
    """test_agg_render_step_gradients_match_oracle_autograd for the baseline pair: 64 rays and 37 rays (a partial 32-point
    tile), each with 64 + 128 samples and with N_importance = 0, against oracle.render_rays' autograd with neither expression
    nor latent code.  That test's bounds: loss 1e-5 relative; GRAD_L2_COARSE / GRAD_L2_FINE / GRAD_MAX for the 24 tensors of
    each network (hp.check_grads); GRAD_L2_FINE for d aud; feature_linear gets none.  The smallest place where "no expression,
    no latent, d latent never requested" can go wrong in the fold and its backward."""
    from idealnerf_amd.helper import img2mse
    net, syn = bc_.baseline_network(dev, ni)
    rays, bc, tgt = bc_.pick_rays(syn, n_rays, n_rays)
    pc = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in net.face_nerf_coarse.state_dict().items()}
    pf = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in net.face_nerf_fine.state_dict().items()}
    aud_o = syn["aud"].clone().requires_grad_(True)
    out_o = oracle.render_rays(rays, bc, pc, pf if ni else None, aud_o, None, None, n_importance=ni, dims=bc_.DIMS)
    loss_o = torch.nn.functional.mse_loss(out_o["rgb_map"], tgt)
    if ni:
        loss_o = loss_o + torch.nn.functional.mse_loss(out_o["rgb0"], tgt)
    loss_o.backward()
    aud = syn["aud"].to(dev).requires_grad_(True)
    ret = net.render_rays(rays.to(dev), bc.to(dev), aud)
    assert ("rgb0" in ret) == bool(ni)
    loss = img2mse(ret["rgb_map"], tgt.to(dev))
    if ni:
        loss = loss + img2mse(ret["rgb0"], tgt.to(dev))
    loss.backward()
    e_loss = abs(float(loss.detach()) - float(loss_o.detach())) / abs(float(loss_o.detach()))
    e_aud = hp.l2_err(aud.grad, aud_o.grad)
    print(f"\nn_rays {n_rays} Ni {ni}: loss {e_loss:.2e}  d aud {e_aud:.2e}")
    assert e_loss < 1e-5
    assert e_aud < hp.GRAD_L2_FINE
    for module, ref, fine in ((net.face_nerf_coarse, pc, False), (net.face_nerf_fine, pf, True)):
        named = list(module.named_parameters())
        if fine and not ni:
            assert all(p.grad is None for _, p in named)
            continue
        assert dict(named)["pts_linears.0.weight"].grad.shape == (256, 127)
        hp.check_grads(named, ref, fine, n_rays)
        assert dict(named)["feature_linear.weight"].grad is None and dict(named)["feature_linear.bias"].grad is None


# ------------------------------------------------------------------------------------------------ the eval forward
def test_baseline_forward_golden(idn, dev, golden):
    """The reference's eval ``forward`` (head_baseline.py:198-242; tests/golden/baseline_forward.npz) on the 32 x 32 frame of a
    10-frame clip, in both audio branches: ``aud_net(auds[index])`` one step before ``nosmo_iters``, and at it the smoothed
    window at both ends of the clip (four zero-padded slots on the left, three on the right).  The audio feature handed to the
    renderer and the rendered frame at test_forward_smoother_golden's bounds: feature rtol 2e-5 / atol 2e-6, rgb0 hp.RGB_TOL,
    and for rgb the end-to-end guards of tests/parity_proof.py that test states for its 144 rays -- no ray beyond E2E_CAP
    (1e-3), and at most max(3, BEYOND_SHARE = 3 % of the rays) beyond hp.RGB_TOL -- here for the 1 024 rays of a 32 x 32 frame:
    at most 30.  (The scene is sharp, density gain 300 on a volume 92 % / 74 % occupied: a last-ulp difference of a coarse weight
    moves an importance sample.  Measured: rgb: 12, 6 and 8 of 1 024 rays beyond 1e-4 in the three cases, max 4.3e-4.)"""
    from idealnerf_amd.head_baseline import Network
    from parity_proof import BEYOND_SHARE, E2E_CAP
    g = golden("baseline_forward")
    net = Network(32, 32, float(g["focal"]), NEAR, FAR, 512, None, 64, 128,
                  args=bc_.render_config(nosmo_iters=int(g["nosmo_iters"]), smo_size=int(g["smo_size"])))
    net.face_nerf_coarse.load_state_dict(bc_.baseline_state(int(g["seed_coarse"])))
    net.face_nerf_fine.load_state_dict(bc_.baseline_state(int(g["seed_fine"])))
    net.aud_net.load_state_dict({k[len("audnet."):]: hp.T(v) for k, v in g.items() if k.startswith("audnet.")})
    net.aud_att_net.load_state_dict({k[len("attnet."):]: hp.T(v) for k, v in g.items() if k.startswith("attnet.")})
    net = net.to(dev).eval()
    real, seen = net.render_dynamic_face, {}

    def spy(*a, **k):
        seen["aud"] = k["aud_para"].detach().clone()
        return real(*a, **k)

    net.render_dynamic_face = spy
    assert [int(s) - int(g["nosmo_iters"]) for s, _ in g["cases"]] == [-1, 0, 0] and [int(i) for _, i in g["cases"]] == [9, 0, 9]
    for c, (step, idx) in enumerate(g["cases"]):
        with torch.no_grad():
            rgb, disp, acc, last_w, extras = net([bc_.forward_data(g, idx), int(step), 10])
        np.testing.assert_allclose(seen["aud"].cpu().numpy(), g[f"aud_feature_{c}"], rtol=2e-5, atol=2e-6, err_msg=f"case {c}")
        assert rgb.shape == (32, 32, 3) and last_w.shape == (32, 32)
        assert hp.rel_err(extras["rgb0"], g[f"rgb0_{c}"]) < hp.RGB_TOL, c     # nothing is sampled before the coarse composite
        e = np.abs(rgb.cpu().numpy().astype(np.float64) - g[f"rgb_{c}"]).reshape(-1, 3).max(1) / np.abs(g[f"rgb_{c}"]).max()
        print(f"\n  baseline forward case {c} (step {int(step)}, frame {int(idx)}): rgb vs the reference max {e.max():.2e}, "
              f"{int((e > hp.RGB_TOL).sum())} of {e.size} rays beyond 1e-4")
        assert e.max() < E2E_CAP and (e > hp.RGB_TOL).sum() <= max(3, BEYOND_SHARE * e.size)


def test_adnerf_checkpoint_renders_like_the_oracle(idn, dev, tmp_path):
    """An AD-NeRF four-dict file built from seeds, read in full by checkpoint.load_adnerf into a fresh head_baseline.Network
    (other weights, stale packed streams): every tensor of the four dicts arrives, and 256 rays of a 32 x 32 frame rendered
    from the loaded weights are held to the CPU oracle on the file's own dicts with parity_proof's fixed budgets (coarse
    weights 1e-5, sampling stage exact, fine pass 1e-4 -- hp.prove_render) and rgb0 to hp.RGB_TOL."""
    from idealnerf_amd import checkpoint
    from idealnerf_amd.head_baseline import Network, init_weights
    ck = bc_.adnerf_checkpoint()
    path = str(tmp_path / "adnerf.tar")
    torch.save(ck, path)
    torch.manual_seed(9)
    net = Network(32, 32, 100.0, NEAR, FAR, 512, None, 64, 128, args=bc_.render_config())
    net.apply(init_weights)
    net = net.to(dev).eval()
    with torch.no_grad():
        net.face_nerf_fine.packed_weights()          # streams of the initialisation: must not survive the load
    assert checkpoint.load_adnerf(path, net, map_location=dev) == 400000
    after = net.state_dict()
    for key, pre in (("network_fn_state_dict", "face_nerf_coarse."), ("network_fine_state_dict", "face_nerf_fine."),
                     ("network_audnet_state_dict", "aud_net."), ("network_audattnet_state_dict", "aud_att_net.")):
        for k, v in ck[key].items():
            assert torch.equal(after[pre + k].cpu(), v), pre + k
    syn = oracle.synthetic_frame(32, 32, seed=5, dims=bc_.DIMS)
    pc, pf = ck["network_fn_state_dict"], ck["network_fine_state_dict"]
    n_rays = 256
    rays = idn.ops.frame_rays(syn["c2w"][:3, :4], 32, 32, syn["focal"], NEAR, FAR, device=dev)[:n_rays].contiguous()
    bc = syn["bc"].to(dev).reshape(-1, 3)[:n_rays].contiguous()
    with torch.no_grad():
        out = net.render_rays(rays, bc, syn["aud"].to(dev), taps=True)
        ff = net.face_nerf_fine.folded_bias(syn["aud"].to(dev), None, None)
        ref = oracle.render_rays(rays.cpu(), bc.cpu(), pc, pf, syn["aud"], None, None, n_samples=64, n_importance=128, dims=bc_.DIMS,
                                 taps=True)
    assert float((ref["rgb_map"] - bc.cpu()).abs().mean()) > 0.02, "the volume must hide part of the background"
    hp.prove_render(idn, "network loaded from an AD-NeRF checkpoint", out, ref, net.face_nerf_fine.packed_weights(), ff, rays, bc,
                    lambda z: hp.oracle_fine_pass(pf, bc_.DIMS, rays, bc, syn["aud"], None, None, z), 1e-3,
                    precision_fine=net.face_nerf_fine.prec_code)
    assert hp.rel_err(out["rgb0"], ref["rgb0"]) < hp.RGB_TOL


# ------------------------------------------------------------------------------------------------ the loop
K = 4


@pytest.fixture(scope="module")
def flat_clip(tmp_path_factory):
    """The flat two-colour 64 x 64 clip the head loop's learning test uses (5 frames, seed 6; three frames train, two are held
    out) as an AD-NeRF dataset: no parsing/, no exp."""
    import shutil
    tmp = tmp_path_factory.mktemp("baseline_loop")
    d = str(tmp / "flat")
    os.makedirs(d)
    flags, meta = write_clip_directory(d, 64, 5, seed=6, flat=True, N_rand=64)
    shutil.rmtree(os.path.join(d, "parsing"))
    for f in meta["frames"]:
        del f["exp"]
    json.dump(dict(meta, frames=meta["frames"][:3]), open(os.path.join(d, "transforms_exp_train.json"), "w"))
    json.dump(dict(meta, frames=meta["frames"][3:]), open(os.path.join(d, "transforms_exp_val.json"), "w"))
    return tmp, d, flags, meta


def test_resident_baseline_frames_against_baseline_getdata(idn, dev, flat_clip, monkeypatch):
    """The resident loader's batches against BaselineGetData on one directory: its draw is the sampler's definition on the
    baseline's byte map (bits 0 / 1 as torso_region_byte_map's, counts rect / outside / mouth / torso = 60 / 4 / 0 / 0), and
    BaselineGetData fed those very pixels returns the same 7-tuple bit for bit; frame() is the eval 7-tuple."""
    from idealnerf_amd import dataset
    tmp, d, flags, meta = flat_clip
    ds = dataset.BaselineGetData(d, "aud.npy", "train", flags, device=dev)
    fr = dataset.ResidentBaselineFrames(d, "aud.npy", "train", flags, device=dev, seed=5)
    assert len(fr) == len(ds) == 3 and fr.counts == (60, 4, 0, 0) and fr.exprs is None
    for i in (0, 2):
        lm = np.loadtxt(ds.all_landmarks[i])
        m = dataset.baseline_region_byte_map(64, 64, ds.all_face_rects[i], lm)
        assert np.array_equal(fr.maps[i].cpu().numpy(), m)
        assert np.array_equal(m & 3, dataset.torso_region_byte_map(64, 64, ds.all_face_rects[i], lm) & 3) and not (m & 8).any()
        coords, mouth_w, rect_w = dataset._box_masks(64, 64, ds.all_face_rects[i], lm)
        assert fr.populations[i].tolist() == [int((rect_w & ~mouth_w).sum()), int((~rect_w).sum()), int(mouth_w.sum()), 0]
        sel = fr.select(i, 3 + i)
        assert torch.equal(sel, torch.from_numpy(sampler_reference(m, fr.counts, 5, 3 + i)).to(dev))
        flat = sel.cpu().numpy()
        monkeypatch.setattr(dataset, "baseline_select_pixels", lambda *a, **k: np.stack([flat // fr.W, flat % fr.W], 1))
        g_item, r_item = ds[i], fr.batch(i, 3 + i)
        assert len(g_item) == len(r_item) == 7
        g_rays, g_tgt, g_bc, g_auds, g_raw, g_pose, g_index = g_item
        r_rays, r_tgt, r_bc, r_auds, r_raw, r_pose, r_index = r_item
        assert r_rays.shape == (2, 64, 3) and torch.equal(r_rays, g_rays)
        assert torch.equal(r_tgt, g_tgt) and torch.equal(r_bc, g_bc.to(torch.float32))
        assert torch.equal(r_auds.cpu(), g_auds) and r_index == g_index == i
        assert torch.equal(r_pose.cpu(), torch.as_tensor(g_pose, dtype=torch.float32)) and torch.equal(r_raw.cpu(), g_raw)   # RGB bytes
        assert all(t.is_cuda for t in (r_rays, r_tgt, r_bc, r_auds, r_raw, r_pose))
    ev = fr.frame(1)
    assert len(ev) == 7 and ev[0].numel() == 0 and not ev[5].is_cuda and ev[5].dtype == torch.float64 and ev[2].dtype == torch.float64
    assert ev[6] == 1 and torch.equal(ev[4], fr.imgs[1])


def _state(run):
    net, opt = run["network"], run["optimizer"]
    st = {"w." + k: v.detach().clone() for k, v in net.state_dict().items()}
    osd = opt.state_dict()
    for i, s in osd["state"].items():
        for k, v in s.items():
            st[f"opt.{i}.{k}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    st["opt.lr"] = torch.tensor([g["lr"] for g in osd["param_groups"]], dtype=torch.float64)
    return st


def test_baseline_train_resume_validation_and_learning(idn, dev, flat_clip):
    """train_baseline.train on the flat clip at N_rand 64, perturb 0, resident loader.  2 K steps == K steps, then new objects
    under another torch seed and K steps resumed from {epoch:06d}_head.tar, bit for bit (weights, optimizer state); the
    checkpoints carry the baseline's three keys, upstream's module. prefix and the completed step count; Adam holds the
    network's parameters and nothing else; the validation image is RGB over RGB: its lower half is the held-out frame's bytes
    / 255 unflipped.  Then 240 steps: the mean loss of the last ten steps is below that of the first ten."""
    from PIL import Image
    from idealnerf_amd import checkpoint, train_baseline
    from idealnerf_amd.head_baseline import Network
    from test_train_loop_gpu import _assert_same_state
    tmp, d, flags, meta = flat_clip
    mk = lambda name, **over: train_flags(d, tmp / "logs", name, flags, **{**dict(perturb=0.0, i_print=2, i_weights=K - 1, N_iters=10,
                                                                                 chunk=8192), **over})
    events = []
    torch.manual_seed(11)
    whole = train_baseline.train(mk("whole"), loader="resident", sample_seed=3, device=dev, steps=2 * K,
                                 on_log=lambda kind, step, payload: events.append((kind, step, payload)))
    assert isinstance(whole["network"], Network) and whole["global_step"] == 2 * K and whole["data_size"] == 3
    assert whole["latent_codes"] is None
    n_params = sum(1 for _ in whole["network"].parameters())
    assert sum(len(g["params"]) for g in whole["optimizer"].param_groups) == n_params
    assert [s for k, s, _ in events if k == "train"] == [0, 2, 4, 6] and [s for k, s, _ in events if k == "val"] == [0]
    assert set([p for k, _, p in events if k == "train"][0]) == {"loss", "psnr", "learning_rate"}
    run_dir = str(tmp / "logs" / "whole")
    assert sorted(f for f in os.listdir(run_dir) if f.endswith(".tar")) == ["000000_head.tar", "000001_head.tar", "000002_head.tar"]
    ck = torch.load(os.path.join(run_dir, "000002_head.tar"), weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer"} and ck["global_step"] == 7
    assert all(k.startswith("module.") for k in ck["model_state_dict"])
    assert tuple(ck["model_state_dict"]["module.face_nerf_coarse.pts_linears.0.weight"].shape) == (256, 127)
    assert not any("ds_aud_net" in k for k in ck["model_state_dict"])
    val = [p for k, _, p in events if k == "val"][0]
    assert val.shape == (3, 128, 64) and torch.isfinite(val).all() and not val.is_cuda
    held = [torch.from_numpy(np.asarray(Image.open(os.path.join(d, "head_imgs", f"{f['img_id']}.jpg"))).copy()).permute(2, 0, 1) / 255.0
            for f in meta["frames"][3:]]
    assert any(torch.equal(val[:, 64:], h) for h in held)                       # RGB over RGB: no channel flip
    assert not any(torch.equal(val[:, 64:], h[[2, 1, 0]]) for h in held)

    torch.manual_seed(11)
    first = train_baseline.train(mk("parts"), loader="resident", sample_seed=3, device=dev, steps=K)
    assert first["global_step"] == K
    assert checkpoint.latest_checkpoint(str(tmp / "logs" / "parts")).endswith("000001_head.tar")
    del first
    torch.manual_seed(999)                       # nothing of the second half may come from anywhere but the checkpoint
    second = train_baseline.train(mk("parts"), loader="resident", sample_seed=3, device=dev, steps=K)
    assert second["global_step"] == 2 * K
    _assert_same_state(_state(whole), _state(second))

    # the reference loader drives the same loop (upstream's numpy draw sequence), with the resident validation clip
    np.random.seed(0)
    torch.manual_seed(11)
    ev2 = []
    ref = train_baseline.train(mk("ref"), loader="reference", device=dev, steps=2, val="resident",
                               on_log=lambda kind, step, payload: ev2.append(kind))
    assert ref["global_step"] == 2 and ev2 == ["train", "val", "val_scores"]

    # a model trained here is a valid ft_path: the AD-NeRF form of the run, read whole, starts a run at step 0 with its weights
    ft = str(tmp / "whole_adnerf.tar")
    checkpoint.save_adnerf(ft, whole["network"], whole["global_step"])
    warm = train_baseline.train(mk("warm", ft_path=ft, lrate=0.0), loader="resident", sample_seed=3, device=dev, steps=1)
    sd_w, sd_0 = warm["network"].state_dict(), whole["network"].state_dict()
    assert warm["global_step"] == 1 and all(torch.equal(sd_w[k], sd_0[k]) for k in sd_0)

    losses = []
    torch.manual_seed(0)
    train_baseline.train(mk("learn", i_print=10 ** 6, i_weights=10 ** 6, N_iters=10 ** 4), loader="resident", sample_seed=0,
                         device=dev, steps=240, on_step=lambda step, info: losses.append(info["loss"]))
    losses = torch.stack(losses).cpu()
    first10, last10 = float(losses[:10].mean()), float(losses[-10:].mean())
    print(f"\nbaseline loop, 240 steps: mean loss of the first ten steps {first10:.5f}, of the last ten {last10:.5f}")
    assert torch.isfinite(losses).all() and last10 < first10


# ------------------------------------------------------------------------------------------------ clips
def test_drive_baseline_clip_and_scores(idn, dev, tmp_path, monkeypatch):
    """A 3-frame 40 x 40 clip (tests/drive_common.py's shape and sample counts) as an AD-NeRF dataset.  drive.drive_baseline on
    an AD-NeRF ft_path: the AVI and the still exist under upstream's names, and the clip's frames equal ``Network.forward``'s
    at global step 0 with the audio row taken by position, converted by ``ops.to8b`` with red and blue exchanged (upstream's
    cvtColor: the swapped bytes go to both writers, so the still holds them as RGB).  Without ft_path the newest *tar of the
    run directory is rendered.  clip.score_head_clip(model="baseline") returns finite values for every group the baseline's
    byte map populates (frame, rect, outside, mouth; there is no parsing, so the torso group has no pixel)."""
    import shutil
    import drive_common as dc
    from PIL import Image
    from idealnerf_amd import checkpoint, clip, config, dataset, drive, synthetic
    from idealnerf_amd.head_baseline import Network, init_weights
    root = tmp_path / "dataset" / "Toy"
    os.makedirs(root)
    d = str(root)
    flags, meta = write_clip_directory(d, dc.SIZE, 3, seed=dc.SEED, face_rect=[1, 1, 24, 24], mouth_range=(36, 39))
    shutil.rmtree(os.path.join(d, "parsing"))
    for f in meta["frames"]:
        del f["exp"]
    for mode in ("train", "val"):
        json.dump(meta, open(os.path.join(d, f"transforms_exp_{mode}.json"), "w"))
    cfg = bc_.render_config(dc.N_IMPORTANCE, chunk=8192, near=synthetic.NEAR, far=synthetic.FAR, N_samples=dc.N_SAMPLES)
    torch.manual_seed(5)
    net = Network(dc.SIZE, dc.SIZE, meta["focal_len"], cfg.near, cfg.far, cfg.chunk, None, dc.N_SAMPLES, dc.N_IMPORTANCE, args=cfg)
    net.apply(init_weights)
    synthetic.xavier_state_dict(net.face_nerf_coarse, 2, 300.0, 0.3)
    synthetic.xavier_state_dict(net.face_nerf_fine, 3, 300.0, 0.3)
    net = net.to(dev).eval()
    ft = str(tmp_path / "adnerf.tar")
    checkpoint.save_adnerf(ft, net, 400000)
    argv = ["--datadir", d, "--basedir", str(tmp_path / "logs"), "--expname", "run", "--save_path", str(tmp_path / "out"),
            "--testskip", "1", "--N_samples", str(dc.N_SAMPLES), "--N_importance", str(dc.N_IMPORTANCE), "--perturb", "0",
            "--chunk", "8192", "--near", repr(synthetic.NEAR), "--far", repr(synthetic.FAR), "--dim_aud", "64", "--aud_file", "aud.npy"]
    ns = config.load_config(argv=argv + ["--ft_path", ft])
    monkeypatch.chdir(tmp_path)                          # upstream's names cut the first eight characters off datadir
    ns.datadir = os.path.join("dataset", "Toy")
    res = drive.drive_baseline(ns, device=dev, codec="raw")
    out = tmp_path / "out"
    assert res["n_frames"] == 3 and res["nonfinite_frames"] == [] and res["path"] == str(out / "V_Toy_aud_N_baseline.avi")
    assert sorted(os.listdir(out)) == ["Toy_aud_ADNeRF_0.jpg", "V_Toy_aud_N_baseline.avi"]
    _, frames = dc.decode_raw(res["path"])
    assert len(frames) == 3
    track = dataset.BaselineTestFrames(d, "aud.npy", "val", ns, skip=1, device=dev)
    aud = np.load(os.path.join(d, "aud.npy"))
    with torch.no_grad():
        for j in range(3):
            item = track[j]
            assert torch.equal(item[3][j], torch.from_numpy(aud[j]))                      # audio by position, not by aud_id
            x = tuple(t[None] if torch.is_tensor(t) else torch.as_tensor(t)[None] for t in item)
            rgb = net([x, 0, track.data_size])[0]
            assert np.array_equal(idn.ops.to8b(rgb, True).cpu().numpy(), frames[j]), j
            if j == 0:
                still = np.asarray(Image.open(out / "Toy_aud_ADNeRF_0.jpg")).astype(np.int32)
                assert still.shape == (dc.SIZE, dc.SIZE, 3)
                assert np.abs(still - frames[0].astype(np.int32)).mean() < 6.0            # the swapped bytes taken as RGB (JPEG, quality 75)
                assert np.abs(still - frames[0][..., ::-1].astype(np.int32)).mean() > np.abs(still - frames[0].astype(np.int32)).mean()

    # without ft_path: the newest *tar of the run directory (natural order), in the baseline's run-file form
    other = Network(dc.SIZE, dc.SIZE, meta["focal_len"], cfg.near, cfg.far, cfg.chunk, None, dc.N_SAMPLES, dc.N_IMPORTANCE, args=cfg)
    other.apply(init_weights)
    run = tmp_path / "logs" / "run"
    checkpoint.save_baseline_checkpoint(str(run / "000002_head.tar"), other, None, 3)
    checkpoint.save_baseline_checkpoint(str(run / "000010_head.tar"), net, None, 11)
    ns2 = config.load_config(argv=argv)
    driven = str(tmp_path / "driven.avi")
    res2 = drive.drive_baseline(ns2, out=driven, device=dev, codec="raw", still_every=0)
    _, frames2 = dc.decode_raw(driven)
    assert res2["n_frames"] == 3 and all(np.array_equal(a, b) for a, b in zip(frames, frames2))

    fr = dataset.ResidentBaselineFrames(d, "aud.npy", "val", flags, device=dev)
    scores = clip.score_head_clip(net, fr, 0, latent_code=None, frame_ids=range(3), model="baseline")
    psnr, ssim = np.asarray(scores["per_frame"]["psnr"]), np.asarray(scores["per_frame"]["ssim"])
    assert psnr.shape == (3, 5) and np.isfinite(psnr[:, :4]).all() and np.isfinite(ssim[:, :4]).all()
    assert np.isfinite(np.asarray(scores["mean"]["psnr"])[:4]).all() and np.isfinite(np.asarray(scores["mean"]["ssim"])[:4]).all()
    assert np.isnan(psnr[:, 4]).all()                                                     # torso: no parsing, no pixel
