"""The AD-NeRF baseline model (head_baseline: audio only, no expression, no latent code) off the GPU: its state dict against the
reference's, the host-side loader against the reference's own draws, the oracle's C = 127 training step against the reference's,
the four shipped configurations, both checkpoint forms, the test-time flow's names and audio rule, and the resident loader's
construction errors."""
import json
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle
import baseline_common as bc_
from idealnerf_amd.synthetic import write_clip_directory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _network(n_importance=128):
    from idealnerf_amd.head_baseline import Network
    return Network(32, 32, 100.0, bc_.NEAR, bc_.FAR, 512, None, 64, n_importance, args=bc_.render_config(n_importance))


def test_state_dict_is_the_reference_networks(golden):
    """Keys, their order and shapes of head_baseline.Network's state dict equal the reference Network's
    (tests/golden/baseline_train_step.npz holds them): pts_linears.0 [256, 127], pts_linears.5 [256, 383], views_linears.0
    [128, 283], the two audio nets, and no ds_aud_net."""
    from idealnerf_amd.agg_aud_exp_nerf import HEAD_MODELS, head_network_class
    from idealnerf_amd.head_baseline import Network
    g = golden("baseline_train_step")
    sd = _network().state_dict()
    assert list(sd) == [str(k) for k in g["state_keys"]]
    for (k, v), shape, nd in zip(sd.items(), g["state_shapes"], g["state_ndim"]):
        assert tuple(v.shape) == tuple(int(x) for x in shape[:int(nd)]), k
    assert tuple(sd["face_nerf_coarse.pts_linears.0.weight"].shape) == (256, 127)
    assert tuple(sd["face_nerf_fine.pts_linears.5.weight"].shape) == (256, 383)
    assert tuple(sd["face_nerf_fine.views_linears.0.weight"].shape) == (128, 283)
    assert not any(k.startswith("ds_aud_net") for k in sd) and any(k.startswith("aud_att_net.") for k in sd)
    assert "baseline" in HEAD_MODELS and head_network_class("baseline") is Network
    with pytest.raises(ValueError):
        head_network_class("adnerf")


def _cpu_frame_rays(pose, H, W, focal, near, far, row0=0, nrows=None, cx=None, cy=None, device=None):
    """ops.frame_rays restated with the oracle: no GPU in this file."""
    ro, rd = oracle.camera_rays(H, W, focal, torch.as_tensor(pose, dtype=torch.float32), cx, cy)
    return oracle.ray_records(ro, rd, near, far)


def test_baseline_sample_rays_golden(golden, monkeypatch):
    """dataset.baseline_sample_rays against the reference's GetData.sample_rays (tests/golden/baseline_sample_rays.npz), TWO
    consecutive calls under one numpy seed: the pixel rows bit for bit on both -- the second call's depend on the zero-size
    draw over the mouth box that ends the first --, the rest at test_dataset_sample_rays_golden's bounds (rays 1e-6, colours
    exact).  Without that draw the second call picks other pixels."""
    from idealnerf_amd import dataset
    g = golden("baseline_sample_rays")
    monkeypatch.setattr(dataset.ops, "frame_rays", _cpu_frame_rays)
    H, W = g["target"].shape[:2]
    args = (g["rect"], g["landmark"], int(g["N_rand"]), float(g["sample_rate"]))
    np.random.seed(int(g["seed"]))
    for call in (0, 1):
        state = np.random.get_state()
        sel = dataset.baseline_select_pixels(H, W, *args)
        np.testing.assert_array_equal(sel, g[f"pixels_{call}"])
        assert sel.dtype == np.int64 and sel.shape == (96, 2)
        after = np.random.get_state()
        np.random.set_state(state)
        br, ts, bs = dataset.baseline_sample_rays(g["pose"], g["rect"], T(g["target"]), T(g["bc"]), g["landmark"], H, W,
                                                  float(g["focal"]), float(g["cx"]), float(g["cy"]), int(g["N_rand"]),
                                                  float(g["sample_rate"]), "cpu")
        assert all(np.array_equal(a, b) for a, b in zip(after[1:3], np.random.get_state()[1:3]))
        assert br.shape == (2, 96, 3)
        assert rel_err(br.numpy(), g[f"batch_rays_{call}"]) < 1e-6
        np.testing.assert_array_equal(ts.numpy(), g[f"target_s_{call}"])
        np.testing.assert_array_equal(bs.numpy(), g[f"bc_s_{call}"])
    # rows: the first int(96 * 0.95) inside the rect and outside the mouth box, the rest outside the rect
    coords, mouth_w, rect_w = dataset._box_masks(H, W, g["rect"], g["landmark"])
    flat = g["pixels_0"][:, 0] * W + g["pixels_0"][:, 1]
    assert (rect_w & ~mouth_w)[flat[:91]].all() and (~rect_w)[flat[91:]].all()
    # the control: the same two draws without the zero-size one give the first call's pixels and then others
    np.random.seed(int(g["seed"]))
    c_rect, c_out = coords[rect_w & ~mouth_w], coords[~rect_w]
    two = []
    for call in (0, 1):
        a = c_rect[np.random.choice(c_rect.shape[0], size=[91], replace=False)]
        b = c_out[np.random.choice(c_out.shape[0], size=[5], replace=False)]
        two.append(np.concatenate([a, b], 0).astype(np.int64))
    assert np.array_equal(two[0], g["pixels_0"]) and not np.array_equal(two[1], g["pixels_1"])


@pytest.fixture(scope="module")
def adnerf_clip(tmp_path_factory):
    """A generated clip as an AD-NeRF dataset: no parsing/ directory, no exp in either JSON."""
    d = str(tmp_path_factory.mktemp("adnerfclip"))
    flags, meta = write_clip_directory(d, 64, 4, seed=3, N_rand=64)
    shutil.rmtree(os.path.join(d, "parsing"))
    for f in meta["frames"]:
        del f["exp"]
    for mode in ("train", "val"):
        json.dump(meta, open(os.path.join(d, f"transforms_exp_{mode}.json"), "w"))
    loader_flags = SimpleNamespace(N_rand=64, sample_rate=0.95, testskip=2, gt_dirs="no_such_dir")   # gt_dirs is not read
    return d, loader_flags, meta


def test_baseline_getdata_on_an_adnerf_dataset(adnerf_clip, monkeypatch):
    """BaselineGetData on a directory without parsing/ and without exp: the 7-tuple, rows = baseline_select_pixels' under the
    same seed, rays / colours gathered at exactly those pixels, raw_img RGB from head_imgs/ whatever gt_dirs says, the whole
    audio table, len(val) == the skipped frame count (no second division by testskip), the whole background outside train
    mode.  The head stage's GetData cannot read this directory."""
    from PIL import Image
    from idealnerf_amd import dataset
    d, flags, meta = adnerf_clip
    monkeypatch.setattr(dataset.ops, "frame_rays", lambda pose, H, W, *a, **k: torch.arange(
        H * W, dtype=torch.float32)[:, None].repeat(1, 11))   # row p of the ray table holds p: no GPU here
    ds = dataset.BaselineGetData(d, "aud.npy", "train", flags, device="cpu")
    assert len(ds) == 4
    i = 2
    np.random.seed(17)
    item = ds[i]
    assert len(item) == 7
    batch_rays, target_s, bc_rgb, auds, raw_img, pose, index = item
    lm = np.loadtxt(os.path.join(d, "ori_imgs", f"{i}.lms"))
    np.random.seed(17)
    want = dataset.baseline_select_pixels(64, 64, np.array(meta["frames"][i]["face_rect"], dtype=np.int32), lm, 64, 0.95)
    flat = torch.from_numpy(want[:, 0] * 64 + want[:, 1])
    assert batch_rays.shape == (2, 64, 3) and torch.equal(batch_rays[0, :, 0], flat.float())
    img = np.asarray(Image.open(os.path.join(d, "head_imgs", f"{i}.jpg")))
    assert torch.equal(raw_img, torch.from_numpy(img.copy())) and raw_img.dtype == torch.uint8   # RGB as stored
    assert torch.equal(target_s, (torch.from_numpy(img.copy()).float() / 255.0).reshape(-1, 3)[flat])
    assert torch.equal(bc_rgb, ds.background_img.reshape(-1, 3)[flat])
    aud = np.load(os.path.join(d, "aud.npy"))
    assert index == i and auds.shape == (4, 16, 29)
    assert torch.equal(auds, torch.from_numpy(aud[[f["aud_id"] for f in meta["frames"]]]))      # the whole table, by aud_id
    assert np.array_equal(pose, np.array(meta["frames"][i]["transform_matrix"])[:3, :4])
    val = dataset.BaselineGetData(d, "aud.npy", "val", flags, skip=flags.testskip, device="cpu")
    assert len(val) == 2 and val[0][2].shape == (64, 64, 3) and len(val[1]) == 7
    with pytest.raises((KeyError, AttributeError, FileNotFoundError)):
        dataset.GetData(d, "aud.npy", "train", flags, device="cpu")


def test_oracle_c127_train_step_golden(golden):
    """One training step of the reference's baseline Network (tests/golden/baseline_train_step.npz) through the oracle with
    C = 127 and neither expression nor latent code, at the bounds tests/test_oracle_golden.py::test_train_step holds
    train_step.npz to: loss 1e-6 relative, gradients 1e-4 of each tensor's largest entry."""
    g, f = golden("baseline_train_step"), golden("frame32")
    assert (int(g["seed_coarse"]), int(g["seed_fine"])) == bc_.SEEDS and float(g["occupancy"].min()) >= 0.15
    pc, pf = bc_.baseline_state(bc_.SEEDS[0]), bc_.baseline_state(bc_.SEEDS[1])
    for p in (pc, pf):
        for v in p.values():
            v.requires_grad_(True)
    syn = bc_.scene()
    sel = T(g["sel"])
    aud = syn["aud"].clone().requires_grad_(True)
    out = oracle.render_rays(T(f["rays"])[sel], syn["bc"].reshape(-1, 3)[sel], pc, pf, aud, None, None, dims=bc_.DIMS)
    tgt = T(g["target"])
    loss = torch.nn.functional.mse_loss(out["rgb_map"], tgt) + torch.nn.functional.mse_loss(out["rgb0"], tgt)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-6 * abs(float(g["loss"]))
    assert rel_err(out["rgb_map"].detach().numpy(), g["rgb_map"]) < 1e-6 and rel_err(out["rgb0"].detach().numpy(), g["rgb0"]) < 1e-6
    assert rel_err(aud.grad.numpy(), g["g_aud"]) < 1e-4
    step = int(g["row_step"])
    n = 0
    for tag, p in (("c", pc), ("f", pf)):
        for key in g:
            if key.startswith(f"g_{tag}_"):
                grad = p[key[4:]].grad.numpy()
                rows = grad[::step] if grad.ndim == 2 and grad.shape[0] >= 128 else grad
                assert rel_err(rows, g[key]) < 1e-4, (tag, key)
                n += 1
        assert p["feature_linear.weight"].grad is None
    assert n == 20


BASELINE_CONFIGS = ("Chinese/chn_adnerf_baseline.txt", "may/may_adnerf_baseline.txt", "obama/adnerf_baseline.txt",
                    "obama3/adnerf_baseline.txt")


def test_shipped_baseline_configs_resolve_and_build():
    """The four shipped adnerf_baseline configs (their lines and the reference parser's values are part of
    tests/golden/configs_parsed.json) through config.load_config, and the baseline network built from each on the meta
    device: nothing is launched."""
    from idealnerf_amd import config
    from idealnerf_amd.agg_aud_exp_nerf import build_head_network
    from idealnerf_amd.head_baseline import Network
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "configs_parsed.json")))
    for name in BASELINE_CONFIGS:
        rel = "NeRFs/HeadNeRF/configs/audio_expr_nerf/" + name
        g = gold[rel]
        assert g["parsed"] is not None, rel
        ns = config.load_config(text="\n".join(g["lines"]))
        assert {k: v for k, v in vars(ns).items() if k != "config"} == g["parsed"], rel
        assert ns.expname == "adnerf_baseline"
        with torch.device("meta"):
            net = build_head_network(ns, 450, 450, 1200.0, model="baseline")
        assert isinstance(net, Network) and not hasattr(net, "ds_aud_net")
        for m in (net.face_nerf_coarse, net.face_nerf_fine):
            assert m.alpha_linear.weight.is_meta and (m.dim_aud, m.dim_expr, m.dim_latent) == (ns.dim_aud, 0, 0)
            assert m.pts_linears[0].weight.shape == (256, 63 + ns.dim_aud) and m.views_linears[0].weight.shape == (128, 283)


def _filled(seed):
    net = _network()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    return net


def _same(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_run_file_round_trip_in_both_key_forms(tmp_path):
    """{epoch:06d}_head.tar of the baseline: {global_step, model_state_dict, optimizer} and nothing else, the keys written with
    upstream's DataParallel prefix; read back with the prefix and without it, strictly, optimizer state included."""
    from idealnerf_amd import checkpoint, train_baseline
    assert train_baseline.checkpoint_name(3) == "000003_head.tar"
    net = _filled(1)
    opt = torch.optim.Adam(list(net.parameters()), lr=5e-4)
    for p in net.parameters():
        p.grad = torch.full_like(p, 1e-3)
    opt.step()
    path = str(tmp_path / "run" / "000003_head.tar")
    checkpoint.save_baseline_checkpoint(path, net, opt, 41)
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"global_step", "model_state_dict", "optimizer"} and ck["global_step"] == 41
    assert list(ck["model_state_dict"]) == ["module." + k for k in net.state_dict()]
    fresh, opt2 = _filled(2), None
    assert not _same(net, fresh)
    opt2 = torch.optim.Adam(list(fresh.parameters()), lr=5e-4)
    assert checkpoint.load_baseline_checkpoint(path, fresh, opt2) == 41 and _same(net, fresh)
    s1, s2 = opt.state_dict()["state"], opt2.state_dict()["state"]
    assert s1.keys() == s2.keys() and all(torch.equal(s1[k]["exp_avg"], s2[k]["exp_avg"]) for k in s1)
    bare = str(tmp_path / "run" / "000004_head.tar")                      # the same file without the prefix
    torch.save(dict(ck, model_state_dict={k[len("module."):]: v for k, v in ck["model_state_dict"].items()}), bare)
    other = _filled(3)
    assert checkpoint.load_baseline_checkpoint(bare, other) == 41 and _same(net, other)
    assert os.path.basename(checkpoint.latest_checkpoint(str(tmp_path / "run"))) == "000004_head.tar"
    torch.save(dict(ck, model_state_dict={k: v for k, v in list(ck["model_state_dict"].items())[1:]}), bare)
    with pytest.raises(RuntimeError):
        checkpoint.load_baseline_checkpoint(bare, _filled(4))               # strict: a missing key is an error


def test_adnerf_form_round_trip_and_strictness(tmp_path):
    """save_adnerf -> load_adnerf is the identity on all four dicts (a model trained here is a valid ft_path upstream: the
    file's dicts are the submodules' own state dicts); load_adnerf refuses a head-model file -- the run file of the paper
    model, and an AD-NeRF-shaped file whose FaceNeRFs have the paper model's widths --, where load_adnerf_finetune stays the
    tolerant warm start it was."""
    from idealnerf_amd import checkpoint
    from idealnerf_amd.audio_exp_nerf import Network as HeadNetwork
    from idealnerf_amd.helper import RenderConfig
    net = _filled(5)
    path = str(tmp_path / "adnerf.tar")
    checkpoint.save_adnerf(path, net, 1234)
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"network_fn_state_dict", "network_fine_state_dict", "network_audnet_state_dict",
                       "network_audattnet_state_dict", "global_step"}
    assert list(ck["network_fn_state_dict"]) == list(net.face_nerf_coarse.state_dict())
    assert tuple(ck["network_fine_state_dict"]["pts_linears.0.weight"].shape) == (256, 127)
    fresh = _filled(6)
    assert checkpoint.load_adnerf(path, fresh) == 1234 and _same(net, fresh)
    third = _filled(7)
    checkpoint.load_adnerf(bc_.adnerf_checkpoint(), third)                 # a dict, as load_adnerf_finetune takes one
    assert torch.equal(third.face_nerf_coarse.state_dict()["pts_linears.0.weight"], bc_.baseline_state(11, 200.0)["pts_linears.0.weight"])
    head = HeadNetwork(32, 32, 100.0, bc_.NEAR, bc_.FAR, 512, None, 64, 128, args=RenderConfig(perturb=0.0, near=bc_.NEAR, far=bc_.FAR))
    head_tar = str(tmp_path / "head.tar")
    checkpoint.save_checkpoint(head_tar, head, None, torch.ones(3, 32), 7)
    with pytest.raises(KeyError, match="not an AD-NeRF checkpoint"):
        checkpoint.load_adnerf(head_tar, _filled(8))
    wide = dict(bc_.adnerf_checkpoint(), network_fn_state_dict=head.face_nerf_coarse.state_dict())
    before = _filled(9)
    with pytest.raises(RuntimeError, match="size mismatch"):
        checkpoint.load_adnerf(wide, before)
    missing = bc_.adnerf_checkpoint()
    del missing["network_audattnet_state_dict"]["attentionNet.0.bias"]
    with pytest.raises(RuntimeError):
        checkpoint.load_adnerf(missing, _filled(10))
    checkpoint.load_adnerf_finetune(bc_.adnerf_checkpoint(), head)           # unchanged: drops the three layers, strict=False
    assert tuple(head.face_nerf_coarse.pts_linears[0].weight.shape) == (256, 235)


def test_drive_baseline_names_and_audio_by_position(adnerf_clip):
    """test_nerf.py's file names, and its audio rule: frame i of the val loader takes aud_features[i] BY POSITION -- the
    generated clip's aud_id runs backwards, so the training loader's table is the reverse."""
    from idealnerf_amd import dataset, drive
    d, flags, meta = adnerf_clip
    ns = SimpleNamespace(datadir="dataset/Obama3", aud_file="aud_eng.npy")
    assert drive.baseline_names(ns) == ("V_Obama3_aud_eng_N_baseline.avi", "Obama3_aud_eng_ADNeRF_{i}.jpg")
    aud = np.load(os.path.join(d, "aud.npy"))
    fr = dataset.BaselineTestFrames(d, "aud.npy", "val", flags, skip=2, device="cpu")
    assert len(fr) == 2 and (fr.H, fr.W) == (64, 64)
    item = fr[1]
    assert len(item) == 7 and item[6] == 1 and item[0].numel() == 0 and item[4].shape == (64, 64, 3)
    assert torch.equal(item[3], torch.from_numpy(aud[:2]))                                     # rows 0, 1: by position
    by_id = aud[[meta["frames"][j]["aud_id"] for j in (0, 2)]]
    assert not np.array_equal(item[3].numpy(), by_id)
    assert np.array_equal(item[5], np.array(meta["frames"][2]["transform_matrix"])[:3, :4])    # the val poses at testskip
    assert item[2].shape == (64, 64, 3) and item[2].dtype == torch.float64
    np.save(os.path.join(d, "short.npy"), aud[:1])
    with pytest.raises(ValueError, match="by position"):
        dataset.BaselineTestFrames(d, "short.npy", "val", flags, skip=2, device="cpu")


def test_resident_baseline_frames_construction_errors(adnerf_clip, tmp_path):
    """ResidentBaselineFrames names what it cannot serve before anything is uploaded: a clip beyond max_bytes, a region with
    fewer pixels than its share of N_rand, a share beyond the sampler's picks per region.  A mouth box of any size is none of
    these: nothing is drawn from it (counts = rect, outside, 0, 0)."""
    from idealnerf_amd import dataset
    from idealnerf_amd._lib import SAMPLE_MAX_REGION
    d, flags, meta = adnerf_clip
    mk = lambda **over: SimpleNamespace(**{**vars(flags), **over})
    with pytest.raises(ValueError, match="max_bytes"):
        dataset.ResidentBaselineFrames(d, "aud.npy", "train", flags, device="cpu", max_bytes=1000)
    with pytest.raises(ValueError, match="region 'outside'"):     # 64 x 64 with a 51 x 51 rect: 1495 pixels outside it
        dataset.ResidentBaselineFrames(d, "aud.npy", "train", mk(N_rand=3000, sample_rate=0.1), device="cpu")
    with pytest.raises(ValueError, match="picks"):
        dataset.ResidentBaselineFrames(d, "aud.npy", "train", mk(N_rand=2 * SAMPLE_MAX_REGION + 2, sample_rate=0.5), device="cpu")
    # the mouth box swallowing the whole rect fails the rect's draw (as upstream's first np.random.choice does) ...
    big = str(tmp_path / "bigmouth")
    shutil.copytree(d, big)
    for i in range(4):
        lm = np.loadtxt(os.path.join(big, "ori_imgs", f"{i}.lms"))
        lm[48:] = np.linspace(0, 63, 20)[:, None]
        np.savetxt(os.path.join(big, "ori_imgs", f"{i}.lms"), lm)
    with pytest.raises(ValueError, match="region 'rect'"):
        dataset.ResidentBaselineFrames(big, "aud.npy", "train", flags, device="cpu")
    # ... an EMPTY mouth box (landmarks far outside the frame) fails nothing
    none = str(tmp_path / "nomouth")
    shutil.copytree(d, none)
    for i in range(4):
        lm = np.loadtxt(os.path.join(none, "ori_imgs", f"{i}.lms"))
        lm[48:] = 500.0
        np.savetxt(os.path.join(none, "ori_imgs", f"{i}.lms"), lm)
    assert dataset.baseline_region_byte_map(64, 64, np.array([4, 4, 50, 50]), np.loadtxt(os.path.join(none, "ori_imgs", "0.lms"))).max() < 4
    fr = dataset.ResidentBaselineFrames(none, "aud.npy", "train", flags, device="cpu")
    assert fr.counts == (60, 4, 0, 0) and fr.populations[:, 2].tolist() == [0, 0, 0, 0] and fr.exprs is None
