"""The feature-aggregation model off the GPU: the reduction to a FaceNeRF anchored to the reference module's own output, the
host-side loader, checkpoint naming and resume bookkeeping, and the two shipped configurations."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle
import agg_common as ac
from idealnerf_amd.synthetic import write_clip_directory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reduction_reproduces_the_reference_module(golden):
    """oracle.facenerf_forward on the reduced parameters (aud := g, views_linears.0 split into its trunk columns and a bias
    term) against tests/golden/facenerf_agg.npz["out"], the reference FaceNeRFAgg's output: 1e-5 of the largest entry, the
    bound test_facenerf_agg_golden holds the kernel to."""
    import test_hip_parity as hp
    g = golden("facenerf_agg")
    p = hp._agg_state(int(g["seed"]))
    x, aud, expr, latent = (hp.T(g[k]) for k in ("x", "aud", "expr", "latent"))
    with torch.no_grad():
        red, feat = ac.reduced(p, aud, expr)
        assert feat.shape == (64,) and red["views_linears.0.weight"].shape == (128, ac.N_H)
        out = oracle.facenerf_forward(red, x, feat, None, latent, ac.reduced_dims())
    err = hp.rel_err(out, g["out"])
    print(f"\nreduction vs the reference module: {err:.2e}")
    assert err < 1e-5


def test_reduced_pair_is_the_reduction_of_each_network():
    """The one-call form the GPU tests feed oracle.render_rays (agg_common.reduced_pair): each network's output on
    aud = cat(g_coarse, g_fine) equals its own reduction's on its own g (zero columns contribute exact zeros; the row sums
    are regrouped, so equality is to rounding)."""
    import test_hip_parity as hp
    rs = np.random.RandomState(0)
    pc, pf = hp._agg_state(4), hp._agg_state(5)
    x = hp.T(rs.standard_normal((33, 90)).astype(np.float32))
    aud, expr, lat = (hp.T(rs.standard_normal(n).astype(np.float32)) for n in (64, 76, 32))
    with torch.no_grad():
        rc, rf, both, dims = ac.reduced_pair(pc, pf, aud, expr)
        for p_pair, p_own in ((rc, pc), (rf, pf)):
            own, g = ac.reduced(p_own, aud, expr)
            a = oracle.facenerf_forward(p_pair, x, both, None, lat, dims)
            b = oracle.facenerf_forward(own, x, g, None, lat, ac.reduced_dims())
            assert hp.rel_err(a, b) < 1e-6


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("aggclip"))
    # at 64 x 64 the mouth box (the landmarks' extent + 20 pixels each way) is 45 x 45 at the most: with this rect it leaves
    # 592 rect pixels outside it, and the 2415 pixels outside the rect are more than the box holds (the mouth block indexes them)
    flags, meta = write_clip_directory(d, 64, 4, seed=3, N_rand=64, dim_expr=79, face_rect=ac.RECT64, mouth_range=ac.MOUTH64)
    flags.use_highlight, flags.testskip = True, 2
    return d, flags, meta


def test_agg_getdata_rows_and_tuple(clip, monkeypatch):
    """AggGetData under one numpy seed: the 8-tuple, rows = torso_select_pixels' rows in order (the same seed, the frame's own
    rect and landmarks), rays / colours gathered at exactly those pixels, raw_img RGB (the file's bytes, not flipped), and
    len(val) == n // testskip."""
    from PIL import Image
    from idealnerf_amd import dataset
    d, flags, meta = clip
    frames = []
    monkeypatch.setattr(dataset.ops, "frame_rays", lambda pose, H, W, *a, **k: frames.append(pose) or torch.arange(
        H * W, dtype=torch.float32)[:, None].repeat(1, 11))   # row p of the ray table holds p: no GPU here
    ds = dataset.AggGetData(d, "aud.npy", "train", flags, device="cpu")
    assert len(ds) == 4
    i = 2
    np.random.seed(17)
    item = ds[i]
    assert len(item) == 8
    batch_rays, target_s, bc_rgb, auds, raw_img, pose, exp, index = item
    lm = np.loadtxt(os.path.join(d, "ori_imgs", f"{i}.lms"))
    np.random.seed(17)
    want = dataset.torso_select_pixels(64, 64, np.array(meta["frames"][i]["face_rect"], dtype=np.int32), lm, 64, True, 0.95)
    assert want.shape == (64, 2) and dataset.torso_mouth_num(64, True) == 16
    flat = torch.from_numpy(want[:, 0] * 64 + want[:, 1])
    assert batch_rays.shape == (2, 64, 3) and torch.equal(batch_rays[0, :, 0], flat.float())    # rect, outside, mouth: in order
    assert len(frames) == 1                                                                      # one camera
    img = np.asarray(Image.open(os.path.join(d, "head_imgs", f"{i}.jpg")))
    assert torch.equal(raw_img, torch.from_numpy(img.copy())) and raw_img.dtype == torch.uint8   # RGB as stored
    assert torch.equal(target_s, (torch.from_numpy(img.copy()).float() / 255.0).reshape(-1, 3)[flat])
    assert torch.equal(bc_rgb, ds.background_img.reshape(-1, 3)[flat])
    assert index == i and exp.shape == (79,) and auds.shape == (4, 16, 29)
    assert np.array_equal(pose, np.array(meta["frames"][i]["transform_matrix"])[:3, :4])
    val = dataset.AggGetData(d, "aud.npy", "val", flags, skip=flags.testskip, device="cpu")
    assert len(val.all_imgs) == 2 and len(val) == 2 // flags.testskip == 1
    assert val[0][2].shape == (64, 64, 3)                                                       # the whole background outside train mode


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(3))


def test_checkpoint_naming_and_newest_checkpoint_resume(tmp_path):
    """'{:06d}_head.tar' per epoch; the loop writes it every i_weights steps with the COMPLETED step count, the newest one is
    what a resume finds, and a resumed loop enters its first epoch at global_step % n_frames."""
    from idealnerf_amd import checkpoint, train as T_, train_agg
    assert train_agg.checkpoint_name(0) == "000000_head.tar" and train_agg.checkpoint_name(12) == "000012_head.tar"
    # i_print 7: steps 1 .. 4 touch neither the log nor the validation hook (multiples of 7 and of 700)
    args = SimpleNamespace(basedir=str(tmp_path), expname="run", N_iters=5, i_print=7, i_weights=2)
    net = _Net()
    opt = torch.optim.Adam(net.parameters(), lr=0.1)
    lat = torch.ones(3, 32)
    seen = []
    step = T_._run_epochs(args, net, opt, lat, 3, 1, 4, 0, None, None, batch=lambda it, s: (it, s),
                          step_fn=lambda data, s: seen.append(data) or {}, scalars_of=None, log_line=None, validate=None,
                          checkpoint_name=train_agg.checkpoint_name)
    assert step == 5 and seen == [(1, 1), (2, 2), (0, 3), (1, 4)]                     # entered epoch 0 at frame 1 % 3
    run = tmp_path / "run"
    assert sorted(f for f in os.listdir(run) if f.endswith(".tar")) == ["000000_head.tar", "000001_head.tar"]   # steps 2 and 4
    newest = checkpoint.latest_checkpoint(str(run))
    assert os.path.basename(newest) == "000001_head.tar"
    got_step, codes = checkpoint.load_checkpoint(newest, _Net())
    assert got_step == 5 and torch.equal(codes, lat)                                   # completed steps: the resume repeats none
    (run / "000010_head.tar").write_bytes((run / "000001_head.tar").read_bytes())
    assert os.path.basename(checkpoint.latest_checkpoint(str(run))) == "000010_head.tar"   # natural order, not string order


def test_shipped_feat_agg_configs_parse_and_build():
    """Both shipped feat_agg.txt files (tests/golden/configs_agg_parsed.json: their lines, and the values the reference's
    parser resolves once it knows the use_highlight switch the agg trainer reads) through config.load_config(kind="agg"), and
    the agg network built from each on the meta device: nothing is launched."""
    from idealnerf_amd import config
    from idealnerf_amd.agg_aud_exp_nerf import Network, build_head_network
    from idealnerf_amd.models.face_nerf_agg import FaceNeRFAgg
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "configs_agg_parsed.json")))
    assert sorted(os.path.basename(os.path.dirname(k)) for k in gold) == ["chn", "obama"]
    for rel, g in gold.items():
        text = "\n".join(g["lines"])
        with pytest.raises(ValueError):
            config.load_config(text=text)                       # the head parser ends on use_highlight, as the reference's does
        assert g["rejected_by_head_parser"] is True
        ns = config.load_config(text=text, kind="agg")
        assert {k: v for k, v in vars(ns).items() if k != "config"} == g["parsed"], rel
        assert ns.use_highlight is True and ns.N_rand == 2048 and (ns.N_samples, ns.N_importance) == (64, 128)
        with torch.device("meta"):
            net = build_head_network(ns, 450, 450, 1200.0, model="agg")
        assert isinstance(net, Network) and not hasattr(net, "ds_aud_net")
        for m in (net.face_nerf_coarse, net.face_nerf_fine):
            assert isinstance(m, FaceNeRFAgg) and m.alpha_linear.weight.is_meta
            assert m.agg_linears[0].weight.shape == (64, ns.dim_aud + 79) and m.views_linears[0].weight.shape == (128, 283 + 64)
            assert m.pts_linears[0].weight.shape == (256, 63 + 64 + 32)
