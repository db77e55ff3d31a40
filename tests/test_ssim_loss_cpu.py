"""The patch SSIM loss without a GPU: the host-side patch-origin recipe, every ValueError of the loader and the trainers, the
three C entries in header, prototypes and library, the struct's layout, and the weight table against its formula."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from idealnerf_amd.synthetic import write_clip_directory
from ssim_loss_common import gauss_taps, reference, ssim_patches64
from train_loop_common import train_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "idealnerf.h")
CSRC = os.path.join(ROOT, "ideal-nerf_amd", "csrc")
ENTRIES = ("idealnerf_patch_pixels", "idealnerf_ssim_patch_fwd", "idealnerf_ssim_patch_bwd")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    return idealnerf_amd


# ------------------------------------------------------------------------------------------------ the origin recipe
def test_origin_range_bounds():
    from idealnerf_amd.ssim_loss import origin_range
    assert origin_range(4, 54, 16, 64) == (4, 36)        # rows 4 .. 54 hold origins 4 .. 39
    assert origin_range(4, 54, 51, 64) == (4, 1)         # exactly as wide as the rect
    assert origin_range(-7, 30, 16, 64) == (0, 16)       # clipped at the frame's first pixel: rows 0 .. 30
    assert origin_range(40, 90, 16, 64) == (40, 9)       # clipped at its last: rows 40 .. 63, origins 40 .. 48
    assert origin_range(20, 27, 16, 64) == (16, 1)       # narrower than p: centred (8 wide -> 4 on either side)
    assert origin_range(0, 5, 16, 64) == (0, 1)          # centred would start at -5: clamped to the frame
    assert origin_range(60, 63, 16, 64) == (48, 1)       # centred would end past the frame: clamped
    assert origin_range(0, 63, 64, 64) == (0, 1)
    with pytest.raises(ValueError):
        origin_range(0, 63, 65, 64)


def test_patch_origins_lie_where_they_should_and_depend_on_three_numbers():
    from idealnerf_amd.ssim_loss import patch_origins
    H, W, rect = 64, 80, [4, 6, 50, 30]                  # pixel rows 4 .. 54, columns 6 .. 36
    seen = set()
    for draw in range(200):
        for oy, ox in patch_origins(5, 2, draw, 3, 16, H, W, rect, "rect"):
            assert 4 <= oy and oy + 16 <= 55 and 6 <= ox and ox + 16 <= 37
            seen.add((oy, ox))
    assert len(seen) > 100
    assert {o[0] for o in seen} == set(range(4, 40)) and {o[1] for o in seen} == set(range(6, 22))   # every origin occurs
    frame = [o for d in range(200) for o in patch_origins(5, 2, d, 2, 16, H, W, rect, "frame")]
    assert all(0 <= oy <= H - 16 and 0 <= ox <= W - 16 for oy, ox in frame)
    assert max(o[1] for o in frame) > 36 and max(o[0] for o in frame) > 40   # past the rect
    # a rect narrower than p on one axis and at the frame's edge on the other
    for oy, ox in patch_origins(0, 0, 0, 4, 16, H, W, [58, 10, 20, 8], "rect"):
        assert oy == 48 and ox == 6                      # rows 58 .. 63 -> clamped to 48; columns 10 .. 18 (9 wide) -> centred
    # a function of (seed, frame, draw) alone: repeatable, in any order of calls, whatever numpy's global state
    a = patch_origins(7, 3, 11, 3, 16, H, W, rect)
    np.random.seed(123)
    patch_origins(7, 3, 12, 3, 16, H, W, rect)
    assert patch_origins(7, 3, 11, 3, 16, H, W, rect) == a
    many = lambda **kw: [patch_origins(**{**dict(seed=7, frame=3, draw=d, k=3, p=16, H=H, W=W, face_rect=rect), **kw}) for d in range(8)]
    assert many() != many(seed=8) and many() != many(frame=4) and many()[0] != many()[1]
    assert patch_origins(7, 3, (1 << 40) + 5, 1, 16, H, W, rect) != patch_origins(7, 3, 5, 1, 16, H, W, rect)
    assert patch_origins(7, 3, 11, 1, 16, H, W, rect) == a[:1]   # patch i does not depend on how many follow it
    with pytest.raises(ValueError):
        patch_origins(7, 3, 11, 1, 16, H, W, rect, "face")
    with pytest.raises(ValueError):
        patch_origins(7, 3, 11, 1, 16, H, W, None, "rect")


# ------------------------------------------------------------------------------------------------ every ValueError
def test_loader_and_trainer_value_errors(tmp_path):
    from idealnerf_amd import dataset, train as T_, train_agg, train_baseline
    d = str(tmp_path / "clip")
    os.makedirs(d)
    flags, _ = write_clip_directory(d, 64, 2, seed=1, N_rand=512, mouth_rays=8, torso_rays=4, sample_rate=0.6)
    # rect share: int(500 * 0.6) = 300; 2 * 16^2 = 512 and 1 * 18^2 = 324 exceed it -- before anything is uploaded
    for cls in (dataset.ResidentFrames, dataset.ResidentAggFrames, dataset.ResidentBaselineFrames):
        flags.use_highlight = False
        with pytest.raises(ValueError, match=r"2 \* 16\^2 = 512 rays .* which is 30[07] of N_rand = 512"):
            cls(d, "aud.npy", "train", flags, device="meta", patches=(2, 16))
    with pytest.raises(ValueError, match="324"):
        dataset.ResidentFrames(d, "aud.npy", "train", flags, device="meta", patches=(1, 18))
    for bad in ((0, 16), (17, 11), (1, 10), (1, 49), (1,), "1x16", 16):
        with pytest.raises(ValueError, match="patches"):
            dataset.ResidentFrames(d, "aud.npy", "train", flags, device="meta", patches=bad)
    with pytest.raises(ValueError, match="patch_region"):
        dataset.ResidentFrames(d, "aud.npy", "train", flags, device="meta", patches=(1, 16), patch_region="face")
    with pytest.raises(ValueError, match="torso"):
        dataset.ResidentTorsoFrames(d, "aud.npy", "train", flags, device="meta", patches=(1, 16))

    args = train_flags(d, tmp_path / "logs", "e", flags)
    for train in (T_.train, train_agg.train, train_baseline.train):
        with pytest.raises(ValueError, match="resident"):
            train(args, loader="reference", device="cpu", steps=1, patches=(1, 16))
        with pytest.raises(ValueError, match="patches"):
            train(args, device="cpu", steps=1, ssim_weight=0.2)
        with pytest.raises(ValueError, match="patches"):
            train(args, device="cpu", steps=1, ssim_weight=0.2, patches=(1, 50))
        with pytest.raises(ValueError, match="patch_region"):
            train(args, device="cpu", steps=1, ssim_weight=0.2, patches=(1, 16), patch_region="face")
        with pytest.raises(ValueError, match="ssim_weight"):
            train(args, device="cpu", steps=1, ssim_weight=-0.1, patches=(1, 16))
        with pytest.raises(ValueError, match=r"324"):
            train(args, device="meta", steps=1, ssim_weight=0.2, patches=(1, 18))
    assert not os.path.exists(str(tmp_path / "logs" / "e"))   # nothing was written on the way to any of them


def test_tool_parses_the_three_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_head_tool", os.path.join(ROOT, "tools", "train_head.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse(["--ssim_weight", "0.2", "--patches", "2x32", "--patch_region", "frame"])
    assert a.ssim_weight == 0.2 and tool._patches(a.patches) == (2, 32) and a.patch_region == "frame"
    a = tool.parse([])
    assert a.ssim_weight == 0.0 and tool._patches(a.patches) is None and a.patch_region == "rect"
    with pytest.raises(SystemExit):
        tool._patches("32")


# ------------------------------------------------------------------------------------------------ the C boundary
def test_entries_in_header_prototypes_and_library(idn):
    L = idn._lib
    lib = L.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRIES:
        decl = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", src)
        assert decl, f"{name} is not declared in include/idealnerf.h"
        assert name in L.PROTOTYPES and hasattr(lib, name)
        res, argtypes = L.PROTOTYPES[name]
        assert res is C.c_int and len(argtypes) == len(decl.group(1).split(","))
    assert L.PROTOTYPES["idealnerf_ssim_patch_bwd"][1][4] is C.c_float
    assert lib.idealnerf_version() == 4 and L.ABI_VERSION == 4
    for macro, val in (("IDN_PATCH_MAX", L.PATCH_MAX), ("IDN_PATCH_MIN_P", L.PATCH_MIN_P), ("IDN_PATCH_MAX_P", L.PATCH_MAX_P)):
        assert re.search(rf"#define {macro} {val}\b", src), macro
    assert (L.PATCH_MAX, L.PATCH_MIN_P, L.PATCH_MAX_P) == (16, 11, 48)


def test_entries_reject_bad_arguments_before_any_launch(idn):
    L = idn._lib
    lib = L.load()
    s = idn.ops.patch_set([(0, 0), (3, 4)], 16)
    assert (s.n_patches, s.p, s.oy[1], s.ox[1]) == (2, 16, 3, 4)
    assert lib.idealnerf_patch_pixels(None, 64, 8, None) == -1
    assert lib.idealnerf_patch_pixels(C.byref(s), 64, None, None) == -1 and b"NULL" in lib.idealnerf_last_error()
    for field, value in (("p", 10), ("p", 49), ("n_patches", 0), ("n_patches", 17)):
        s = idn.ops.patch_set([(0, 0)], 16)
        setattr(s, field, value)
        assert lib.idealnerf_patch_pixels(C.byref(s), 64, 8, None) == -1, (field, value)
        assert b"outside" in lib.idealnerf_last_error()
    s = idn.ops.patch_set([(0, 49)], 16)
    assert lib.idealnerf_patch_pixels(C.byref(s), 64, 8, None) == -1 and b"leaves" in lib.idealnerf_last_error()
    s = idn.ops.patch_set([(-1, 0)], 16)
    assert lib.idealnerf_patch_pixels(C.byref(s), 64, 8, None) == -1
    for k, p in ((0, 16), (17, 16), (1, 10), (1, 49)):
        assert lib.idealnerf_ssim_patch_fwd(8, 8, k, p, 8, None) == -1
        assert lib.idealnerf_ssim_patch_bwd(8, 8, k, p, 1.0, 8, None) == -1
    assert lib.idealnerf_ssim_patch_fwd(None, 8, 1, 16, 8, None) == -1 and b"NULL" in lib.idealnerf_last_error()
    assert lib.idealnerf_ssim_patch_bwd(8, 8, 1, 16, 1.0, None, None) == -1 and b"NULL" in lib.idealnerf_last_error()
    # the host layer names the same limits, and refuses the CPU like every operator here
    for k, p in ((1, 10), (1, 49), (17, 11)):
        with pytest.raises(idn._lib.IdealNerfError):
            idn.ops.patch_set([(0, 0)] * k, p)
    x = torch.rand(16 * 16, 3)
    with pytest.raises(idn._lib.IdealNerfError, match="GPU"):
        idn.ops.ssim_patch_fwd(x, x, 1, 16)
    with pytest.raises(idn._lib.IdealNerfError, match="GPU"):
        idn.ops.ssim_patch_bwd(x, x, 1, 16)
    with pytest.raises(idn._lib.IdealNerfError, match="GPU"):
        idn.ops.patch_pixels([(0, 0)], 16, 64, out=torch.empty(256, dtype=torch.int64))
    from idealnerf_amd.ssim_loss import ssim_patch_loss
    with pytest.raises(idn._lib.IdealNerfError, match="GPU"):
        ssim_patch_loss(x.clone().requires_grad_(True), x, 1, 16)
    with pytest.raises(idn._lib.IdealNerfError):
        idn.ops.ssim_patch_fwd(x, x, 1, 15)              # 225 rows asked of 256


def test_patch_set_matches_c_layout(idn, tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "idealnerf.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(idn_patch_set), offsetof(idn_patch_set, n_patches), '
                    'offsetof(idn_patch_set, p), offsetof(idn_patch_set, oy), offsetof(idn_patch_set, ox));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = idn._lib.PatchSet
    assert got == [C.sizeof(P), P.n_patches.offset, P.p.offset, P.oy.offset, P.ox.offset] == [136, 0, 4, 8, 72]


def test_weight_table_equals_the_formula():
    """Both kernels' tables, as written in their sources, are exp(-(k - 5)^2 / 4.5) normalised in fp64 and rounded to fp32."""
    want = gauss_taps()
    assert want.dtype == np.float32 and abs(float(want.astype(np.float64).sum()) - 1.0) < 1e-7
    for name, table in (("metrics.hip", "kGauss"), ("ssim_loss.hip", "kGaussL")):
        src = open(os.path.join(CSRC, name)).read()
        body = re.search(rf"{table}\[\w+\]\s*=\s*\{{([^}}]*)\}}", src).group(1)
        got = np.array([np.float32(v.strip().rstrip("f")) for v in body.split(",")], dtype=np.float32)
        assert got.shape == (11,) and np.array_equal(got, want), name


def test_reference_is_the_ssim_index():
    """The fp64 reference the GPU tests compare with, against the definition written out for a single window."""
    torch.manual_seed(0)
    x, t = torch.rand(1, 11, 11, 3), torch.rand(1, 11, 11, 3)
    w = np.outer(gauss_taps().astype(np.float64), gauss_taps().astype(np.float64))
    vals = []
    for c in range(3):
        a, b = x[0, :, :, c].double().numpy(), t[0, :, :, c].double().numpy()
        mx, mt = (w * a).sum(), (w * b).sum()
        vx, vt, cov = (w * a * a).sum() - mx * mx, (w * b * b).sum() - mt * mt, (w * a * b).sum() - mx * mt
        vals.append((2 * mx * mt + 1e-4) * (2 * cov + 9e-4) / ((mx * mx + mt * mt + 1e-4) * (vx + vt + 9e-4)))
    out, g = reference(x, t, 1, 11)
    assert abs(float(out[0]) - np.mean(vals)) < 1e-13 and abs(float(out[1]) - (1 - np.mean(vals))) < 1e-13
    assert g.shape == x.shape and g.dtype == torch.float64
    assert abs(float(ssim_patches64(t.double(), t.double(), 1, 11)[0]) - 1.0) < 1e-12
