"""Host side of the training loop's resident data path (no GPU): the sampler's definition and its uniformity, the region
helper shared with ``select_pixels``, ``ResidentFrames``' refusals, the rank / step / draw mapping, the two C entries'
declarations and bindings, and the ISA audit of csrc/sampler.hip."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle.philox import philox4x32_10
from idealnerf_amd.synthetic import write_clip_directory
from train_loop_common import random_region_map, sampler_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    return idealnerf_amd


def test_sampler_definition_counts_order_membership():
    """The numpy restatement of idealnerf_sample_pixels: counts as upstream computes them, the regions in upstream's order,
    no pixel twice inside a region, every pick inside its region, each region's picks in ascending (key, p) order."""
    from idealnerf_amd import ops
    counts = ops.sample_counts(3072, 256, 0, 0.95)
    assert counts == (2675, 141, 256, 0) and sum(counts) == 3072
    assert ops.sample_counts(64, 8, 4, 0.95) == (49, 3, 8, 4)
    H, W = 48, 80
    m = random_region_map(H, W, seed=1)
    counts = (37, 11, 5, 9)
    seed, draw = 0x123456789ABCDEF, (1 << 32) + 7
    sel = sampler_reference(m, counts, seed, draw)
    assert sel.shape == (sum(counts),) and sel.dtype == np.int64
    flat, at = m.reshape(-1), 0
    for g, c in enumerate(counts):
        part = sel[at:at + c]
        at += c
        assert len(set(part.tolist())) == c                       # without replacement
        assert (((flat[part] >> g) & 1) == 1).all()               # inside its region
        p = part.astype(np.uint64)
        key = philox4x32_10((p, np.full_like(p, g), np.full_like(p, draw & 0xFFFFFFFF), np.full_like(p, draw >> 32)),
                            (seed & 0xFFFFFFFF, seed >> 32))[0]
        pairs = list(zip(key.tolist(), p.tolist()))
        assert pairs == sorted(pairs)                             # ascending (key, p)
        # ... and nothing outside the picks has a smaller pair than the largest pick
        rest = np.setdiff1d(np.nonzero((flat >> g) & 1)[0], part).astype(np.uint64)
        rkey = philox4x32_10((rest, np.full_like(rest, g), np.full_like(rest, draw & 0xFFFFFFFF), np.full_like(rest, draw >> 32)),
                             (seed & 0xFFFFFFFF, seed >> 32))[0]
        assert min(zip(rkey.tolist(), rest.tolist())) > pairs[-1]
    # a count equal to the population is a permutation of the region; other draws and seeds give other picks
    pop2 = int(((flat >> 2) & 1).sum())
    full = sampler_reference(m, (0, 0, pop2, 0), seed, draw)
    assert sorted(full.tolist()) == np.nonzero((flat >> 2) & 1)[0].tolist()
    assert not np.array_equal(sel, sampler_reference(m, counts, seed, draw + 1))
    assert not np.array_equal(sel, sampler_reference(m, counts, seed + 1, draw))


def test_sampler_definition_is_uniform():
    """16 x 16 map, a region of 100 pixels, 10 picked, 4 000 consecutive draws at a fixed seed: every pixel's inclusion count
    lies within 5 binomial standard deviations of 4000 * 10 / 100 = 400 (sd = sqrt(4000 * 0.1 * 0.9) = 18.97: +-94.9).
    Deterministic: Philox is a function of (seed, draw, pixel)."""
    m = np.zeros((16, 16), np.uint8)
    region = np.random.RandomState(5).permutation(256)[:100]
    m.reshape(-1)[region] = 1 << 2                                   # the mouth region
    hits = np.zeros(256, np.int64)
    first = np.zeros(256, np.int64)
    for t in range(4000):
        sel = sampler_reference(m, (0, 0, 10, 0), 20240607, t)
        hits[sel] += 1
        first[sel[0]] += 1
    assert hits.sum() == 40000 and (hits[np.setdiff1d(np.arange(256), region)] == 0).all()
    bound = 5.0 * np.sqrt(4000 * 0.1 * 0.9)
    dev = np.abs(hits[region] - 400.0)
    print(f"inclusion counts: min {hits[region].min()} max {hits[region].max()} (bound +-{bound:.1f})")
    assert dev.max() <= bound, (hits[region].min(), hits[region].max())
    # the ORDER is uniform as well: each pixel leads the picks 4000 / 100 = 40 times, sd sqrt(4000 * 0.01 * 0.99) = 6.29
    assert np.abs(first[region] - 40.0).max() <= 5.0 * np.sqrt(4000 * 0.01 * 0.99), (first[region].min(), first[region].max())


def test_region_helper_is_select_pixels_masks(idn, golden, monkeypatch):
    """region_byte_map holds the very populations select_pixels draws from, on the sample_rays golden's inputs: the same
    sizes in the same call order (mouth, torso, rect, outside), and every pick of the golden's seed inside its region's bit."""
    from idealnerf_amd import dataset
    g = golden("sample_rays")
    H, W = g["parse"].shape[:2]
    m = dataset.region_byte_map(H, W, g["rect"], g["landmark"], g["parse"])
    assert m.shape == (H, W) and m.dtype == np.uint8 and int(m.max()) < 16
    pops = [int(((m >> b) & 1).sum()) for b in range(4)]
    assert pops[0] + pops[1] + int((((m >> 2) & 1) & ~((m >> 1) & 1)).sum()) == H * W     # rect-minus-mouth | outside | mouth-in-rect
    seen = []
    real = np.random.choice
    monkeypatch.setattr(np.random, "choice", lambda a, size=None, replace=True: (seen.append(int(a)), real(a, size=size, replace=replace))[1])
    np.random.seed(int(g["seed"]))
    n_rand, mouth_rays, torso_rays, rate = int(g["N_rand"]), int(g["mouth_rays"]), int(g["torso_rays"]), float(g["sample_rate"])
    sel = dataset.select_pixels(H, W, g["rect"], g["landmark"], g["parse"], n_rand, mouth_rays, torso_rays, rate)
    assert seen == [pops[2], pops[3], pops[0], pops[1]]
    np.testing.assert_array_equal(g["target"][sel[:, 0], sel[:, 1]], g["target_s"])           # select_pixels' output is unchanged
    counts = idn.ops.sample_counts(n_rand, mouth_rays, torso_rays, rate)
    at = 0
    for b, c in enumerate(counts):
        rows = sel[at:at + c]
        at += c
        assert (((m[rows[:, 0], rows[:, 1]] >> b) & 1) == 1).all(), dataset.REGION_NAMES[b]
    # the masks themselves, against select_pixels' expressions written out once more
    coords, mouth_w, rect_w, torso = dataset.region_masks(H, W, g["rect"], g["landmark"], g["parse"])
    assert np.array_equal(((m >> 0) & 1).reshape(-1).astype(bool), rect_w & ~mouth_w)
    assert np.array_equal(((m >> 1) & 1).reshape(-1).astype(bool), ~rect_w)
    assert np.array_equal(((m >> 2) & 1).reshape(-1).astype(bool), mouth_w)
    assert np.array_equal(((m >> 3) & 1).astype(bool), torso)


def test_resident_frames_refusals(idn, tmp_path):
    """Both refusals come at construction from host-side numbers, before any upload: a region smaller than its share of
    N_rand (named with its frame), and a clip over max_bytes."""
    from idealnerf_amd import dataset
    d = str(tmp_path / "clip")
    os.makedirs(d)
    flags, _ = write_clip_directory(d, 64, 3)
    with pytest.raises(ValueError, match=r"max_bytes"):
        dataset.ResidentFrames(d, "aud.npy", "train", flags, device="cpu", max_bytes=3 * 64 * 64 * 4)
    par = np.zeros((64, 64, 3), np.uint8)
    par[60:, :2] = (255, 0, 0)                      # frame 1 keeps 8 torso pixels, the batch wants 12
    from PIL import Image
    Image.fromarray(par).save(os.path.join(d, "parsing", "1.png"))
    flags.torso_rays = 12
    with pytest.raises(ValueError, match=r"frame 1 .*'torso' holds 8 pixels.*12"):
        dataset.ResidentFrames(d, "aud.npy", "train", flags, device="cpu")
    flags.torso_rays = 8                            # exactly the population: accepted (the upload itself needs no GPU)
    fr = dataset.ResidentFrames(d, "aud.npy", "train", flags, device="cpu")
    assert len(fr) == 3 and fr.populations[1, 3] == 8 and fr.imgs.shape == (3, 64, 64, 3) and fr.maps.dtype.is_floating_point is False
    with pytest.raises(idn._lib.IdealNerfError):
        fr.batch(0, 0)                              # the draw is a device kernel: no CPU fallback
    flags.N_rand, flags.mouth_rays, flags.torso_rays = 5000, 0, 0
    with pytest.raises(ValueError, match=r"4096"):
        dataset.ResidentFrames(d, "aud.npy", "train", flags, device="cpu")


def test_draw_index_is_a_bijection():
    """rank r of N at step s uses draw s N + r: over steps 0..S-1 the N ranks use every draw in [0, S N) exactly once."""
    from idealnerf_amd.train import draw_index
    for world in (1, 2, 8):
        draws = [draw_index(s, r, world) for s in range(13) for r in range(world)]
        assert sorted(draws) == list(range(13 * world))
        assert [draw_index(s, 0, world) for s in range(3)] == [0, world, 2 * world]
    assert draw_index(7) == 7
    with pytest.raises(ValueError):
        draw_index(0, 2, 2)


def test_sampler_entries_are_declared_and_bound(idn):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "idealnerf.h")).read(), flags=re.S)
    lib = idn._lib.load()
    for name in ("idealnerf_sample_pixels", "idealnerf_gather_rays", "idealnerf_sample_pixels_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in idn._lib.PROTOTYPES and hasattr(lib, name)
    assert "#define IDN_SAMPLE_MAX_REGION 4096" in src and idn._lib.SAMPLE_MAX_REGION == 4096
    assert lib.idealnerf_version() == 4 and lib.idealnerf_sample_pixels_workspace_bytes() == 16
    assert "sampler.hip" in open(os.path.join(ROOT, "ideal-nerf_amd", "build.py")).read()
    # argument checks that need no device: a count above the stated maximum is an error code, not a truncation
    assert lib.idealnerf_sample_pixels(None, 64, 64, 4097, 0, 0, 0, 0, 0, None, 0, None, None) == -2
    assert b"IDN_SAMPLE_MAX_REGION" in lib.idealnerf_last_error()
    assert lib.idealnerf_sample_pixels(None, 64, 64, 1, 0, 0, 0, 0, 0, None, 0, None, None) == -1


def test_sampler_isa_audit(tmp_path):
    """tools/audit_asm_loads.py on the device assembly of csrc/sampler.hip, as test_boundary_cpu.py runs it on the other
    kernel files; every device function inlined."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        import torch
        assert not torch.cuda.is_available(), "a GPU box without hipcc"
        pytest.skip("hipcc not available")
    out = tmp_path / "sampler.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                    os.path.join(ROOT, "ideal-nerf_amd", "csrc", "sampler.hip"), "-o", str(out)], check=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_loads.py"), str(out), ""], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 suspicious touches" in r.stdout
    isa = open(out).read()
    assert "sample_pixels_kernel" in isa and "gather_rays_kernel" in isa and "s_swappc_b64" not in isa
