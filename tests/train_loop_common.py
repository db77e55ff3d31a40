"""Shared by tests/test_train_loop_cpu.py and tests/test_train_loop_gpu.py (not collected by pytest): the sampler's definition
restated in numpy, a plausible region map, and the trainer's flags for a generated directory."""
import numpy as np

from oracle.philox import philox4x32_10


def sampler_reference(region_map, counts, seed, draw):
    """include/idealnerf.h: idealnerf_sample_pixels, word for word.  Region g contributes its counts[g] pixels with the
    smallest (key, p) pairs in ascending order, key(p, g) = word 0 of Philox4x32-10(key = seed, counter = (p, g, draw lo, draw hi));
    regions in the order rect, outside, mouth, torso.  -> int64 [sum(counts)] flat row-major indices."""
    flat = np.asarray(region_map, dtype=np.uint8).reshape(-1)
    out = []
    for g, c in enumerate(counts):
        p = np.nonzero((flat >> g) & 1)[0].astype(np.uint64)
        assert c <= p.size, (g, c, p.size)
        key = philox4x32_10((p, np.full_like(p, g), np.full_like(p, draw & 0xFFFFFFFF), np.full_like(p, (draw >> 32) & 0xFFFFFFFF)),
                            (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[0]
        composite = (key << np.uint64(32)) | p          # distinct: p is part of it
        out.append(p[np.argsort(composite, kind="stable")[:c]])
    return np.concatenate(out).astype(np.int64)


def random_region_map(H, W, seed, torso_rows=0.25):
    """A plausible byte map: a face rect, a mouth box inside it, torso rows at the bottom that overlap the other regions."""
    rs = np.random.RandomState(seed)
    r0, c0 = rs.randint(0, H // 4), rs.randint(0, W // 4)
    rh, cw = rs.randint(H // 3, H // 2), rs.randint(W // 3, W // 2)
    rect = np.zeros((H, W), bool)
    rect[r0:r0 + rh, c0:c0 + cw] = True
    mouth = np.zeros((H, W), bool)
    mouth[r0 + rh // 3:r0 + 2 * rh // 3, c0 + cw // 4:c0 + 3 * cw // 4] = True
    torso = np.zeros((H, W), bool)
    torso[int(H * (1 - torso_rows)):, W // 8:] = True
    return ((rect & ~mouth).astype(np.uint8) | ((~rect).astype(np.uint8) << 1) | (mouth.astype(np.uint8) << 2) |
            (torso.astype(np.uint8) << 3))


def train_flags(datadir, basedir, expname, loader_flags, **over):
    """The head trainer's flags (helper.config_parser's defaults) for a generated directory, as a namespace."""
    from idealnerf_amd import config
    ns = config.load_config(argv=["--datadir", str(datadir), "--basedir", str(basedir), "--expname", expname,
                                  "--dim_aud", "64", "--dim_expr", "76", "--near", "0.3", "--far", "0.9"])
    for k, v in vars(loader_flags).items():
        setattr(ns, k, v)
    for k, v in over.items():
        setattr(ns, k, v)
    return ns
