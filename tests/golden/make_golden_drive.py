#!/usr/bin/env python3
"""Generate tests/golden/drive_loaders.npz by running the REFERENCE's two test-time loaders on the CPU.

Runs only where the reference checkout is present (it never travels with the tests):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_drive.py [/path/to/reference]

The dataset directory is ``tests/drive_common.build_directory`` (seeded; the tests rebuild it).  On it run

- ``load_test_data`` of NeRFs/TorsoNeRF/load_audface.py (:87-114), in the three cases of LOAD_CASES, and
- the constructor of ``GetData`` of NeRFs/HeadNeRF/test/eval_aud_exp_nerf.py (:46-98) for skip 1 and 2; only the constructor
  runs, and its attributes are read.

The loaders' audio and expression outputs are rows of the directory's random tables, copied: what is stored of them is WHICH
row of the table each output row equals exactly (``rows_of``), the background once (the loaders agree on it), and everything
else -- poses, intrinsics, audio ids, the torso pose -- as returned.

Stand-ins as in make_golden.py (configargparse -> argparse, empty cv2 / face_alignment, natsort, a no-op SummaryWriter,
``Tensor.cuda`` a no-op), plus: ``imageio.imread`` through Pillow (imageio is absent here; both decode with libjpeg), a no-op
``torch.set_default_tensor_type`` while the eval module is imported (it selects the CUDA tensor type at import), and the flags
through ``sys.argv`` before the import (the module parses them at import time).  Only the resulting arrays are stored.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (REPO, os.path.join(REPO, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import drive_common as dc  # noqa: E402
from make_golden import REF, install_shims  # noqa: E402

# name -> (audio file key, testskip, test_size, aud_start)
LOAD_CASES = {"short": ("short", 1, -1, 0), "clamped": ("short", 2, 3, 4), "long": ("long", 1, -1, 0)}
SKIPS = (1, 2)


def rows_of(got, table, must=True):
    """For every row of `got` the index of the row of `table` it equals exactly (one and only one: the tables are random) ->
    int64 [len(got)].  must=False: the rows that have an equal at all, instead."""
    table = np.asarray(table)
    hits = [[i for i in range(len(table)) if np.array_equal(np.asarray(row, dtype=table.dtype), table[i])] for row in got]
    if not must:
        return np.asarray([h[0] for h in hits if h], dtype=np.int64)
    assert all(len(h) == 1 for h in hits), hits
    return np.asarray([h[0] for h in hits], dtype=np.int64)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    install_shims()
    from PIL import Image
    sys.modules["imageio"].imread = lambda path: np.asarray(Image.open(path))
    try:
        import tqdm  # noqa: F401
    except ImportError:
        m = types.ModuleType("tqdm")
        m.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = m
    for p in (ref, os.path.join(ref, "NeRFs", "TorsoNeRF")):
        sys.path.insert(0, p)
    import importlib
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = dc.build_directory(os.path.join(tmp, "May"))

        la = importlib.import_module("NeRFs.TorsoNeRF.load_audface")
        bcs = []
        for name, (aud, skip, size, start) in LOAD_CASES.items():
            poses, auds, bc, hwfcxy, aud_ids, torso_pose = la.load_test_data(paths["dir"], paths[aud], paths["identity"], skip, size, start)
            bcs.append(np.asarray(bc))
            assert auds.dtype == np.float32 and poses.dtype == np.float32 and bcs[-1].dtype == np.uint8
            out.update({f"ltd_{name}_poses": poses, f"ltd_{name}_aud_rows": rows_of(auds, np.load(paths[aud])),
                        f"ltd_{name}_hwfcxy": np.asarray(hwfcxy, dtype=np.float64),
                        f"ltd_{name}_aud_ids": np.asarray(aud_ids, dtype=np.int64), f"ltd_{name}_torso_pose": np.asarray(torso_pose)})
        assert all(np.array_equal(b, bcs[0]) for b in bcs)
        out["bc"] = bcs[0]

        sys.argv = [sys.argv[0], "--evalExpr_path", paths["driving"], "--datadir", paths["dir"], "--aud_file", paths["long"],
                    "--vis_path", os.path.join(tmp, "vis"), "--dim_aud", "64", "--dim_expr", str(dc.DIM_EXPR)]
        real = torch.set_default_tensor_type
        torch.set_default_tensor_type = lambda *a, **k: None
        try:
            ev = importlib.import_module("NeRFs.HeadNeRF.test.eval_aud_exp_nerf")
        finally:
            torch.set_default_tensor_type = real
        for skip in SKIPS:
            ds = ev.GetData(paths["dir"], paths["long"], mode="val", args=ev.args, skip=skip)
            identity, driving = dc.metas(paths)
            exprs = np.asarray(ds.all_exprs, dtype=np.float64)
            assert ds.auds.dtype == torch.float32 and ds.background_img.dtype == torch.float64
            assert np.array_equal(ds.background_img.numpy(), bcs[0] / 255.0)     # stored once, as `bc`
            assert not len(rows_of(exprs, [f["exp"] for f in identity["frames"]], must=False))
            out.update({f"gd_skip{skip}_poses": np.asarray(ds.all_poses), f"gd_skip{skip}_aud_rows": rows_of(ds.auds.numpy(), np.load(paths["long"])),
                        f"gd_skip{skip}_expr_rows": rows_of(exprs, [f["exp"] for f in driving["frames"]]),
                        f"gd_skip{skip}_scalars": np.asarray([ds.focal, ds.cx, ds.cy, ds.H, ds.W, ds.data_size], dtype=np.float64)})
    target = os.path.join(HERE, "drive_loaders.npz")
    np.savez_compressed(target, **out)
    print(f"wrote {target}: {len(out)} arrays, {os.path.getsize(target) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
