"""Whole-clip rendering, the parts that need no GPU: which rank renders which frame, the ordered assembly of the
ranks' frames in front of one writer (child ranks over gloo, worker tests/clip_worker.py), and the C ABI's declaration of
the fused clip tail."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frames_of_partitions_the_clip():
    """Rank r renders frames r, r + N, ...: disjoint increasing shares that cover the clip and differ by at most one."""
    from idealnerf_amd.parallel import frames_of
    for world in (1, 2, 3, 8):
        for n in (0, 1, 7, 10, 16):
            shares = [list(frames_of(r, world, n)) for r in range(world)]
            flat = [j for s in shares for j in s]
            assert len(flat) == len(set(flat)) and sorted(flat) == list(range(n)), (world, n, shares)
            assert all(s == sorted(s) and len(set(s)) == len(s) for s in shares)
            sizes = [len(s) for s in shares]
            assert max(sizes) - min(sizes) <= 1, (world, n, sizes)
            assert all(s == list(range(r, n, world)) for r, s in enumerate(shares))
    with pytest.raises(ValueError):
        frames_of(2, 2, 4)


def _decode_raw(path, H, W):
    from idealnerf_amd.frame_io import read_avi_chunks
    info, chunks = read_avi_chunks(path)
    row = (W * 3 + 3) & ~3
    frames = [np.frombuffer(c, dtype=np.uint8).reshape(H, row)[::-1, :W * 3].reshape(H, W, 3) for c in chunks]
    return info, frames


def test_ordered_assembly_gloo_three_ranks(tmp_path):
    """10 frames over 3 ranks (shares of 4, 3, 3: the last round is uneven), one gather per round, rank 0 writes: the raw
    AVI holds frames 0..9 in order, byte-equal; the frame rank 2 marked non-finite is reported; and one rank without a
    process group writes the same file byte for byte."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, OMP_NUM_THREADS="1", IDN_DIST_TIMEOUT_S="90")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    many = str(tmp_path / "three.avi")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "tests", "clip_worker.py"), "assemble", many],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = sorted((json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")), key=lambda d: d["rank"])
    assert [d["rank"] for d in lines] == [0, 1, 2]
    assert lines[0]["result"] == {"n_frames": cw.ASM_FRAMES, "nonfinite_frames": [cw.ASM_BAD]}
    assert lines[1]["result"] is None and lines[2]["result"] is None
    assert cw.ASM_BAD % 3 == 2     # rank 2's frame
    info, frames = _decode_raw(many, cw.ASM_H, cw.ASM_W)
    assert info["frames"] == cw.ASM_FRAMES == len(frames) and (info["width"], info["height"]) == (cw.ASM_W, cw.ASM_H)
    for j, f in enumerate(frames):
        np.testing.assert_array_equal(f, cw.assembly_frame(j), err_msg=f"frame {j}")
    assert len({cw.assembly_frame(j).tobytes() for j in range(cw.ASM_FRAMES)}) == cw.ASM_FRAMES   # the frames do differ
    one = str(tmp_path / "one.avi")
    assert not torch.distributed.is_initialized()
    assert cw.assemble(one, 0, 1) == {"n_frames": cw.ASM_FRAMES, "nonfinite_frames": [cw.ASM_BAD]}
    assert open(one, "rb").read() == open(many, "rb").read()


def test_assembler_refuses_a_wrong_call_sequence(tmp_path):
    from idealnerf_amd.parallel import ClipAssembler
    sink = cw.HostSink(str(tmp_path / "x.avi"), cw.ASM_W, cw.ASM_H)
    asm = ClipAssembler(sink, 2)
    with pytest.raises(ValueError):
        asm.push(None)                 # rank 0 owes frame 0
    asm.push(cw.assembly_frame(0))
    with pytest.raises(RuntimeError):
        asm.close()                    # one round short
    asm.push(cw.assembly_frame(1))
    with pytest.raises(RuntimeError):
        asm.push(cw.assembly_frame(2))
    assert asm.close() == {"n_frames": 2, "nonfinite_frames": []}
    with pytest.raises(ValueError):
        ClipAssembler(None, 2)         # rank 0 without a sink


def test_compose_to8b_is_declared_and_bound():
    import idealnerf_amd
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "idealnerf.h")).read(), flags=re.S)
    m = re.search(r"int\s+idealnerf_compose_to8b\s*\(([^)]*)\)", src)
    assert m, "include/idealnerf.h does not declare idealnerf_compose_to8b"
    assert len(m.group(1).split(",")) == 9
    res, args = idealnerf_amd._lib.PROTOTYPES["idealnerf_compose_to8b"]
    assert len(args) == 9
    lib = idealnerf_amd._lib.load()
    assert hasattr(lib, "idealnerf_compose_to8b") and lib.idealnerf_version() == 4
    # argument errors come back before any launch (no GPU is touched: this runs on the CPU box)
    assert lib.idealnerf_compose_to8b(None, None, None, 0, 0, None, None, None, None) == 0       # nothing to do
    assert lib.idealnerf_compose_to8b(None, None, None, 4, 0, None, None, None, None) != 0
    assert lib.idealnerf_compose_to8b(None, None, None, -1, 0, None, None, None, None) != 0
    with pytest.raises(idealnerf_amd._lib.IdealNerfError):
        idealnerf_amd.ops.compose_to8b(torch.zeros(4, 3), torch.zeros(4), torch.zeros(4, 3))    # CPU tensors: no fallback
