"""The positional encoding's truth, bound and probes, without a GPU (tests/pe_common.py; the GPU side: tests/test_pe_gpu.py).

1  the reference encoder (oracle.positional_encoding, fp32 torch) is within 2^-23 of the fp64 truth on the test vectors;
2  the arithmetic csrc/mlp_common.h states, restated in numpy, stays within the bound on them -- so a GPU failure points at
   the implementation, not at the scheme;
3  the probe networks return the selected columns of [gamma_10(p) | gamma_4(d)] through oracle.facenerf_forward."""
import numpy as np
import pytest
import torch

import oracle
import pe_common as pc


@pytest.fixture(scope="module")
def V():
    return pc.vectors()


def test_vectors_cover_the_edges(V):
    assert V.shape == (386, 3) and V.shape[0] % 128 == 2
    flat = V.reshape(-1)
    assert np.unique(flat).size == flat.size - 1                       # +0.0 == -0.0, every other value once
    assert sorted(np.signbit(flat[flat == 0]).tolist()) == [False, True]
    a = np.abs(V)
    assert (a[:, 0] != a[:, 1]).all() and (a[:, 1] != a[:, 2]).all() and (a[:, 0] != a[:, 2]).all()
    have = set(pc.bits(flat).tolist())
    for e in range(-30, 18):
        for s in (1.0, -1.0):
            assert int(np.float32(s * 2.0 ** e).view(np.int32)) in have
    for b in range(10):
        for k in range(-9, 10):
            v = np.float32(k * np.pi / 2 / 2.0 ** b)
            for w in (v, np.nextafter(v, np.float32(np.inf), dtype=np.float32)):
                assert w == 0 or int(w.view(np.int32)) in have, (b, k)
    assert float(a.max()) > 2.0 ** 16 and float(a[a > 0].min()) < 2.0 ** -39
    small = pc.small_rows(V)
    assert small.size > 256, "the 16-bit probes need more than two tiles of vectors"
    assert float(np.abs(V[small]).max()) == float(np.abs(pc.directions(V)[small]).max()) == pc.SMALL
    assert np.array_equal(V, pc.vectors()), "deterministic"


def test_reference_encoder_is_within_half_an_ulp_of_the_truth(V):
    for L in (pc.L_PTS, pc.L_DIR):
        got = oracle.positional_encoding(torch.from_numpy(V), L).numpy()
        assert got.dtype == np.float32 and got.shape == (386, pc.channels(L))
        want = pc.truth(V, L)
        assert np.array_equal(pc.bits(got[:, :3]), pc.bits(V))
        err = np.abs(got.astype(np.float64) - want)[:, 3:].max()
        print(f"\noracle.positional_encoding, {L} bands: worst |fp32 - fp64 truth| = {err:.2e} (bound 2^-23 = {2.0 ** -23:.2e})")
        assert err <= 2.0 ** -23, err


def test_the_header_arithmetic_meets_the_bound(V):
    """fp64 fract, 64-bit phase, shift, offset, int32 residual, five coefficients with fp32 roundings: every element."""
    for L in (pc.L_PTS, pc.L_DIR):
        got = pc.header_encoding(V, L)
        assert got.dtype == np.float32 and np.array_equal(pc.bits(got[:, :3]), pc.bits(V))
        err = np.abs(got.astype(np.float64) - pc.truth(V, L))
        bnd = pc.bound(V, L)
        share = err[:, 3:] / bnd[:, 3:]
        r, c = np.unravel_index(np.argmax(share), share.shape)
        b, fn, ax = pc.column_band(c + 3)
        print(f"\nheader arithmetic, {L} bands: worst abs err {err[:, 3:].max():.3e}; worst share of the bound {share.max():.2f} "
              f"at {fn}(2^{b} x), x = {V[r, ax]!r}")
        assert (err[:, 3:] <= bnd[:, 3:]).all(), (share.max(), b, fn, V[r, ax])


def test_probe_networks_return_the_selected_columns(V):
    x = torch.from_numpy(V)
    d = torch.from_numpy(pc.directions(V))
    ep, ed = oracle.positional_encoding(x, pc.L_PTS), oracle.positional_encoding(d, pc.L_DIR)
    rows = torch.cat([ep, ed], dim=-1)
    zero = lambda n: torch.zeros(n)
    groups = pc.probe_groups()
    assert len(groups) == 23
    for sig, rgb in groups:
        p = pc.probe_params(sig, rgb)
        with torch.no_grad():
            out = oracle.facenerf_forward(p, rows, zero(64), zero(76), zero(32), pc.DIMS)
        assert torch.equal(out, pc.probe_columns(ep, ed, sig, rgb)), (sig, rgb)
