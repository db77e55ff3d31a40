"""Shared by tests/test_pe_cpu.py and tests/test_pe_gpu.py (not collected by pytest): the inputs, the fp64 truth, the bound
and the probe networks of the positional-encoding tests.

The kernels compute gamma_10(point) and gamma_4(view direction) themselves (csrc/mlp_common.h: PeAxes, pe_phase, pe_slot):
a 64-bit fixed-point phase from one fp64 multiply and fract, a funnel shift per band, a quarter-turn offset for cos, an
integer half-turn reduction and sign, one odd polynomial.  ``header_encoding`` restates that arithmetic in numpy.

Truth: fp64 sin / cos of the exact fp32 argument fl32(2^b x) -- what the reference evaluates (helper.py:183-201), and 2^b x
is exact.  Bound, per element and absolute: 2^-22 + 2^b |x| 2^-51.  2^-22 is the header comment's own claim (2 ulp at 1.0);
the second term is the phase's three roundings of relative size 2^-53 each (the constant 1 / 2pi, the product, the
conversion to fixed point), each worth 2pi 2^b |x / 2pi| 2^-53 = 2^b |x| 2^-53 radians: 3 <= 4 = 2^2 of them."""
import numpy as np
import torch

import oracle

L_PTS, L_DIR = 10, 4
N_VEC = 3 * 128 + 2        # three 128-point tiles and a ragged tail of two
SMALL = 4.0                # the plain-bf16 and the fp16x3 probes run on the vectors with every |axis| <= SMALL


def channels(octaves: int) -> int:
    return 3 + 6 * octaves


def _band_edges():
    """fl32(k pi / 2 / 2^b) and its fp32 neighbour (towards +inf) for every band b < 10, k = -9..9: the features' zeros, their
    +-1 extrema and the half-turn rounding edge, where the residual reaches +-2^31."""
    out = []
    for b in range(L_PTS):
        for k in range(-9, 10):
            v = np.float32(k * np.pi / 2 / 2.0 ** b)
            out += [v, np.nextafter(v, np.float32(np.inf), dtype=np.float32)]
    return np.array(out, np.float32)


def vectors() -> np.ndarray:
    """V [386, 3] fp32, deterministic.  1158 different values (+0.0 and -0.0 count as two): the band edges, the exact powers
    of two 2^-30 .. 2^17 of both signs, both zeros, and the rest half uniform in [-1.5, 1.5], half log-uniform in magnitude
    over 2^-40 .. 2^17 with a random sign.  The values with |x| <= SMALL fill the first rows and the larger ones the last, so
    that most vectors qualify for the 16-bit probes; then the rows are shuffled over the tiles.  The three axes of a vector
    always differ (in magnitude, too), so an axis mix-up between the lane halves shows."""
    rs = np.random.RandomState(20)
    fixed = np.concatenate([_band_edges(),
                            [s * np.float32(2.0 ** e) for e in range(-30, 18) for s in (1, -1)]]).astype(np.float32)
    fixed = np.unique(fixed[fixed != 0])
    n_rest = 3 * N_VEC - 2 - fixed.size
    uni = rs.uniform(-1.5, 1.5, n_rest // 2).astype(np.float32)
    logu = (np.exp2(rs.uniform(-40.0, 17.0, n_rest - n_rest // 2)) * rs.choice([-1.0, 1.0], n_rest - n_rest // 2)).astype(np.float32)
    vals = np.concatenate([fixed, uni, logu])
    assert np.unique(vals).size == vals.size == 3 * N_VEC - 2
    small, large = vals[np.abs(vals) <= SMALL], vals[np.abs(vals) > SMALL]
    zeros = np.array([0.0, -0.0], np.float32)
    for attempt in range(64):
        flat = np.concatenate([rs.permutation(np.concatenate([small, zeros])), rs.permutation(large)])
        V = flat.reshape(N_VEC, 3)
        a = np.abs(V)
        if (a[:, 0] != a[:, 1]).all() and (a[:, 1] != a[:, 2]).all() and (a[:, 0] != a[:, 2]).all():
            break
    else:
        raise AssertionError("no arrangement with three different magnitudes per vector")
    V = np.ascontiguousarray(V[rs.permutation(N_VEC)])
    assert V.dtype == np.float32 and V.shape == (N_VEC, 3) and np.isfinite(V).all()
    return V


def directions(V: np.ndarray) -> np.ndarray:
    """The view directions that go with the points V: the same vectors in reverse order -- the same set through both
    encodings, never the same vector in both of one point, so that a point / direction mix-up cannot cancel."""
    return np.ascontiguousarray(V[::-1])


def small_rows(V: np.ndarray) -> np.ndarray:
    """Rows whose point V[r] and direction directions(V)[r] both have every |axis| <= SMALL."""
    return np.nonzero((np.abs(V) <= SMALL).all(1) & (np.abs(directions(V)) <= SMALL).all(1))[0]


def truth(V: np.ndarray, octaves: int) -> np.ndarray:
    """gamma_L(V) in fp64 [n, 3 + 6 L]: the raw columns, then sin / cos of the exact fp32 argument fl32(2^b x)."""
    V = np.asarray(V, np.float32)
    cols = [V.astype(np.float64)]
    for b in range(octaves):
        arg = (V * np.float32(2.0 ** b)).astype(np.float32)
        assert np.array_equal(arg.astype(np.float64), V.astype(np.float64) * 2.0 ** b), "2^b x is exact"
        cols += [np.sin(arg.astype(np.float64)), np.cos(arg.astype(np.float64))]
    return np.concatenate(cols, axis=1)


def bound(V: np.ndarray, octaves: int) -> np.ndarray:
    """The absolute bound of every column of gamma_L(V) [n, 3 + 6 L]; 0 for the raw columns (they are compared bit for bit)."""
    a = np.abs(np.asarray(V, np.float32).astype(np.float64))
    cols = [np.zeros_like(a)]
    for b in range(octaves):
        cols += [2.0 ** -22 + 2.0 ** b * a * 2.0 ** -51] * 2
    return np.concatenate(cols, axis=1)


def column_band(k: int):
    """(band, 'sin' / 'cos', axis) of trig column k >= 3 of an encoding."""
    t = k - 3
    return t // 6, ("sin", "cos")[(t % 6) // 3], k % 3


def per_band_worst(got: np.ndarray, V: np.ndarray, octaves: int):
    """{"sin": [...], "cos": [...]} per band: the worst |got - truth| and its share of the bound at that element."""
    err = np.abs(np.asarray(got, np.float64) - truth(V, octaves))
    share = np.divide(err, bound(V, octaves), out=np.zeros_like(err), where=bound(V, octaves) > 0)
    out = {"sin": [], "cos": []}
    for b in range(octaves):
        for i, fn in enumerate(("sin", "cos")):
            sl = slice(3 + 6 * b + 3 * i, 6 + 6 * b + 3 * i)
            out[fn].append(dict(band=b, worst_abs_err=float(err[:, sl].max()), worst_share_of_bound=float(share[:, sl].max())))
    return out


def bits(a) -> np.ndarray:
    """The int32 bit patterns of an fp32 array (torch or numpy)."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------ the header's arithmetic
def _fma(a, b, c):
    """fl32(a b + c): the product of two fp32 is exact in fp64; the sum rounds in fp64, then to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def header_encoding(V: np.ndarray, octaves: int) -> np.ndarray:
    """gamma_L(V) fp32 [n, 3 + 6 L] by the arithmetic csrc/mlp_common.h states: phase = fract(x * fl64(1 / 2pi)) in fp64 as
    64-bit fixed point (two truncating 32-bit conversions), band b = the 32 bits from bit 63 - b down, cos = + a quarter
    turn, + 2^30 to round to the nearest half turn (bit 31 of the sum = the half turn's parity), the residual times two as an
    int32, to fp32, times fl32(2pi / 2^33), the five-coefficient odd polynomial with fp32 roundings, the sign."""
    V = np.asarray(V, np.float32)
    ph = V.astype(np.float64) * 0.15915494309189535
    fr = np.minimum(ph - np.floor(ph), 1.0 - 2.0 ** -53)          # v_fract_f64: x - floor(x), clamped below 1
    t = fr * 4294967296.0
    hi = np.floor(t)
    lo = np.floor((t - hi) * 4294967296.0)
    phase = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    cols = [V]
    M = np.uint64(0xFFFFFFFF)
    for b in range(octaves):
        T = ((phase << np.uint64(b)) >> np.uint64(32)) & M
        for sc in (0, 1):
            u = (T + np.uint64((sc << 30) + (1 << 30))) & M
            rr2 = (((u << np.uint64(1)) + np.uint64(0x80000000)) & M).astype(np.uint32).view(np.int32)
            x = rr2.astype(np.float32) * np.float32(7.3145905512e-10)
            s2 = x * x
            pp = np.full_like(x, np.float32(-2.391218132e-08))
            for c in (2.752665757e-06, -1.984089153e-04, 8.333331268e-03, -1.666666663e-01):
                pp = _fma(pp, s2, np.full_like(x, np.float32(c)))
            r = _fma(x * s2, pp, x)
            cols.append(np.where((u >> np.uint64(31)) & np.uint64(1), -r, r).astype(np.float32))
    return np.concatenate(cols, axis=1)


# ------------------------------------------------------------------------------------------------ probe networks
DIMS = oracle.facenerf_dims()          # 63 / 27 input columns, 64 / 76 / 32 conditioning columns


def probe_groups():
    """23 groups of four features ("p", column of gamma_10) / ("d", column of gamma_4): (sigma's, rgb's three).  sigma can
    read a point feature only (it leaves the trunk); the 23 sigmas take point columns 0..22, the 69 colour channels the
    other 40 point columns and the 27 direction columns (the last group repeats two direction columns).  All 90 are read."""
    rest = [("p", j) for j in range(23, 63)] + [("d", k) for k in range(27)] + [("d", 0), ("d", 1)]
    groups = [(("p", g), tuple(rest[3 * g:3 * g + 3])) for g in range(23)]
    seen = {groups[g][0] for g in range(23)} | {f for _, rgb in groups for f in rgb}
    assert seen == {("p", j) for j in range(63)} | {("d", k) for k in range(27)}
    return groups


def probe_params(sigma_feature, rgb_features, dims=DIMS):
    """A FaceNeRF of unit weights whose four outputs ARE four input features.

    pts_linears.0: +1 at column j in row j and -1 at column j in row 64 + j (every j < 63), so a1 = [relu(f) | relu(-f) | 0];
    layers 1..7 are identities (on the skip layer: on its a4 block); alpha_linear takes row j minus row 64 + j = f_j;
    views_linears.0 has a +-1 row pair (c, 64 + c) per colour channel on that difference of h7 columns or on one direction
    column; views_linears.1 / .2 are identities and rgb_linear takes row c minus row 64 + c.  Conditioning columns and
    biases are zero.  Every sum has one non-zero term, so fp32 evaluation in any order returns the feature itself (a -0.0
    comes back as +0.0)."""
    shapes = oracle.facenerf_param_shapes(dims)
    p = {k: torch.zeros(s, dtype=torch.float32) for k, s in shapes.items()}
    pc, W = dims["input_ch"], dims["W"]
    c_all = pc + dims["dim_aud"] + dims["dim_expr"] + dims["dim_latent"]
    for j in range(pc):
        p["pts_linears.0.weight"][j, j] = 1.0
        p["pts_linears.0.weight"][64 + j, j] = -1.0
    eye = torch.eye(W)
    for i in range(1, dims["D"]):
        if (i - 1) in dims["skips"]:
            p[f"pts_linears.{i}.weight"][:, c_all:] = eye
        else:
            p[f"pts_linears.{i}.weight"].copy_(eye)
    kind, j = sigma_feature
    assert kind == "p"
    p["alpha_linear.weight"][0, j] = 1.0
    p["alpha_linear.weight"][0, 64 + j] = -1.0
    v0 = p["views_linears.0.weight"]           # columns [h (W) | gamma(dir) | expr / 3], face_nerf.py:67
    for c, (kind, j) in enumerate(rgb_features):
        if kind == "p":
            v0[c, j], v0[c, 64 + j] = 1.0, -1.0
            v0[64 + c, j], v0[64 + c, 64 + j] = -1.0, 1.0
        else:
            v0[c, W + j], v0[64 + c, W + j] = 1.0, -1.0
        p["rgb_linear.weight"][c, c] = 1.0
        p["rgb_linear.weight"][c, 64 + c] = -1.0
    for i in (1, 2):
        p[f"views_linears.{i}.weight"].copy_(torch.eye(W // 2))
    return p


def probe_columns(enc_pts, enc_dir, sigma_feature, rgb_features):
    """The [n, 4] block (rgb, sigma) a probe network returns: the selected columns of the two encodings."""
    pick = lambda f: (enc_pts if f[0] == "p" else enc_dir)[:, f[1]]
    return torch.stack([pick(f) for f in rgb_features] + [pick(sigma_feature)], dim=1)
