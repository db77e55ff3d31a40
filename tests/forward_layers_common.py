"""Shared by tests/test_forward_layers_cpu.py and tests/test_forward_layers_gpu.py (not collected by pytest): the slab views,
the layer-by-layer reference, the exact operands and the comparison helpers of the training-forward tests.  No GPU and no
library import here: everything is torch on whatever device the operands live on.

The activation slab (csrc/idn_internal.h: act_off, kActCols): matrix i is the row-major [p_pad, width_i] block at floats
[act_off(i) p_pad, (act_off(i) + width_i) p_pad), in the order x0 64 | dir 64 | a1..a8 256 each | v1..v3 128 each, p_pad = n
rounded up to 128; behind the 2560 columns stand 88 floats of ReLU mask words per point.

``ref_layers`` restates oracle.facenerf_forward layer by layer and returns the thirteen outputs of OUT_NAMES; with ``given``
(the kernel's own stored matrices) every layer is evaluated on the stored output of the layer before it, so a layer's figure
is the rounding of that layer alone.

The exact operands (``exact_net`` / ``exact_rows`` / ``exact_reference``): weights +-1 at a few columns per row, integer
biases, inputs and conditioning, such that every layer's sum |w||in| + |b| is an integer below 2^24.  Then every partial sum,
in any order, is exact in fp32; every value splits exactly into three bf16 pieces of 8 significand bits each; against a +-1
weight (one non-zero piece) only the products a1 w1, a2 w1, a3 w1 are non-zero, and the six-piece kernel keeps all three.
fp32 MFMA chains, bf16 piece products and fp64 therefore agree exactly, and the assertions are equalities."""
import torch

import oracle

DIMS = [(64, 76, 32), (106, 0, 0), (64, 0, 0)]       # (dim_aud, dim_expr, dim_latent): head, torso, no expr / latent
DIMS_ID = ["head", "torso", "aud"]
ACT_COLS, MASK_FLOATS = 2560, 88
ACT_NAMES = ["x0", "dir"] + [f"a{i}" for i in range(1, 9)] + ["v1", "v2", "v3"]
ACT_WIDTH = [64, 64] + [256] * 8 + [128] * 3
ACT_OFF = [sum(ACT_WIDTH[:i]) for i in range(13)]
HIDDEN = ACT_NAMES[2:]                               # the eleven stored hidden matrices, in mask-layer order
OUT_NAMES = [f"a{i}" for i in range(1, 9)] + ["sigma", "v1", "v2", "v3", "rgb"]
KEY = {**{f"a{i + 1}": f"pts_linears.{i}" for i in range(8)}, "sigma": "alpha_linear", "v1": "views_linears.0",
       "v2": "views_linears.1", "v3": "views_linears.2", "rgb": "rgb_linear"}
# where the folded bias block holds the bias of each output (csrc/idn_internal.h: bias_off; sigma is channel 128 of the
# 160-wide block of views_linears.0)
FOLD_OFF = {**{f"a{i + 1}": 256 * i for i in range(8)}, "v1": 2048, "sigma": 2048 + 128, "v2": 2208, "v3": 2336, "rgb": 2464}
FOLD_BIASES, FOLD_ALPHA, FOLD_RGB, FOLD_FLOATS = 2496, 2496, 2752, 3136


def padded(n):
    return (n + 127) // 128 * 128


def oracle_dims(dims3, widths=(63, 27)):
    return oracle.facenerf_dims(dim_aud=dims3[0], dim_expr=dims3[1], dim_latent=dims3[2], input_ch=widths[0],
                                input_ch_views=widths[1])


# ------------------------------------------------------------------------------------------------ slab views
def slab_matrix(acts, i, p_pad):
    """Matrix i (index into ACT_NAMES) of a slab as a [p_pad, width] view."""
    return acts[ACT_OFF[i] * p_pad:(ACT_OFF[i] + ACT_WIDTH[i]) * p_pad].view(p_pad, ACT_WIDTH[i])


def slab_views(acts, p_pad):
    """{name: [p_pad, width] view} of the thirteen matrices."""
    return {name: slab_matrix(acts, i, p_pad) for i, name in enumerate(ACT_NAMES)}


# ------------------------------------------------------------------------------------------------ reference
def layer_operands(w, dims, x_pts, x_dir, cond, given=None, folded0=None):
    """The thirteen layers as oracle.facenerf_forward evaluates them, in OUT_NAMES' order: a list of (name, W, input, bias,
    output), output = relu(input . W^T + bias) for the eleven hidden layers and without the ReLU for sigma and rgb.

    w: state-dict-keyed tensors; dims: oracle.facenerf_dims; cond = (aud, expr, latent), each of its width (possibly 0);
    everything of one dtype and device.  Layer 0 reads [x_pts | aud | expr / 3 | latent], layer 5 [x_pts | cond | a5], sigma
    a8, views_linears.0 [a8 | x_dir | expr / 3]; feature_linear is not applied.
    given {name: matrix}: the input of every layer behind the first is the GIVEN output of the layer before it.
    folded0 [256]: layer 0 is evaluated as the kernel runs it -- on x_pts alone, with this folded bias."""
    n = x_pts.shape[0]
    aud, expr, latent = cond
    expr3 = expr * 1 / 3
    c = torch.cat([aud, expr3, latent])[None, :].expand(n, -1)
    initial = torch.cat([x_pts, c], 1)
    out, got = [], {}

    def run(name, inp, relu, W=None, b=None):
        W = w[KEY[name] + ".weight"] if W is None else W
        b = w[KEY[name] + ".bias"] if b is None else b
        y = torch.addmm(b, inp, W.t())
        y = torch.relu(y) if relu else y
        out.append((name, W, inp, b, y))
        got[name] = y if given is None else given.get(name, y).to(y.dtype)

    if folded0 is None:
        run("a1", initial, True)
    else:
        run("a1", x_pts, True, w["pts_linears.0.weight"][:, :x_pts.shape[1]], folded0)
    for i in range(1, 8):
        h = got[f"a{i}"]
        run(f"a{i + 1}", torch.cat([initial, h], 1) if (i - 1) in dims["skips"] else h, True)
    run("sigma", got["a8"], False)
    run("v1", torch.cat([got["a8"], x_dir, expr3[None, :].expand(n, -1)], 1), True)
    run("v2", got["v1"], True)
    run("v3", got["v2"], True)
    run("rgb", got["v3"], False)
    return out


def ref_layers(w, dims, x_pts, x_dir, cond, given=None, folded0=None):
    """The thirteen outputs a1..a8, sigma [n, 1], v1, v2, v3, rgb [n, 3], in the dtype of the operands."""
    return [y for _, _, _, _, y in layer_operands(w, dims, x_pts, x_dir, cond, given, folded0)]


def layer_units(w, dims, x_pts, x_dir, cond, given=None, folded0=None):
    """sum |w||in| + |b| per element of the thirteen outputs: the unit every figure of these tests is stated in."""
    return [torch.addmm(b.abs(), inp.abs(), W.abs().t()) for _, W, inp, b, _ in layer_operands(w, dims, x_pts, x_dir, cond, given, folded0)]


def raw_of(outs):
    """[n, 4] = (rgb, sigma) of a list in OUT_NAMES' order: what the entries return."""
    return torch.cat([outs[OUT_NAMES.index("rgb")], outs[OUT_NAMES.index("sigma")]], 1)


def fold_reference(w, dims, cond):
    """The folded bias block (csrc/prep.hip: fold_kernel) in the dtype of the operands, [3136], and the unit
    |b| + sum |w||cond| of its first 2496 floats.  Slots no layer uses (channels 129..159 of views_linears.0's block,
    3..31 of rgb_linear's) hold 0.0 = the kernel's own b + dot with both left at zero; behind the biases stand copies of
    alpha_linear's weight row and rgb_linear's three."""
    aud, expr, latent = cond
    pc, vc = dims["input_ch"], dims["input_ch_views"]
    C = aud.numel() + expr.numel() + latent.numel()
    expr3 = expr * 1 / 3
    c = torch.cat([aud, expr3, latent])
    ref = torch.zeros(FOLD_FLOATS, dtype=c.dtype, device=c.device)
    unit = torch.zeros(FOLD_BIASES, dtype=c.dtype, device=c.device)
    for name in OUT_NAMES:
        W, b = w[KEY[name] + ".weight"], w[KEY[name] + ".bias"]
        o = FOLD_OFF[name]
        part, v = None, None
        if name in ("a1", "a6"):
            part, v = W[:, pc:pc + C], c
        elif name == "v1":
            part, v = W[:, 256 + vc:], expr3
        ref[o:o + b.numel()] = b if part is None else b + part @ v
        unit[o:o + b.numel()] = b.abs() if part is None else b.abs() + part.abs() @ v.abs()
    ref[FOLD_ALPHA:FOLD_RGB] = w["alpha_linear.weight"].reshape(-1)
    ref[FOLD_RGB:] = w["rgb_linear.weight"].reshape(-1)
    return ref, unit


# ------------------------------------------------------------------------------------------------ bf16 pieces
def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32; finite input.  csrc/prep.hip: bf16_rne."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return torch.where(r >= 2 ** 31, r - 2 ** 32, r).to(torch.int32).view(torch.float32).view(x.shape)


def bf16_pieces(x):
    """(p1, p2, p3) as fp32: p1 = bf16(x), p2 = bf16(x - p1), p3 = bf16(x - p1 - p2) -- the split of pack_bf16x6_kernel and
    of the six-piece kernels' activations."""
    p1 = bf16_rne(x)
    r1 = x - p1
    p2 = bf16_rne(r1)
    return p1, p2, bf16_rne(r1 - p2)


# ------------------------------------------------------------------------------------------------ comparison
def assert_same(got, ref, ctx, names=OUT_NAMES):
    """Equality by value of every matrix (+0 == -0), with the first differing element named (as the delta-chain tests do)."""
    assert len(got) == len(ref) == len(names), (len(got), len(ref), len(names))
    for name, g, r in zip(names, got, ref):
        assert g.shape == r.shape, (ctx, name, tuple(g.shape), tuple(r.shape))
        if not torch.equal(g, r):
            bad = (g != r).nonzero()
            row, col = (int(v) for v in bad[0])
            raise AssertionError(f"{ctx}: {name} differs in {bad.shape[0]} of {g.numel()} elements, first at row {row} (tile {row // 128}, "
                                 f"wave {row % 128 // 32}, point {row % 32}) column {col}: got {float(g[row, col])}, want {float(r[row, col])}")


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ exact operands
NNZ = 12           # non-zeros per weight row of a 256-wide trunk layer: the activations grow ~ sqrt(NNZ / 2) per layer
VIEW_NNZ = 8       # ... of pts_linears.0 and the 128-wide layers
HEAD_NNZ = 16      # ... of alpha_linear's row and rgb_linear's three
X_MAX, B_MAX, COND_MAX = 63, 255, 7
# (encoding, conditioning, trunk, direction, expression) non-zeros per row of the three layers with several sources; a share
# whose source has no columns (expr of the torso net) goes to the first source
SHARE = {"pts_linears.0": dict(enc=6, cond=2), "pts_linears.5": dict(enc=2, cond=2, trunk=8),
         "views_linears.0": dict(trunk=5, dir=2, expr=1)}


def exact_net(dims3, seed, widths=(63, 27)):
    """Weights in state-dict layout (CPU fp32).  Every row of every hidden layer has exactly NNZ (VIEW_NNZ) entries of +-1 at random
    columns (a row is one output channel: every output is a short sum); in the layers with several sources every source has
    its own share of them (SHARE), so that the encoding, conditioning, trunk and direction parts are present in every row,
    hence in every 32-row block.  alpha_linear's row and rgb_linear's three have HEAD_NNZ.  Biases: integers in [-B_MAX, B_MAX]
    drawn without replacement, so no two channels of a layer share one."""
    a, e, l = dims3
    pc, vc = widths
    C = a + e + l
    g = torch.Generator().manual_seed(seed)

    def block(rows, cols, nnz):
        """[rows, cols] with nnz entries of +-1 in every row, at distinct random columns."""
        if cols == 0 or nnz == 0:
            return torch.zeros(rows, cols)
        at = torch.rand((rows, cols), generator=g).argsort(1)[:, :nnz]
        sign = torch.randint(0, 2, (rows, nnz), generator=g).float() * 2 - 1
        return torch.zeros(rows, cols).scatter_(1, at, sign)

    def sourced(rows, parts):
        """parts: [(columns, share)]; the share of an empty source goes to the first."""
        spare = sum(s for c, s in parts if c == 0)
        parts = [(c, (s + spare if i == 0 else s) if c else 0) for i, (c, s) in enumerate(parts)]
        return torch.cat([block(rows, c, s) for c, s in parts], 1)

    def bias(n):
        return (torch.randperm(2 * B_MAX + 1, generator=g)[:n] - B_MAX).float()

    sd = {}
    s0, s5, sv = SHARE["pts_linears.0"], SHARE["pts_linears.5"], SHARE["views_linears.0"]
    sd["pts_linears.0.weight"] = sourced(256, [(pc, s0["enc"]), (C, s0["cond"])])
    for i in range(1, 8):
        sd[f"pts_linears.{i}.weight"] = block(256, 256, NNZ)
    sd["pts_linears.5.weight"] = sourced(256, [(256, s5["trunk"]), (pc, s5["enc"]), (C, s5["cond"])])
    sd["pts_linears.5.weight"] = torch.cat([sd["pts_linears.5.weight"][:, 256:], sd["pts_linears.5.weight"][:, :256]], 1).contiguous()
    sd["views_linears.0.weight"] = sourced(128, [(256, sv["trunk"]), (vc, sv["dir"]), (e, sv["expr"])])
    sd["views_linears.1.weight"], sd["views_linears.2.weight"] = block(128, 128, VIEW_NNZ), block(128, 128, VIEW_NNZ)
    sd["feature_linear.weight"] = torch.zeros(256, 256)          # built but never applied
    sd["alpha_linear.weight"], sd["rgb_linear.weight"] = block(1, 256, HEAD_NNZ), block(3, 128, HEAD_NNZ)
    for k in list(sd):
        sd[k.replace(".weight", ".bias")] = bias(sd[k].shape[0])
    want = oracle.facenerf_param_shapes(oracle_dims(dims3, widths))
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in want.items()}
    return sd


def exact_cond(dims3, seed):
    """(aud, expr, latent): integers in [-COND_MAX, COND_MAX]; expr three times such an integer, so that the kernels'
    expr * 1.0f / 3.0f and the reference's expr * 1 / 3 are the same exact integer."""
    g = torch.Generator().manual_seed(seed)
    draw = lambda d: torch.randint(-COND_MAX, COND_MAX + 1, (d,), generator=g).float()
    return draw(dims3[0]), 3 * draw(dims3[1]), draw(dims3[2])


def exact_rows(n, seed, widths=(63, 27), x_max=None):
    """x [n, pts_ch + views_ch] fp32, integers in [-x_max, x_max], no two rows alike (so a row stored in another's place
    shows)."""
    x_max = X_MAX if x_max is None else x_max
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-x_max, x_max + 1, (n, sum(widths)), generator=g).float()
    assert torch.unique(x, dim=0).shape[0] == n
    return x


def three_piece_rows(n, seed, widths=(63, 27)):
    """x [n, pts_ch + views_ch] fp32: integers of either sign with 2^19 <= |x| < 2^20 and three non-zero bf16 pieces each
    (an integer of 20 bits needs the third piece unless its low bits happen to vanish: those are drawn again)."""
    g = torch.Generator().manual_seed(seed)
    shape = (n, sum(widths))
    x = torch.zeros(shape)
    todo = torch.ones(shape, dtype=torch.bool)
    for _ in range(64):
        if not bool(todo.any()):
            break
        mag = torch.randint(2 ** 19, 2 ** 20, shape, generator=g).float()
        new = mag * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
        x = torch.where(todo, new, x)
        p1, p2, p3 = bf16_pieces(x)
        todo = (p2 == 0) | (p3 == 0)
    assert not bool(todo.any())
    p1, p2, p3 = bf16_pieces(x)
    assert torch.equal(p1 + p2 + p3, x) and bool((x.abs() < 2 ** 20).all()) and torch.unique(x, dim=0).shape[0] == n
    return x


def exact_reference(w64, dims, x, cond, check=OUT_NAMES, quantum=1.0, spread=True):
    """The fp64 ``ref_layers`` of x [n, pts_ch + views_ch] (any float dtype, exact values), cast to fp32, after the conditions
    that make equality legitimate -- asserted for every output named in `check`:
      * sum |w||in| + |b| of every element is below 2^24 quanta, and every value is a whole number of quanta (quantum 1: an
        integer), so every partial sum of any evaluation order is exact in fp32 and in three bf16 pieces;
    and, with `spread`, the conditions that make it telling:
      * every hidden matrix has an on-fraction in (0.05, 0.95);
      * at least 5 % of v3 and at least one element of a8 are >= 2^16: the third bf16 piece of an activation carries value.
    -> the thirteen outputs in OUT_NAMES' order (fp32)."""
    pc = dims["input_ch"]
    x64 = x.double()
    cond64 = [c.double().to(x.device) for c in cond]
    ops = layer_operands(w64, dims, x64[:, :pc], x64[:, pc:], cond64)
    for name, W, inp, b, y in ops:
        if name not in check:
            continue
        unit = torch.addmm(b.abs(), inp.abs(), W.abs().t())
        assert float(unit.max()) < 2 ** 24 * quantum, (name, float(unit.max()))
        assert bool((y / quantum == (y / quantum).round()).all()), name
        if spread and name in HIDDEN:
            frac = float((y > 0).double().mean())
            assert 0.05 < frac < 0.95, (name, frac)
    outs = [y for _, _, _, _, y in ops]
    if spread:
        v3, a8 = outs[OUT_NAMES.index("v3")], outs[OUT_NAMES.index("a8")]
        assert float((v3 >= 2 ** 16).double().mean()) >= 0.05, "fewer than 5 % of v3 reach the third bf16 piece"
        assert bool((a8 >= 2 ** 16).any()), "no element of a8 reaches the third bf16 piece"
    f32 = [y.float() for y in outs]
    for name, y, f in zip(OUT_NAMES, outs, f32):
        if name in check:
            assert torch.equal(f.double(), y), name
    return f32


def reference_stats(w64, dims, x, cond):
    """What exact_reference asserts, as figures: {name: (largest unit, on-fraction, share >= 2^16)}."""
    pc = dims["input_ch"]
    x64 = x.double()
    out = {}
    for name, W, inp, b, y in layer_operands(w64, dims, x64[:, :pc], x64[:, pc:], [c.double() for c in cond]):
        unit = torch.addmm(b.abs(), inp.abs(), W.abs().t())
        out[name] = (float(unit.max()), float((y > 0).double().mean()), float((y >= 2 ** 16).double().mean()))
    return out


# the cases of the exact tests: (dims3, n, widths); E2's n depends on the CU count (multi_tile_rows)
E1_ROWS = (128, 185, 640)
NARROW = (33, 15)


def multi_tile_rows(cus):
    """E2: 2 cus + 3 tiles, the last one ragged: every workgroup of a grid of `cus` walks two tiles, three a third."""
    return 128 * (2 * cus + 3) - 37


def net_seed(dims3, widths=(63, 27)):
    return 300 + 10 * DIMS.index(dims3) + (1 if widths != (63, 27) else 0)


def exact_case(dims3, n, widths=(63, 27), device="cpu"):
    """(sd fp32, w64, oracle dims, cond, x, reference) of one exact case, everything on `device`."""
    dims = oracle_dims(dims3, widths)
    sd = {k: v.to(device).contiguous() for k, v in exact_net(dims3, net_seed(dims3, widths), widths).items()}
    w64 = {k: v.double() for k, v in sd.items()}
    cond = [c.to(device) for c in exact_cond(dims3, 40 + DIMS.index(dims3))]
    x = exact_rows(n, 7 * n + DIMS.index(dims3), widths).to(device)
    return dict(sd=sd, w64=w64, dims=dims, cond=cond, x=x, ref=exact_reference(w64, dims, x, cond))


# E3: pts_linears.0 scaled to +-(2 + 2^-8 + 2^-16): three non-zero bf16 pieces per weight, 2, 2^-8 and 2^-16.  (Rounding to
# nearest, a weight in [1, 2) on a grid of 2^-16 never has a third piece: its remainder behind the first piece is at most 2^-8
# and spans bits 2^-9 .. 2^-16, eight of them, which one bf16 holds; 1 + 2^-8 + 2^-16 itself rounds UP to 1 + 2^-7 and leaves
# -(2^-8 - 2^-16), one piece.  In [2, 4) the remainder spans nine bits.)  |x| <= 7 and half-integer biases of at most 127.5
# keep sum |w||in| + |b| below 2^8, i.e. below 2^24 quanta of 2^-16.
E3_SCALE, E3_XMAX, E3_QUANTUM = 2.0 + 2.0 ** -8 + 2.0 ** -16, 7, 2.0 ** -16


def weight_piece_case(n, device="cpu"):
    """E3: the head net with layer 0 scaled by E3_SCALE and its bias halved; only a1 is exact (checked in quanta of 2^-16)."""
    dims3 = DIMS[0]
    dims = oracle_dims(dims3)
    sd = exact_net(dims3, net_seed(dims3))
    sd["pts_linears.0.weight"] = sd["pts_linears.0.weight"] * E3_SCALE
    sd["pts_linears.0.bias"] = sd["pts_linears.0.bias"] / 2
    p1, p2, p3 = bf16_pieces(sd["pts_linears.0.weight"])
    nz = sd["pts_linears.0.weight"] != 0
    assert bool((p1[nz].abs() == 2).all()) and bool((p2[nz].abs() == 2.0 ** -8).all()) and bool((p3[nz].abs() == 2.0 ** -16).all())
    sd = {k: v.to(device).contiguous() for k, v in sd.items()}
    w64 = {k: v.double() for k, v in sd.items()}
    cond = [c.to(device) for c in exact_cond(dims3, 40)]
    x = exact_rows(n, 7 * n + 50, x_max=E3_XMAX).to(device)
    ref = exact_reference(w64, dims, x, cond, check=("a1",), quantum=E3_QUANTUM, spread=False)
    frac = float((ref[0] > 0).double().mean())
    assert 0.05 < frac < 0.95 and bool((ref[0] * 2 ** 16 % 2 == 1).any()), "a1 must carry the third weight piece"
    return dict(sd=sd, w64=w64, dims=dims, cond=cond, x=x, ref=ref)


def input_piece_case(n, device="cpu"):
    """E4: the head net on rows of 20-bit integers with three non-zero bf16 pieces each; only a1 is exact (6 + 2 terms below
    2^20 each plus the bias: below 2^23)."""
    dims3 = DIMS[0]
    c = exact_case(dims3, 128, device=device)
    x = three_piece_rows(n, 7 * n + 60).to(device)
    ref = exact_reference(c["w64"], c["dims"], x, c["cond"], check=("a1",), spread=False)
    frac = float((ref[0] > 0).double().mean())
    assert 0.05 < frac < 0.95 and float((ref[0] >= 2 ** 16).double().mean()) > 0.3
    return dict(sd=c["sd"], w64=c["w64"], dims=c["dims"], cond=c["cond"], x=x, ref=ref)


# ------------------------------------------------------------------------------------------------ graded operands
def graded_net(dims3, seed, widths=(63, 27)):
    """Xavier weights (oracle.xavier_facenerf_params) with every bias replaced by uniform(-0.1, 0.1) per channel: a bias read
    from the wrong channel shows, which the initialisation's 0.01 everywhere cannot."""
    sd = oracle.xavier_facenerf_params(seed, oracle_dims(dims3, widths))
    g = torch.Generator().manual_seed(1000 + seed)
    for k in sd:
        if k.endswith(".bias"):
            sd[k] = (torch.rand(sd[k].shape, generator=g) * 0.2 - 0.1).float()
    return sd


def graded_cond(dims3, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(d, generator=g) * 0.3).float() for d in dims3]


STAGE_BOUND = 2e-7         # the floor of the rule: what the delta-chain T3 and the dW tests hold one fp32-grade product to
TORCH_MULT = 4.0           # ... or this multiple of torch's fp32 addmm of the same layer on the same inputs
X6_OVER_F32 = (4.0, 3e-8)  # bf16 pieces below 4 x the fp32 pipe + 3e-8


def chain_ceiling(k):
    """The derived ceiling of a layer of input width k in the unit sum |w||in| + |b|: k products summed in one fp32 chain
    ((k - 1) additions, each rounding a partial sum no larger than the unit), the bias addition and the three roundings a
    six-piece product may add -- (k + 3) 2^-24."""
    return (k + 3) * 2.0 ** -24
