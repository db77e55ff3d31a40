"""Shared by tests/test_inference_modes_cpu.py and tests/test_inference_modes_gpu.py (not collected by pytest): the exact
operands of the three 16-bit inference kernels (csrc/mlp_bf16x3.hip: mlp_bf16x3_kernel, mlp_bf16_kernel; csrc/mlp_fp16x3.hip)
and the comparison of their [n, 4] output.  No GPU and no library import here; the layer-by-layer reference, the piece
arithmetic and the graded operands are those of tests/forward_layers_common.py.

What each kernel does with a product a w (a: an input or a hidden activation, w: a weight; the bias is fp32 in all three):
  bf16x3   a = a_hi + a_lo, a_hi = bf16(a), a_lo = bf16(a - a_hi), round to nearest even; the weight stream holds w_hi and
           w_lo of the same split; a_hi w_hi + a_hi w_lo + a_lo w_hi on the bf16 matrix pipe, fp32 accumulators;
  fp16x3   the same with fp16 halves: the activations are split by truncation (v_cvt_pkrtz_f16_f32), the weights by rounding
           to nearest (pack_bf16x3_kernel, fmt 1);
  bf16     a and w rounded to one bf16 each.

The placed network (``placed_net``): weights +-1, integer biases, and the non-zeros of every row PLACED so that, for every
weight matrix and every source of it the kernels stream (the encoding, trunk and direction columns; the conditioning columns
are folded into the fp32 bias), every (32-row tile, 16-column k-step) pair holds a non-zero and every column is read by some
row -- no fragment of the packed stream is all zeros and no channel of an activation goes unread.  A hidden row has two
non-zeros per source, one +1 and one -1: relu(a - a' + b) is at most max a + |b|, so the activations grow by addition from
layer to layer and their range is bounded by the construction, whatever the number of rows.  alpha_linear's row and
rgb_linear's three are dense: every channel of a8 and of v3 reaches the output of every point.

The three operand sets, all with COND_MAX = 7:
  T(bf16x3)  |x| <= 1023, |b| <= 255: every input and hidden activation is an integer below 2^16, which two bf16 pieces hold
             exactly (the remainder behind 8 significand bits is an integer of at most 2^7), and most need the second;
  T(fp16x3)  |x| <= 8191, |b| <= 2047: integers below 65504 in two fp16 pieces of 11 bits each;
  P          |x| <= 31, |b| <= 7: every input and hidden activation is an integer of at most 8 bits, one bf16 -- by the
             construction at most 76 in a1, 7 more per layer and 45 more at each of the two joins: 222.  (With |x| <= 7 the
             biases outweigh the inputs and up to 45 of a layer's 256 channels are zero in every row: nothing behind a
             dead channel is observed.)
  W(mode, L) the P net with the weights of layer L multiplied by 1 + 2^-8 (bf16x3) or 1 + 2^-12 (fp16x3): w_hi = +-1,
             w_lo = +-2^-8 / +-2^-12; the inputs of L have one piece, so the dropped a_lo w_lo is zero and a_hi w_lo carries
             the fractions; everything is a whole number of quanta 2^-8 / 2^-12.
On each of them every sum |w||in| + |b| is below 2^24 quanta: every partial sum in any order is exact in fp32, the kept
products are all the non-zero ones, and the fp64 reference cast to fp32 is what a correct kernel returns -- bit for bit."""
import math

import torch

import oracle
import forward_layers_common as fc

X3_MODES = ("bf16x3", "fp16x3")
MODES16 = X3_MODES + ("bf16",)
ALL_MODES = ("f32",) + MODES16 + ("bf16x6",)
TILE = {"f32": 128, "bf16x3": 128, "fp16x3": 128, "bf16x6": 128, "bf16": 256}    # points per pass of a workgroup
RAW_NAMES = ("rgb0", "rgb1", "rgb2", "sigma")
LAYERS = fc.OUT_NAMES                                # the thirteen, in the reference's order (alpha_linear = "sigma")

# (x_max, b_max) of the sets
T_RANGE = {"bf16x3": (1023, 255), "fp16x3": (8191, 2047)}
P_RANGE = (31, 7)
W_LO = {"bf16x3": 2.0 ** -8, "fp16x3": 2.0 ** -12}
# non-zeros per row and source: (encoding, conditioning, trunk, direction, expression); a share whose source has no columns
# is dropped (the torso net has no expression)
SHARE = {"pts_linears.0": dict(enc=2, cond=1), "pts_linears.5": dict(trunk=2, enc=1, cond=1),
         "views_linears.0": dict(trunk=2, dir=1, expr=1)}
HIDDEN_NNZ = 2
P_ROWS = (256, 313, 1280)


def multi_tile_rows(cus, mode):
    """2 cus + 3 passes of the mode's tile, the last one ragged."""
    return TILE[mode] * (2 * cus + 3) - 37


# ------------------------------------------------------------------------------------------------ the splits
def rtz16(x):
    """fp32 -> fp16 toward zero, as fp32: the fp32 significand cut to 11 bits.  Valid where the result is a normal fp16:
    asserted, 2^-14 <= |x| < 65504 or x == 0."""
    mag = x.abs()
    assert bool(((x == 0) | ((mag >= 2.0 ** -14) & (mag < 65504))).all()), "outside the normal fp16 range"
    return (x.contiguous().view(torch.int32) & -8192).view(torch.float32).view(x.shape)


def f16_rne(x):
    """fp32 -> the nearest fp16, as fp32 (pack_bf16x3_kernel, fmt 1)."""
    return x.half().float()


def act_split(mode, v):
    """(hi, lo) as the kernel of `mode` splits an input or an activation v (fp32)."""
    if mode == "bf16x3":
        hi = fc.bf16_rne(v)
        return hi, fc.bf16_rne(v - hi)
    if mode == "fp16x3":
        hi = rtz16(v)
        return hi, rtz16(v - hi)
    assert mode == "bf16", mode
    return fc.bf16_rne(v), torch.zeros_like(v)


def weight_split(mode, w):
    """(hi, lo) as the pack kernel of `mode` splits a weight (fp32)."""
    if mode == "fp16x3":
        hi = f16_rne(w)
        return hi, f16_rne(w - hi)
    return act_split(mode, w)


def splits_exactly(mode, v64):
    """Every element of v64 (fp64) is an fp32 number whose pieces in `mode` add up to it."""
    v = v64.float()
    hi, lo = act_split(mode, v)
    return torch.equal(v.double(), v64) and torch.equal(hi.double() + lo.double(), v64)


def lo_share(mode, v64, of=None):
    """The share of the elements of v64 (of those where `of` holds) whose lo piece in `mode` is not zero."""
    lo = act_split(mode, v64.float())[1]
    pick = torch.ones_like(lo, dtype=torch.bool) if of is None else of
    return float((lo[pick] != 0).double().mean()) if bool(pick.any()) else 0.0


# ------------------------------------------------------------------------------------------------ the placed network
def placed_block(rows, cols, nnz, g, dense=False):
    """[rows, cols] of 0 / +-1 with nnz non-zeros in every row (all of them with `dense`).  Non-zero j of row r stands at
    position m = r + j rows of the sequence c(m) = 16 (m mod KS) + (m div KS) mod 16, KS = ceil(cols / 16) -- consecutive
    positions walk the k-steps, so any 32 consecutive rows touch every k-step, and positions 0 .. 16 KS - 1 hold every
    column -- for as many j as it takes rows to exhaust the sequence; a column beyond the matrix (the padding of the last
    k-step) becomes the last column.  What is left of the nnz is drawn from the generator.  Signs alternate from a drawn
    first one, so a row of two is one +1 and one -1; a dense row's are drawn."""
    if cols == 0 or nnz == 0:
        return torch.zeros(rows, cols)
    if dense or nnz >= cols:
        return torch.randint(0, 2, (rows, cols), generator=g).float() * 2 - 1
    ks = (cols + 15) // 16
    period = 16 * ks
    built = min(nnz, (period + rows - 1) // rows)
    first = torch.randint(0, 2, (rows,), generator=g).tolist()
    rs, cs, signs = [], [], []
    for r in range(rows):
        at = []
        for j in range(built):
            m = (r + j * rows) % period
            c = min(16 * (m % ks) + m // ks % 16, cols - 1)
            if c not in at:
                at.append(c)
        if len(at) < nnz:
            for c in torch.randperm(cols, generator=g).tolist():
                if c not in at:
                    at.append(c)
                    if len(at) == nnz:
                        break
        rs += [r] * len(at)
        cs += at
        signs += [(1.0 if first[r] else -1.0) * (-1.0) ** j for j in range(len(at))]
    out = torch.zeros(rows, cols)
    out[rs, cs] = torch.tensor(signs)
    return out


def placed_net(dims3, seed, widths=(63, 27), b_max=7, head_nnz=None):
    """Weights in state-dict layout (CPU fp32), see the module docstring.  Biases: integers in [-b_max, b_max] drawn WITH
    replacement (there may be fewer values than channels).  head_nnz None: dense heads."""
    a, e, l = dims3
    pc, vc = widths
    C = a + e + l
    g = torch.Generator().manual_seed(seed)
    s0, s5, sv = SHARE["pts_linears.0"], SHARE["pts_linears.5"], SHARE["views_linears.0"]
    blk = lambda rows, cols, nnz: placed_block(rows, cols, nnz, g)
    head = lambda rows, cols: placed_block(rows, cols, head_nnz or cols, g, dense=head_nnz is None)
    sd = {"pts_linears.0.weight": torch.cat([blk(256, pc, s0["enc"]), blk(256, C, s0["cond"])], 1)}
    for i in range(1, 8):
        sd[f"pts_linears.{i}.weight"] = blk(256, 256, HIDDEN_NNZ)
    sd["pts_linears.5.weight"] = torch.cat([blk(256, pc, s5["enc"]), blk(256, C, s5["cond"]), blk(256, 256, s5["trunk"])], 1)
    sd["views_linears.0.weight"] = torch.cat([blk(128, 256, sv["trunk"]), blk(128, vc, sv["dir"]), blk(128, e, sv["expr"])], 1)
    sd["views_linears.1.weight"], sd["views_linears.2.weight"] = blk(128, 128, HIDDEN_NNZ), blk(128, 128, HIDDEN_NNZ)
    sd["feature_linear.weight"] = torch.zeros(256, 256)          # built but never applied
    sd["alpha_linear.weight"], sd["rgb_linear.weight"] = head(1, 256), head(3, 128)
    for k in list(sd):
        sd[k.replace(".weight", ".bias")] = torch.randint(-b_max, b_max + 1, (sd[k].shape[0],), generator=g).float()
    want = oracle.facenerf_param_shapes(fc.oracle_dims(dims3, widths))
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in want.items()}
    return {k: v.contiguous() for k, v in sd.items()}


def streamed_sources(dims3, widths=(63, 27)):
    """{layer name: [(first column, columns)]}: the column ranges of each weight matrix that the kernels stream."""
    pc, vc = widths
    C = sum(dims3)
    out = {name: [(0, 256)] for name in ("a2", "a3", "a4", "a5", "a7", "a8", "sigma")}
    out.update(a1=[(0, pc)], a6=[(0, pc), (pc + C, 256)], v1=[(0, 256), (256, vc)], v2=[(0, 128)], v3=[(0, 128)], rgb=[(0, 128)])
    return out


def coverage(sd, dims3, widths=(63, 27)):
    """-> (empty, unread): the (layer, source, 32-row tile, k-step) pairs without a non-zero and the (layer, column) pairs no
    row reads, over every streamed source of every layer.  A head's one or three rows are one tile."""
    empty, unread = [], []
    for name, sources in streamed_sources(dims3, widths).items():
        W = sd[fc.KEY[name] + ".weight"]
        for si, (c0, cols) in enumerate(sources):
            part = W[:, c0:c0 + cols] != 0
            unread += [(name, c0 + int(c)) for c in (~part.any(0)).nonzero()]
            for t in range((W.shape[0] + 31) // 32):
                for s in range((cols + 15) // 16):
                    if not bool(part[32 * t:32 * t + 32, 16 * s:16 * s + 16].any()):
                        empty.append((name, si, t, s))
    return empty, unread


def integer_cond(dims3, seed):
    return fc.exact_cond(dims3, seed)


def integer_rows(n, seed, widths, x_max):
    return fc.exact_rows(n, seed, widths, x_max=x_max)


# ------------------------------------------------------------------------------------------------ the conditions
def checked_reference(kind, mode, w64, dims, x, cond, quantum=1.0, scaled=None):
    """The fp64 ``ref_layers`` of x, cast to fp32, after the conditions of the set -- kind "T" (two pieces of `mode`), "P" (one
    bf16) or "W" (layer `scaled` carries weight lo pieces of `quantum`):
      * every value is a whole number of quanta and every sum |w||in| + |b| is below 2^24 quanta;
      * every hidden matrix has an on-fraction in (0.05, 0.95), and at most 1 % of its channels are zero in every row;
      * T: every input and hidden activation splits exactly in two pieces of the mode; at least 5 % of the positive elements
        of a8 and of v3, of the input elements and of the input columns carry a non-zero lo piece;
      * P: every input and hidden activation is one bf16;
      * W: every input of layer `scaled` -- and every activation in front of it -- is one piece of the mode, at least one of
        its outputs is not a whole number, and every hidden activation behind it splits exactly in two pieces of the mode.
    -> the thirteen outputs in OUT_NAMES' order (fp32)."""
    pc = dims["input_ch"]
    x64 = x.double()
    ops = fc.layer_operands(w64, dims, x64[:, :pc], x64[:, pc:], [c.double().to(x.device) for c in cond])
    one = "bf16" if kind == "P" else mode
    behind = False
    for name, W, inp, b, y in ops:
        unit = torch.addmm(b.abs(), inp.abs(), W.abs().t())
        assert float(unit.max()) < 2 ** 24 * quantum, (name, float(unit.max()), quantum)
        assert bool((y / quantum == (y / quantum).round()).all()), name
        if name in fc.HIDDEN:
            frac = float((y > 0).double().mean())
            assert 0.05 < frac < 0.95, (name, frac)
            dead = int((y.max(0)[0] == 0).sum())
            assert dead <= y.shape[1] // 100, (name, dead, "channels are zero in every row")
    for name, W, inp, b, y in ops:                       # (in OUT_NAMES' order sigma stands behind a8 and reads nothing new)
        if kind == "W" and name == scaled:
            assert bool((inp == act_split(one, inp.float())[0].double()).all()), f"an input of {name} has a lo piece"
            assert bool((y != y.round()).any()), f"no output of {name} carries a weight lo piece"
            behind = name in fc.HIDDEN
        if name not in fc.HIDDEN:
            continue
        if kind == "T" or (kind == "W" and behind):
            assert splits_exactly(mode, y), f"{name} does not split into two pieces of {mode}"
        else:
            assert bool((y == act_split(one, y.float())[0].double()).all()), f"{name} is not one piece of {one}"
    if kind == "T":
        assert splits_exactly(mode, x64), "an input does not split into two pieces"
        outs = {name: y for name, _, _, _, y in ops}
        for name in ("a8", "v3"):
            share = lo_share(mode, outs[name], outs[name] > 0)
            assert share >= 0.05, (name, share)
        x_lo = act_split(mode, x)[1] != 0
        assert float(x_lo.double().mean()) >= 0.05 and float(x_lo[:, :pc].any(0).double().mean()) >= 0.05
    else:
        assert bool((x64 == act_split(one, x)[0].double()).all()), "an input is not one piece"
    f32 = [y.float() for _, _, _, _, y in ops]
    for name, (_, _, _, _, y), f in zip(fc.OUT_NAMES, ops, f32):
        assert torch.equal(f.double(), y), name
    return f32


def set_stats(mode, w64, dims, x, cond):
    """What checked_reference asserts, as figures: {name: (largest |value|, largest unit, on-fraction, lo share of the positive)}."""
    pc = dims["input_ch"]
    x64 = x.double()
    out = {}
    for name, W, inp, b, y in fc.layer_operands(w64, dims, x64[:, :pc], x64[:, pc:], [c.double() for c in cond]):
        unit = torch.addmm(b.abs(), inp.abs(), W.abs().t())
        out[name] = (float(y.abs().max()), float(unit.max()), float((y > 0).double().mean()),
                     lo_share(mode, y, y > 0) if name in fc.HIDDEN and mode != "bf16" else 0.0)
    return out


# ------------------------------------------------------------------------------------------------ the cases
def net_seed(kind, dims3, widths=(63, 27)):
    return 700 + 100 * "TPW".index(kind) + 10 * fc.DIMS.index(dims3) + (1 if widths != (63, 27) else 0)


def _case(kind, mode, sd, dims3, n, widths, x_max, device, quantum=1.0, scaled=None):
    dims = fc.oracle_dims(dims3, widths)
    sd = {k: v.to(device).contiguous() for k, v in sd.items()}
    w64 = {k: v.double() for k, v in sd.items()}
    cond = [c.to(device) for c in integer_cond(dims3, 60 + fc.DIMS.index(dims3))]
    x = integer_rows(n, 11 * n + fc.DIMS.index(dims3) + x_max, widths, x_max).to(device)
    ref = checked_reference(kind, mode, w64, dims, x, cond, quantum, scaled)
    return dict(kind=kind, mode=mode, sd=sd, w64=w64, dims=dims, dims3=dims3, widths=widths, cond=cond, x=x, ref=ref, raw=fc.raw_of(ref))


def two_piece_case(mode, dims3, n, widths=(63, 27), device="cpu"):
    """Set T of `mode` ("bf16x3" / "fp16x3")."""
    x_max, b_max = T_RANGE[mode]
    return _case("T", mode, placed_net(dims3, net_seed("T", dims3, widths), widths, b_max), dims3, n, widths, x_max, device)


def one_piece_case(dims3, n, widths=(63, 27), device="cpu"):
    """Set P."""
    x_max, b_max = P_RANGE
    return _case("P", "bf16", placed_net(dims3, net_seed("P", dims3, widths), widths, b_max), dims3, n, widths, x_max, device)


def weight_lo_case(mode, layer, n=185, device="cpu"):
    """Set W: the head-layout P net with the weights of `layer` (a name of LAYERS) times 1 + W_LO[mode]."""
    dims3 = fc.DIMS[0]
    x_max, b_max = P_RANGE
    sd = placed_net(dims3, net_seed("P", dims3), b_max=b_max)
    key = fc.KEY[layer] + ".weight"
    sd[key] = sd[key] * (1.0 + W_LO[mode])
    hi, lo = weight_split(mode, sd[key])
    nz = sd[key] != 0
    assert bool((hi[nz].abs() == 1).all()) and torch.equal(lo[nz], hi[nz] * W_LO[mode]) and not bool(hi[~nz].any()) and not bool(lo[~nz].any())
    assert torch.equal(hi.double() + lo.double(), sd[key].double())
    return _case("W", mode, sd, dims3, n, (63, 27), x_max, device, quantum=W_LO[mode], scaled=layer)


# ------------------------------------------------------------------------------------------------ mutated evaluations
def forward_with(w64, dims, x, cond, product=None):
    """raw [n, 4] (fp64) of ``ref_layers`` with every layer's product restated: product(name, inp, W) -> inp . W^T [n, rows]
    (fp64).  Without it this is the reference."""
    pc = dims["input_ch"]
    x64 = x.double()
    n = x64.shape[0]
    aud, expr, latent = [c.double() for c in cond]
    expr3 = expr * 1 / 3
    initial = torch.cat([x64[:, :pc], torch.cat([aud, expr3, latent])[None, :].expand(n, -1)], 1)
    got = {}

    def run(name, inp, relu):
        W, b = w64[fc.KEY[name] + ".weight"], w64[fc.KEY[name] + ".bias"]
        y = b + (inp @ W.t() if product is None else product(name, inp, W))
        got[name] = torch.relu(y) if relu else y

    run("a1", initial, True)
    for i in range(1, 8):
        h = got[f"a{i}"]
        run(f"a{i + 1}", torch.cat([initial, h], 1) if (i - 1) in dims["skips"] else h, True)
    run("sigma", got["a8"], False)
    run("v1", torch.cat([got["a8"], x64[:, pc:], expr3[None, :].expand(n, -1)], 1), True)
    run("v2", got["v1"], True)
    run("v3", got["v2"], True)
    run("rgb", got["v3"], False)
    return torch.cat([got["rgb"], got["sigma"]], 1)


def mode_product(mode, change=None):
    """The product of `mode` restated in torch for ``forward_with``: the operands split as the kernel and its pack kernel
    split them, the kept piece products summed in fp64 -- a_hi w_hi + a_hi w_lo + a_lo w_hi, or for "bf16" the one product
    of the rounded operands.  change(name, pieces) may alter the pieces {"a_hi", "a_lo", "w_hi", "w_lo"} (fp64, a: [n, cols],
    w: [rows, cols]) of a layer in place: a mistake of a kernel, restated."""
    def product(name, inp, W):
        a = inp.float()
        w = W.float()
        assert torch.equal(a.double(), inp) and torch.equal(w.double(), W), name
        a_hi, a_lo = act_split(mode, a)
        w_hi, w_lo = weight_split(mode, w)
        p = dict(a_hi=a_hi.double(), a_lo=a_lo.double(), w_hi=w_hi.double(), w_lo=w_lo.double())
        if change is not None:
            change(name, p)
        return p["a_hi"] @ p["w_hi"].t() + p["a_hi"] @ p["w_lo"].t() + p["a_lo"] @ p["w_hi"].t()
    return product


# ------------------------------------------------------------------------------------------------ comparison
def assert_same_raw(got, ref, ctx, tile=128):
    """Equality by value of raw [n, 4] (+0 == -0), with the first differing element named: which of rgb0..2 / sigma, in which
    pass of `tile` points, wave (32 points each) and point -- and how many differ per output and per wave of a pass."""
    assert got.shape == ref.shape and got.shape[1] == 4, (ctx, tuple(got.shape), tuple(ref.shape))
    if torch.equal(got, ref):
        return
    bad = got != ref
    idx = bad.nonzero()
    row, col = (int(v) for v in idx[0])
    per_col = {RAW_NAMES[c]: int(bad[:, c].sum()) for c in range(4) if bool(bad[:, c].any())}
    rows = bad.any(1).nonzero().flatten()
    waves = torch.bincount(rows % tile // 32, minlength=tile // 32).tolist()
    tiles = torch.unique(rows // tile)
    raise AssertionError(f"{ctx}: raw differs in {idx.shape[0]} of {got.numel()} elements ({per_col}; rows per wave of a pass {waves}; "
                         f"{tiles.numel()} of {math.ceil(got.shape[0] / tile)} tiles, the first {tiles[:8].tolist()}), first at row {row} "
                         f"(tile {row // tile}, wave {row % tile // 32}, point {row % 32}) {RAW_NAMES[col]}: got {float(got[row, col])!r}, "
                         f"want {float(ref[row, col])!r}")


# ------------------------------------------------------------------------------------------------ graded figures
def graded_figures(got, w64, dims, x, cond):
    """{"unit_max", "unit_median", "rel_max", "rel_median"}: four figures each (rgb0..2, sigma) of |got - fp64| per output
    column, in the unit sum |w||in| + |b| of the last layer (rgb_linear / alpha_linear on the reference's own v3 / a8) and
    relative to the column's largest |reference|."""
    pc = dims["input_ch"]
    x64 = x.double()
    c64 = [c.double() for c in cond]
    ref = fc.raw_of(fc.ref_layers(w64, dims, x64[:, :pc], x64[:, pc:], c64))
    units = fc.layer_units(w64, dims, x64[:, :pc], x64[:, pc:], c64)
    unit = torch.cat([units[fc.OUT_NAMES.index("rgb")], units[fc.OUT_NAMES.index("sigma")]], 1)
    err = (got.double() - ref).abs()
    return dict(unit_max=(err / unit).max(0)[0].tolist(), unit_median=(err / unit).median(0)[0].tolist(),
                rel_max=(err.max(0)[0] / ref.abs().max(0)[0]).tolist(), rel_median=(err.median(0)[0] / ref.abs().max(0)[0]).tolist())
