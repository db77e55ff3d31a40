"""The exact operands of the inference-kernel tests, without a GPU (tests/inference_modes_common.py; the GPU side:
tests/test_inference_modes_gpu.py).

1  the splits: ``rtz16`` is truncation to fp16, and the weight splits of 1 + 2^-8 / 1 + 2^-12 are (1, 2^-8) / (1, 2^-12);
2  the placed network: every (32-row tile, 16-column k-step) pair of every streamed source holds a non-zero, every column is
   read, the rows have the shares they are meant to have -- for every layout, both network widths and every set;
3  every case the GPU file runs builds -- the split conditions, the 2^24 bound, the on-fractions, the lo-piece shares and, for
   W, the piece values are asserted while it does (``checked_reference``) -- and torch's fp32 and the arithmetic of the mode
   restated in torch (``mode_product``) return the reference's numbers exactly;
4  the mistakes the sets are for, restated in torch, each change raw: a lo half of the weight stream zeroed in one layer (W), the
   w_lo a_hi product dropped for one tile of one layer (W), two channels of the plain-bf16 stream swapped within one k-step
   (P), the lo word of one k-step of an activation lost (T), a bias taken from the next tile (P);
5  ``assert_same_raw`` names the output, the pass, the wave and the point."""
import pytest
import torch

import forward_layers_common as fc
import inference_modes_common as im

ASSUMED_CUS = 256          # the multi-tile cases are built for an MI355X's CU count here; the GPU tests use the device's own
HEAD = fc.DIMS[0]


# ------------------------------------------------------------------------------------------------ 1
def test_rtz16_is_truncation_to_fp16():
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(20000, generator=g) * 2 - 1) * 2.0 ** torch.randint(-13, 16, (20000,), generator=g).float()
    x = torch.cat([x, torch.tensor([0.0, 1.0, -1.0, 2047.0, 2049.0, -4097.0, 65503.0, 2.0 ** -14, 1 + 2.0 ** -12])])
    x = x[(x.abs() < 65504) & ((x == 0) | (x.abs() >= 2.0 ** -14))]
    assert x.numel() > 15000
    t = im.rtz16(x)
    assert torch.equal(t.half().float(), t), "not an fp16"
    assert bool((t.abs() <= x.abs()).all()) and bool((t * x >= 0).all()), "not toward zero"
    up = torch.nextafter(t.half(), (torch.sign(x) * 65504).half()).float()          # the next fp16 away from zero
    assert bool((up.abs() > x.abs())[x != 0].all()) and bool((t[x == 0] == 0).all()), "not the nearest fp16 toward zero"
    with pytest.raises(AssertionError):
        im.rtz16(torch.tensor([70000.0]))
    with pytest.raises(AssertionError):
        im.rtz16(torch.tensor([2.0 ** -16]))


def test_the_two_piece_ranges():
    """Every integer below 2^16 is two bf16 pieces and most above 2^8 need the second; every integer below 65504 is two fp16
    pieces and every odd one above 2^11 needs the second; 2^17 + 257 is not two bf16 pieces (a remainder of nine bits)."""
    v = torch.arange(-65535, 65536).double()
    assert im.splits_exactly("bf16x3", v) and im.lo_share("bf16x3", v, v.abs() > 256) > 0.9
    assert not im.splits_exactly("bf16x3", torch.tensor([131329.0]).double())
    h = torch.arange(-65503, 65504).double()
    assert im.splits_exactly("fp16x3", h)
    odd = h[(h.abs() > 2048) & (h % 2 == 1)]
    assert im.lo_share("fp16x3", odd) == 1.0 and im.lo_share("fp16x3", h[h.abs() <= 2048]) == 0.0


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("widths", [(63, 27), fc.NARROW], ids=["63-27", "33-15"])
@pytest.mark.parametrize("dims3", fc.DIMS, ids=fc.DIMS_ID)
@pytest.mark.parametrize("b_max", [im.P_RANGE[1]] + [r[1] for r in im.T_RANGE.values()])
def test_placed_net_covers_every_fragment_and_every_column(dims3, widths, b_max):
    sd = im.placed_net(dims3, im.net_seed("T", dims3, widths), widths, b_max)
    empty, unread = im.coverage(sd, dims3, widths)
    assert not empty, empty[:8]
    assert not unread, unread[:8]
    pc, vc = widths
    C, e = sum(dims3), dims3[1]
    parts = {"pts_linears.0": [(0, pc, 2), (pc, C, 1)], "pts_linears.5": [(0, pc, 1), (pc, C, 1), (pc + C, 256, 2)],
             "views_linears.0": [(0, 256, 2), (256, vc, 1), (256 + vc, e, 1)], "views_linears.1": [(0, 128, 2)], "views_linears.2": [(0, 128, 2)]}
    parts.update({f"pts_linears.{i}": [(0, 256, 2)] for i in (1, 2, 3, 4, 6, 7)})
    for key, ranges in parts.items():
        W = sd[key + ".weight"]
        assert bool(((W == 0) | (W.abs() == 1)).all()) and W.shape[1] == sum(c for _, c, _ in ranges), key
        for c0, cols, nnz in ranges:
            if cols:
                part = W[:, c0:c0 + cols]
                assert bool(((part != 0).sum(1) == nnz).all()), (key, c0)
                if nnz == 2:
                    assert bool((part.sum(1) == 0).all()), (key, c0, "a row of two is one +1 and one -1")
    for key in ("alpha_linear", "rgb_linear"):
        assert bool((sd[key + ".weight"].abs() == 1).all()), key
    for k, v in sd.items():
        if k.endswith(".bias"):
            assert bool((v == v.round()).all()) and float(v.abs().max()) <= b_max, k
            assert k.startswith(("alpha", "rgb")) or torch.unique(v).numel() > min(b_max, 100), k


def test_thin_heads_still_touch_every_k_step():
    """placed_block with fewer non-zeros than columns and fewer rows than a tile: one row of 16 over 256 columns stands in
    every k-step, three rows of 16 over 128 columns too."""
    g = torch.Generator().manual_seed(3)
    for rows, cols in ((1, 256), (3, 128)):
        W = im.placed_block(rows, cols, 16, g)
        assert bool(((W != 0).sum(1) == 16).all())
        assert all(bool((W[:, 16 * s:16 * s + 16] != 0).any()) for s in range(cols // 16))


# ------------------------------------------------------------------------------------------------ 3
def _fp32_raw(c):
    pc = c["dims"]["input_ch"]
    return fc.raw_of(fc.ref_layers(c["sd"], c["dims"], c["x"][:, :pc], c["x"][:, pc:], c["cond"]))


def _restated(c, mode, change=None):
    return im.forward_with(c["w64"], c["dims"], c["x"], c["cond"], im.mode_product(mode, change))


def _agrees(c, modes, ctx, fp32=True):
    if fp32:
        im.assert_same_raw(_fp32_raw(c), c["raw"], f"torch fp32 {ctx}")
    for mode in modes:
        got = _restated(c, mode)
        assert torch.equal(got, c["raw"].double()), f"{mode} restated, {ctx}"


T_CASES = [(d, n, (63, 27)) for d in fc.DIMS for n in fc.E1_ROWS] + [(HEAD, 185, fc.NARROW)]


@pytest.mark.parametrize("dims3,n,widths", T_CASES, ids=[f"{fc.DIMS_ID[fc.DIMS.index(d)]}-{n}-{w[0]}" for d, n, w in T_CASES])
@pytest.mark.parametrize("mode", im.X3_MODES)
def test_two_piece_cases_build(mode, dims3, n, widths):
    """X1 / X2b: the conditions of set T hold; torch fp32 and the mode's three kept products give the reference exactly."""
    c = im.two_piece_case(mode, dims3, n, widths)
    _agrees(c, (mode,), f"T {mode} {dims3} n {n}")
    st = im.set_stats(mode, c["w64"], c["dims"], c["x"], c["cond"])
    print(f"\n  T {mode} {dims3} n {n} {widths}: largest hidden value {max(st[k][0] for k in fc.HIDDEN):.0f}, largest unit "
          f"{max(s[1] for s in st.values()):.3g}, on-fractions {min(st[k][2] for k in fc.HIDDEN):.2f}..{max(st[k][2] for k in fc.HIDDEN):.2f}, "
          f"lo shares of the positive {min(st[k][3] for k in fc.HIDDEN):.2f}..{max(st[k][3] for k in fc.HIDDEN):.2f}")


P_CASES = [(d, n, (63, 27)) for d in fc.DIMS for n in im.P_ROWS] + [(HEAD, 313, fc.NARROW)] + [(HEAD, n, (63, 27)) for n in fc.E1_ROWS]


@pytest.mark.parametrize("dims3,n,widths", P_CASES, ids=[f"{fc.DIMS_ID[fc.DIMS.index(d)]}-{n}-{w[0]}" for d, n, w in P_CASES])
def test_one_piece_cases_build(dims3, n, widths):
    """P1 / P2b / C1 / F1: the conditions of set P hold, and all three 16-bit arithmetics restated give the reference."""
    c = im.one_piece_case(dims3, n, widths)
    _agrees(c, im.MODES16, f"P {dims3} n {n}")
    st = im.set_stats("bf16", c["w64"], c["dims"], c["x"], c["cond"])
    assert max(st[k][0] for k in fc.HIDDEN) <= 222, "the bound of the construction: 76, 7 per layer, 45 at each of the two joins"


def test_multi_tile_cases_build():
    """X2 / P2 / F1 at the row counts of a device of 256 CUs: the conditions hold there as well (the ranges are the
    construction's, not the sample's)."""
    for mode in im.X3_MODES:
        n = im.multi_tile_rows(ASSUMED_CUS, mode)
        assert n == 128 * 515 - 37 == fc.multi_tile_rows(ASSUMED_CUS)
        im.two_piece_case(mode, HEAD, n)
    assert im.multi_tile_rows(ASSUMED_CUS, "bf16") == 256 * 515 - 37
    im.one_piece_case(HEAD, im.multi_tile_rows(ASSUMED_CUS, "bf16"))


@pytest.mark.parametrize("layer", im.LAYERS)
@pytest.mark.parametrize("mode", im.X3_MODES)
def test_weight_lo_cases_build_and_see_a_lost_lo_half(mode, layer):
    """W: the piece values (asserted in weight_lo_case), the conditions, fp32 and the mode restated exact; and the two
    mistakes a W case is for change raw: the lo half of the layer's stream zeroed, and the w_lo a_hi product dropped for
    any ONE 32-row tile of the layer."""
    c = im.weight_lo_case(mode, layer)
    _agrees(c, (mode,), f"W {mode} {layer}")
    want = c["raw"].double()

    def zero_lo(rows):
        def change(name, p):
            if name == layer:
                p["w_lo"][rows] = 0
        return change

    assert not torch.equal(_restated(c, mode, zero_lo(slice(None))), want), "a zeroed lo half goes unseen"
    rows = c["sd"][fc.KEY[layer] + ".weight"].shape[0]
    for t in range((rows + 31) // 32):
        assert not torch.equal(_restated(c, mode, zero_lo(slice(32 * t, 32 * t + 32))), want), f"tile {t} without w_lo a_hi goes unseen"
    # the same mistake on the sets with +-1 weights is invisible: there is no lo half to lose -- what W is for
    p = im.one_piece_case(HEAD, 313)
    assert torch.equal(_restated(p, mode, zero_lo(slice(None))), p["raw"].double())


# ------------------------------------------------------------------------------------------------ 4
def test_swapped_channels_of_the_plain_stream_change_raw():
    """P, head layout, 313 rows: channel 0 of any one k-step of any streamed source of any layer, swapped in the stream
    (pack_bf16_kernel) with the next channel of the k-step whose weights are not the same, changes raw."""
    c = im.one_piece_case(HEAD, 313)
    want = c["raw"].double()
    for layer, sources in im.streamed_sources(HEAD).items():
        W = c["w64"][fc.KEY[layer] + ".weight"]
        for c0, cols in sources:
            for s in range((cols + 15) // 16):
                at = c0 + 16 * s
                other = next(k for k in range(at + 1, min(at + 16, c0 + cols)) if not torch.equal(W[:, k], W[:, at]))

                def change(name, p, at=at, other=other):
                    if name == layer:
                        p["w_hi"][:, [at, other]] = p["w_hi"][:, [other, at]]
                assert not torch.equal(_restated(c, "bf16", change), want), (layer, c0, s)


@pytest.mark.parametrize("mode", im.X3_MODES)
def test_a_lost_activation_lo_word_changes_raw(mode):
    """T, head layout, 185 rows: the lo pieces of one k-step of a layer's input lost (a split that wrote its lo word to the
    wrong register, an a_lo w_hi product that read a stale operand): raw changes, for every k-step of every layer."""
    c = im.two_piece_case(mode, HEAD, 185)
    want = c["raw"].double()
    for layer, sources in im.streamed_sources(HEAD).items():
        for c0, cols in sources:
            for s in range((cols + 15) // 16):
                def change(name, p, lo=c0 + 16 * s, hi=min(c0 + 16 * s + 16, c0 + cols)):
                    if name == layer:
                        p["a_lo"][:, lo:hi] = 0
                assert not torch.equal(_restated(c, mode, change), want), (layer, c0, s)


def test_a_bias_quad_of_the_next_tile_changes_raw():
    """P, 313 rows: channels 4 q .. 4 q + 3 of one 32-channel tile taking the bias of the tile behind it -- in every hidden
    layer, every tile but the last, every quad.  (Biases drawn with replacement from 15 values: a quad of four equal to
    the four 32 channels on has a chance of 15^-4.)"""
    c = im.one_piece_case(HEAD, 313)
    want = c["raw"].double()
    for name in fc.HIDDEN:
        key = fc.KEY[name] + ".bias"
        b = c["w64"][key]
        for t in range(b.numel() // 32 - 1):
            for q in range(8):
                w = dict(c["w64"])
                w[key] = b.clone()
                w[key][32 * t + 4 * q:32 * t + 4 * q + 4] = b[32 * t + 32 + 4 * q:32 * t + 36 + 4 * q]
                if torch.equal(w[key], b):
                    continue
                assert not torch.equal(im.forward_with(w, c["dims"], c["x"], c["cond"]), want), (name, t, q)


# ------------------------------------------------------------------------------------------------ 5
def test_assert_same_raw_names_the_place():
    c = im.one_piece_case(HEAD, 313)
    ref = c["raw"]
    im.assert_same_raw(ref.clone(), ref, "unchanged")
    bad = ref.clone()
    bad[256 + 32 + 5, 3] += 1
    with pytest.raises(AssertionError, match=r"first at row 293 \(tile 1, wave 1, point 5\) sigma"):
        im.assert_same_raw(bad, ref, "plain", tile=256)
    with pytest.raises(AssertionError, match=r"first at row 293 \(tile 2, wave 1, point 5\) sigma"):
        im.assert_same_raw(bad, ref, "x3", tile=128)
    bad = ref.clone()
    bad[64:96, 1] = torch.roll(bad[64:96, 1], 1, 0)
    with pytest.raises(AssertionError, match=r"rows per wave of a pass \[0, 0, \d+, 0\].* rgb1"):
        im.assert_same_raw(bad, ref, "rolled", tile=128)
