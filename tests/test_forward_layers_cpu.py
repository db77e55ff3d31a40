"""The reference, the exact operands and the comparison of the training-forward tests, without a GPU
(tests/forward_layers_common.py; the GPU side: tests/test_forward_layers_gpu.py).

1  ``ref_layers`` in fp64 is oracle.facenerf_forward in fp64, on weights whose biases differ from channel to channel;
2  every exact case the GPU file runs builds -- the conditions that make equality legitimate are asserted while it does -- and
   torch's fp32 on the CPU returns the identical numbers;
3  a reference with one small mutation fails ``assert_same``: the exact cases would see such a mistake in a kernel;
4  what the graded metric cannot see, as a figure: a weight stream that lost its third bf16 piece."""
import pytest
import torch

import oracle
import forward_layers_common as fc

ASSUMED_CUS = 256          # the multi-tile case is built for an MI355X's CU count here; the GPU test uses the device's own


@pytest.mark.parametrize("widths", [(63, 27), fc.NARROW], ids=["63-27", "33-15"])
@pytest.mark.parametrize("dims3", fc.DIMS, ids=fc.DIMS_ID)
def test_ref_layers_is_the_oracle_forward(dims3, widths):
    """fp64, Xavier weights with per-channel random biases, 200 rows: raw to 1e-12 of the largest output, and with `given`
    = the reference's own matrices the same numbers again."""
    dims = fc.oracle_dims(dims3, widths)
    w = {k: v.double() for k, v in fc.graded_net(dims3, 3, widths).items()}
    cond = [c.double() for c in fc.graded_cond(dims3, 4)]
    g = torch.Generator().manual_seed(5)
    x = (torch.rand((200, sum(widths)), generator=g) * 2 - 1).double()
    want = oracle.facenerf_forward(w, x, *cond, dims=dims)
    outs = fc.ref_layers(w, dims, x[:, :widths[0]], x[:, widths[0]:], cond)
    got = fc.raw_of(outs)
    assert got.shape == want.shape == (200, 4)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert [tuple(o.shape) for o in outs] == [(200, 256)] * 8 + [(200, 1)] + [(200, 128)] * 3 + [(200, 3)]
    given = dict(zip(fc.OUT_NAMES, outs))
    again = fc.ref_layers(w, dims, x[:, :widths[0]], x[:, widths[0]:], cond, given=given)
    for name, a, b in zip(fc.OUT_NAMES, outs, again):
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max()), name
    units = fc.layer_units(w, dims, x[:, :widths[0]], x[:, widths[0]:], cond)
    assert all(bool((u >= o.abs()).all()) for u, o in zip(units, outs))
    # the fold, restated: layer 0 on the encoding alone with the folded bias is layer 0
    folded, unit = fc.fold_reference(w, dims, cond)
    a1 = fc.ref_layers(w, dims, x[:, :widths[0]], x[:, widths[0]:], cond, folded0=folded[:256])[0]
    assert float((a1 - outs[0]).abs().max()) <= 1e-12 * float(outs[0].abs().max())
    assert folded.shape == (fc.FOLD_FLOATS,) and bool((unit >= folded[:fc.FOLD_BIASES].abs() - 1e-15).all())


def _fp32_outputs(c):
    """The same layers through torch fp32 on the CPU."""
    pc = c["dims"]["input_ch"]
    return fc.ref_layers(c["sd"], c["dims"], c["x"][:, :pc], c["x"][:, pc:], c["cond"])


CASES = [(d, n, (63, 27)) for d in fc.DIMS for n in fc.E1_ROWS] + [(fc.DIMS[0], 185, fc.NARROW),
                                                                    (fc.DIMS[0], fc.multi_tile_rows(ASSUMED_CUS), (63, 27))]


@pytest.mark.parametrize("dims3,n,widths", CASES, ids=[f"{fc.DIMS_ID[fc.DIMS.index(d)]}-{n}-{w[0]}" for d, n, w in CASES])
def test_exact_cases_build_and_fp32_agrees(dims3, n, widths):
    """E1 / E2 / E2b: exact_reference's assertions hold (units below 2^24, integers, on-fractions, the third piece carries
    value), and torch fp32 on the CPU gives the identical thirteen matrices."""
    c = fc.exact_case(dims3, n, widths)
    fc.assert_same(_fp32_outputs(c), c["ref"], f"torch fp32 {dims3} n {n}")
    stats = fc.reference_stats(c["w64"], c["dims"], c["x"], c["cond"])
    print(f"\n  {dims3} n {n} widths {widths}: largest unit {max(s[0] for s in stats.values()):.3g}; on-fractions "
          f"{min(stats[k][1] for k in fc.HIDDEN):.2f}..{max(stats[k][1] for k in fc.HIDDEN):.2f}; share >= 2^16: v3 {stats['v3'][2]:.2f}, "
          f"a8 {stats['a8'][2]:.3f}")
    for k in ("pts_linears.0", "pts_linears.5", "views_linears.0"):     # every source present in every row
        W = c["sd"][k + ".weight"]
        pc, C = widths[0], sum(dims3)
        edges = {"pts_linears.0": [0, pc, pc + C], "pts_linears.5": [0, pc, pc + C, pc + C + 256],
                 "views_linears.0": [0, 256, 256 + widths[1], 256 + widths[1] + dims3[1]]}[k]
        for lo, hi in zip(edges[:-1], edges[1:]):
            assert hi == lo or bool((W[:, lo:hi] != 0).any(1).all()), (k, lo, hi)
    for k, v in c["sd"].items():
        if k.endswith(".bias") and not k.startswith("feature_linear"):
            assert torch.unique(v).numel() == v.numel(), k


def test_piece_cases_build_and_fp32_agrees():
    """E3 (three-piece weights in layer 0) and E4 (three-piece inputs): a1 exact in fp32 as well."""
    for c in (fc.weight_piece_case(185), fc.input_piece_case(185)):
        got = _fp32_outputs(c)
        fc.assert_same(got[:1], c["ref"][:1], "torch fp32", names=["a1"])
        assert all(bool(torch.isfinite(t).all()) for t in got)
    x = fc.three_piece_rows(185, 7 * 185 + 60)
    assert all(bool((p != 0).all()) for p in fc.bf16_pieces(x))


def _mutated(c, change):
    sd = {k: v.clone() for k, v in c["sd"].items()}
    change(sd)
    pc = c["dims"]["input_ch"]
    w64 = {k: v.double() for k, v in sd.items()}
    return [t.float() for t in fc.ref_layers(w64, c["dims"], c["x"][:, :pc].double(), c["x"][:, pc:].double(), [t.double() for t in c["cond"]])]


def test_a_small_mistake_fails_the_exact_comparison():
    """Head net, 185 rows: each of four mutations of the reference makes assert_same raise, naming the matrix it hits."""
    c = fc.exact_case(fc.DIMS[0], 185)
    ref = c["ref"]
    C = sum(fc.DIMS[0])

    def swap_bias(sd):
        b = sd["views_linears.1.bias"]
        b[[3, 70]] = b[[70, 3]]

    def move_across_skip(sd):
        W = sd["pts_linears.5.weight"]
        first = 63 + C                                             # the first trunk column
        rows = (W[:, first] != 0).nonzero()
        if rows.numel():                                           # a trunk entry into the last conditioning column
            r = int(rows[0])
            W[r, first - 1], W[r, first] = W[r, first - 1] + W[r, first], 0.0
        else:                                                      # or a conditioning entry into the first trunk column
            r = int((W[:, first - 1] != 0).nonzero()[0])
            W[r, first], W[r, first - 1] = W[r, first - 1], 0.0

    def zero_alpha_bias(sd):
        sd["alpha_linear.bias"].zero_()

    for change, hit in ((swap_bias, "v2"), (move_across_skip, "a6"), (zero_alpha_bias, "sigma")):
        with pytest.raises(AssertionError, match=f": {hit} differs"):
            fc.assert_same(_mutated(c, change), ref, change.__name__)
    rotated = [t.clone() for t in ref]
    a3 = rotated[fc.OUT_NAMES.index("a3")]
    a3[64:96] = torch.roll(a3[64:96], 1, 0)                        # one wave tile's rows stored one row down
    with pytest.raises(AssertionError, match=r": a3 differs .* first at row 64 \(tile 0, wave 2, point 0\)"):
        fc.assert_same(rotated, ref, "rotated")
    fc.assert_same([t.clone() for t in ref], ref, "unchanged")


def test_what_the_graded_metric_cannot_see():
    """A statement, not an assertion of a bound: Xavier weights truncated to their first two bf16 pieces (a pack kernel whose
    third piece is lost), one 256-wide layer in fp64 on inputs in [0, 1]: the figure in the graded unit
    max |got - ref| / (sum |w||in| + |b|), next to the floor of the graded rule and to torch's fp32 addmm of the same layer.
    A stream that lost the third piece altogether sits a few times above the floor and within reach of 4 x torch's figure:
    the graded test may or may not see it, and a third piece that is merely wrong in its low bits it cannot see.  The exact
    cases E3 / E4 are what holds the third piece."""
    sd = fc.graded_net(fc.DIMS[0], 3)
    W, b = sd["pts_linears.2.weight"], sd["pts_linears.2.bias"]
    p1, p2, p3 = fc.bf16_pieces(W)
    assert torch.equal((p1.double() + p2.double() + p3.double()).float(), W) and bool((p3 != 0).any())
    g = torch.Generator().manual_seed(8)
    x = torch.rand((1280, 256), generator=g)
    ref = torch.addmm(b.double(), x.double(), W.double().t())
    got = torch.addmm(b.double(), x.double(), (p1.double() + p2.double()).t())
    unit = torch.addmm(b.double().abs(), x.double().abs(), W.double().abs().t())
    figure = float(((got - ref).abs() / unit).max())
    fp32 = float(((torch.addmm(b, x, W.t()).double() - ref).abs() / unit).max())
    print(f"\n  two-piece weights, one 256-wide layer: max |err| / (sum |w||in| + |b|) = {figure:.2e}; floor of the graded rule "
          f"{fc.STAGE_BOUND:.1e}, torch fp32 addmm {fp32:.2e} (x {fc.TORCH_MULT:.0f} = {fc.TORCH_MULT * fp32:.2e}); a lost third piece "
          f"moves a weight by at most 2^-17 = {2.0 ** -17:.2e} of itself")
    assert 0 < figure < 2.0 ** -16          # (a sanity range of the statement itself: two pieces hold 16 significand bits)
