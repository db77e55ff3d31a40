"""The inference kernels on exact operands (run with ``-m gpu``): mlp_bf16x3_kernel, mlp_fp16x3_kernel and mlp_bf16_kernel
(csrc/mlp_bf16x3.hip, csrc/mlp_fp16x3.hip), which only rendering runs, and the non-saving instantiations of the fp32 and
six-piece kernels (mlp_f32_kernel<*, false>, mlp_bf16x6_kernel<*, false>), with the pack kernels in front of them
(csrc/prep.hip: pack_bf16x3_kernel fmt 0 and 1, pack_bf16_kernel).  Operands, conditions and comparison:
tests/inference_modes_common.py; the CPU side: tests/test_inference_modes_cpu.py.

Every run (``run_raw``) is mode X of the inference entry, twice: idealnerf_facenerf_fwd_ch on a raw of exactly n rows filled
with a sentinel NaN between guard words -- guards intact, every value finite -- and idn.ops.facenerf_fwd on its own fresh
output -- the same bits.  Every comparison with the fp64 reference is an EQUALITY.

X1   bf16x3, fp16x3 on their two-piece sets T x three conditioning layouts x n in {128, 185, 640};
X2   the same, head layout, n = 128 (2 CUs + 3) - 37, the fp64 reference on the device;
X2b  the same for a 33 / 15 network, n = 185;
P1   plain bf16 (8 waves, 256 points per pass) on the one-piece set P x three layouts x n in {256, 313, 1280};
P2   n = 256 (2 CUs + 3) - 37;   P2b  the 33 / 15 network, n = 313;
W    bf16x3, fp16x3: the P net with the weights of one layer times 1 + 2^-8 / 1 + 2^-12, each of the thirteen layers: the lo
     half of the packed stream and the a_hi w_lo product of exactly that layer;
F1   f32 and bf16x6 through the inference entry on forward_layers_common.exact_case, on T (both) and on P, head layout,
     n in {128, 185, 640} and the E2 row count;
C1   all five precision codes on P, n = 313: the same bits from every one;
G    Xavier weights, 640 rows of uniform(-1, 1): |out - fp64| per output column of the three 16-bit modes and of the fp32
     kernel, recorded and not asserted.

$IDN_INFER_MODES_RECORD names a JSON file the figures are merged into (profiles/inference_modes.json)."""
import json
import os

import pytest
import torch

import forward_layers_common as fc
import inference_modes_common as im
from test_delta_chain_gpu import guarded, guards_intact

pytestmark = pytest.mark.gpu

FULL = (63, 27)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()  # fail loudly if the HIP library is missing
    return idealnerf_amd


def _record(key, value):
    path = os.environ.get("IDN_INFER_MODES_RECORD")
    if not path:
        return
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(old, open(path, "w"), indent=1, sort_keys=True)


def _code(idn, mode):
    L = idn._lib
    return {"f32": L.IDN_PREC_F32, "bf16x3": L.IDN_PREC_BF16X3, "bf16": L.IDN_PREC_BF16, "fp16x3": L.IDN_PREC_FP16X3,
            "bf16x6": L.IDN_PREC_BF16X6}[mode]


# ------------------------------------------------------------------------------------------------ the runner
def device_net(idn, dev, sd, dims3, cond, widths=FULL):
    """What the entry reads: the folded bias block, and the weight stream of a mode once it is asked for (``stream_of``)."""
    sd = {k: v.to(dev).contiguous() for k, v in sd.items()}
    ps = idn.ops.params_struct(sd, *dims3, pts_ch=widths[0], views_ch=widths[1])
    cond = [c.to(dev).contiguous() for c in cond]
    folded = idn.ops.fold_conditioning(ps, *[c if c.numel() else None for c in cond], dev)
    torch.cuda.synchronize()
    return dict(idn=idn, sd=sd, ps=ps, cond=cond, folded=folded, packed={}, widths=widths)


def stream_of(net, mode):
    if mode not in net["packed"]:
        net["packed"][mode] = net["idn"].ops.pack_weights(net["ps"], net["folded"].device, _code(net["idn"], mode))
        torch.cuda.synchronize()
    return net["packed"][mode]


def run_raw(idn, net, mode, x, ctx):
    """Mode X twice on fresh buffers, with the assertions of the module docstring.  -> raw [n, 4]."""
    lib = idn._lib.load()
    pc, vc = net["widths"]
    n = x.shape[0]
    assert x.is_contiguous() and x.shape[1] == pc + vc and x.dtype == torch.float32
    packed, folded, code = stream_of(net, mode), net["folded"], _code(idn, mode)
    whole, raw = guarded((n, 4), x.device)
    rc = lib.idealnerf_facenerf_fwd_ch(packed.data_ptr(), folded.data_ptr(), code, x.data_ptr(), pc, vc, n, raw.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.idealnerf_last_error()
    torch.cuda.synchronize()
    assert guards_intact(whole), f"{ctx}: a write outside raw's {n} rows"
    assert bool(torch.isfinite(raw).all()), f"{ctx}: not every row of raw was written with a finite value"
    again = idn.ops.facenerf_fwd(packed, folded, x, code, pc, vc)
    torch.cuda.synchronize()
    assert again.shape == (n, 4) and again.dtype == torch.float32
    if not fc.same_bits(raw, again):
        im.assert_same_raw(again, raw, f"{ctx}: the second run against the first", im.TILE[mode])
        raise AssertionError(f"{ctx}: two runs differ in the sign of a zero")
    return raw


def check(idn, c, mode, ctx):
    raw = run_raw(idn, c["net"], mode, c["x"], ctx)
    im.assert_same_raw(raw, c["raw"], ctx, im.TILE[mode])
    return raw


_cases = {}


def case_on_device(idn, dev, key, build):
    """One case (operands, fp64 reference with its conditions, device buffers): built once, shared, never written again."""
    if key not in _cases:
        c = build()
        c["net"] = device_net(idn, dev, c["sd"], c["dims3"], c["cond"], c["widths"])
        _cases[key] = c
    return _cases[key]


def t_case(idn, dev, mode, dims3, n, widths=FULL):
    return case_on_device(idn, dev, ("T", mode, dims3, n, widths), lambda: im.two_piece_case(mode, dims3, n, widths, device=dev))


def p_case(idn, dev, dims3, n, widths=FULL):
    return case_on_device(idn, dev, ("P", dims3, n, widths), lambda: im.one_piece_case(dims3, n, widths, device=dev))


def e_case(idn, dev, dims3, n):
    def build():
        c = fc.exact_case(dims3, n, device=dev)
        c.update(dims3=dims3, widths=FULL, raw=fc.raw_of(c["ref"]))
        return c
    return case_on_device(idn, dev, ("E", dims3, n), build)


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ------------------------------------------------------------------------------------------------ X1, X2, X2b
@pytest.mark.parametrize("n", fc.E1_ROWS)
@pytest.mark.parametrize("dims3", fc.DIMS, ids=fc.DIMS_ID)
@pytest.mark.parametrize("mode", im.X3_MODES)
def test_two_piece_operands(idn, dev, mode, dims3, n):
    """X1: one tile, a ragged second tile, five tiles.  Every input and activation has a hi and a lo piece, every weight is
    +-1: a_hi w_hi and a_lo w_hi of every k-step of every layer, the split of the inputs and of every accumulator tile
    (the deferred one included), every bias by channel and every position of the hi half of the stream."""
    check(idn, t_case(idn, dev, mode, dims3, n), mode, f"{mode} T {dims3} n {n}")
    _record(f"X1/{mode}/{fc.DIMS_ID[fc.DIMS.index(dims3)]}/{n}", dict(equal=True))


@pytest.mark.parametrize("mode", im.X3_MODES)
def test_two_piece_operands_beyond_the_grid(idn, dev, mode):
    """X2: head layout, n = 128 (2 CUs + 3) - 37: with one workgroup per CU every workgroup walks two tiles, three a third --
    the weight ring's slot phase and the cur / nxt hand-over of the prefetched point carry from tile to tile -- and the
    last tile is ragged."""
    cus = _cus(dev)
    n = im.multi_tile_rows(cus, mode)
    c = im.two_piece_case(mode, fc.DIMS[0], n, device=dev)      # (its conditions again, for this device's CU count)
    c["net"] = device_net(idn, dev, c["sd"], fc.DIMS[0], c["cond"])
    check(idn, c, mode, f"{mode} T n {n} ({cus} CUs)")
    _record(f"X2/{mode}", dict(cus=cus, rows=n, tiles=2 * cus + 3, equal=True))
    del c
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", im.X3_MODES)
def test_two_piece_operands_of_a_narrow_network(idn, dev, mode):
    """X2b: a 33 / 15 network, head layout, n = 185: the zeros the pack writes beyond a narrow network's columns."""
    check(idn, t_case(idn, dev, mode, fc.DIMS[0], 185, fc.NARROW), mode, f"{mode} T 33/15 n 185")
    _record(f"X2b/{mode}", dict(rows=185, equal=True))


# ------------------------------------------------------------------------------------------------ P1, P2, P2b
@pytest.mark.parametrize("n", im.P_ROWS)
@pytest.mark.parametrize("dims3", fc.DIMS, ids=fc.DIMS_ID)
def test_one_piece_operands(idn, dev, dims3, n):
    """P1: the plain-bf16 kernel, eight waves on 256 points per pass: one pass, a ragged second, five."""
    check(idn, p_case(idn, dev, dims3, n), "bf16", f"bf16 P {dims3} n {n}")
    _record(f"P1/{fc.DIMS_ID[fc.DIMS.index(dims3)]}/{n}", dict(equal=True))


def test_one_piece_operands_beyond_the_grid(idn, dev):
    """P2: n = 256 (2 CUs + 3) - 37."""
    cus = _cus(dev)
    n = im.multi_tile_rows(cus, "bf16")
    c = im.one_piece_case(fc.DIMS[0], n, device=dev)
    c["net"] = device_net(idn, dev, c["sd"], fc.DIMS[0], c["cond"])
    check(idn, c, "bf16", f"bf16 P n {n} ({cus} CUs)")
    _record("P2", dict(cus=cus, rows=n, tiles=2 * cus + 3, equal=True))
    del c
    torch.cuda.empty_cache()


def test_one_piece_operands_of_a_narrow_network(idn, dev):
    """P2b: a 33 / 15 network, n = 313."""
    check(idn, p_case(idn, dev, fc.DIMS[0], 313, fc.NARROW), "bf16", "bf16 P 33/15 n 313")
    _record("P2b", dict(rows=313, equal=True))


# ------------------------------------------------------------------------------------------------ W
@pytest.mark.parametrize("layer", im.LAYERS)
@pytest.mark.parametrize("mode", im.X3_MODES)
def test_weight_lo_pieces(idn, dev, mode, layer):
    """W: w_hi = +-1 and w_lo = +-2^-8 (bf16x3) / +-2^-12 (fp16x3) in one layer, one-piece inputs in front of it: its outputs
    carry the fractions that only a_hi w_lo brings, and a lo half of the stream that is missing, misplaced or paired with
    the wrong hi half shows in raw.  n = 185."""
    c = case_on_device(idn, dev, ("W", mode, layer), lambda: im.weight_lo_case(mode, layer, 185, device=dev))
    check(idn, c, mode, f"{mode} W {layer}")
    _record(f"W/{mode}/{layer}", dict(rows=185, equal=True))


# ------------------------------------------------------------------------------------------------ F1
def _f1_case(idn, dev, operands, n):
    head = fc.DIMS[0]
    if operands == "E":
        return e_case(idn, dev, head, n)
    if operands == "P":
        return p_case(idn, dev, head, n)
    return t_case(idn, dev, operands[2:], head, n)


F1_OPERANDS = ("E", "T-bf16x3", "T-fp16x3", "P")


@pytest.mark.parametrize("n", fc.E1_ROWS)
@pytest.mark.parametrize("operands", F1_OPERANDS)
@pytest.mark.parametrize("pipe", ("f32", "bf16x6"))
def test_non_saving_kernels_on_exact_operands(idn, dev, pipe, operands, n):
    """F1: the instantiations every render runs, through the inference entry: forward_layers_common.exact_case (E), T of both
    formats and P -- all integers with sums below 2^24, exact in fp32 and in three bf16 pieces."""
    check(idn, _f1_case(idn, dev, operands, n), pipe, f"{pipe} {operands} n {n}")
    _record(f"F1/{pipe}/{operands}/{n}", dict(equal=True))


def test_non_saving_kernels_beyond_the_grid(idn, dev):
    """F1 at the E2 row count, 128 (2 CUs + 3) - 37: E, T (bf16x3) and P, both pipes on one reference each."""
    cus = _cus(dev)
    n = fc.multi_tile_rows(cus)
    head = fc.DIMS[0]
    for operands in ("E", "T-bf16x3", "P"):
        if operands == "E":
            c = fc.exact_case(head, n, device=dev)
            c.update(dims3=head, widths=FULL, raw=fc.raw_of(c["ref"]))
        elif operands == "P":
            c = im.one_piece_case(head, n, device=dev)
        else:
            c = im.two_piece_case("bf16x3", head, n, device=dev)
        c["net"] = device_net(idn, dev, c["sd"], head, c["cond"])
        for pipe in ("f32", "bf16x6"):
            check(idn, c, pipe, f"{pipe} {operands} n {n} ({cus} CUs)")
        del c
        torch.cuda.empty_cache()
    _record("F1/beyond", dict(cus=cus, rows=n, equal=True))


# ------------------------------------------------------------------------------------------------ C1
def test_every_code_returns_the_same_bits(idn, dev):
    """C1: P, head layout, n = 313: one bf16 per value is exact in all five arithmetics; each returns the reference, and the
    same bits as every other."""
    c = p_case(idn, dev, fc.DIMS[0], 313)
    raws = {mode: check(idn, c, mode, f"{mode} P n 313") for mode in im.ALL_MODES}
    for mode in im.ALL_MODES[1:]:
        assert fc.same_bits(raws[mode], raws["f32"]), f"{mode} and f32 differ in the sign of a zero"
    _record("C1", dict(rows=313, codes=list(im.ALL_MODES), equal=True))


# ------------------------------------------------------------------------------------------------ G
def test_graded_figures_are_recorded(idn, dev):
    """G: head layout, forward_layers_common.graded_net / graded_cond, 640 rows of uniform(-1, 1).  Per output column, the
    largest and the median |out - fp64| in the unit sum |w||in| + |b| of the last layer and relative to max |ref|, for the
    three 16-bit modes and for the fp32 kernel on the same rows.  Recorded, not asserted: this is the part the equalities
    do not pin -- the dropped a_lo w_lo product and the accumulation order on operands that round; the tolerances of
    test_hip_parity.py stay what holds it."""
    dims3 = fc.DIMS[0]
    sd = fc.graded_net(dims3, 5)
    cond = fc.graded_cond(dims3, 6)
    net = device_net(idn, dev, sd, dims3, cond)
    g = torch.Generator().manual_seed(29)
    x = (torch.rand((640, 90), generator=g) * 2 - 1).to(dev).contiguous()
    w64 = {k: v.double() for k, v in net["sd"].items()}
    record = dict(rows=640, columns=list(im.RAW_NAMES))
    print()
    for mode in ("f32",) + im.MODES16:
        raw = run_raw(idn, net, mode, x, f"{mode} graded")
        record[mode] = im.graded_figures(raw, w64, fc.oracle_dims(dims3), x, net["cond"])
        print(f"  {mode:7s} " + "  ".join(f"{k} {max(v):.2e}" for k, v in record[mode].items()))
    _record("G", record)
    _record("device", dict(cus=_cus(dev), name=torch.cuda.get_device_properties(dev).name))
