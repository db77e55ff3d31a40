"""Every weight-gradient (dW) product of the training backward, shape by shape, through the pass plan a training pass runs
them with (csrc/dw_gemm.hip behind DwPass, csrc/dw_gemm.h), against torch fp64 on the device.  ``ops.dw_products`` runs a
list of products through ONE DwPass and reports the plan (splits, chunks per split) each product ran with; the tests assert
their coverage on that report: one, two and three chunks per split, the steady state of the three-buffer chunk ring (from
the fifth chunk on), a last split of a single chunk and one that is merely short.

T1 / T2 / T3 use small-integer operands: every partial sum is an integer below 2^24 and every value is one exact bf16
piece, so the fp32 chains, the six piece products, the fp64 reduction and its cast are exact in any order -- the
assertions are equalities.  T4 grades the rounding at long splits with the project's metric and bounds.  Needs an MI355X.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

X6, F32 = 0, 1                       # IDN_DW_PIPE_BF16X6, IDN_DW_PIPE_F32
X6_ITEMS_PER_PASS = 9                # kX6ItemsPerPass (csrc/dw_gemm.h)
MAX_SPLITS = 256                     # kMaxSplits
# points per chunk of each instantiation (N, K): gemm_tn_kernel<NTW, KTW, NB, R> in csrc/dw_gemm.hip; the x6 kernel: 16
CHUNK_ROWS = {(256, 256): 16, (128, 128): 16, (128, 256): 16, (256, 64): 32, (128, 64): 64, (64, 128): 64}
# the pitches the pass uses: (N, K) -> (ld_delta, ld_acts, column sums)
PASS_FORMS = {(64, 128): (64, 128, True),       # rgb_linear
              (128, 128): (256, 128, True),     # views_linears.2 / .1 on the fp32 pipe (their deltas side by side)
              (128, 64): (256, 64, False),      # direction columns of views_linears.0
              (256, 64): (256, 64, True),       # pts_linears.0 (the encoding columns of pts_linears.5: the same without sums)
              (256, 256): (256, 256, True),     # the trunk
              (128, 256): (256, 256, True)}     # named by no pass (views_linears.0 runs as a 256 x 256 product)
# row counts (multiples of 128) that reach every class of plan with 256 splits at most, per chunk size -- on any device
F32_ROWS = {64: (128, 16384, 32768, 49152, 32896, 65664, 65792),
            32: (128, 8192, 16384, 24576, 16640, 33152, 32896),
            16: (128, 4096, 8192, 12288, 8320, 25216, 16512)}
ALL_CLASSES = {"cps1", "cps2", "cps3-equal", "cps3-last1", "long-last1", "long-short-last"}
DIM_AUD, DIM_EXPR, DIM_LATENT = 64, 79, 32
COND = DIM_AUD + DIM_EXPR + DIM_LATENT
LD0, LD5, LDV = 63 + COND, 63 + COND + 256, 256 + 27 + DIM_EXPR   # row pitches of pts_linears.0 / .5 and views_linears.0
SIGMA = 128                                                        # alpha_linear's delta: column 128 of views_linears.0's
SENTINEL = 0x7fc5a5a5                                              # one quiet-NaN bit pattern no kernel here produces
UNEVEN_ROWS = 32896   # chunks per split 3 / 5 / 9 at 64 / 32 / 16 rows per chunk, the last split 1 / 3 / 4 chunks (256 splits)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def idn():
    import idealnerf_amd
    idealnerf_amd._lib.load()  # fail loudly if the HIP library is missing
    return idealnerf_amd


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ---------------------------------------------------------------------------------------------- plans
def plan_class(rows, chunk_rows, plan):
    """The class of a REPORTED plan (splits, chunks per split) and the chunks of its last split."""
    splits, cps = plan
    chunks = rows // chunk_rows
    last = chunks - (splits - 1) * cps
    assert splits >= 1 and cps >= 1 and 1 <= last <= cps, (rows, chunk_rows, plan)
    if cps <= 2:
        name = f"cps{cps}" if last == cps else "other"
    elif cps == 3:
        name = "cps3-equal" if last == 3 else "cps3-last1" if last == 1 else "other"
    elif cps >= 5:
        name = "long-last1" if last == 1 else "long-short-last" if last < cps else "other"
    else:
        name = "other"
    return name, last


def x6_rows(cus, items, limit=66048):
    """Row counts at which the x6 kernel (2 #CUs / items splits, at most 256) reaches every class of plan: chosen here from
    the device's CU count, asserted by the callers on the plan the library reports."""
    max_splits = max(1, min(2 * cus // items, MAX_SPLITS))
    found = {}
    for rows in range(128, limit + 1, 128):
        chunks = rows // 16
        cps = -(-chunks // min(max_splits, chunks))
        name, _ = plan_class(rows, 16, (-(-chunks // cps), cps))
        if name in ALL_CLASSES and name not in found:
            found[name] = rows
    return found


# ---------------------------------------------------------------------------------------------- operands and outputs
def int_operand(rows, width, used, lo, hi, zeros, gen, pad="ints", col0=0):
    """[rows, width] fp32 of small integers in lo..hi (about `zeros` of them zero); the columns outside col0 .. col0 + used
    hold other integers ("ints": a kernel that reads them gets a wrong sum) or NaN ("nan": it gets no number at all)."""
    dev = gen.device
    t = torch.randint(lo, hi + 1, (rows, width), generator=gen, device=dev).float()
    if zeros:
        t *= torch.rand((rows, width), generator=gen, device=dev) >= zeros
    if pad == "nan":
        t[:, :col0] = float("nan")
        t[:, col0 + used:] = float("nan")
    return t


def int_delta(rows, width, used, gen, pad="ints", col0=0):
    return int_operand(rows, width, used, -3, 3, 0.5, gen, pad, col0)


def int_acts(rows, width, used, gen, pad="ints"):
    return int_operand(rows, width, used, 0, 4, 0.0, gen, pad)


def act_pair(rows, gen, make=None):
    """The two 128-column matrices of a split B from ONE allocation, [0] below [1], as the activation slab of a pass holds
    them: the kernel reaches both from the lower address with 32-bit offsets, and the library refuses a pair 2 GiB apart --
    which two allocations of a long-lived process can be."""
    both = torch.stack([(make or int_acts)(rows, 128, 128, gen) for _ in range(2)])
    return both[0], both[1]


def sentinel(shape, dev):
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def assert_blocks(out, blocks, what):
    """`out` was a sentinel tensor: every block (row0, col0, expected fp32) equals its reference EXACTLY and every other
    element still has the sentinel's bits."""
    out2 = out if out.dim() == 2 else out[None]
    expect = torch.full(out2.shape, SENTINEL, dtype=torch.int32, device=out.device)
    for row0, col0, ref in blocks:
        ref2 = ref if ref.dim() == 2 else ref[None]
        h, w = ref2.shape
        got = out2[row0:row0 + h, col0:col0 + w]
        bad = got != ref2
        assert not bad.any(), (f"{what}: {int(bad.sum())} of {h * w} elements of the block at ({row0}, {col0}) differ, first at "
                               f"{bad.nonzero()[0].tolist()}: got {got[bad][0].item()}, want {ref2[bad][0].item()}")
        expect[row0:row0 + h, col0:col0 + w] = got.view(torch.int32)
    touched = out2.view(torch.int32) != expect
    assert not touched.any(), f"{what}: {int(touched.sum())} elements outside the taken blocks were written, first at {touched.nonzero()[0].tolist()}"


def ref_product(delta, acts, N, K, col0=0):
    """fp64 on the device; exact for the integer operands, so its fp32 cast is THE result."""
    d = delta[:, col0:col0 + N].double()
    return (d.t() @ acts[:, :K].double()).float(), d.sum(0).float()


def whole_block(N, K, ld_delta, ld_acts, colsum, rows, gen, pad="ints"):
    """One product in a pass's form with its whole block (and column sums) taken into sentinel tensors one row, three columns
    and five elements larger than the take."""
    dev = gen.device
    p = dict(delta=int_delta(rows, ld_delta, N, gen, pad), N=N, acts=int_acts(rows, ld_acts, K, gen, pad), K=K, colsum=colsum)
    p["out"], p["sums"] = sentinel((N + 2, K + 3), dev), sentinel(N + 5, dev)
    p["takes"] = [(0, 0, N, K, p["out"], 1, 2)]
    p["colsum_takes"] = [(0, N, p["sums"], 3)] if colsum else []
    return p


def check_whole_block(p, what, acts2=None):
    dW, db = ref_product(p["delta"], p["acts"], p["N"], p["K"])
    if acts2 is not None:
        dW = torch.cat([dW[:, :128], ref_product(p["delta"], acts2, 256, 128)[0]], 1)
    assert_blocks(p["out"], [(1, 2, dW)], what + " dW")
    if p["colsum"]:
        assert_blocks(p["sums"], [(0, 3, db)], what + " column sums")


# ---------------------------------------------------------------------------------------------- T1
@pytest.mark.parametrize("N,K", sorted(CHUNK_ROWS))
def test_every_fp32_shape_is_exact_at_every_class_of_plan(idn, dev, N, K):
    """T1, the six gemm_tn_kernel instantiations on the fp32 pipe, in the pass's pitches: integer operands, so every output
    and column sum EQUALS the fp64 product; at one, two and three chunks per split, three with a last split of one chunk, and
    in the ring's steady state (five and more) with a last split of one chunk and a short one -- by the reported plan."""
    ld_delta, ld_acts, colsum = PASS_FORMS[(N, K)]
    R = CHUNK_ROWS[(N, K)]
    gen = torch.Generator(device=dev).manual_seed(1000 + N + K)
    reached = set()
    for rows in F32_ROWS[R]:
        p = whole_block(N, K, ld_delta, ld_acts, colsum, rows, gen)
        (plan,) = idn.ops.dw_products(rows, [p], pipe=F32)
        name, last = plan_class(rows, R, plan)
        reached.add(name)
        check_whole_block(p, f"{N} x {K}, {rows} rows, {plan[0]} splits of {plan[1]} chunks (last {last}: {name})")
    assert reached >= ALL_CLASSES, (N, K, sorted(ALL_CLASSES - reached))


@pytest.mark.parametrize("form", ["plain", "split-B, acts2 above acts", "split-B, acts2 below acts"])
@pytest.mark.parametrize("items", [1, X6_ITEMS_PER_PASS])
def test_x6_kernel_is_exact_at_every_class_of_plan(idn, dev, cus, items, form):
    """T1, gemm_tn_x6_kernel: alone (every CU its own split) and with the CUs divided among the nine products of a pass;
    one B matrix, and the split-B form that pairs views_linears.2 | .1 with its second matrix on either side of the first."""
    gen = torch.Generator(device=dev).manual_seed(2000 + items + len(form))
    rows_for = x6_rows(cus, items)
    reached = set()
    for rows in sorted(rows_for.values()):
        p = whole_block(256, 256, 256, 256 if form == "plain" else 128, True, rows, gen)
        acts2 = None
        if form != "plain":
            low, high = act_pair(rows, gen)
            p["acts"], acts2 = (low, high) if "above" in form else (high, low)
            assert (acts2.data_ptr() > p["acts"].data_ptr()) == ("above" in form)
            p["acts2"] = acts2
        (plan,) = idn.ops.dw_products(rows, [p], pipe=X6, x6_items=items)
        name, last = plan_class(rows, 16, plan)
        reached.add(name)
        check_whole_block(p, f"x6 {form}, {items} items, {rows} rows, {plan[0]} splits of {plan[1]} chunks (last {last}: {name})", acts2)
    assert reached >= ALL_CLASSES, (items, form, cus, sorted(ALL_CLASSES - reached))


# ---------------------------------------------------------------------------------------------- T2
def run_and_check(idn, rows, pipe, x6_items, products, expect, want_uneven=True):
    """One call; `expect`: [(out, [(row0, col0, reference)], name)].  Every plan must be uneven (a short last split)."""
    plans = idn.ops.dw_products(rows, products, pipe=pipe, x6_items=x6_items)
    for p, plan in zip(products, plans):
        x6 = pipe == X6 and (p["N"], p["K"]) == (256, 256)
        name, last = plan_class(rows, 16 if x6 else CHUNK_ROWS[(p["N"], p["K"])], plan)
        if want_uneven:
            assert plan[1] >= 3 and last < plan[1], (p["N"], p["K"], plan, name)
    for out, blocks, name in expect:
        assert_blocks(out, blocks, name)
    return plans


@pytest.mark.parametrize("pipe", [X6, F32])
def test_takes_read_and_write_nothing_outside_their_blocks(idn, dev, pipe):
    """T2, the pass's own forms: operand columns a product does not name hold NaN, every output tensor is larger than its
    takes and prefilled with one NaN bit pattern; afterwards each taken block is exact and every other element of every
    output still has the sentinel's bits (fold_bwd_kernel fills the conditioning columns between the blocks in a pass)."""
    rows = UNEVEN_ROWS
    gen = torch.Generator(device=dev).manual_seed(3000 + pipe)
    S = lambda *shape: sentinel(shape, dev)
    products, expect = [], []
    x0 = int_acts(rows, 64, 64, gen)                 # the encoded input [encoding 63 | 0]
    # pts_linears.0: 256 x 64, 63 columns into pts_w[0] at ld0; its column sums
    dA0, w0, b0 = int_delta(rows, 256, 256, gen), S(256 + 2, LD0), S(256 + 4)
    products.append(dict(delta=dA0, N=256, acts=x0, K=64, colsum=True, takes=[(0, 0, 256, 63, w0, 1, 0)], colsum_takes=[(0, 256, b0, 2)]))
    dW, db = ref_product(dA0, x0, 256, 64)
    expect += [(w0, [(1, 0, dW[:, :63])], "pts_linears.0 weight"), (b0, [(0, 2, db)], "pts_linears.0 bias")]
    # pts_linears.5: 256 x 256 at column 63 + C of pts_w[5] at ld5, beside the 256 x 63 block of its encoding columns
    dA5, a5, w5, b5 = int_delta(rows, 256, 256, gen), int_acts(rows, 256, 256, gen), S(256 + 2, LD5), S(256 + 4)
    products.append(dict(delta=dA5, N=256, acts=a5, K=256, colsum=True, takes=[(0, 0, 256, 256, w5, 1, 63 + COND)], colsum_takes=[(0, 256, b5, 2)]))
    products.append(dict(delta=dA5, N=256, acts=x0, K=64, colsum=False, takes=[(0, 0, 256, 63, w5, 1, 0)]))
    dW, db = ref_product(dA5, a5, 256, 256)
    expect += [(w5, [(1, 63 + COND, dW), (1, 0, ref_product(dA5, x0, 256, 64)[0][:, :63])], "pts_linears.5 weight"), (b5, [(0, 2, db)], "pts_linears.5 bias")]
    # views_linears.0 + alpha_linear: delta columns 0..127 and 128 of a 256-column matrix whose columns 129..255 hold NaN,
    # against a8 -- rows 0..127 into views_w[0] at ldv, row 128 into alpha_w, column sums 0..127 and 128; and the direction
    # columns, 128 x 27 of a 128 x 64 product of the same delta matrix (its unread columns: 128 and the NaNs), at column 256
    dV0, a8, xd = int_delta(rows, 256, 129, gen, "nan"), int_acts(rows, 256, 256, gen), int_acts(rows, 64, 64, gen)
    wv0, bv0, wa, ba = S(128 + 2, LDV), S(128 + 4), S(1 + 2, 256 + 3), S(1 + 4)
    products.append(dict(delta=dV0, N=256, acts=a8, K=256, colsum=True,
                         takes=[(0, 0, 128, 256, wv0, 1, 0), (SIGMA, 0, 1, 256, wa, 1, 2)], colsum_takes=[(0, 128, bv0, 2), (SIGMA, 1, ba, 2)]))
    products.append(dict(delta=dV0, N=128, acts=xd, K=64, colsum=False, takes=[(0, 0, 128, 27, wv0, 1, 256)]))
    dW, db = ref_product(dV0, a8, 129, 256)
    expect += [(wv0, [(1, 0, dW[:128]), (1, 256, ref_product(dV0, xd, 128, 64)[0][:, :27])], "views_linears.0 weight"),
               (bv0, [(0, 2, db[:128])], "views_linears.0 bias"), (wa, [(1, 2, dW[128:129])], "alpha_linear weight"),
               (ba, [(0, 2, db[128:129])], "alpha_linear bias")]
    # rgb_linear: 3 x 128 of the 64-row product, column sums 0..2
    dR, v3, wr, br = int_delta(rows, 64, 64, gen), int_acts(rows, 128, 128, gen), S(3 + 2, 128 + 3), S(3 + 4)
    products.append(dict(delta=dR, N=64, acts=v3, K=128, colsum=True, takes=[(0, 0, 3, 128, wr, 1, 2)], colsum_takes=[(0, 3, br, 2)]))
    dW, db = ref_product(dR, v3, 64, 128)
    expect += [(wr, [(1, 2, dW[:3])], "rgb_linear weight"), (br, [(0, 2, db[:3])], "rgb_linear bias")]
    # views_linears.2 | .1: their deltas side by side in one 256-column matrix, two 128-column activation matrices
    v2, v1 = act_pair(rows, gen)
    wv, bv = [S(128 + 2, 128 + 3), S(128 + 2, 128 + 3)], [S(128 + 4), S(128 + 4)]
    if pipe == X6:   # one split-B product, its diagonal blocks
        dV = int_delta(rows, 256, 256, gen)
        products.append(dict(delta=dV, N=256, acts=v2, K=256, acts2=v1, colsum=True,
                             takes=[(0, 0, 128, 128, wv[0], 1, 2), (128, 128, 128, 128, wv[1], 1, 2)],
                             colsum_takes=[(0, 128, bv[0], 2), (128, 128, bv[1], 2)]))
        halves = [(dV, 0), (dV, 128)]
    else:            # two products; the half of the matrix the other one owns holds NaN
        halves = [(int_delta(rows, 256, 128, gen, "nan", 0), 0), (int_delta(rows, 256, 128, gen, "nan", 128), 128)]
        for (d, c0), v, w, b in zip(halves, (v2, v1), wv, bv):
            products.append(dict(delta=d, delta_col0=c0, N=128, acts=v, K=128, colsum=True, takes=[(0, 0, 128, 128, w, 1, 2)], colsum_takes=[(0, 128, b, 2)]))
    for (d, c0), v, w, b, layer in zip(halves, (v2, v1), wv, bv, (2, 1)):
        dW, db = ref_product(d, v, 128, 128, c0)
        expect += [(w, [(1, 2, dW)], f"views_linears.{layer} weight"), (b, [(0, 2, db)], f"views_linears.{layer} bias")]
    # the pass's split count for the 256 x 256 products (its nine items); the order of a pass is T3's business
    run_and_check(idn, rows, pipe, X6_ITEMS_PER_PASS, products, expect)


# ---------------------------------------------------------------------------------------------- T3
def pass_list(pipe, rows, gen):
    """kPassProducts (csrc/dw_gemm.h) in order with the takes of bwd_tail (csrc/train.hip), distinct integer operands per
    product, the gradient tensors at their own pitches (three rows longer, sentinel-filled)."""
    dev = gen.device
    S = lambda n_rows, ld: sentinel((n_rows + 3, ld), dev)
    V = lambda n: sentinel(n + 3, dev)
    products, expect = [], []

    def add(N, K, ld_delta, ld_acts, colsum, takes, ctakes, acts2=False, delta_used=None):
        d = int_delta(rows, ld_delta, N if delta_used is None else delta_used, gen, "nan" if delta_used else "ints")
        a, a2 = act_pair(rows, gen) if acts2 else (int_acts(rows, ld_acts, min(K, ld_acts), gen), None)
        p = dict(delta=d, N=N, acts=a, K=K, colsum=colsum, takes=[(r0, c0, h, w, out, 0, oc) for r0, c0, h, w, out, oc, _ in takes],
                 colsum_takes=[(c0, w, out, 0) for c0, w, out, _ in ctakes])
        dW, db = ref_product(d, a, N if delta_used is None else delta_used, min(K, ld_acts))
        if acts2:
            p["acts2"] = a2
            dW = torch.cat([dW, ref_product(d, p["acts2"], N, ld_acts)[0]], 1)
        products.append(p)
        for r0, c0, h, w, out, oc, name in takes:
            expect.append([out, [(0, oc, dW[r0:r0 + h, c0:c0 + w])], name])
        for c0, w, out, name in ctakes:
            expect.append([out, [(0, 0, db[c0:c0 + w])], name])

    add(64, 128, 64, 128, True, [(0, 0, 3, 128, S(3, 128), 0, "rgb_linear.weight")], [(0, 3, V(3), "rgb_linear.bias")])
    if pipe == X6:
        add(256, 256, 256, 128, True, [(0, 0, 128, 128, S(128, 128), 0, "views_linears.2.weight"), (128, 128, 128, 128, S(128, 128), 0, "views_linears.1.weight")],
            [(0, 128, V(128), "views_linears.2.bias"), (128, 128, V(128), "views_linears.1.bias")], acts2=True)
    else:
        for layer in (2, 1):
            add(128, 128, 256, 128, True, [(0, 0, 128, 128, S(128, 128), 0, f"views_linears.{layer}.weight")], [(0, 128, V(128), f"views_linears.{layer}.bias")])
    wv0 = S(128, LDV)
    add(256, 256, 256, 256, True, [(0, 0, 128, 256, wv0, 0, "views_linears.0.weight"), (SIGMA, 0, 1, 256, S(1, 256), 0, "alpha_linear.weight")],
        [(0, 128, V(128), "views_linears.0.bias"), (SIGMA, 1, V(1), "alpha_linear.bias")], delta_used=129)
    add(128, 64, 256, 64, False, [(0, 0, 128, 27, wv0, 256, "views_linears.0.weight")], [])
    for layer in range(7, 0, -1):
        if layer == 5:
            w5 = S(256, LD5)
            add(256, 256, 256, 256, True, [(0, 0, 256, 256, w5, 63 + COND, "pts_linears.5.weight")], [(0, 256, V(256), "pts_linears.5.bias")])
            add(256, 64, 256, 64, False, [(0, 0, 256, 63, w5, 0, "pts_linears.5.weight")], [])
        else:
            add(256, 256, 256, 256, True, [(0, 0, 256, 256, S(256, 256), 0, f"pts_linears.{layer}.weight")], [(0, 256, V(256), f"pts_linears.{layer}.bias")])
    add(256, 64, 256, 64, True, [(0, 0, 256, 63, S(256, LD0), 0, "pts_linears.0.weight")], [(0, 256, V(256), "pts_linears.0.bias")])
    # two products write the same tensor twice (views_linears.0, pts_linears.5): one check per tensor, with both blocks
    merged = {}
    for out, blocks, name in expect:
        merged.setdefault(id(out), [out, [], name])[1].extend(blocks)
    return products, list(merged.values())


@pytest.mark.parametrize("pipe", [X6, F32])
def test_a_whole_pass_of_products_in_one_call(idn, dev, pipe):
    """T3: the list of a training pass in ONE call -- the nine-item x6 batch (blockIdx.z / splits), the carving of the two
    pools over thirteen / fourteen slabs and the multi-item search of reduce_batch_kernel over all 28 takes -- every gradient
    block exact, everything around the blocks untouched, and the same bits from a second call."""
    rows = UNEVEN_ROWS
    products, expect = pass_list(pipe, rows, torch.Generator(device=dev).manual_seed(4000 + pipe))
    shapes = [(p["N"], p["K"]) for p in products]
    assert shapes.count((256, 256)) == (9 if pipe == X6 else 8) and len(products) == (13 if pipe == X6 else 14)
    assert sum(len(p["takes"]) + len(p["colsum_takes"]) for p in products) == 28
    plans = run_and_check(idn, rows, pipe, X6_ITEMS_PER_PASS, products, expect)
    if pipe == X6:   # the batch's items share one split count
        assert len({pl for pl, sh in zip(plans, shapes) if sh == (256, 256)}) == 1
    first = [out.clone() for out, _, _ in expect]
    assert idn.ops.dw_products(rows, products, pipe=pipe, x6_items=X6_ITEMS_PER_PASS) == plans
    for (out, _, name), before in zip(expect, first):
        assert torch.equal(out.view(torch.int32), before.view(torch.int32)), name


# ---------------------------------------------------------------------------------------------- T4
DW_BOUND, DB_BOUND = 2e-7, 3e-7     # what test_dw_gemm_bf16_pieces_match_the_fp32_pipe_against_fp64 holds the 256 x 256 kernels to


def normal_operands(rows, ld_delta, ld_acts, kind, gen):
    dev = gen.device
    d = torch.randn((rows, ld_delta), generator=gen, device=dev)
    a = torch.randn((rows, ld_acts), generator=gen, device=dev)
    if kind == "relu":     # post-ReLU activations, sparse deltas
        a = torch.relu(a)
        d = d * (torch.rand((rows, ld_delta), generator=gen, device=dev) < 0.1)
    return d, a


def graded(idn, rows, pipe, items, N, K, d, a, colsum, a2=None, col0=0):
    """max |err| / sum |a||b| of the whole block against fp64, and of the column sums / max sum |delta|; the block's errors."""
    dev = d.device
    out, sums = sentinel((N + 1, K + 1), dev), sentinel(N + 1, dev)
    p = dict(delta=d, delta_col0=col0, N=N, acts=a, K=K, colsum=colsum, takes=[(0, 0, N, K, out, 0, 0)],
             colsum_takes=[(0, N, sums, 0)] if colsum else [])
    if a2 is not None:
        p["acts2"] = a2
    (plan,) = idn.ops.dw_products(rows, [p], pipe=pipe, x6_items=items)
    d64 = d[:, col0:col0 + N].double()
    a64 = a[:, :K].double() if a2 is None else torch.cat([a[:, :128], a2[:, :128]], 1).double()
    err = (out[:N, :K].double() - d64.t() @ a64).abs() / (d64.abs().t() @ a64.abs())
    assert torch.isfinite(err).all()
    assert_blocks(out, [(0, 0, out[:N, :K].clone())], "graded block")     # (the sentinels around it)
    eb = float((sums[:N].double() - d64.sum(0)).abs().max() / d64.abs().sum(0).max()) if colsum else 0.0
    return err, eb, plan


@pytest.mark.parametrize("kind", ["normal", "relu"])
def test_rounding_grade_at_long_splits(idn, dev, cus, kind):
    """T4: standard-normal operands (and the post-ReLU kind: activations >= 0, 10 % of the deltas non-zero) at the row counts
    whose splits run five and more chunks: max |err| / sum |a||b| against fp64 below 2e-7 and the column sums' max |err| / max
    sum |delta| below 3e-7 -- the bounds the 256 x 256 kernels are held to; a correct fp32 fma chain per split with fp64
    across the splits measures 2.1e-8 .. 7.7e-8 on these kinds at splits of 64 .. 2 304 rows, so the bounds leave the
    reference arithmetic a factor of 2.6 and more.  The split-B form must also stay within 4 x the error of two fp32-pipe
    128 x 128 products of the same operands + 3e-8 on its diagonal blocks.

    Measured on an MI355X (256 CUs), worst over the shapes (profiles/dw_products_parity.log): dW 9.7e-9 (normal) / 1.6e-8
    (relu) on the fp32 pipe, 2.0e-8 / 6.1e-8 on the bf16 pieces, plain and split-B alike; column sums at most 1.1e-8; the
    split-B diagonal blocks at most 2.9 x the two fp32-pipe products (4.0e-8 against 1.4e-8)."""
    gen = torch.Generator(device=dev).manual_seed(5000 + len(kind))
    print()
    for (N, K), R in sorted(CHUNK_ROWS.items()):
        ld_delta, ld_acts, colsum = PASS_FORMS[(N, K)]
        for rows in F32_ROWS[R][-2:]:
            d, a = normal_operands(rows, ld_delta, ld_acts, kind, gen)
            err, eb, plan = graded(idn, rows, F32, 1, N, K, d, a, colsum)
            name, last = plan_class(rows, R, plan)
            assert name in ("long-last1", "long-short-last"), (N, K, rows, plan)
            print(f"  dW {kind:6s} fp32 {N:3d} x {K:3d} rows {rows:6d} ({plan[0]:3d} splits of {plan[1]:2d} chunks, last {last:2d}): "
                  f"dW {float(err.max()):.2e}  db " + (f"{eb:.2e}" if colsum else "(none kept)"))
            assert float(err.max()) < DW_BOUND and eb < DB_BOUND, (kind, N, K, rows, float(err.max()), eb)
    for items in (1, X6_ITEMS_PER_PASS):
        rows_for = x6_rows(cus, items)
        for rows in sorted({rows_for["long-last1"], rows_for["long-short-last"], 16512}):
            d, a = normal_operands(rows, 256, 256, kind, gen)
            err, eb, plan = graded(idn, rows, X6, items, 256, 256, d, a, True)
            name, last = plan_class(rows, 16, plan)
            assert plan[1] >= 5, (items, rows, plan)
            print(f"  dW {kind:6s} x6 plain, {items} item(s)  rows {rows:6d} ({plan[0]:3d} splits of {plan[1]:2d} chunks, last {last:2d}): "
                  f"dW {float(err.max()):.2e}  db {eb:.2e}")
            assert float(err.max()) < DW_BOUND and eb < DB_BOUND, (kind, "x6", items, rows, float(err.max()), eb)
            # split-B: B columns 0..127 from a[:, :128]'s matrix, 128..255 from a second one -- against two fp32-pipe products
            b0, b1 = torch.stack([a[:, :128], a[:, 128:]])     # one allocation
            err, eb, plan = graded(idn, rows, X6, items, 256, 256, d, b0, True, a2=b1)
            diag = max(float(err[:128, :128].max()), float(err[128:, 128:].max()))
            f32 = max(float(graded(idn, rows, F32, 1, 128, 128, d, b0, True)[0].max()),
                      float(graded(idn, rows, F32, 1, 128, 128, d, b1, True, col0=128)[0].max()))
            print(f"  dW {kind:6s} x6 split-B, {items} item(s) rows {rows:6d} ({plan[0]:3d} splits of {plan[1]:2d} chunks): "
                  f"dW {float(err.max()):.2e} (diagonal blocks {diag:.2e}, two fp32 128 x 128 products {f32:.2e})  db {eb:.2e}")
            assert float(err.max()) < DW_BOUND and eb < DB_BOUND and diag < 4 * f32 + 3e-8, (kind, "split-B", items, rows, float(err.max()), diag, f32, eb)
