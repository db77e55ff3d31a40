"""The backward delta chain of the training step (csrc/mlp_f32_bwd.hip: delta_chain_kernel and x6::delta_chain_x6_kernel),
stage by stage and element by element against torch fp64 on the device.  ``ops.delta_chain`` runs the chain alone -- the
pack and the chain launch of a pass, on either pipe, with the grid capped so that a few hundred rows make one workgroup walk
several tiles -- and reports the grid that ran; the tests assert their coverage on that report.

The reference, with m(l) the ReLU on-mask of layer l (``ref_chain``):
    dV2 = m(v3) (.) d_rgb[:, :3] . rgb_w                  dV1 = m(v2) (.) dV2 . views_w[2]
    dV0[:, :128] = m(v1) (.) dV1 . views_w[1]             dA[7] = m(a8) (.) (dV0[:, :128] . views_w[0][:, :256] + d_sigma (x) alpha_w)
    dA[l-1] = m(a_l) (.) dA[l] . W_l,  l = 7 .. 1,  W_5 = pts_w[5][:, 63 + C:]
The masks are GIVEN, as packed bits (``pack_masks``, held to the training forward bit for bit by T0), so no ReLU kink can
interfere with an element-wise comparison.

T1 / T2 use operands whose every product and partial sum is an integer below 2^24: the fp32 chains, the six bf16 piece
products and fp64 agree exactly in any order, and the assertions are equalities.  T3 grades the rounding of each stage on the
stage's own stored input; T4 ties the aid to the pass.  Needs an MI355X.
"""
import os

import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

X6, F32 = 0, 1                                       # IDN_DW_PIPE_BF16X6, IDN_DW_PIPE_F32
PIPE_NAME = {X6: "x6", F32: "f32"}
DIMS = [(64, 76, 32), (106, 0, 0), (64, 0, 0)]       # (dim_aud, dim_expr, dim_latent): head, torso, no expr / latent
ACT_COLS = 2560                                      # kActCols: x0 64 | dir 64 | a1..a8 256 each | v1..v3 128 each
ACT_OFF = [128 + 256 * i for i in range(8)] + [2176 + 128 * i for i in range(3)]   # first slab column of mask layer id
WIDTH = [256] * 8 + [128] * 3                        # mask layer id 0..7 = a1..a8, 8..10 = v1..v3
MASK_ID = [10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]         # the layer whose ReLU bits mask the output of stage s
NAMES = ["dV2", "dV1", "dV0", "dA7", "dA6", "dA5", "dA4", "dA3", "dA2", "dA1", "dA0"]   # the output of stage s
SENTINEL = 0x7fc5a5a5                                # one quiet-NaN bit pattern no kernel here produces
GUARD = 4096                                         # sentinel words in front of and behind every output matrix
NAN = float("nan")


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


# ---------------------------------------------------------------------------------------------- masks
def pack_masks(on, tail=0):
    """11 bool matrices [p_pad, W] (True = the unit is on) -> the slab's mask words, int32 [11, p_pad / 32, 64, 4]
    (csrc/idn_internal.h): entry [id][point // 32][lane = point % 32 + 32 h] is four dwords; register r of tile T of that
    lane is channel 32 T + (r & 3) + 8 (r >> 2) + 4 h, and bit 31 - (16 (T & 1) + r) of dword T >> 1 is 1 where the unit is
    OFF.  The 128-wide layers (ids 8..10) use dwords 0 and 1; their dwords 2 and 3 are filled with `tail`."""
    assert len(on) == 11
    p_pad, dev = on[0].shape[0], on[0].device
    words = torch.full((11, p_pad // 32, 64, 4), tail, dtype=torch.int32, device=dev)
    bit = torch.ones((), dtype=torch.int64, device=dev) << (31 - torch.arange(32, device=dev))
    for i, m in enumerate(on):
        W = WIDTH[i]
        assert m.dtype == torch.bool and tuple(m.shape) == (p_pad, W), (i, m.shape)
        off = ~m.reshape(p_pad // 32, 32, W // 32, 4, 2, 4)        # [wave tile, point, T, r >> 2, h, r & 3]
        off = off.permute(0, 4, 1, 2, 3, 5).reshape(p_pad // 32, 64, W // 64, 32)   # [wave tile, lane, T >> 1, 16 (T & 1) + r]
        w = (off.to(torch.int64) * bit).sum(-1)
        words[i, :, :, :W // 64] = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    return words


def mask_words(acts, p_pad):
    """The mask tail of an activation slab as int32 [11, p_pad / 32, 64, 4] (a view)."""
    return acts[ACT_COLS * p_pad:].view(torch.int32).view(11, p_pad // 32, 64, 4)


def slab_with(on, tail=0):
    """A slab whose activation part is NaN (the chain must not read it) and whose mask tail is pack_masks(on)."""
    p_pad = on[0].shape[0]
    acts = torch.full((p_pad * (ACT_COLS + 88),), NAN, dtype=torch.float32, device=on[0].device)
    mask_words(acts, p_pad).copy_(pack_masks(on, tail))
    return acts


def random_masks(p_pad, p_on, gen, dev):
    return [(torch.rand((p_pad, W), generator=gen) < p_on).to(dev) for W in WIDTH]


# ---------------------------------------------------------------------------------------------- reference
def stage_product(w, C, s, x, d_sigma):
    """The pre-mask output of stage s from its input x [P, K]: delta_in = delta_out . W (W in nn.Linear layout [out, in])."""
    if s == 0:
        return x @ w["rgb_linear.weight"]
    if s in (1, 2):
        return x @ w[f"views_linears.{3 - s}.weight"]
    if s == 3:
        return x @ w["views_linears.0.weight"][:, :256] + d_sigma[:, None] * w["alpha_linear.weight"]
    l = 11 - s                                                    # stages 4..10: pts_linears.7 .. .1
    W = w[f"pts_linears.{l}.weight"]
    return x @ (W[:, 63 + C:] if l == 5 else W)


def ref_chain(w, C, on, d_rgb3, d_sigma):
    """The eleven delta matrices in NAMES' order, in the dtype of the operands (fp64 in every test)."""
    out, x = [], d_rgb3
    for s in range(11):
        x = on[MASK_ID[s]].to(x.dtype) * stage_product(w, C, s, x, d_sigma)
        out.append(x)
    return out


# ---------------------------------------------------------------------------------------------- running the aid
def guarded(shape, dev):
    """(whole int32 buffer, float32 view of `shape` in its middle): SENTINEL everywhere, GUARD words on either side."""
    n = 1
    for d in shape:
        n *= d
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return whole, whole[GUARD:GUARD + n].view(torch.float32).view(shape)


def guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def run_chain(idn, p, pipe, acts, d_rgb3, d_sigma, max_blocks=0):
    """One call of the aid on fresh guarded buffers.  d_rgb carries NaN in columns 3..63, dv0 the sentinel in every column but
    128: afterwards columns 129..255 of dv0 and the guards of all three outputs hold the sentinel bit for bit and every
    written value is finite.  -> (the eleven matrices in NAMES' order, blocks)."""
    dev, p_pad = acts.device, d_rgb3.shape[0]
    d_rgb = torch.full((p_pad, 64), NAN, dtype=torch.float32, device=dev)
    d_rgb[:, :3] = d_rgb3
    w0, dv0 = guarded((p_pad, 256), dev)
    w21, dv21 = guarded((p_pad, 256), dev)
    wa, da = guarded((8, p_pad, 256), dev)
    dv0[:, 128] = d_sigma
    r21, ra, blocks = idn.ops.delta_chain(p, pipe, acts, d_rgb, dv0, max_blocks=max_blocks, dv21=dv21, da=da)
    assert r21.data_ptr() == dv21.data_ptr() and ra.data_ptr() == da.data_ptr()
    assert guards_intact(w0) and guards_intact(w21) and guards_intact(wa), "a write outside the delta matrices"
    assert bool((dv0[:, 129:].view(torch.int32) == SENTINEL).all()), "columns 129..255 of dv0 were written"
    assert torch.equal(dv0[:, 128], d_sigma), "d sigma was overwritten"
    outs = [dv21[:, :128], dv21[:, 128:], dv0[:, :128]] + [da[l] for l in range(7, -1, -1)]
    for name, t in zip(NAMES, outs):
        assert bool(torch.isfinite(t).all()), f"{name}: not every element was written with a finite value"
    return outs, blocks


def assert_same(got, ref, ctx):
    """Equality by value of every matrix (+0 == -0), with the first differing element named."""
    for name, g, r in zip(NAMES, got, ref):
        if not torch.equal(g, r):
            bad = (g != r).nonzero()
            row, col = (int(v) for v in bad[0])
            raise AssertionError(f"{ctx}: {name} differs in {bad.shape[0]} of {g.numel()} elements, first at row {row} (tile {row // 128}, "
                                 f"wave {row % 128 // 32}, point {row % 32}) column {col}: got {float(g[row, col])}, want {float(r[row, col])}")


# ---------------------------------------------------------------------------------------------- exact operands
def exact_net(dims3, seed):
    """Weights in state-dict layout (CPU fp32): every stage's matrix has exactly 4 non-zeros (+-1, rows at random) per
    output channel of the stage, i.e. per COLUMN of the nn.Linear weight; alpha_linear's one row and rgb_linear's three are
    +-1 throughout.  Everything the chain must not read is NaN: pts_linears.0, the encoding / conditioning columns of
    pts_linears.5, the direction / expression columns of views_linears.0 and every bias."""
    a, e, l = dims3
    C = a + e + l
    g = torch.Generator().manual_seed(seed)

    def sparse(k, n, nnz=4):
        rows = torch.rand((k, n), generator=g).argsort(0)[:nnz]          # nnz distinct rows in every column
        sign = torch.randint(0, 2, (nnz, n), generator=g).float() * 2 - 1
        return torch.zeros(k, n).scatter_(0, rows, sign)

    sd = {"pts_linears.0.weight": torch.full((256, 63 + C), NAN)}
    for i in range(1, 8):
        sd[f"pts_linears.{i}.weight"] = sparse(256, 256)
    sd["pts_linears.5.weight"] = torch.cat([torch.full((256, 63 + C), NAN), sd["pts_linears.5.weight"]], 1)
    sd["views_linears.0.weight"] = torch.cat([sparse(128, 256), torch.full((128, 27 + e), NAN)], 1)
    sd["views_linears.1.weight"], sd["views_linears.2.weight"] = sparse(128, 128), sparse(128, 128)
    sd["alpha_linear.weight"], sd["rgb_linear.weight"] = sparse(1, 256, 1), sparse(3, 128, 3)
    for k in list(sd):
        sd[k.replace(".weight", ".bias")] = torch.full((sd[k].shape[0],), NAN)
    return sd


def distinct_seeds(p_pad, gen):
    """[p_pad, 4] (d rgb, d sigma): integers in [-255, 255], no two rows alike (rows drawn without replacement)."""
    codes = torch.unique(torch.randint(0, 511 ** 4, (p_pad + p_pad // 4 + 64,), generator=gen))
    assert codes.numel() >= p_pad
    codes = codes[torch.randperm(codes.numel(), generator=gen)][:p_pad]
    seeds = torch.stack([codes // 511 ** k % 511 - 255 for k in range(4)], 1)
    assert torch.unique(seeds, dim=0).shape[0] == p_pad and int(seeds.abs().max()) <= 255
    return seeds.float()


_nets, _cases = {}, {}


def exact_case(idn, dev, dims3, p_pad):
    """Weights, head seeds (integers in [-255, 255], no two rows alike), random masks (75 % on), the slab and the fp64
    reference of one (dims, p_pad): built once, shared by both pipes and every launch form, never written again."""
    if dims3 not in _nets:
        sd = {k: v.to(dev).contiguous() for k, v in exact_net(dims3, 100 + DIMS.index(dims3)).items()}
        _nets[dims3] = (sd, idn.ops.params_struct(sd, *dims3), {k: v.double() for k, v in sd.items()})
    sd, p, w64 = _nets[dims3]
    key = (dims3, p_pad)
    if key not in _cases:
        g = torch.Generator().manual_seed(7 * p_pad + DIMS.index(dims3))
        seeds = distinct_seeds(p_pad, g).to(dev)
        on = random_masks(p_pad, 0.75, g, dev)
        _cases[key] = dict(p=p, w64=w64, C=sum(dims3), seeds=seeds, on=on, acts=slab_with(on),
                           ref=exact_reference(w64, sum(dims3), on, seeds))
    return _cases[key]


def exact_reference(w64, C, on, seeds, need_spread=True):
    """fp64 reference cast to fp32, after the conditions that make the comparison exact (and, with random masks, telling)."""
    ref = ref_chain(w64, C, on, seeds[:, :3].double(), seeds[:, 3].double())
    wabs = {k: v.abs() for k, v in w64.items()}
    x = seeds[:, :3].double().abs()
    for s in range(11):      # sum |in| |W| of every stage below 2^24: every partial sum, in any order and of any pieces, is exact
        assert float(stage_product(wabs, C, s, x, seeds[:, 3].double().abs()).max()) < 2 ** 24, NAMES[s]
        x = ref[s].abs()
        assert float(x.max()) <= 2 ** 23, NAMES[s]
        assert bool((ref[s] == ref[s].round()).all())
    if need_spread:
        last = ref[10].abs()
        assert float((last != 0).double().mean()) >= 0.5, "fewer than half of dA[0] non-zero"
        assert float((last >= 2 ** 16).double().mean()) >= 0.05, "fewer than 5 % of dA[0] reach the third bf16 piece"
    return [t.float() for t in ref]


# ---------------------------------------------------------------------------------------------- T0
def test_pack_masks_is_the_training_forward_bit_for_bit(idn, dev):
    """T0: at n = 185 (p_pad 256) both activation-saving forwards write, for every row below n, exactly the words
    pack_masks makes of [a_l > 0] -- all 11 layers, every bit (dwords 2 and 3 of the 128-wide layers excluded: unspecified).
    The padding rows are reported, not asserted."""
    a, e, l = DIMS[0]
    dims = oracle.facenerf_dims(dim_aud=a, dim_expr=e, dim_latent=l)
    net = idn.FaceNeRF(dim_aud=a, dim_latent=l, dim_expr=e)
    net.load_state_dict(oracle.xavier_facenerf_params(5, dims))
    net = net.to(dev)
    g = torch.Generator().manual_seed(3)
    n, p_pad = 185, 256
    x = (torch.rand((n, 90), generator=g) * 2 - 1).to(dev)
    cond = [(torch.randn(d, generator=g) * 0.3).to(dev) for d in (a, e, l)]
    folded = net.folded_bias(*cond)
    point = torch.arange(p_pad // 32, device=dev)[:, None] * 32 + torch.arange(64, device=dev)[None, :] % 32    # [wave tile, lane]
    for prec, code in (("f32", idn._lib.IDN_PREC_F32), ("bf16x6", idn._lib.IDN_PREC_BF16X6)):
        _, acts = idn.ops.facenerf_train_fwd(net.packed_weights(prec), folded, x, code)
        assert acts.numel() == p_pad * (ACT_COLS + 88)
        on = [acts[ACT_OFF[i] * p_pad:(ACT_OFF[i] + WIDTH[i]) * p_pad].view(p_pad, WIDTH[i]) > 0 for i in range(11)]
        want, got = pack_masks(on), mask_words(acts, p_pad)
        for i in range(11):
            frac = float(on[i][:n].double().mean())
            assert 0.05 < frac < 0.95, (prec, i, frac)       # (a layer all on or all off would check nothing)
            nd = WIDTH[i] // 64
            same = (got[i, :, :, :nd] == want[i, :, :, :nd]).all(-1)
            assert bool(same[point < n].all()), f"{prec}: mask layer {i}: {int((~same[point < n]).sum())} (point, lane half) entries differ"
        pad = point >= n
        pad_same = all(bool((got[i, :, :, :WIDTH[i] // 64] == want[i, :, :, :WIDTH[i] // 64]).all(-1)[pad].all()) for i in range(11))
        last_lane = (n - 1) % 32 + 32 * (torch.arange(64, device=dev) // 32)       # row n - 1's entry of the same lane half
        last = all(bool((got[i, :, :, :WIDTH[i] // 64] == got[i, (n - 1) // 32, last_lane, :WIDTH[i] // 64][None]).all(-1)[pad].all())
                   for i in range(11))
        print(f"\n  {prec}: padding rows {n}..{p_pad - 1}: mask words equal pack_masks of the slab's own padding activations: {pad_same}; "
              f"equal the words of row {n - 1}: {last}; "
              f"dwords 2, 3 of ids 8..10 over all rows: {sorted(set(got[8:, :, :, 2:].flatten().tolist()))[:4]}")


# ---------------------------------------------------------------------------------------------- T1
# (p_pad, max_blocks, the grid that must run): one tile; two blocks; one block walking five tiles (ring phase from tile to tile,
# finish_pass, the prefetch hand-over); blocks walking 3 + 2 and 4 + 3 + 3 tiles
FORMS = [(128, 0, 1), (256, 0, 2), (640, 1, 1), (640, 2, 2), (1280, 3, 3)]


@pytest.mark.parametrize("p_pad,max_blocks,grid", FORMS, ids=[f"{r}-{b}" for r, b, _ in FORMS])
@pytest.mark.parametrize("dims3", DIMS, ids=["head", "torso", "aud"])
@pytest.mark.parametrize("pipe", [X6, F32], ids=["x6", "f32"])
def test_exact_chain(idn, dev, pipe, dims3, p_pad, max_blocks, grid):
    """T1: all eleven matrices equal the fp64 reference element for element, both pipes, the three layouts of the skip layer and
    views_linears.0 in the pack kernels, every launch form."""
    c = exact_case(idn, dev, dims3, p_pad)
    got, blocks = run_chain(idn, c["p"], pipe, c["acts"], c["seeds"][:, :3], c["seeds"][:, 3].contiguous(), max_blocks)
    assert blocks == grid
    assert_same(got, c["ref"], f"{PIPE_NAME[pipe]} {dims3} rows {p_pad} blocks {blocks}")


@pytest.mark.parametrize("pipe", [X6, F32], ids=["x6", "f32"])
def test_exact_chain_at_the_grid_of_a_pass(idn, dev, cus, pipe):
    """T1, a pass's own grid: 128 (CUs + 3) rows, one workgroup per CU, three of them taking a second tile."""
    p_pad = 128 * (cus + 3)
    c = exact_case(idn, dev, DIMS[0], p_pad)
    got, blocks = run_chain(idn, c["p"], pipe, c["acts"], c["seeds"][:, :3], c["seeds"][:, 3].contiguous(), 0)
    assert blocks == cus
    assert_same(got, c["ref"], f"{PIPE_NAME[pipe]} rows {p_pad} blocks {blocks}")


# ---------------------------------------------------------------------------------------------- T2
def _edge_run(idn, c, pipe, on, d_sigma=None, tail=0):
    """Twice on the same operands: the same bits; -> the outputs and the fp64 reference."""
    d_sigma = c["seeds"][:, 3].contiguous() if d_sigma is None else d_sigma
    acts = slab_with(on, tail)
    got, blocks = run_chain(idn, c["p"], pipe, acts, c["seeds"][:, :3], d_sigma)
    again, _ = run_chain(idn, c["p"], pipe, acts, c["seeds"][:, :3], d_sigma)
    assert blocks == 2
    for name, g, h in zip(NAMES, got, again):
        assert torch.equal(g.contiguous().view(torch.int32), h.contiguous().view(torch.int32)), f"{name}: a second run gave other bits"
    ref = exact_reference(c["w64"], c["C"], on, torch.cat([c["seeds"][:, :3], d_sigma[:, None]], 1), need_spread=False)
    return got, ref


def one_unit_masks(c):
    """(c): exactly one unit on per point and layer, chosen stage by stage among the NON-ZERO pre-mask values of the point's
    row -- the k-th of them, k stepping from point to point -- so that the unit that is on carries a value all the way down:
    a bit that wrongly blocks it shows as one that wrongly lets another value through does.  A row whose pre-mask values
    are all zero (a weight row without non-zeros) takes its position by formula.  -> (masks, on-column of every point)."""
    seeds, dev = c["seeds"], c["seeds"].device
    p_pad = seeds.shape[0]
    rows = torch.arange(p_pad, device=dev)
    on, cols = [None] * 11, [None] * 11
    x, d_sigma = seeds[:, :3].double(), seeds[:, 3].double()
    for s in range(11):
        i = MASK_ID[s]
        pre = stage_product(c["w64"], c["C"], s, x, d_sigma)
        nz = pre != 0
        count = nz.sum(1)
        step = rows * 5 + 37 * i + 3
        kth = nz & ((nz.cumsum(1) - 1) == (step % count.clamp_min(1))[:, None])
        cols[i] = torch.where(count > 0, kth.double().argmax(1), step % WIDTH[i])
        on[i] = torch.zeros((p_pad, WIDTH[i]), dtype=torch.bool, device=dev)
        on[i][rows, cols[i]] = True
        x = on[i].double() * pre
    return on, cols


@pytest.mark.parametrize("pipe", [X6, F32], ids=["x6", "f32"])
def test_mask_edges(idn, dev, pipe):
    """T2 at p_pad 256, the exact operands: (a) every unit on; (b) one layer all off -- a head layer (v2) and a trunk layer
    (a4): everything downstream exactly zero, everything upstream as in (a); (c) exactly one unit on per point and layer, at a
    position that differs from point to point and carries a value (one_unit_masks); (d) dwords 2 and 3 of the 128-wide layers all ones and all zeros: the same
    outputs.  In every run (run_chain) the slab's activations and d_rgb's columns 3..63 are NaN, dv0's columns 129..255 and the
    surroundings of the outputs hold a sentinel that must survive bit for bit, every output is finite, and a second run
    gives the same bits."""
    p_pad = 256
    c = exact_case(idn, dev, DIMS[0], p_pad)
    ctx = PIPE_NAME[pipe]
    all_on = [torch.ones((p_pad, W), dtype=torch.bool, device=dev) for W in WIDTH]
    a_got, a_ref = _edge_run(idn, c, pipe, all_on)                                            # (a)
    assert_same(a_got, a_ref, f"{ctx} all on")
    assert all(float((t != 0).double().mean()) > 0.5 for t in a_ref)
    zero_sigma = torch.zeros(p_pad, device=dev)    # (d sigma enters BELOW the head layers: it is zero where their downstream must be)
    for layer, d_sigma in ((9, zero_sigma), (3, None)):                                       # (b): v2 (stage 1), a4 (stage 7)
        on = [torch.zeros_like(m) if i == layer else m for i, m in enumerate(all_on)]
        got, ref = _edge_run(idn, c, pipe, on, d_sigma)
        assert_same(got, ref, f"{ctx} layer {layer} off")
        s_off = MASK_ID.index(layer)
        for s in range(11):
            if s >= s_off:
                assert not bool(got[s].any()), f"{ctx} layer {layer} off: {NAMES[s]} is not zero"
            else:
                assert torch.equal(got[s], a_got[s]), f"{ctx} layer {layer} off: {NAMES[s]} changed upstream of it"
    one, cols = one_unit_masks(c)                                                             # (c)
    for i, col in enumerate(cols):        # the position steps from point to point and reaches every tile of the layer
        assert float((col[1:] != col[:-1]).double().mean()) > 0.9 and torch.unique(col // 32).numel() == WIDTH[i] // 32, i
    got, ref = _edge_run(idn, c, pipe, one)
    assert_same(got, ref, f"{ctx} one unit per point and layer")
    for name, t in zip(NAMES, got):       # ... and the one unit carries a value in most rows of every stage, down to dA0
        per_row = (t != 0).sum(1)
        assert int(per_row.max()) == 1 and float((per_row == 1).double().mean()) >= 0.5, name
    ones_got, ref = _edge_run(idn, c, pipe, c["on"], tail=-1)                                 # (d)
    zeros_got, _ = _edge_run(idn, c, pipe, c["on"], tail=0)
    assert_same(ones_got, ref, f"{ctx} dwords 2, 3 all ones")
    assert_same(zeros_got, ones_got, f"{ctx} dwords 2, 3 all zeros against all ones")


# ---------------------------------------------------------------------------------------------- T3
STAGE_BOUND = 2e-7         # what test_dw_gemm_bf16_pieces_match_the_fp32_pipe_against_fp64 holds the same two arithmetics to
TORCH_MULT = 4.0           # a stage measured above it: this multiple of torch's fp32 matmul of the same stage and inputs
X6_OVER_F32 = (4.0, 3e-8)  # bf16 pieces below 4 x the fp32 pipe + 3e-8, as there
# The (pipe, stage) pairs a correct kernel was measured above 2e-7 at, with (its figure, torch's fp32 matmul of the same stage on
# the same inputs) from profiles/delta_chain_parity.log; every other pair is held to 2e-7.
WIDENED = {("x6", "dV2"): (2.24e-07, 1.34e-07), ("f32", "dV1"): (2.17e-07, 2.40e-07),
           ("x6", "dV1"): (2.82e-07, 2.16e-07), ("f32", "dV0"): (2.24e-07, 2.18e-07),
           ("x6", "dV0"): (2.80e-07, 2.69e-07), ("f32", "dA7"): (2.04e-07, 2.14e-07),
           ("x6", "dA7"): (2.51e-07, 2.34e-07), ("f32", "dA6"): (2.23e-07, 2.19e-07),
           ("x6", "dA6"): (3.27e-07, 2.40e-07), ("f32", "dA5"): (2.53e-07, 2.53e-07),
           ("x6", "dA5"): (2.66e-07, 2.91e-07), ("f32", "dA4"): (2.60e-07, 2.42e-07),
           ("x6", "dA4"): (3.47e-07, 2.60e-07), ("f32", "dA3"): (2.66e-07, 2.61e-07),
           ("x6", "dA3"): (3.54e-07, 2.42e-07), ("f32", "dA2"): (2.85e-07, 2.59e-07),
           ("x6", "dA2"): (3.02e-07, 2.71e-07), ("f32", "dA1"): (2.52e-07, 2.52e-07),
           ("x6", "dA1"): (3.17e-07, 2.52e-07), ("f32", "dA0"): (2.24e-07, 2.42e-07),
           ("x6", "dA0"): (2.89e-07, 2.29e-07)}


def test_rounding_grade_stage_by_stage(idn, dev):
    """T3: Xavier weights, random masks (50 % on), head seeds normal x 2^u with u uniform in [-40, 0] per row (the spread of
    transmittance-weighted gradients along a ray), 1280 rows on 3 workgroups.  Every stage is graded against fp64 applied to the
    kernel's OWN stored output of the stage before -- exactly what the stage consumed -- in the project's unit,
    max |got - ref| / (|in| . |W|) per element, next to torch's fp32 matmul of the same stage on the same inputs.

    Each pipe below 2e-7, the bf16 pieces below 4 x the fp32 pipe + 3e-8 -- except the pairs of WIDENED, where the kernel and
    torch's fp32 matmul alike were measured above 2e-7 and the kernel is held to 4 x torch's figure instead.  That is every
    pair but the fp32 pipe's dV2 (1.34e-7): a stage adds 3 .. 256 terms per element and the worst of 1280 x 256 elements is
    taken, where a dW element adds thousands of rows whose rounding errors average out against a sum |a||b| that grows with
    the row count.  Worst stage in profiles/delta_chain_parity.log: fp32 pipe 2.85e-7 (torch 2.59e-7, dA2), bf16 pieces
    3.54e-7 (torch 2.42e-7, dA3); the bf16 pieces' dV2, a sum of three terms, 2.24e-7 (torch 1.34e-7)."""
    dims3, p_pad = DIMS[0], 1280
    C = sum(dims3)
    params = oracle.xavier_facenerf_params(5, oracle.facenerf_dims(dim_aud=dims3[0], dim_expr=dims3[1], dim_latent=dims3[2]))
    sd = {k: v.to(dev).contiguous() for k, v in params.items()}
    p = idn.ops.params_struct(sd, *dims3)
    w64 = {k: v.double() for k, v in sd.items()}
    wabs = {k: v.abs() for k, v in w64.items()}
    g = torch.Generator().manual_seed(17)
    seeds = (torch.randn((p_pad, 4), generator=g) * torch.exp2(torch.rand((p_pad, 1), generator=g) * -40)).to(dev)
    on = random_masks(p_pad, 0.5, g, dev)
    acts = slab_with(on)
    d_sigma = seeds[:, 3].contiguous()
    err = {}
    for pipe in (F32, X6):
        got, blocks = run_chain(idn, p, pipe, acts, seeds[:, :3], d_sigma, max_blocks=3)
        assert blocks == 3
        err[pipe], err["torch", pipe] = [], []
        for s in range(11):
            x = (seeds[:, :3] if s == 0 else got[s - 1])
            m = on[MASK_ID[s]].double()
            ref = m * stage_product(w64, C, s, x.double(), d_sigma.double())
            scale = stage_product(wabs, C, s, x.double().abs(), d_sigma.double().abs())
            assert float(scale.min()) > 0
            err[pipe].append(float(((got[s].double() - ref).abs() / scale).max()))
            t32 = (m.float() * stage_product(sd, C, s, x.contiguous(), d_sigma)).double()
            err["torch", pipe].append(float(((t32 - ref).abs() / scale).max()))
    print(f"\n  delta chain, {p_pad} rows, 3 workgroups: max |got - ref| / (|in| . |W|) per stage (torch's fp32 matmul of the same stage on the same inputs)")
    for s in range(11):
        print(f"    {NAMES[s]:4s} fp32 pipe {err[F32][s]:.2e} (torch {err['torch', F32][s]:.2e})   bf16 pieces {err[X6][s]:.2e} (torch {err['torch', X6][s]:.2e})")
    for s in range(11):
        for pipe in (F32, X6):
            bound = TORCH_MULT * err["torch", pipe][s] if (PIPE_NAME[pipe], NAMES[s]) in WIDENED else STAGE_BOUND
            assert err[pipe][s] < bound, (NAMES[s], PIPE_NAME[pipe], err[pipe][s], err["torch", pipe][s], bound)
        assert err[X6][s] < X6_OVER_F32[0] * err[F32][s] + X6_OVER_F32[1], (NAMES[s], err[F32][s], err[X6][s])


# ---------------------------------------------------------------------------------------------- T4
def test_the_aid_is_the_pass(idn, dev):
    """T4: on a real slab (facenerf_train_fwd, n = 4096) and a random g_out, with d_rgb and column 128 of dv0 seeded as
    head_seed_kernel seeds them, the fp64 column sums of the aid's eleven matrices are the bias gradients idealnerf_facenerf_bwd
    returns, to 3e-7 of the column's sum |delta| (the db bound of the dW tests) -- on the pipe this process's backward runs."""
    from idealnerf_amd import autograd, ops
    a, e, l = DIMS[0]
    dims = oracle.facenerf_dims(dim_aud=a, dim_expr=e, dim_latent=l)
    net = idn.FaceNeRF(dim_aud=a, dim_latent=l, dim_expr=e)
    net.load_state_dict(oracle.xavier_facenerf_params(5, dims))
    net = net.to(dev)
    g = torch.Generator().manual_seed(21)
    n = 4096
    x = (torch.rand((n, 90), generator=g) * 2 - 1).to(dev)
    cond = [(torch.randn(d, generator=g) * 0.3).to(dev) for d in (a, e, l)]
    g_out = torch.randn((n, 4), generator=g).to(dev)
    _, acts = ops.facenerf_train_fwd(net.packed_weights("bf16x6"), net.folded_bias(*cond), x, idn._lib.IDN_PREC_BF16X6)
    sd = dict(net.named_parameters())
    grads = {k: torch.full_like(sd[k], NAN) for k in autograd.PARAM_KEYS}
    ops.facenerf_bwd(net.kernel_params(), grads, *cond, acts, g_out)
    d_rgb = torch.zeros((n, 64), device=dev)
    d_rgb[:, :3] = g_out[:, :3]
    dv0 = torch.zeros((n, 256), device=dev)
    dv0[:, 128] = g_out[:, 3]
    pipe = F32 if os.environ.get("IDN_BACKWARD_PIPE") == "f32" else X6
    dv21, da, blocks = ops.delta_chain(net.kernel_params(), pipe, acts, d_rgb, dv0)
    assert blocks == n // 128
    pairs = [(da[i], f"pts_linears.{i}.bias") for i in range(8)]
    pairs += [(dv21[:, :128], "views_linears.2.bias"), (dv21[:, 128:], "views_linears.1.bias"), (dv0[:, :128], "views_linears.0.bias")]
    worst = 0.0
    for delta, key in pairs:
        d64 = delta.double()
        unit = d64.abs().sum(0)
        assert float(unit.max()) > 0, key
        worst = max(worst, float(((d64.sum(0) - grads[key].double()).abs() / unit.clamp_min(1e-300)).max()))
        assert bool(((d64.sum(0) - grads[key].double()).abs() <= 3e-7 * unit).all()), key
    print(f"\n  column sums of the aid's deltas vs the pass's bias gradients: worst |err| / sum |delta| = {worst:.2e}")
