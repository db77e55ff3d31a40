"""Every layer of the two activation-saving forwards (csrc/mlp_f32.hip: mlp_f32_kernel<*, true>, csrc/mlp_bf16x6.hip:
mlp_bf16x6_kernel<*, true>) and of the preparation kernels in front of them (csrc/prep.hip: fold_kernel, pack_f32_kernel,
pack_bf16x6_kernel), element by element on the GPU (run with ``-m gpu``).  Operands, reference and comparison:
tests/forward_layers_common.py; the CPU side: tests/test_forward_layers_cpu.py.

Every run (``run_forward``) calls the C entry on a slab filled with a sentinel NaN between guard words and asserts: the guards
intact; every float of the 2560 columns finite, padding rows included; the padding rows of every matrix equal to row n - 1
bit for bit; raw written in exactly n rows; the mask words of the rows below n equal to pack_masks of the slab's own a_l > 0.

E1   mode X, exact operands, both pipes x three conditioning layouts x n in {128, 185, 640}: x0 / dir bit for bit, a1..a8,
     v1..v3 and raw EQUAL to fp64 -- the fold, every bias by channel, every pack position, the skip concatenation, the transpose
     patch and the row stores at once;
E2   the same at 128 (2 CUs + 3) - 37 rows: every workgroup walks two tiles, three a third, the last tile is ragged;
E2b  the same for a 33 / 15 network (the zeros the pack writes beyond a narrow network's columns);
E3   weights of three non-zero bf16 pieces in layer 0;  E4  inputs of three non-zero bf16 pieces: a1 exact;
R1   rays mode against mode X on the rays-mode slab's own x0 / dir: the same bits;
G1   Xavier weights, random biases: the rounding of every layer on its own stored input, graded against fp64;
G2   the fold alone against fp64.

$IDN_FWD_LAYERS_RECORD names a JSON file the measured figures are merged into (profiles/forward_layers.json).  No measured
figure is an assertion: the bounds are the number formats' and the project's rule for one fp32-grade product."""
import json
import math
import os

import pytest
import torch

import forward_layers_common as fc
from test_delta_chain_gpu import guarded, guards_intact, mask_words, pack_masks

pytestmark = pytest.mark.gpu

PIPES = ("f32", "bf16x6")
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
    path = os.environ.get("IDN_FWD_LAYERS_RECORD")
    if not path:
        return
    old = json.load(open(path)) if os.path.exists(path) else {}
    old[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(old, open(path, "w"), indent=1, sort_keys=True)


def _code(idn, pipe):
    return {"f32": idn._lib.IDN_PREC_F32, "bf16x6": idn._lib.IDN_PREC_BF16X6}[pipe]


# ------------------------------------------------------------------------------------------------ the runner
def device_net(idn, dev, sd, dims3, cond, widths=FULL):
    """What the entries read: {pipe: weight stream}, the folded bias block, and the tensors they were made of."""
    sd = {k: v.to(dev).contiguous() for k, v in sd.items()}
    ps = idn.ops.params_struct(sd, *dims3, pts_ch=widths[0], views_ch=widths[1])
    cond = [c.to(dev).contiguous() for c in cond]
    folded = idn.ops.fold_conditioning(ps, *[c if c.numel() else None for c in cond], dev)
    packed = {pipe: idn.ops.pack_weights(ps, dev, _code(idn, pipe)) for pipe in PIPES}
    torch.cuda.synchronize()
    return dict(sd=sd, ps=ps, cond=cond, folded=folded, packed=packed, widths=widths)


def run_forward(idn, net, pipe, x=None, rays=None, z=None):
    """One call of idealnerf_facenerf_train_fwd_ch (x [n, pts_ch + views_ch]) or idealnerf_query_rays_train_fwd_ch (rays
    [n_rays, 11], z [n_rays, S]) on fresh guarded buffers, with the assertions of the module docstring.
    -> dict(n, p_pad, acts, views {name: [p_pad, width]}, raw [n, 4], masks int32 [11, p_pad / 32, 64, 4])."""
    lib = idn._lib.load()
    pc, vc = net["widths"]
    dev = net["folded"].device
    n = x.shape[0] if x is not None else z.numel()
    p_pad = fc.padded(n)
    floats = lib.idealnerf_train_acts_floats(n)
    assert floats == p_pad * (fc.ACT_COLS + fc.MASK_FLOATS)
    whole, acts = guarded((floats,), dev)
    whole_raw, raw = guarded((n, 4), dev)
    packed, folded, code = net["packed"][pipe], net["folded"], _code(idn, pipe)
    stream = torch.cuda.current_stream().cuda_stream
    if x is not None:
        assert x.is_contiguous() and x.shape[1] == pc + vc and x.dtype == torch.float32
        rc = lib.idealnerf_facenerf_train_fwd_ch(packed.data_ptr(), folded.data_ptr(), code, x.data_ptr(), pc, vc, n, raw.data_ptr(),
                                                 acts.data_ptr(), stream)
    else:
        assert rays.is_contiguous() and z.is_contiguous() and rays.shape == (z.shape[0], 11)
        rc = lib.idealnerf_query_rays_train_fwd_ch(packed.data_ptr(), folded.data_ptr(), code, rays.data_ptr(), z.data_ptr(), z.shape[0],
                                                   z.shape[1], pc, vc, raw.data_ptr(), acts.data_ptr(), stream)
    assert rc == 0, lib.idealnerf_last_error()
    torch.cuda.synchronize()
    ctx = f"{pipe} n {n}"
    assert guards_intact(whole), f"{ctx}: a write outside the slab"
    assert guards_intact(whole_raw), f"{ctx}: a write outside raw's n rows"
    assert bool(torch.isfinite(raw).all()), f"{ctx}: not every row of raw was written with a finite value"
    assert bool(torch.isfinite(acts[:fc.ACT_COLS * p_pad]).all()), f"{ctx}: not every float of the 2560 columns was written"
    views = fc.slab_views(acts, p_pad)
    if p_pad > n:
        for name, m in views.items():
            assert fc.same_bits(m[n:], m[n - 1:n].expand(p_pad - n, -1)), f"{ctx}: the padding rows of {name} do not repeat row {n - 1}"
    masks = mask_words(acts, p_pad)
    want = pack_masks([views[name] > 0 for name in fc.HIDDEN])
    point = torch.arange(p_pad // 32, device=dev)[:, None] * 32 + torch.arange(64, device=dev)[None, :] % 32     # [wave tile, lane]
    for i, name in enumerate(fc.HIDDEN):
        nd = views[name].shape[1] // 64          # (dwords 2 and 3 of the 128-wide layers are unspecified)
        same = (masks[i, :, :, :nd] == want[i, :, :, :nd]).all(-1)
        assert bool(same[point < n].all()), f"{ctx}: mask words of {name}: {int((~same[point < n]).sum())} (point, lane half) entries differ"
    return dict(n=n, p_pad=p_pad, acts=acts, views=views, raw=raw, masks=masks)


def outputs_of(run):
    """The thirteen outputs of a run in OUT_NAMES' order, rows below n."""
    n, v, raw = run["n"], run["views"], run["raw"]
    return [v[f"a{i}"][:n] for i in range(1, 9)] + [raw[:, 3:4]] + [v[k][:n] for k in ("v1", "v2", "v3")] + [raw[:, :3]]


def assert_inputs_stored(run, x, widths, ctx):
    """x0[:, :pts_ch] / dir[:, :views_ch] are x bit for bit, the columns behind them +0.0."""
    n, (pc, vc) = run["n"], widths
    x0, dr = run["views"]["x0"][:n], run["views"]["dir"][:n]
    assert fc.same_bits(x0[:, :pc], x[:, :pc]), f"{ctx}: x0 is not x[:, :{pc}]"
    assert fc.same_bits(dr[:, :vc], x[:, pc:]), f"{ctx}: dir is not x[:, {pc}:]"
    assert not bool(x0[:, pc:].contiguous().view(torch.int32).any()), f"{ctx}: columns {pc}..63 of x0 must be +0.0"
    assert not bool(dr[:, vc:].contiguous().view(torch.int32).any()), f"{ctx}: columns {vc}..63 of dir must be +0.0"


# ------------------------------------------------------------------------------------------------ E1, E2, E2b
_exact = {}


def exact_on_device(idn, dev, dims3, n, widths=FULL):
    """One exact case (operands, fp64 reference, device buffers): built once, shared by both pipes, never written again."""
    key = (dims3, n, widths)
    if key not in _exact:
        c = fc.exact_case(dims3, n, widths, device=dev)
        c["net"] = device_net(idn, dev, c["sd"], dims3, c["cond"], widths)
        _exact[key] = c
    return _exact[key]


def check_exact(idn, c, pipe, ctx, widths=FULL):
    run = run_forward(idn, c["net"], pipe, x=c["x"])
    assert_inputs_stored(run, c["x"], widths, ctx)
    fc.assert_same(outputs_of(run), c["ref"], ctx)
    return run


@pytest.mark.parametrize("n", fc.E1_ROWS)
@pytest.mark.parametrize("dims3", fc.DIMS, ids=fc.DIMS_ID)
@pytest.mark.parametrize("pipe", PIPES)
def test_exact_layers(idn, dev, pipe, dims3, n):
    """E1: one tile, a ragged second tile, five tiles."""
    check_exact(idn, exact_on_device(idn, dev, dims3, n), pipe, f"{pipe} {dims3} n {n}")


def test_exact_layers_beyond_the_grid_of_a_pass(idn, dev):
    """E2: head layout, n = 128 (2 CUs + 3) - 37, both pipes on one reference (fp64 on the device): with one workgroup per CU
    every workgroup walks at least two tiles with saving on -- the weight ring's slot phase, the prefetch hand-over and the
    per-wave patch carry from tile to tile -- three walk a third, and the last tile is ragged."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n = fc.multi_tile_rows(cus)
    c = fc.exact_case(fc.DIMS[0], n, device=dev)            # (its assertions again, for this device's CU count)
    c["net"] = device_net(idn, dev, c["sd"], fc.DIMS[0], c["cond"])
    for pipe in PIPES:
        run = check_exact(idn, c, pipe, f"{pipe} n {n} ({cus} CUs)")
        assert run["p_pad"] == 128 * (2 * cus + 3)
        del run
    _record("E2", dict(cus=cus, rows=n, tiles=2 * cus + 3, equal=True))
    del c
    torch.cuda.empty_cache()


@pytest.mark.parametrize("pipe", PIPES)
def test_exact_layers_of_a_narrow_network(idn, dev, pipe):
    """E2b: a 33 / 15 network, head layout, n = 185: rows of 48 columns in, the pack's zeros beyond them."""
    c = exact_on_device(idn, dev, fc.DIMS[0], 185, fc.NARROW)
    check_exact(idn, c, pipe, f"{pipe} 33/15 n 185", fc.NARROW)


# ------------------------------------------------------------------------------------------------ E3, E4
_pieces = {}


def piece_case(idn, dev, which):
    if which not in _pieces:
        c = {"weights": fc.weight_piece_case, "inputs": fc.input_piece_case}[which](185, device=dev)
        c["net"] = device_net(idn, dev, c["sd"], fc.DIMS[0], c["cond"])
        _pieces[which] = c
    return _pieces[which]


@pytest.mark.parametrize("pipe", PIPES)
def test_three_piece_weights(idn, dev, pipe):
    """E3: pts_linears.0 = +-(2 + 2^-8 + 2^-16) at 8 columns per row, |x| <= 7, half-integer biases: every product and sum is
    a multiple of 2^-16 below 2^8.  In the six-piece arithmetic only a1 w1, a1 w2 and a1 w3 are non-zero and all three are
    kept; a wrong second or third weight piece in the pack shows in a1.  a1 exact; everything else finite (run_forward)."""
    c = piece_case(idn, dev, "weights")
    run = run_forward(idn, c["net"], pipe, x=c["x"])
    assert_inputs_stored(run, c["x"], FULL, pipe)
    fc.assert_same(outputs_of(run)[:1], c["ref"][:1], f"{pipe} three-piece weights", names=["a1"])


@pytest.mark.parametrize("pipe", PIPES)
def test_three_piece_inputs(idn, dev, pipe):
    """E4: the exact head net on rows of 20-bit integers with three non-zero bf16 pieces each -- the pieces the six-piece
    kernel makes of its inputs outside the k-step pipeline.  x0 / dir bit for bit, a1 exact (8 terms below 2^20 plus the
    bias); everything else finite (run_forward)."""
    c = piece_case(idn, dev, "inputs")
    run = run_forward(idn, c["net"], pipe, x=c["x"])
    assert_inputs_stored(run, c["x"], FULL, pipe)
    fc.assert_same(outputs_of(run)[:1], c["ref"][:1], f"{pipe} three-piece inputs", names=["a1"])


# ------------------------------------------------------------------------------------------------ graded operands
@pytest.fixture(scope="module")
def graded(idn, dev):
    """Head layout: Xavier weights, biases uniform(-0.1, 0.1) per channel, conditioning 0.3 N(0, 1)."""
    dims3 = fc.DIMS[0]
    net = device_net(idn, dev, fc.graded_net(dims3, 5), dims3, fc.graded_cond(dims3, 6))
    net["dims"] = fc.oracle_dims(dims3)
    net["w64"] = {k: v.double() for k, v in net["sd"].items()}
    return net


def some_rays(n_rays, S, seed, dev):
    """(rays [n_rays, 11] = (o, d, near, far, unit view direction), z [n_rays, S] increasing in [near, far])."""
    g = torch.Generator().manual_seed(seed)
    o = torch.rand((n_rays, 3), generator=g) * 0.4 - 0.2
    d = torch.randn((n_rays, 3), generator=g)
    view = d / d.norm(dim=1, keepdim=True)
    near, far = 0.3, 1.1
    rays = torch.cat([o, d, torch.full((n_rays, 1), near), torch.full((n_rays, 1), far), view], 1)
    z = near + (far - near) * torch.sort(torch.rand((n_rays, S), generator=g), 1)[0]
    return rays.contiguous().to(dev), z.contiguous().to(dev)


# ------------------------------------------------------------------------------------------------ R1
@pytest.mark.parametrize("n_rays,S", [(37, 5), (3, 129)])
@pytest.mark.parametrize("pipe", PIPES)
def test_rays_mode_is_mode_x_on_its_own_encoding(idn, dev, graded, pipe, n_rays, S):
    """R1: the rays-mode slab's x0[:, :63] | dir[:, :27] fed to the mode-X entry: a1..v3, the mask words and raw of the two
    runs are the same bits -- the arithmetic and the operand order are the same, only the input stage and the prefetch hook
    differ."""
    rays, z = some_rays(n_rays, S, 100 * n_rays + S, dev)
    r = run_forward(idn, graded, pipe, rays=rays, z=z)
    n = r["n"]
    x = torch.cat([r["views"]["x0"][:n, :63], r["views"]["dir"][:n, :27]], 1).contiguous()
    m = run_forward(idn, graded, pipe, x=x)
    for name in fc.ACT_NAMES:
        assert fc.same_bits(r["views"][name], m["views"][name]), f"{pipe} {n_rays} x {S}: {name} differs between the modes"
    assert fc.same_bits(r["raw"], m["raw"]), f"{pipe} {n_rays} x {S}: raw differs between the modes"
    point = torch.arange(r["p_pad"] // 32, device=dev)[:, None] * 32 + torch.arange(64, device=dev)[None, :] % 32
    for i, name in enumerate(fc.HIDDEN):
        nd = r["views"][name].shape[1] // 64
        same = (r["masks"][i, :, :, :nd] == m["masks"][i, :, :, :nd]).all(-1)
        assert bool(same[point < n].all()), f"{pipe} {n_rays} x {S}: mask words of {name} differ between the modes"
    _record(f"R1/{pipe}/{n_rays}x{S}", dict(equal=True))


# ------------------------------------------------------------------------------------------------ G1
# (pipe, mode, output) a correct kernel was measured above the per-layer rule at: (its figure, torch's); held to chain_ceiling
# instead.  None.
WIDENED = {}
# (mode, output) whose bf16-piece figure was measured above 4 x the fp32 pipe's + 3e-8 with both kernels correct: (bf16 pieces,
# fp32 pipe), profiles/forward_layers.json.  sigma: the fp32 kernel takes it on the vector unit as EIGHT chains of 32 fmaf per
# point (four per lane half) added as a tree, the six-piece kernel as channel 128 of views_linears.0, one MFMA chain over all
# 288 input columns like every hidden unit -- its 2.02e-7 is a hidden layer's figure and inside its own per-layer bound
# (3.65e-7); the fp32 pipe's 3.74e-8 is the short chains', a third of torch's 9.8e-8.  The pair is held to the ceiling of the
# longer chain, chain_ceiling(256), instead; the per-layer rule holds for both as for every other layer.
PAIR_WIDENED = {("x", "sigma"): (2.02e-07, 3.74e-08)}
IN_WIDTH = {**{f"a{i}": 256 for i in range(2, 9)}, "a1": 63, "a6": 63 + 172 + 256, "sigma": 256, "v1": 256 + 27 + 76, "v2": 128,
            "v3": 128, "rgb": 128}


def grade(net, run, folded):
    """{pipe figure, torch figure} per output: max |got - ref| / (sum |w||in| + |b|) of the run's thirteen outputs against
    fp64 ref_layers on the run's OWN stored matrices (layer 0: on x0 with the folded bias the kernel read), and the same for
    torch's fp32 addmm of the same layers on the same inputs."""
    n, v = run["n"], run["views"]
    given = {name: v[name][:n] for name in fc.HIDDEN}
    x_pts, x_dir = v["x0"][:n, :63], v["dir"][:n, :27]
    args64 = (net["w64"], net["dims"], x_pts.double(), x_dir.double(), [c.double() for c in net["cond"]])
    kw64 = dict(given={k: t.double() for k, t in given.items()}, folded0=folded[:256].double())
    ref, unit = fc.ref_layers(*args64, **kw64), fc.layer_units(*args64, **kw64)
    t32 = fc.ref_layers(net["sd"], net["dims"], x_pts.contiguous(), x_dir.contiguous(), net["cond"], given=given, folded0=folded[:256])
    out = {}
    for name, g, t, r, u in zip(fc.OUT_NAMES, outputs_of(run), t32, ref, unit):
        assert float(u.min()) > 0, name
        out[name] = (float(((g.double() - r).abs() / u).max()), float(((t.double() - r).abs() / u).max()))
    return out


def test_rounding_grade_layer_by_layer(idn, dev, graded):
    """G1: 1243 rows in mode X (x uniform in [-1, 1]) and 37 rays x 33 samples in rays mode (1221 points, the same ten tiles),
    both pipes.  The forward ReLU is 1-Lipschitz, so the post-ReLU matrices are compared as they are.

    The rule (delta-chain T3, the dW tests): every layer below max(2e-7, 4 x torch's figure); the bf16 pieces below 4 x the
    fp32 pipe + 3e-8.  A (pipe, mode, layer) of WIDENED is held to the ceiling of its chain, (K + 3) 2^-24 with K the layer's
    input width, instead of the first; a (mode, layer) of PAIR_WIDENED instead of the second.

    Measured (profiles/forward_layers.json): every (pipe, mode, layer) meets the per-layer rule -- hidden layers 1.8e-7 .. 4.2e-7
    on the fp32 pipe and 2.0e-7 .. 3.9e-7 on the bf16 pieces, next to torch's 2.0e-7 .. 4.8e-7; sigma 3.7e-8 / 2.0e-7 (mode X)
    and 4.8e-8 / 1.4e-7 (rays), rgb 9.7e-8 / 1.7e-7 and 8.6e-8 / 2.1e-7.  One pair misses the second rule: sigma in mode X,
    bf16 pieces 2.02e-7 against 4 x 3.74e-8 + 3e-8 = 1.80e-7, for the reason PAIR_WIDENED states; it is held to
    (256 + 3) 2^-24 = 1.54e-5."""
    g = torch.Generator().manual_seed(23)
    n = 1280 - 37
    x = (torch.rand((n, 90), generator=g) * 2 - 1).to(dev).contiguous()
    rays, z = some_rays(37, 33, 9, dev)
    figures = {}
    for pipe in PIPES:
        figures[pipe, "x"] = grade(graded, run_forward(idn, graded, pipe, x=x), graded["folded"])
        figures[pipe, "rays"] = grade(graded, run_forward(idn, graded, pipe, rays=rays, z=z), graded["folded"])
    record, failures = {}, []
    for mode in ("x", "rays"):
        print(f"\n  mode {mode}: max |got - ref| / (sum |w||in| + |b|) per layer (torch's fp32 addmm of the same layer on the same inputs)")
        for name in fc.OUT_NAMES:
            line = f"    {name:5s}"
            for pipe in PIPES:
                fig, tor = figures[pipe, mode][name]
                widened = (pipe, mode, name) in WIDENED
                bound = fc.chain_ceiling(IN_WIDTH[name]) if widened else max(fc.STAGE_BOUND, fc.TORCH_MULT * tor)
                record[f"{pipe}/{mode}/{name}"] = dict(kernel=fig, torch=tor, bound=bound, rule="chain ceiling" if widened else "max(2e-7, 4 x torch)")
                line += f"  {pipe} {fig:.2e} (torch {tor:.2e}, bound {bound:.2e})"
                if not fig < bound:
                    failures.append((pipe, mode, name, fig, tor, bound))
            f32, x6 = figures["f32", mode][name][0], figures["bf16x6", mode][name][0]
            pair_widened = (mode, name) in PAIR_WIDENED
            pair_bound = fc.chain_ceiling(IN_WIDTH[name]) if pair_widened else fc.X6_OVER_F32[0] * f32 + fc.X6_OVER_F32[1]
            record[f"pair/{mode}/{name}"] = dict(bf16x6=x6, f32=f32, bound=pair_bound, rule="chain ceiling" if pair_widened else "4 x f32 + 3e-8")
            if not x6 < pair_bound:
                failures.append(("bf16x6 over f32", mode, name, x6, f32, pair_bound))
            print(line)
    _record("G1", record)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ G2
@pytest.mark.parametrize("dims3", fc.DIMS, ids=fc.DIMS_ID)
def test_fold_against_fp64(idn, dev, dims3):
    """G2: all 3136 floats of fold_conditioning.

    The 2496 biases, in the unit |b| + sum |w||cond|, below (ceil(C / 64) + 9) 2^-24.  The count, from fold_kernel's longest
    rounding path: a lane's chain of ceil(C / 64) fmaf steps (one rounding each), the six shuffle adds of the wave reduction,
    the final b + dot and the division expr / 3 that rounds an operand -- ceil(C / 64) + 8 roundings, each at most 2^-24 of a
    quantity the unit bounds; the ninth covers the second-order terms.  A channel without conditioning columns is b + 0: exact.
    The 256 + 384 copied weight rows bit for bit; the slots no layer uses (channels 129..159 of views_linears.0's block, 3..31
    of rgb_linear's) are the kernel's b + dot with both left at 0.0f: +0.0, bit for bit."""
    C = sum(dims3)
    dims = fc.oracle_dims(dims3)
    net = device_net(idn, dev, fc.graded_net(dims3, 11 + fc.DIMS.index(dims3)), dims3, fc.graded_cond(dims3, 12))
    got = net["folded"]
    assert got.shape == (fc.FOLD_FLOATS,)
    ref, unit = fc.fold_reference({k: v.double() for k, v in net["sd"].items()}, dims, [c.double() for c in net["cond"]])
    used = torch.zeros(fc.FOLD_BIASES, dtype=torch.bool, device=dev)
    for name in fc.OUT_NAMES:
        used[fc.FOLD_OFF[name]:fc.FOLD_OFF[name] + net["sd"][fc.KEY[name] + ".bias"].numel()] = True
    assert int(used.sum()) == 8 * 256 + 129 + 128 + 128 + 3 and int((~used).sum()) == 31 + 29
    bound = (math.ceil(C / 64) + 9) * 2.0 ** -24
    share = (got[:fc.FOLD_BIASES].double() - ref[:fc.FOLD_BIASES]).abs()[used] / unit[used]
    worst = float(share.max())
    at = int(used.nonzero()[int(share.argmax())])
    print(f"\n  fold {dims3}: worst |got - ref| / (|b| + sum |w||cond|) = {worst:.2e} at float {at} (bound {bound:.2e})")
    _record(f"G2/{fc.DIMS_ID[fc.DIMS.index(dims3)]}", dict(worst=worst, at=at, bound=bound))
    assert worst < bound, (worst, at, bound)
    plain = used.clone()                         # the channels without conditioning columns: the bias itself
    plain[0:256] = plain[5 * 256:6 * 256] = False
    if dims3[1]:
        plain[2048:2048 + 128] = False
    assert fc.same_bits(got[:fc.FOLD_BIASES][plain], ref[:fc.FOLD_BIASES][plain].float()), "a bias without conditioning columns is not the bias"
    assert not bool(got[:fc.FOLD_BIASES][~used].view(torch.int32).any()), "an unused slot is not +0.0"
    assert fc.same_bits(got[fc.FOLD_ALPHA:fc.FOLD_RGB], net["sd"]["alpha_linear.weight"].reshape(-1)), "alpha_linear's row"
    assert fc.same_bits(got[fc.FOLD_RGB:], net["sd"]["rgb_linear.weight"].reshape(-1)), "rgb_linear's rows"
