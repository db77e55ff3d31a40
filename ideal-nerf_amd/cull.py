"""Empty-space skipping for clip renders: a per-clip occupancy grid and the culled frame route.

A ray all of whose coarse and fine samples have ``sigma_raw <= 0`` renders to its background pixel exactly: every
``alpha = 1 - expf(-1e-6 dist)`` is ``0.0f`` while the sample spacing stays at or below ``idealnerf_colour_gate_max_dist()``,
the last sample's alpha is 1, its colour is the background pixel and the transmittance in front of it is exactly 1.  A
``CullGrid`` records, for one coarse / fine pair and one clip, where either network's sigma can be positive under any of the
clip's conditioning vectors; ``render_culled`` renders only the pixels whose rays come near such a place, with the unchanged
kernels on the ray records the frame mode would derive, and writes the other pixels down.  Opt-in (``Network.set_cull``, the
``cull=`` argument of the clip flows); with no grid installed nothing here is imported by a render.

The grid is conservative for the scene when sigma_raw <= 0 wherever no marked lattice corner is within one cell: sigma is
sampled at the (G+1)^3 corners only, so a density feature narrower than a cell between corners is the one thing it can miss.
``dilate >= 1`` and a march step of at most half a cell then make a culled ray miss every cell with a marked corner.
"""
import time

import numpy as np
import torch

from . import ops
from ._lib import IdealNerfError

RAW_CHUNK_BYTES = 64 << 20   # no more than this much network output `raw` is alive at once while a grid is built
DEFAULTS = dict(G=128, dilate=1, sigma_min=0.0, frame_stride=1, samples=False)


def _camera(c2w):
    m = np.asarray(torch.as_tensor(c2w).detach().cpu().to(torch.float32).numpy(), dtype=np.float64)
    if m.ndim != 2 or m.shape not in ((3, 4), (4, 4)):
        raise IdealNerfError(f"c2w must be [3, 4] or [4, 4], got {list(m.shape)}")
    return m[:3, :4]


def _principal(H, W, cx, cy):
    return (W * 0.5 if cx is None or cx < 0 else float(cx)), (H * 0.5 if cy is None or cy < 0 else float(cy))


def corner_dirs(c2w, H, W, focal, cx=None, cy=None, row0=0, nrows=None):
    """The ray directions of the four corner pixels of rows [row0, row0 + nrows), fp64 [4, 3], from the fp32 values the
    kernels receive.  |d| is a convex function of the pixel, and o + d z is affine in it: the band's extremes are here."""
    m = _camera(c2w)
    nrows = H - row0 if nrows is None else nrows
    cx, cy = _principal(H, W, cx, cy)
    f = float(np.float32(focal))
    out = []
    for row in (row0, row0 + max(nrows, 1) - 1):
        for col in (0, W - 1):
            d_cam = np.array([(col - cx) / f, -(row - cy) / f, -1.0])
            out.append(m[:, :3] @ d_cam)
    return np.stack(out)


def frustum_corners(c2w, H, W, focal, near, far, cx=None, cy=None, row0=0, nrows=None):
    """The 8 points o + d z of the band's corner pixels at z = near and z = far, fp64 [8, 3]: every sample point of the
    band lies in their convex hull."""
    d = corner_dirs(c2w, H, W, focal, cx, cy, row0, nrows)
    o = _camera(c2w)[:, 3]
    return np.concatenate([o + d * float(np.float32(near)), o + d * float(np.float32(far))])


def frustum_box(cameras, H, W, focal, near, far, G, cx=None, cy=None):
    """The grid's box: the fp64 bounding box of the frustum corners of every camera, padded by one cell on every side, as
    G^3 cubic cells.  -> (lo fp64 [3], cell): the box is lo + [0, G cell]^3."""
    pts = np.concatenate([frustum_corners(c, H, W, focal, near, far, cx, cy) for c in cameras])
    lo, hi = pts.min(0), pts.max(0)
    cell = float((hi - lo).max()) / (G - 2)
    if not cell > 0.0:
        raise IdealNerfError("the cameras' frustum is a point: near == far?")
    return (lo + hi) * 0.5 - 0.5 * G * cell, cell


def march_steps(cell, d_max, near, far):
    """(dz, K) of the classification march z_k = near + k dz (k < K), z_K = far: the fewest steps with dz d_max <= cell / 2,
    dz as the fp32 value the kernel receives."""
    near, far = float(np.float32(near)), float(np.float32(far))
    if not far > near:
        raise IdealNerfError(f"the march needs far > near, got {near} .. {far}")
    K = max(1, int(np.ceil((far - near) * d_max * (1.0 + 1e-6) / (0.5 * cell))))
    dz = float(np.float32((far - near) / K))
    while dz * d_max > 0.5 * cell:   # the fp32 rounding of dz went up across the bound
        K += 1
        dz = float(np.float32((far - near) / K))
    return dz, K


_POPCOUNT = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64)


class CullGrid:
    """The occupancy of one coarse / fine pair over one clip.  bits: int32 [G^3 / 32] on the device, 32 cells per word along
    x; corners: uint8 [(G+1)^3], the marked lattice points (before dilation); lo (fp32 values) / cell: the box.
    `classify_calls` counts the classifications that ran (a frame whose camera and band are those of the call before is
    answered from the cache: the torso pair's camera never changes within a clip, so it is classified once).
    `samples`: the live rays' network passes skip the samples in clear cells too (ops.render_rays_sparse_fwd), which counts
    the points it saw and the points it evaluated here."""

    def __init__(self, bits, corners, G, lo, cell, dilate, sigma_min, frame_stride=1, stats=None, samples=False):
        self.bits, self.corners, self.G = bits, corners, int(G)
        self.lo = tuple(float(np.float32(v)) for v in lo)
        self.cell = float(np.float32(cell))
        self.dilate, self.sigma_min, self.frame_stride = int(dilate), float(sigma_min), int(frame_stride)
        self.stats = dict(stats or {})
        self.classify_calls = 0
        self.live_pixels = self.seen_pixels = 0
        self.samples = bool(samples)
        self.points_seen = self.points_evaluated = 0
        self._cache = None

    @property
    def occupied_share(self):
        counts = _POPCOUNT.to(self.bits.device)[self.bits.view(torch.uint8).to(torch.int64)]
        return float(counts.sum().item()) / self.G ** 3

    @property
    def live_share(self):
        return self.live_pixels / self.seen_pixels if self.seen_pixels else float("nan")

    @property
    def evaluated_share(self):
        """Of the live rays' samples, the share a network evaluated (1 - the sample cull's saving)."""
        return self.points_evaluated / self.points_seen if self.points_seen else float("nan")

    def check_contains(self, frame):
        """IdealNerfError unless the box holds the frustum of the frame's band (points outside it were never evaluated)."""
        pts = frustum_corners(torch.tensor(list(frame.c2w)).reshape(3, 4), frame.H, frame.W, frame.focal, frame.near_, frame.far_,
                              frame.cx, frame.cy, frame.row0, frame.nrows)
        lo = np.asarray(self.lo, dtype=np.float64)
        if (pts < lo).any() or (pts > lo + self.G * self.cell).any():
            raise IdealNerfError("the cull grid's box does not contain this frame's frustum: the grid was built for other cameras, "
                                 "another frame size, focal length or near / far (build it from the cameras the clip uses)")

    def steps(self, frame):
        d = corner_dirs(torch.tensor(list(frame.c2w)).reshape(3, 4), frame.H, frame.W, frame.focal, frame.cx, frame.cy, frame.row0,
                        frame.nrows)
        return march_steps(self.cell, float(np.sqrt((d * d).sum(1)).max()), frame.near_, frame.far_)

    def live(self, frame):
        """(sel int64 [nrows W] on the device, n_live int): sel[:n_live] = the band's live pixels, ascending.  One
        classification and ONE host read (n_live) -- none when the frame is the one of the call before."""
        key = (bytes(frame.c2w), frame.H, frame.W, frame.focal, frame.cx, frame.cy, frame.near_, frame.far_, frame.row0, frame.nrows)
        if self._cache is None or self._cache[0] != key:
            self.check_contains(frame)
            dz, K = self.steps(frame)
            sel, n_dev = ops.cull_classify(self.bits, self.G, self.lo, self.cell, frame, dz, K)
            self._cache = (key, sel, int(n_dev.item()))
            self.classify_calls += 1
        _, sel, n = self._cache
        self.live_pixels += n
        self.seen_pixels += frame.nrows * frame.W
        return sel, n


def build_grid(nets, conds, cameras, H, W, focal, near, far, *, G=128, dilate=1, sigma_min=0.0, frame_stride=1, cx=None, cy=None,
               samples=False):
    """The CullGrid of the networks `nets` (the coarse and the fine network of a pair) for a clip.
      conds    one (aud_para, expr, latent_code) per frame of the clip: the tensors the render loop passes to the pair
      cameras  every camera the pair is rendered from ([3, 4] / [4, 4] each; the torso pair: its one torso_pose)
    Every `frame_stride`-th frame's conditioning is folded as `_render` folds it, both networks are evaluated on the
    (G+1)^3 corner lattice of the box in their own arithmetic, and the corners with sigma_raw > sigma_min are marked; marks
    are ORed over frames and networks.  frame_stride > 1 gives up the guarantee: density that only the skipped frames'
    conditioning produces is not seen.  `samples`: the grid also culls the live rays' samples (CullGrid.samples).  At most RAW_CHUNK_BYTES (64 MiB) of network output is alive at once."""
    ops._cull_G(G)
    if isinstance(frame_stride, bool) or not isinstance(frame_stride, int) or frame_stride < 1:
        raise IdealNerfError(f"frame_stride = {frame_stride!r}: a whole number >= 1")
    if not isinstance(samples, bool):
        raise IdealNerfError(f"samples = {samples!r}: True or False")
    if not conds or not len(cameras):
        raise IdealNerfError("a cull grid needs the clip's conditioning (one triple per frame) and its cameras")
    t0 = time.perf_counter()
    lo64, cell64 = frustum_box(cameras, H, W, focal, near, far, G, cx, cy)
    lo, cell = [float(np.float32(v)) for v in lo64], float(np.float32(cell64))
    dev = nets[0].alpha_linear.weight.device
    C1 = G + 1
    axis = lambda a: torch.tensor(lo[a], dtype=torch.float32, device=dev) + \
        torch.arange(C1, dtype=torch.float32, device=dev) * torch.tensor(cell, dtype=torch.float32, device=dev)
    xs, ys, zs = axis(0), axis(1), axis(2)
    # lattice rows: one (iz, iy) line of G + 1 points along x each; corner index ((iz C1) + iy) C1 + ix
    pts = torch.stack([xs.view(1, 1, C1).expand(C1, C1, C1), ys.view(1, C1, 1).expand(C1, C1, C1),
                       zs.view(C1, 1, 1).expand(C1, C1, C1)], dim=-1).reshape(C1 * C1, C1, 3).contiguous()
    dirs = torch.zeros((C1 * C1, 3), dtype=torch.float32, device=dev)
    dirs[:, 2] = -1.0   # any unit direction: sigma does not depend on it
    corners = torch.zeros(C1 ** 3, dtype=torch.uint8, device=dev)
    rows = max(1, RAW_CHUNK_BYTES // (16 * C1))
    events = []
    with torch.no_grad():
        for aud, expr, latent in conds[::frame_stride]:
            for net in nets:
                folded, packed = net.folded_bias(aud, expr, latent), net.packed_weights()
                for r0 in range(0, C1 * C1, rows):
                    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    ev[0].record(torch.cuda.current_stream(dev))
                    raw = ops.query_points_fwd(packed, folded, pts[r0:r0 + rows], dirs[r0:r0 + rows], net.prec_code)
                    ev[1].record(torch.cuda.current_stream(dev))
                    events.append(ev)
                    ops.cull_mark(raw.view(-1, 4), sigma_min, corners[r0 * C1:(r0 + rows) * C1])
                    del raw
        bits = ops.cull_cells(corners, G, int(dilate))
    torch.cuda.synchronize(dev)
    stats = dict(build_seconds=time.perf_counter() - t0, network_seconds=sum(a.elapsed_time(b) for a, b in events) * 1e-3,
                 frames_marked=len(conds[::frame_stride]))
    return CullGrid(bits, corners, G, lo, cell, dilate, sigma_min, frame_stride, stats, samples)


def options(cull):
    """The flows' ``cull=`` argument -> build_grid's keywords (None stays None)."""
    if cull is None:
        return None
    unknown = set(cull) - set(DEFAULTS)
    if unknown:
        raise IdealNerfError(f"cull= takes {sorted(DEFAULTS)}, got {sorted(unknown)}")
    return {**DEFAULTS, **{k: v for k, v in cull.items() if v is not None}}


def summary(grids):
    """The ``cull`` entry of a clip's result: build time, occupied share and live share per pair; with the sample cull on, the
    share of the live rays' samples that a network evaluated."""
    grids = {k: g for k, g in grids.items() if g is not None}
    extra = {}
    if any(g.samples for g in grids.values()):
        extra["evaluated_share"] = {k: g.evaluated_share for k, g in grids.items() if g.samples}
    return dict(**extra, build_seconds=sum(g.stats.get("build_seconds", 0.0) for g in grids.values()),
                network_seconds=sum(g.stats.get("network_seconds", 0.0) for g in grids.values()),
                occupied_share={k: g.occupied_share for k, g in grids.items()},
                live_share={k: g.live_share for k, g in grids.items()})


# what a culled pixel holds, per output of ops.render_rays_fwd: (channels, fill)
def _fills(far):
    disp = float(np.float32(1.0) / np.maximum(np.float32(1e-10), np.float32(far) / np.float32(1.0)))   # raw2outputs' 1 / max(1e-10, depth / acc)
    return dict(rgb_map=(3, "bc"), rgb0=(3, "bc"), acc_map=(1, 1.0), acc0=(1, 1.0), last_weight=(1, 1.0), last_weight0=(1, 1.0),
                rgb_fg=(3, 0.0), rgb_fg0=(3, 0.0), disp_map=(1, disp), disp0=(1, disp), z_std=(1, 0.0))


def refuse(grid_name, taps, retraw, white_bkgd, raw_noise_std, lindisp):
    """The options a culled render does not take, named before any C call."""
    bad = [n for n, on in (("taps", taps), ("retraw", retraw), ("white_bkgd", white_bkgd), ("raw_noise_std > 0", raw_noise_std > 0.),
                           ("lindisp", lindisp), ("a fused arrangement (IDN_FUSED_MARCH)", ops.FUSED_MARCH_DEFAULT != 0)) if on]
    if bad:
        raise IdealNerfError(f"{', '.join(bad)} with a cull grid installed for the {grid_name} pair: a culled frame has no per-sample "
                             "taps, and its background argument holds for the plain kernel sequence without density noise or a "
                             "white background; remove the grid (set_cull) for this render")


def render_culled(grid, frame, bc_rgb, render_live, names):
    """The culled route of one frame: classify, read n_live, gather, `render_live(rays, bc_live, n_live)` (the unchanged
    ops.render_rays_fwd on the live records; not called when n_live == 0), fill + scatter.  names: the outputs of
    render_rays_fwd the caller wants back, dense [nrows W(, 3)] fp32."""
    sel, n_live = grid.live(frame)
    fills = _fills(frame.far_)
    out = {}
    if n_live:
        rays, bc_live = ops.cull_gather(sel[:n_live], frame, bc_rgb)
        out = render_live(rays, bc_live, n_live)
    return ops.cull_scatter(sel, n_live, bc_rgb, {k: (out.get(k), *fills[k]) for k in names})
