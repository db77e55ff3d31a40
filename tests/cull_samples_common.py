"""What tests/test_cull_samples_cpu.py and tests/test_cull_samples_gpu.py share (not collected by pytest): the sample cull's
predicate (csrc/cull.hip: cull_sample_count_kernel) restated in numpy fp32, operation for operation, and its fp64 model with
the set of samples whose answer the fp32 rounding may decide."""
import numpy as np

import cull_common as cc

MAX_DIST = np.float32(0.0125)   # idealnerf_colour_gate_max_dist()
FACE_MARGIN = 1e-4              # cells: an fp64 cell coordinate this close to a cell face may fall on either side in fp32
DIST_MARGIN = 1e-6              # relative: an fp64 |dist| this close to the threshold may fall on either side in fp32
AMBIGUOUS_CAP = 0.01            # at most this share of the samples may be of either kind


def np_points(rays, z):
    """p = o + d z as point_of<kModeRays> forms it: fp32 product, then fp32 sum.  rays [n, 11], z [n, S] -> [n, S, 3] fp32."""
    rays, z = np.asarray(rays, dtype=np.float32), np.asarray(z, dtype=np.float32)
    prod = rays[:, None, 3:6] * z[:, :, None]
    return rays[:, None, 0:3] + prod


def np_dist(rays, z):
    """composite_ray's dist of every sample but the last: (z[s + 1] - z[s]) * sqrtf((dx dx + dy dy) + dz dz), fp32 [n, S - 1]."""
    rays, z = np.asarray(rays, dtype=np.float32), np.asarray(z, dtype=np.float32)
    d = rays[:, 3:6]
    dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return (z[:, 1:] - z[:, :-1]) * dn[:, None]


def np_occupied(occ, G, lo, cell, p):
    """cull_point_occupied: fp32 (p - lo) / cell, inside [0, G) on every axis or occupied (a NaN too), truncation, the bit."""
    lo, cell = np.asarray(lo, dtype=np.float32), np.float32(cell)
    with np.errstate(invalid="ignore"):
        t = (p - lo) / cell
        inside = ((t >= np.float32(0)) & (t < np.float32(G))).all(-1)
        idx = np.where(inside[..., None], t, np.float32(0)).astype(np.int32)
    return ~inside | occ[idx[..., 2], idx[..., 1], idx[..., 0]]


def np_sample_live(occ, G, lo, cell, rays, z):
    """live bool [n, S]: NOT (cell clear AND (last sample OR |dist| <= 0.0125)); a NaN anywhere makes the point live."""
    z = np.asarray(z, dtype=np.float32)
    occupied = np_occupied(occ, G, lo, cell, np_points(rays, z))
    close = np.ones(z.shape, dtype=bool)   # the last sample needs no spacing
    with np.errstate(invalid="ignore"):
        close[:, :-1] = np.abs(np_dist(rays, z)) <= MAX_DIST
    return ~(~occupied & close)


def model64(occ, G, lo, cell, rays, z):
    """The predicate in fp64 from the same fp32 inputs -> (live [n, S], ambiguous [n, S]): ambiguous where the fp64 cell
    coordinate lies within FACE_MARGIN of a cell face on any axis, or the fp64 |dist| within DIST_MARGIN (relative) of the
    threshold.  NaN inputs are not modelled (the callers keep them out)."""
    rays, z = np.asarray(rays, dtype=np.float32).astype(np.float64), np.asarray(z, dtype=np.float32).astype(np.float64)
    lo, cell = np.asarray(lo, dtype=np.float32).astype(np.float64), float(np.float32(cell))
    p = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    t = (p - lo) / cell
    inside = ((t >= 0) & (t < G)).all(-1)
    idx = np.clip(np.floor(t), 0, G - 1).astype(np.int64)
    occupied = ~inside | occ[idx[..., 2], idx[..., 1], idx[..., 0]]
    near_face = (np.abs(t - np.round(t)) <= FACE_MARGIN).any(-1)
    dn = np.sqrt((rays[:, 3:6] ** 2).sum(-1))
    dist = np.abs((z[:, 1:] - z[:, :-1]) * dn[:, None])
    thr = float(MAX_DIST)
    close = np.ones(z.shape, dtype=bool)
    close[:, :-1] = dist <= thr
    near_thr = np.zeros(z.shape, dtype=bool)
    near_thr[:, :-1] = np.abs(dist - thr) <= DIST_MARGIN * thr
    return ~(~occupied & close), near_face | near_thr


def np_ray_records(c2w, H, W, focal, near, far, row0=0, nrows=None):
    """[nrows W, 11] fp32 ray records from cull_common.rays64 (fp64 directions rounded to fp32: for host-only tests, where the
    exact bits of the device's records do not matter)."""
    o, d = cc.rays64(np.asarray(c2w), H, W, focal, row0, nrows)
    n = d.shape[0]
    rec = np.empty((n, 11), dtype=np.float32)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 7] = o, d, near, far
    rec[:, 8:11] = d / np.sqrt((d * d).sum(1, keepdims=True))
    return rec


def box_occupancy(G, lo, cell, centre=cc.CENTRE, half=cc.HALF, margin_cells=2):
    """occupied bool [G, G, G] ([z, y, x]): the cells within `margin_cells` cells of the box |x - centre| <= half -- what a
    grid of the analytic box scene looks like, without a network."""
    idx = np.stack(np.meshgrid(*[np.arange(G)] * 3, indexing="ij"), -1)[..., ::-1]
    c_lo, c_hi = np.asarray(lo) + idx * cell, np.asarray(lo) + (idx + 1) * cell
    b_lo, b_hi = np.asarray(centre) - half, np.asarray(centre) + half
    gap = np.maximum(np.maximum(b_lo - c_hi, c_lo - b_hi), 0.0)
    return gap.max(-1) <= margin_cells * cell
