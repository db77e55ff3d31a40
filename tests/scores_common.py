"""Shared by tests/test_scores_cpu.py and tests/test_scores_gpu.py (not collected by pytest): the definition of
idealnerf_frame_scores (include/idealnerf.h) restated in numpy, in fp64 -- once separably and once window by window."""
import numpy as np

WIN, SIGMA, C1, C2 = 11, 1.5, 1e-4, 9e-4
GROUPS = 5


def window_weights():
    """The 11 weights as the header defines them: computed and normalised in fp64, rounded to fp32 (returned as fp64)."""
    k = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return (g / g.sum()).astype(np.float32).astype(np.float64)


def unit_truth(truth_u8):
    """t = float(truth) / 255.0f: an fp32 division."""
    return (np.asarray(truth_u8).astype(np.float32) / np.float32(255.0)).astype(np.float32)


def _ssim_of_moments(mx, mt, xx, tt, xt):
    vx, vt, cov = xx - mx * mx, tt - mt * mt, xt - mx * mt
    return ((2.0 * mx * mt + C1) * (2.0 * cov + C2)) / ((mx * mx + mt * mt + C1) * (vx + vt + C2))


def ssim_map(pred, truth_u8):
    """SSIM index of every valid window and channel, separable evaluation -> fp64 [H - 10, W - 10, 3] (empty if H or W < 11)."""
    x, t = np.asarray(pred, np.float32).astype(np.float64), unit_truth(truth_u8).astype(np.float64)
    H, W = x.shape[:2]
    if H < WIN or W < WIN:
        return np.zeros((max(H - WIN + 1, 0), max(W - WIN + 1, 0), 3))
    w = window_weights()

    def blur(a):
        rows = sum(w[k] * a[:, k:k + W - WIN + 1] for k in range(WIN))
        return sum(w[k] * rows[k:k + H - WIN + 1] for k in range(WIN))

    return _ssim_of_moments(blur(x), blur(t), blur(x * x), blur(t * t), blur(x * t))


def ssim_window(pred, truth_u8, y, x0, ch):
    """The index of ONE window (top-left pixel (y, x0), channel ch), brute force: the 121 weights w[i] w[j] applied directly."""
    w = window_weights()
    w2 = np.outer(w, w)
    x = np.asarray(pred, np.float32)[y:y + WIN, x0:x0 + WIN, ch].astype(np.float64)
    t = unit_truth(truth_u8)[y:y + WIN, x0:x0 + WIN, ch].astype(np.float64)
    return float(_ssim_of_moments((w2 * x).sum(), (w2 * t).sum(), (w2 * x * x).sum(), (w2 * t * t).sum(), (w2 * x * t).sum()))


def ssim_map_brute(pred, truth_u8):
    H, W = np.asarray(pred).shape[:2]
    out = np.zeros((H - WIN + 1, W - WIN + 1, 3))
    for y in range(out.shape[0]):
        for x in range(out.shape[1]):
            for ch in range(3):
                out[y, x, ch] = ssim_window(pred, truth_u8, y, x, ch)
    return out


def reference_scores(pred, truth_u8, regions=None):
    """-> fp64 [5, 4]: rows whole frame, then bits 0..3 of the region byte; columns n_pixels, sse, n_windows, ssim_sum."""
    pred = np.asarray(pred, np.float32)
    H, W = pred.shape[:2]
    d = (pred - unit_truth(truth_u8)).astype(np.float32)
    se = (d * d).astype(np.float32).astype(np.float64).sum(-1)         # per pixel, over the channels
    ss = ssim_map(pred, truth_u8).sum(-1)                              # per window
    out = np.zeros((GROUPS, 4))
    for g in range(GROUPS):
        if g == 0:
            member = np.ones((H, W), bool)
        elif regions is None:
            continue
        else:
            member = ((np.asarray(regions) >> (g - 1)) & 1).astype(bool)
        centres = member[WIN // 2:H - WIN // 2, WIN // 2:W - WIN // 2] if ss.size else np.zeros((0, 0), bool)
        out[g] = [member.sum(), se[member].sum(), centres.sum(), ss[centres].sum() if ss.size else 0.0]
    return out


def check_against_reference(got, want, label=""):
    """The derived bounds: counts exact; sse within 1e-6 relative (at most 3 x 2^-24 per term, fp64 accumulation); mean SSIM
    within 1e-9 absolute (fp64 throughout: 1000 x what two fp64 evaluation orders differ by).  Every group is checked."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape == (GROUPS, 4)
    for g in range(GROUPS):
        assert got[g, 0] == want[g, 0] and got[g, 2] == want[g, 2], (label, g, got[g], want[g])
        assert abs(got[g, 1] - want[g, 1]) <= 1e-6 * abs(want[g, 1]), (label, g, got[g, 1], want[g, 1])
        if want[g, 2] > 0:
            err = abs(got[g, 3] - want[g, 3]) / (3.0 * want[g, 2])
            assert err <= 1e-9, (label, g, got[g, 3], want[g, 3], err)
        else:
            assert got[g, 3] == 0.0, (label, g, got[g, 3])
