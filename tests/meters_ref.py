"""numpy restatements of the image error statistics behind DepthMeter / IntensityMeter (include/lidar4d_eval.h), shared by
tests/test_meters_cpu.py and tests/test_gpu_meters.py.

``errors_f64`` is the formula the kernels implement: fp32 clamp and subtraction, everything after that in float64, the SSIM
window means as 49 shifted-slice sums.  ``errors_ref32`` is the reference's literal path (utils/metrics.py:64-86) on float32
numpy arrays, with skimage.metrics.structural_similarity at its defaults written out the way skimage runs it for float32
input: scipy.ndimage.uniform_filter(size=7) on float32, sample covariance, crop 3, mean in float64.  skimage itself is not a
dependency and could not be run against this code, so SSIM is restated from its published source and is NOT pinned against a
skimage build.  LPIPS is out of both (its weights are no part of this package).
"""
import warnings

import numpy as np

WIN = 7
NP = WIN * WIN
COV_NORM = NP / (NP - 1.0)  # sample covariance (use_sample_covariance=True)
K1, K2 = 0.01, 0.03
LO = 1e-6  # both meters' lower clamp bound

# name -> (H, W, hi, p_gt_drop, p_pred_drop, seed): the shapes both test files use
CASES = {
    "7x7": (7, 7, 80.0, 0.3, 0.1, 0),                  # one window; odd count
    "8x9": (8, 9, 80.0, 0.3, 0.1, 0),                  # even count: two-middle median; 2 x 3 windows
    "33x70_intensity": (33, 70, 1.0, 0.3, 0.1, 0),     # ragged tiles in both directions; the intensity bounds
    "66x1030": (66, 1030, 80.0, 0.3, 0.1, 0),          # the real frame: several tiles, histogram over several workgroups
    "66x1030_ties": (66, 1030, 80.0, 0.7, 0.0, 0),     # more than half the pixels have |d| = 0: mass ties, median exactly 0
    # past the bounded grids of csrc/evalmeter.hip (EM_THREADS 256, EM_CHUNK 2048, EM_MAX_BLOCKS 1024), eight rows tall:
    "8x65600": (8, 65600, 80.0, 0.3, 0.1, 0),          # 524,800 pixels = 257 partials: the `i += EM_THREADS` loops turn twice
    "8x262160": (8, 262160, 80.0, 0.3, 0.1, 0),        # 2,097,280 pixels = 1025 chunks: errors / select kernels stride the grid
    "8x262160_ties": (8, 262160, 80.0, 0.7, 0.0, 0),   # the same with mass ties: the selection's strided histogram
}


def make_pair(H, W, hi, p_gt_drop, p_pred_drop, seed):
    """(pred, gt) float32 [H, W]: a smooth field with dropped (zero) pixels against a noisy render of it that predicts the
    ground truth's drops and adds drops of its own.  One pixel of each image is -1 and one is 2 * hi: both clamps work."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    smooth = 0.5 * hi * (0.55 + 0.4 * np.sin(x / 37.0) * np.cos(y / 9.0))
    keep_gt = rng.random((H, W)) >= p_gt_drop
    keep_pred = rng.random((H, W)) >= p_pred_drop
    gt = smooth * keep_gt
    pred = (smooth + rng.normal(0.0, 0.02 * hi, (H, W))) * keep_gt * keep_pred
    pred[H // 2, W // 3] = -1.0
    pred[H // 3, W // 2] = 2.0 * hi
    gt[H // 2, (2 * W) // 3] = -1.0
    gt[(2 * H) // 3, W // 2] = 2.0 * hi
    return pred.astype(np.float32), gt.astype(np.float32)


def clamp32(x, lo, hi):
    """The reference's masked assignments x[x < lo] = lo; x[x > hi] = hi on a float32 copy: a NaN stays."""
    x = np.array(x, dtype=np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(invalid="ignore"):
        x[x < lo] = lo
        x[x > hi] = hi
    return x


def _median32(a):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (numpy warns when the median of data with a NaN is NaN)
        return np.median(a)


def window_means_f64(a):
    """Means over the 7x7 windows that lie inside the image -> [H-6, W-6] float64 (49 shifted slices)."""
    H, W = a.shape
    acc = np.zeros((H - WIN + 1, W - WIN + 1), dtype=np.float64)
    for dy in range(WIN):
        for dx in range(WIN):
            acc += a[dy:dy + H - WIN + 1, dx:dx + W - WIN + 1]
    return acc / NP


def ssim_map(ux, uy, uxx, uyy, uxy, R):
    vx = COV_NORM * (uxx - ux * ux)
    vy = COV_NORM * (uyy - uy * uy)
    vxy = COV_NORM * (uxy - ux * uy)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def errors_f64(pred, gt, lo, hi):
    """-> float64 [4]: rmse, medae, ssim, psnr (the semantics of l4de_image_errors)."""
    p32, g32 = clamp32(pred, lo, hi), clamp32(gt, lo, hi)
    d = g32 - p32                                   # one fp32 subtraction
    with np.errstate(invalid="ignore", divide="ignore"):
        mse = np.mean(d.astype(np.float64) ** 2)
        rmse = np.sqrt(mse)
        psnr = 10.0 * np.log10(float(np.float32(hi)) ** 2 / mse)
    medae = float(_median32(np.abs(d)))             # float32 selection; (a + b) / 2 in float32 for an even count
    p, g = p32.astype(np.float64), g32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        R = float(np.max(g)) - float(np.min(g))
        S = ssim_map(window_means_f64(p), window_means_f64(g), window_means_f64(p * p), window_means_f64(g * g),
                     window_means_f64(p * g), R)
    return np.array([rmse, medae, np.mean(S), psnr], dtype=np.float64)


def errors_ref32(pred, gt, lo, hi):
    """The reference's compute_depth_errors / compute_intensity_errors without LPIPS, in its own arithmetic.  SSIM is
    skimage's structural_similarity written out on its own, constants included (nothing shared with errors_f64): win_size 7,
    K1 0.01, K2 0.03, use_sample_covariance=True."""
    from scipy.ndimage import uniform_filter
    pred, gt = clamp32(pred, lo, hi), clamp32(gt, lo, hi)
    rmse = np.sqrt(((gt - pred) ** 2).mean())
    medae = _median32(np.abs(gt - pred))
    data_range = np.max(gt) - np.min(gt)
    im1, im2 = pred, gt
    win_size = 7
    ndim = 2
    NP = win_size ** ndim
    cov_norm = NP / (NP - 1)
    ux = uniform_filter(im1, size=win_size)          # float32 in, float32 out, 'reflect' border (cropped away below)
    uy = uniform_filter(im2, size=win_size)
    uxx = uniform_filter(im1 * im1, size=win_size)
    uyy = uniform_filter(im2 * im2, size=win_size)
    uxy = uniform_filter(im1 * im2, size=win_size)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    R = data_range
    C1 = (0.01 * R) ** 2
    C2 = (0.03 * R) ** 2
    A1, A2, B1, B2 = (2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = (A1 * A2) / (B1 * B2)
    pad = (win_size - 1) // 2
    ssim = S[pad:-pad, pad:-pad].mean(dtype=np.float64)
    psnr = 10 * np.log10(hi ** 2 / np.mean((pred - gt) ** 2))
    return np.array([rmse, medae, ssim, psnr], dtype=np.float64)


def errors_loops(pred, gt, lo, hi):
    """errors_f64's SSIM, RMSE and PSNR as plain python loops over pixels and windows (small images only), with the
    window size and the constants written out."""
    p, g = clamp32(pred, lo, hi).astype(np.float64), clamp32(gt, lo, hi).astype(np.float64)
    H, W = p.shape
    R = g.max() - g.min()
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    total, count = 0.0, 0
    for y in range(H - 6):
        for x in range(W - 6):
            sx = sy = sxx = syy = sxy = 0.0
            for dy in range(7):
                for dx in range(7):
                    a, b = p[y + dy, x + dx], g[y + dy, x + dx]
                    sx, sy, sxx, syy, sxy = sx + a, sy + b, sxx + a * a, syy + b * b, sxy + a * b
            ux, uy = sx / 49.0, sy / 49.0
            vx, vy, vxy = 49.0 / 48.0 * (sxx / 49.0 - ux * ux), 49.0 / 48.0 * (syy / 49.0 - uy * uy), 49.0 / 48.0 * (sxy / 49.0 - ux * uy)
            total += (2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
            count += 1
    sq = 0.0
    for y in range(H):
        for x in range(W):
            d = float(np.float32(g[y, x]) - np.float32(p[y, x]))
            sq += d * d
    mse = sq / (H * W)
    return np.array([np.sqrt(mse), np.nan, total / count, 10.0 * np.log10(float(np.float32(hi)) ** 2 / mse)])


class RefMeter:
    """DepthMeter / IntensityMeter on errors_f64: mean of [rmse, medae, lpips (NaN), ssim, psnr] over the updates.  The
    images are taken as they are (already divided by the meter's scale)."""

    def __init__(self, lo, hi):
        self.lo, self.hi, self.rows = lo, hi, []

    def update(self, pred, gt):
        e = errors_f64(pred, gt, self.lo, self.hi)
        self.rows.append(np.array([e[0], e[1], np.nan, e[2], e[3]]))

    def measure(self):
        return np.stack(self.rows).mean(0)
