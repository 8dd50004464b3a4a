"""NumPy restatement of the evaluation sweep's SSIM (the yardstick of afx_ssim): torchmetrics' StructuralSimilarityIndexMeasure(data_range=1.0)
as the reference calls it (visualization/visualization.py:267, 411-417), i.e. torchmetrics.functional.image.ssim._ssim_update with a
Gaussian kernel of 11 taps, sigma 1.5, computed in fp64.

Written the way torchmetrics computes it, not the way the kernel does: the 11 x 11 window (the outer product of the 1-D kernel) applied as
one literal 121-tap 2-D correlation to the image reflect-padded by 5 on every side, the map of the whole padded-and-convolved image, then
the crop of 5 from every side and the mean."""
import numpy as np

KERNEL = 11
SIGMA = 1.5
C1 = (0.01 * 1.0) ** 2
C2 = (0.03 * 1.0) ** 2


def gaussian_1d(size=KERNEL, sigma=SIGMA):
    """torchmetrics _gaussian: exp(-(dist / sigma)^2 / 2) at dist = -(size - 1)/2 .. (size - 1)/2, normalised to sum 1."""
    dist = np.arange((1 - size) / 2, (1 + size) / 2, 1.0)
    g = np.exp(-((dist / sigma) ** 2) / 2)
    return g / g.sum()


def window_2d():
    g = gaussian_1d()[None, :]
    return g.T @ g                                      # torchmetrics _gaussian_kernel_2d: matmul(kernel_x^T, kernel_y)


def _correlate_valid(img, win):
    """F.conv2d without padding (a cross-correlation): out[i, j] = sum_{a, b} win[a, b] img[i + a, j + b], all 121 taps per output."""
    k = win.shape[0]
    h, w = img.shape[0] - k + 1, img.shape[1] - k + 1
    out = np.zeros((h, w))
    for a in range(k):
        for b in range(k):
            out += win[a, b] * img[a:a + h, b:b + w]
    return out


def ssim_map(x, y):
    """The SSIM map of two [H, W] images on the (H - 10) x (W - 10) windows inside them (torchmetrics pads by 5 and crops 5 again)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 2 or min(x.shape) < KERNEL:
        raise ValueError("ssim: two [H, W] images of one shape, H, W >= 11")
    pad = (KERNEL - 1) // 2
    win = window_2d()
    # torchmetrics: F.pad(..., mode='reflect') of preds, target, preds^2, target^2, preds*target, then one grouped conv2d
    stack = [x, y, x * x, y * y, x * y]
    outs = [_correlate_valid(np.pad(s, pad, mode="reflect"), win) for s in stack]
    mu_x, mu_y, exx, eyy, exy = outs
    mu_x_sq, mu_y_sq, mu_xy = mu_x ** 2, mu_y ** 2, mu_x * mu_y
    s_x = np.maximum(exx - mu_x_sq, 0.0)
    s_y = np.maximum(eyy - mu_y_sq, 0.0)
    s_xy = exy - mu_xy
    upper = 2 * s_xy + C2
    lower = (s_x + s_y) + C2
    full = ((2 * mu_xy + C1) * upper) / ((mu_x_sq + mu_y_sq + C1) * lower)
    return full[pad:-pad, pad:-pad]


def ssim(x, y):
    """SSIM of one pair of [H, W] images (float)."""
    return float(ssim_map(x, y).mean())


def ssim_batch(xs, ys):
    return np.array([ssim(a, b) for a, b in zip(xs, ys)])


def vessel_views(n, h, w, seed=0):
    """n X-ray-like views in fp32: a near-1 background with thin dark vessels (most pixels flat, where E[x^2] - mu^2 cancels hard)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((n, h, w), dtype=np.float32)
    for i in range(n):
        img = np.full((h, w), 0.985 + 0.01 * rng.random())
        for _ in range(3):
            a, b = rng.uniform(0, np.pi), rng.uniform(-0.3, 0.3)
            d = np.abs((xx - w / 2) * np.sin(a) - (yy - h / 2) * np.cos(a) - b * min(h, w))
            img -= rng.uniform(0.1, 0.5) * np.exp(-(d / rng.uniform(0.6, 2.0)) ** 2)
        out[i] = img + rng.normal(0, 1e-3, (h, w))
    return out
