"""An independent CPU restatement, in NumPy / SciPy, of the projection ray-sampling weights (get_weighted_img with the Frangi
filter of scikit-image 0.18.3, include/afx.h): the yardstick of the HIP kernels behind afx_frangi, afx_distance_transform_edt
and afx_sampling_weights.  scikit-image itself is not a dependency; this file is written from the definition:

  frangi(I), per sigma: black_ridges -> I = 1 - I; G = scipy.ndimage.gaussian_filter(I, sigma) (truncate 4, mode 'reflect');
  Hessian from np.gradient of np.gradient (0.18.3's hessian_matrix(order='rc') differentiates d/dc G along the rows for the mixed
  term), times sigma^2; eigenvalues l+- = (Hrr + Hcc) / 2 +- sqrt(4 Hrc^2 + (Hrr - Hcc)^2) / 2, sorted by magnitude (a tie: l+
  first); v = exp(-rb / 2 beta^2) (1 - exp(-(l1^2 + l2^2) / 2 gamma^2)), rb = (l1 / |l2|)^2 with |l2| = 0 -> 1e-10; v = 0 where
  l2 > 0; the max over the sigmas.  alpha has no effect in 2-D.
  weights(img): binary False -> pixels > np.percentile(img, 10) set to 1; f = frangi(img); f -= min; f /= max; e = EDT(f);
  e -= min; e /= max; e += 1e-10 (a max of 0 raises ValueError)."""
import numpy as np
from scipy import ndimage as ndi

SIGMAS = (1, 3, 5, 7, 9)


def frangi(image, sigmas=SIGMAS, alpha=0.5, beta=0.5, gamma=15, black_ridges=True):
    del alpha
    img = np.asarray(image, dtype=np.float64)
    if black_ridges:
        img = 1 - img
    best = None
    for s in sigmas:
        g = ndi.gaussian_filter(img, sigma=s, mode="reflect", truncate=4.0)
        gr, gc = np.gradient(g)
        hcc, hrc, hrr = np.gradient(gc, axis=1), np.gradient(gc, axis=0), np.gradient(gr, axis=0)
        s2 = s * s
        m00, m01, m11 = s2 * hcc, s2 * hrc, s2 * hrr
        tr = (m00 + m11) / 2
        disc = np.sqrt(4 * m01 ** 2 + (m00 - m11) ** 2) / 2
        lp, lm = tr + disc, tr - disc
        swap = np.abs(lm) < np.abs(lp)
        l1, l2 = np.where(swap, lm, lp), np.where(swap, lp, lm)
        d = np.abs(l2)
        d[d == 0] = 1e-10
        rb = (l1 / d) ** 2
        rg = l1 ** 2 + l2 ** 2
        v = np.exp(-rb / (2 * beta ** 2)) * (1 - np.exp(-rg / (2 * gamma ** 2)))
        v[l2 > 0] = 0
        best = v if best is None else np.maximum(best, v)
    return best


def hessian_l2(image, sigma, black_ridges=True):
    """lambda2 (the larger-magnitude eigenvalue) of one scale: what decides the background rule v = 0 where lambda2 > 0."""
    img = np.asarray(image, dtype=np.float64)
    img = 1 - img if black_ridges else img
    g = ndi.gaussian_filter(img, sigma=sigma, mode="reflect", truncate=4.0)
    gr, gc = np.gradient(g)
    m00, m01, m11 = (sigma * sigma * h for h in (np.gradient(gc, axis=1), np.gradient(gc, axis=0), np.gradient(gr, axis=0)))
    tr, disc = (m00 + m11) / 2, np.sqrt(4 * m01 ** 2 + (m00 - m11) ** 2) / 2
    lp, lm = tr + disc, tr - disc
    return np.where(np.abs(lm) < np.abs(lp), lp, lm)


def prestep(img, binary):
    x = np.array(img, dtype=np.float64)
    if not binary:
        x[x > np.percentile(x, 10)] = 1
    return x


def sampling_weights(img, binary=True, sigmas=SIGMAS, beta=0.5, gamma=15):
    x = prestep(img, binary)
    f = frangi(x, sigmas, alpha=12 if binary else 0.5, beta=beta, gamma=gamma)
    f -= f.min()
    if f.max() == 0:
        raise ValueError("flat vesselness")
    f /= f.max()
    e = ndi.distance_transform_edt(f)
    e -= e.min()
    if e.max() == 0:
        raise ValueError("flat distance transform")
    e /= e.max()
    return e + 1e-10


def dark_line_image(h=64, w=64, row=32, width=3, value=0.0):
    img = np.ones((h, w))
    img[row - width // 2: row - width // 2 + width] = value
    return img


def vessel_image(h, w, seed=0, n_lines=6, background=None):
    """Dark, blurred line segments of widths 1..5 px on a bright background (optionally non-uniform): a non-binary projection."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.ones((h, w)) if background is None else background
    for _ in range(n_lines):
        a, b = rng.uniform((0, 0), (h, w)), rng.uniform((0, 0), (h, w))
        ab = b - a
        t = np.clip(((yy - a[0]) * ab[0] + (xx - a[1]) * ab[1]) / (ab @ ab), 0, 1)
        dist = np.hypot(yy - (a[0] + t * ab[0]), xx - (a[1] + t * ab[1]))
        r = rng.uniform(0.5, 2.5)
        img = img * (1 - 0.6 * np.exp(-0.5 * (dist / r) ** 2))
    return img
