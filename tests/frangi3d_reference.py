"""An independent CPU restatement, in NumPy / SciPy, of the 3-D Frangi vesselness of a density volume (Frangi et al. 1998; the definition
is this project's own, stated in include/afx.h): the yardstick of the HIP kernels behind afx_frangi_3d.  Everything is fp64 and every
expression is evaluated operation by operation.

  frangi_3d(x [n0, n1, n2], sigmas, alpha, beta, gamma, black_ridges): black_ridges -> x = 1 - x (the default is False: a density
  volume has bright vessels).  Per sigma s: G = scipy.ndimage.gaussian_filter(x, s, mode='reflect', truncate=4) (axes 0, 1, 2 in that
  order); g_a = np.gradient(G, axis=a), H_ab = (s * s) * np.gradient(g_a, axis=b) for a <= b; the eigenvalues of H by 5 cyclic Jacobi
  sweeps over the pairs (0,1), (0,2), (1,2) (+ - * / and sqrt only: `jacobi_eigenvalues`), ordered by |lambda| ascending (stable: on a
  tie the earlier diagonal position first) -> l1, l2, l3;  ra = (|l2| / d3)^2, d3 = |l3| (1e-10 where 0);  rb = (|l1| / d23)^2,
  d23 = sqrt(|l2 l3|) (1e-10 where 0);  S = l1^2 + l2^2 + l3^2;
  v = (1 - exp(-ra / 2 alpha^2)) exp(-rb / 2 beta^2) (1 - exp(-S / 2 gamma_s^2)), 0 where l2 > 0 or l3 > 0;
  gamma None: gamma_s = sqrt(max S over the volume) / 2 (1 where that is 0), else the given value at every scale.
  The result is the max over the scales (a NaN propagates); scale_index (uint8) the first scale that attains it (np.argmax)."""
import numpy as np
from scipy import ndimage as ndi

SIGMAS = (1, 2, 3)
SWEEPS = 5
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))            # (p, q, the third index r)


def jacobi_eigenvalues(h00, h01, h02, h11, h12, h22, sweeps=SWEEPS):
    """The diagonal after `sweeps` cyclic Jacobi sweeps of the symmetric 3 x 3 matrices [[h00 h01 h02] [. h11 h12] [. . h22]] (arrays of
    one shape) -> (e0, e1, e2) in diagonal order.  A pair whose off-diagonal element is 0 is skipped."""
    a = {}
    for (i, j), v in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), (h00, h01, h02, h11, h12, h22)):
        a[i, j] = a[j, i] = np.array(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q, r in PAIRS:
                apq = a[p, q]
                on = apq != 0
                den = np.where(on, 2 * apq, 1.0)
                theta = (a[q, q] - a[p, p]) / den
                t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1))
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                tau = s / (1 + c)
                tapq = t * apq
                arp, arq = a[r, p], a[r, q]
                new_pp, new_qq = a[p, p] - tapq, a[q, q] + tapq
                new_rp = arp - s * (arq + tau * arp)
                new_rq = arq + s * (arp - tau * arq)
                a[p, p], a[q, q] = np.where(on, new_pp, a[p, p]), np.where(on, new_qq, a[q, q])
                a[p, q] = a[q, p] = np.where(on, 0.0, apq)
                a[r, p] = a[p, r] = np.where(on, new_rp, arp)
                a[r, q] = a[q, r] = np.where(on, new_rq, arq)
    return a[0, 0], a[1, 1], a[2, 2]


def order_by_magnitude(e0, e1, e2):
    """Stable ascending order by |e| (a three-element bubble sort that swaps on strictly-less only) -> (l1, l2, l3)."""
    def step(x, y):
        sw = np.abs(y) < np.abs(x)
        return np.where(sw, y, x), np.where(sw, x, y)
    e0, e1 = step(e0, e1)
    e1, e2 = step(e1, e2)
    e0, e1 = step(e0, e1)
    return e0, e1, e2


def hessian(g, s):
    """(H00, H01, H02, H11, H12, H22) of the smoothed volume g, times s * s."""
    s2 = s * s
    d = [np.gradient(g, axis=a) for a in range(3)]
    return tuple(s2 * np.gradient(d[a], axis=b) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))


def scale_eigenvalues(x, s, eig="jacobi", sweeps=SWEEPS):
    """(l1, l2, l3) of one scale of the (already inverted, fp64) volume x.  eig='eigvalsh': LAPACK instead of the Jacobi sweeps."""
    g = ndi.gaussian_filter(x, sigma=s, mode="reflect", truncate=4.0)
    h = hessian(g, float(s))
    if eig == "eigvalsh":
        m = np.empty(x.shape + (3, 3))
        for (i, j), v in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), h):
            m[..., i, j] = m[..., j, i] = v
        w = np.linalg.eigvalsh(m)
        e = (w[..., 0], w[..., 1], w[..., 2])
    else:
        e = jacobi_eigenvalues(*h, sweeps=sweeps)
    return order_by_magnitude(*e)


def sum_of_squares(l1, l2, l3):
    return l1 * l1 + l2 * l2 + l3 * l3


def auto_gamma(S):
    g = np.sqrt(np.max(S)) / 2
    return 1.0 if g == 0 else float(g)


def vesselness(l1, l2, l3, alpha, beta, gamma):
    with np.errstate(all="ignore"):
        d3 = np.abs(l3)
        d3 = np.where(d3 == 0, 1e-10, d3)
        d23 = np.sqrt(np.abs(l2 * l3))
        d23 = np.where(d23 == 0, 1e-10, d23)
        qa, qb = np.abs(l2) / d3, np.abs(l1) / d23
        ra, rb = qa * qa, qb * qb
        S = sum_of_squares(l1, l2, l3)
        v = (1 - np.exp(-ra / (2 * (alpha * alpha)))) * np.exp(-rb / (2 * (beta * beta))) * (1 - np.exp(-S / (2 * (gamma * gamma))))
    return np.where((l2 > 0) | (l3 > 0), 0.0, v)


def frangi_3d(x, sigmas=SIGMAS, alpha=0.5, beta=0.5, gamma=None, black_ridges=False, return_scale=False, eig="jacobi", sweeps=SWEEPS,
              return_parts=False):
    """The vesselness [n0, n1, n2] (and with return_scale the uint8 index of the first scale attaining it).  return_parts: also a dict with
    the per-scale vesselness, the gammas used and the per-scale largest |lambda| (what the GPU tests need to judge the zero pattern)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3 or min(x.shape) < 2:
        raise ValueError(f"frangi_3d: expected [n0, n1, n2] with every side >= 2, got {x.shape}")
    if black_ridges:
        x = 1 - x
    vs, gammas, lmax = [], [], []
    for s in sigmas:
        l1, l2, l3 = scale_eigenvalues(x, s, eig, sweeps)
        g = auto_gamma(sum_of_squares(l1, l2, l3)) if gamma is None else float(gamma)
        vs.append(vesselness(l1, l2, l3, float(alpha), float(beta), g))
        gammas.append(g)
        lmax.append(np.abs(l3))
    vs = np.stack(vs)
    out = np.max(vs, axis=0)
    res = (out,)
    if return_scale:
        res += (np.argmax(vs, axis=0).astype(np.uint8),)
    if return_parts:
        res += ({"per_scale": vs, "gammas": gammas, "lambda_max": np.max(np.stack(lmax), axis=0)},)
    return res[0] if len(res) == 1 else res


def shapes_phantom(shape=(32, 32, 32), seed=None, amplitude=1.0):
    """A Gaussian tube (along the last of the shortest axes: axis 2 of a cube), a Gaussian blob and a half-plate (normal along axis 0,
    covering the lower half of axis 2) on an exact-zero background, float64 `shape`, with the three centres: {"tube", "blob", "plate"} ->
    index triple.  Every profile exp(-d^2 / 2 w^2) is cut to exact zero beyond 3 w.  The layout scales with the shape, so it also serves
    non-cubic volumes; no structure runs along a long axis, which keeps the rim of almost-zero smoothed values around them short."""
    n0, n1, n2 = shape
    idx = np.meshgrid(np.arange(n0), np.arange(n1), np.arange(n2), indexing="ij")
    i0, i1, i2 = idx
    w = max(1.0, min(shape) / 16.0)

    def prof(d2):
        return np.where(d2 <= 9 * w * w, np.exp(-d2 / (2 * w * w)), 0.0)

    t = max(a for a in range(3) if shape[a] == min(shape))
    c_tube = [shape[a] // 2 if a == t else shape[a] // 4 for a in range(3)]
    tube = prof(sum((idx[a] - c_tube[a]) ** 2.0 for a in range(3) if a != t))
    c_blob = (n0 // 4, (3 * n1) // 4, n2 // 2)
    blob = prof((i0 - c_blob[0]) ** 2.0 + (i1 - c_blob[1]) ** 2.0 + (i2 - c_blob[2]) ** 2.0)
    p0 = (3 * n0) // 4
    plate = prof((i0 - p0) ** 2.0) * (i2 < n2 // 2)
    x = amplitude * np.maximum(np.maximum(tube, blob), plate)
    centres = {"tube": tuple(c_tube), "blob": c_blob, "plate": (p0, n1 // 2, n2 // 4)}
    if seed is not None:
        x = x * (1 + 0.05 * np.random.default_rng(seed).random(shape))
    return x, centres
