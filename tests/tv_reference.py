"""NumPy restatement of afx_tv_denoise_3d (include/afx.h), operation by operation in fp64: the loop over the iterations is sequential,
everything inside one is vectorised over the voxels.  The device must equal it exactly.  Also the total variation, the ROF energy and the
SIRT-TV iteration engine.sirt_reconstruct(tv_weight=...) runs, built on sirt_reference's project, backproject and update."""
import numpy as np

import sirt_reference as sr


def _low(p, axis):
    """p_a[i - e_a] where i_a > 0, else +0.0."""
    out = np.zeros_like(p)
    hi = [slice(None)] * 3
    lo = [slice(None)] * 3
    hi[axis], lo[axis] = slice(1, None), slice(None, -1)
    out[tuple(hi)] = p[tuple(lo)]
    return out


def divergence(p):
    """div = (b_0 + b_1) + b_2, b_a = p_a[i] - (i_a > 0 ? p_a[i - e_a] : +0)."""
    b = [p[a] - _low(p[a], a) for a in range(3)]
    return (b[0] + b[1]) + b[2]


def gradient(u):
    """g_a[i] = i_a < n_a - 1 ? u[i + e_a] - u[i] : +0 -> three arrays."""
    g = []
    for a in range(3):
        d = np.zeros_like(u)
        hi = [slice(None)] * 3
        lo = [slice(None)] * 3
        hi[a], lo[a] = slice(1, None), slice(None, -1)
        d[tuple(lo)] = u[tuple(hi)] - u[tuple(lo)]
        g.append(d)
    return g


def _norm(g):
    return np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])


def tv_denoise(x, weight, iterations=50, tau=1.0 / 6.0, nonneg=False, mask=None):
    """afx_tv_denoise_3d -> out, float64 of x's shape."""
    x = np.asarray(x, np.float64)
    assert x.ndim == 3
    tau = np.float64(tau)
    c = tau / np.float64(weight)
    p = [np.zeros_like(x) for _ in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(int(iterations)):
            u = x - divergence(p)
            g = gradient(u)
            den = 1.0 + c * _norm(g)
            p = [(p[a] - tau * g[a]) / den for a in range(3)]
        out = x - divergence(p) if int(iterations) > 0 else x.copy()
        if nonneg:
            out = np.where(out > 0.0, out, 0.0)
    if mask is not None:
        out = np.where(np.asarray(mask) == 0, 0.0, out)
    return out


def total_variation(u):
    """The isotropic total variation: the sum of m over the gradient of u itself."""
    return float(_norm(gradient(np.asarray(u, np.float64))).sum())


def rof_energy(u, x, weight):
    """0.5 sum (u - x)^2 + weight TV(u)."""
    d = np.asarray(u, np.float64) - np.asarray(x, np.float64)
    return 0.5 * float((d * d).sum()) + float(weight) * total_variation(u)


def sirt_tv(line_integrals, shape, a12, records, width, height, near, far, n_samples, iterations, tv_weight, tv_iterations=10, relax=1.0,
            mask=None, x0=None, nonneg=True):
    """engine.sirt_reconstruct(tv_weight=...) -> x: sirt_reference.sirt's iteration with tv_denoise (p from zero, the same nonneg and
    mask) after every update."""
    b12 = sr.world_to_index(a12)
    weight = sr.sirt_weight(shape, b12, records, width, height, near, far, n_samples)
    x = np.zeros(shape, np.float64) if x0 is None else np.array(x0, np.float64)
    for _ in range(int(iterations)):
        r = sr.project(x, b12, records, width, height, near, far, n_samples, target=line_integrals, weight=weight)
        acc, cnt = sr.backproject(r, records, shape, a12)
        x = sr.update(x, acc, cnt, relax, nonneg, mask)
        x = tv_denoise(x, tv_weight, tv_iterations, nonneg=nonneg, mask=mask)
    return x
