"""NumPy / SciPy restatement of the surface-distance scores (include/afx.h: afx_distance_transform_edt_3d, afx_surface_metrics_3d): the
yardstick of tests/test_surface_metrics_cpu.py and tests/test_gpu_surface_metrics.py.  The definitions are those of
medpy.metric.binary (dc, assd, hd, hd95) at unit spacing, restated with the SciPy calls medpy makes:

  A = pred >= thr_pred, B = gt >= thr_gt
  S(M) = M & ~binary_erosion(M, generate_binary_structure(3, 1), border_value=0)     voxels of M with a face neighbour outside M
  D_A->B = distance_transform_edt(~S(B))[S(A)], D_B->A = distance_transform_edt(~S(A))[S(B)]
  dice_vessel = 2 |A & B| / (|A| + |B|);  assd = (mean D_A->B + mean D_B->A) / 2;  hd = max of both;
  hd_percentile = np.percentile(hstack(D_A->B, D_B->A), q)
"""
import numpy as np
from scipy import ndimage


def edt(fg):
    """The distance from every voxel to the nearest zero voxel (float64).  Meaningful only when fg has a zero voxel."""
    return ndimage.distance_transform_edt(np.asarray(fg) != 0)


def edt_brute(fg):
    """The exact integer squared distance to the nearest zero voxel by a minimum over all of them (small volumes only)."""
    fg = np.asarray(fg) != 0
    zeros = np.argwhere(~fg)
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in fg.shape], indexing="ij"), -1).reshape(-1, 1, fg.ndim)
    return ((idx - zeros[None]) ** 2).sum(-1).min(-1).reshape(fg.shape)


def surface(mask):
    mask = np.asarray(mask, dtype=bool)
    return mask & ~ndimage.binary_erosion(mask, structure=ndimage.generate_binary_structure(mask.ndim, 1), border_value=0)


def surface_by_neighbours(mask):
    """The same rule spelled out: a voxel of the mask with one of its 6 face neighbours outside it (beyond the grid counts as outside)."""
    mask = np.asarray(mask, dtype=bool)
    p = np.pad(mask, 1, constant_values=False)
    inner = np.ones_like(mask)
    for axis in range(mask.ndim):
        for shift in (-1, 1):
            inner &= np.roll(p, shift, axis=axis)[(slice(1, -1),) * mask.ndim]
    return mask & ~inner


def surface_distances(a, b):
    """(D_A->B, D_B->A) of two boolean masks, each a 1-D float64 array in C order of the surface voxels."""
    sa, sb = surface(a), surface(b)
    return ndimage.distance_transform_edt(~sb)[sa], ndimage.distance_transform_edt(~sa)[sb]


def surface_metrics(pred, gt, thr_pred, thr_gt, q=95.0):
    a = np.asarray(pred) >= np.float32(thr_pred)
    b = np.asarray(gt) >= np.float32(thr_gt)
    if not a.any() or not b.any():
        raise ValueError("empty volume")
    dab, dba = surface_distances(a, b)
    return {"dice_vessel": 2.0 * np.count_nonzero(a & b) / (np.count_nonzero(a) + np.count_nonzero(b)),
            "assd": float(np.mean((dab.mean(), dba.mean()))), "hd": float(max(dab.max(), dba.max())),
            "hd_percentile": float(np.percentile(np.hstack((dab, dba)), q)),
            "n_pred": int(np.count_nonzero(a)), "n_gt": int(np.count_nonzero(b)), "n_overlap": int(np.count_nonzero(a & b)),
            "n_surface_pred": int(dab.size), "n_surface_gt": int(dba.size)}


def assd_bound(n_surface_pred, n_surface_gt):
    """Relative bound on assd between two orders of summation: a sum of n non-negative fp64 terms is within (n - 1) u, u = 2^-53, of
    the exact sum in any order, so two orders differ by at most 2 (n - 1) u relative; the divisions and the final mean are the same
    operations on both sides.  Rounded up to 2 max(n) 2^-53."""
    return 2.0 * max(n_surface_pred, n_surface_gt) * 2.0 ** -53


def tube_and_ball(shape, offset=(0, 0, 0), radius=2.2, ball=4.3):
    """A float32 phantom: a bent tube with a ball at one end, density 1 inside falling off linearly over one voxel outside."""
    idx = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), -1)
    off = np.asarray(offset, dtype=np.float64)
    t = np.linspace(0.0, 1.0, 60)[:, None]
    lo, hi = 0.2 * np.asarray(shape) + off, 0.8 * np.asarray(shape) + off
    line = lo + (hi - lo) * t + np.stack([np.zeros(60), 3.0 * np.sin(3.0 * t[:, 0]), np.zeros(60)], -1)
    d = np.full(shape, np.inf)
    for pt in line:
        d = np.minimum(d, np.sqrt(((idx - pt) ** 2).sum(-1)) - radius)
    d = np.minimum(d, np.sqrt(((idx - hi) ** 2).sum(-1)) - ball)
    return np.clip(1.0 - d, 0.0, 1.0).astype(np.float32)


def box(shape, lo, hi):
    v = np.zeros(shape, np.float32)
    v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1.0
    return v
