"""The yardstick of the lumen-profile tests (include/afx.h: afx_lumen_profile): a NumPy restatement of the definition, vectorised over the
points and the rays, every scalar operation in the stated order (NumPy's elementwise + - * / sqrt and floor are IEEE operations rounded
one by one; nothing here goes through a dot product or a sum whose order NumPy chooses), the pairwise tree of the reductions, and the
lower median of the per-branch summary.  Plus the tube phantoms of the tests."""
import numpy as np

NO_TANGENT, CENTRE_OUTSIDE = 1, 2


def lookup(vol64, w, x0, x1, x2):
    """Step 4: the volume (already float64) at world points (x0, x1, x2 arrays of one shape); 0.0 outside."""
    n = vol64.shape
    w = np.asarray(w, np.float64).reshape(3, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        q = [((w[a, 0] * x0 + w[a, 1] * x1) + w[a, 2] * x2) + w[a, 3] for a in range(3)]
        inside = np.ones(np.shape(x0), bool)
        for a in range(3):
            inside &= (q[a] >= 0.0) & (q[a] <= float(n[a] - 1))
    i, tau = [], []
    for a in range(3):
        qa = np.where(inside, q[a], 0.0)                   # nothing is converted or loaded for an outside point
        fl = np.minimum(np.floor(qa), float(n[a] - 2))
        i.append(fl.astype(np.int64))
        tau.append(qa - fl)
    p = lambda a, b, c: vol64[i[0] + a, i[1] + b, i[2] + c]
    lerp = lambda lo, hi, t: lo + (hi - lo) * t
    c00, c01 = lerp(p(0, 0, 0), p(0, 0, 1), tau[2]), lerp(p(0, 1, 0), p(0, 1, 1), tau[2])
    c10, c11 = lerp(p(1, 0, 0), p(1, 0, 1), tau[2]), lerp(p(1, 1, 0), p(1, 1, 1), tau[2])
    c0, c1 = lerp(c00, c01, tau[1]), lerp(c10, c11, tau[1])
    return np.where(inside, lerp(c0, c1, tau[0]), 0.0)


def tree_sum(x):
    """s(l+1)_j = s(l)_2j + s(l)_2j+1 over the last axis (a power of two) -> the root."""
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _unit(t):
    n2 = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
    return n2, t / np.sqrt(n2)[:, None]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def lumen_profile(vol, world_to_index, points, seg_first, seg_last, half_window, n_rays, ray_cs, area_coef, iso, step, max_steps):
    """-> (profile float64 [P, 8], flags int32 [P], radii float64 [P, R]) of the definition in include/afx.h."""
    vol64 = np.asarray(vol).astype(np.float64)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    P, R, M, ds, iso = pts.shape[0], int(n_rays), int(max_steps), float(step), float(iso)
    cs, sn = np.asarray(ray_cs, np.float64)[0::2], np.asarray(ray_cs, np.float64)[1::2]
    profile, flags, radii = np.zeros((P, 8)), np.zeros(P, np.int32), np.zeros((P, R))
    if P == 0:
        return profile, flags, radii
    # 1. tangent
    k = np.arange(P, dtype=np.int64)
    a = np.clip(np.maximum(k - int(half_window), np.asarray(seg_first, np.int64)), 0, P - 1)
    b = np.clip(np.minimum(k + int(half_window), np.asarray(seg_last, np.int64)), 0, P - 1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n2, t = _unit(pts[b] - pts[a])
        no_tangent = (b <= a) | (n2 == 0.0)
        # 5. centre
        f0 = lookup(vol64, world_to_index, pts[:, 0], pts[:, 1], pts[:, 2])
        outside = ~(f0 >= iso)
        flags[:] = np.where(no_tangent, NO_TANGENT, 0) | np.where(outside, CENTRE_OUTSIDE, 0)
        profile[:, 6] = f0
        go = np.flatnonzero(flags == 0)
        if go.size == 0:
            return profile, flags, radii
        t, c, f0 = t[go], pts[go], f0[go]
        # 2. frame
        e = np.eye(3)[np.argmin(np.abs(t), axis=1)]          # argmin: the first smallest
        _, u = _unit(_cross(t, e))
        v = _cross(t, u)
        # 3. directions [G, R, 3]
        d = cs[None, :, None] * u[:, None, :] + sn[None, :, None] * v[:, None, :]
        # 6. march
        r = np.full((go.size, R), float(M) * ds)
        done = np.zeros((go.size, R), bool)
        f_prev = np.repeat(f0[:, None], R, axis=1)
        for m in range(1, M + 1):
            s = float(m) * ds
            f = lookup(vol64, world_to_index, c[:, None, 0] + s * d[:, :, 0], c[:, None, 1] + s * d[:, :, 1], c[:, None, 2] + s * d[:, :, 2])
            hit = ~done & (f < iso)
            r = np.where(hit, ds * (float(m - 1) + (f_prev - iso) / np.where(hit, f_prev - f, 1.0)), r)
            done |= hit
            f_prev = np.where(done, f_prev, f)
            if done.all():
                break
    # 7. reductions
    h = R // 2
    dia = r[:, :h] + r[:, h:]
    profile[go, 0] = area_coef * tree_sum(r * np.roll(r, -1, axis=1))
    profile[go, 1] = tree_sum(r) / float(R)
    profile[go, 2], profile[go, 3] = r.min(axis=1), r.max(axis=1)
    profile[go, 4], profile[go, 5] = dia.min(axis=1), dia.max(axis=1)
    flags[go] |= ((~done).sum(axis=1) << 8).astype(np.int32)
    radii[go] = r
    return profile, flags, radii


def branch_summary(area, flags, branch, min_points=5):
    """Per branch id (ascending) -> dict of arrays: n_valid, area_min, argmin (first, position within the branch), area_ref (the LOWER
    median sorted[(n - 1) // 2]), area_stenosis, diameter_stenosis; NaN / -1 with fewer than min_points valid points."""
    area, flags, branch = np.asarray(area, np.float64), np.asarray(flags), np.asarray(branch)
    ids = sorted(set(branch.tolist()))
    out = {"branch": np.array(ids, np.int64), "n_valid": [], "area_min": [], "argmin": [], "area_ref": [], "area_stenosis": [], "diameter_stenosis": []}
    for b in ids:
        where = [i for i in range(len(branch)) if branch[i] == b]
        ok = [i for i in where if flags[i] == 0]
        out["n_valid"].append(len(ok))
        if len(ok) < max(min_points, 1):
            for name, v in (("area_min", np.nan), ("argmin", -1), ("area_ref", np.nan), ("area_stenosis", np.nan), ("diameter_stenosis", np.nan)):
                out[name].append(v)
            continue
        vals = [area[i] for i in ok]
        lo = min(vals)
        ref = sorted(vals)[(len(vals) - 1) // 2]
        out["area_min"].append(lo)
        out["argmin"].append(ok[vals.index(lo)] - where[0])
        out["area_ref"].append(ref)
        out["area_stenosis"].append(1.0 - lo / ref)
        out["diameter_stenosis"].append(1.0 - np.sqrt(lo / ref))
    return {k: np.asarray(v) for k, v in out.items()}


def oblique_tube(n, rho, half_length, width=1.0):
    """The tube phantom: float32 [n, n, n] = clip((rho(s) + width - dist) / (2 width), 0, 1) about the axis through (n/2 - 0.3, n/2 + 0.2,
    n/2) along (1, 0.6, 0.35) normalised (rho a number or a function of the position s along the axis), and its centreline: the axis
    sampled at unit arc length over +-half_length and ROUNDED to voxel centres, as a skeleton gives it -> (volume, points [P, 3], s [P])."""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"), -1)
    c0 = np.array([n / 2 - 0.3, n / 2 + 0.2, n / 2])
    ax = np.array([1.0, 0.6, 0.35])
    ax /= np.sqrt((ax * ax).sum())
    rel = g - c0
    along = rel @ ax
    dist = np.sqrt(np.maximum((rel * rel).sum(-1) - along ** 2, 0.0))
    radius = rho(along) if callable(rho) else float(rho)
    vol = np.clip((radius + width - dist) / (2.0 * width), 0.0, 1.0).astype(np.float32)
    s = np.arange(-half_length, half_length + 1e-9, 1.0)
    return vol, np.rint(c0 + s[:, None] * ax), s


def stenosis_radius(s):
    return 4.0 - 2.0 * np.exp(-s ** 2 / 18.0)


def smooth_volume(shape, seed, dtype=np.float32):
    """A Gaussian-filtered random field plus a tube along the longest diagonal direction of the box, scaled into about [0, 1]."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    x = ndimage.gaussian_filter(rng.standard_normal(shape), 1.5, mode="nearest")
    x = 0.25 * x / max(np.abs(x).max(), 1e-30)
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)
    c0 = (np.array(shape, np.float64) - 1.0) / 2.0
    ax = np.array(shape, np.float64) - 1.0
    ax /= np.sqrt((ax * ax).sum())
    rel = g - c0
    along = rel @ ax
    dist = np.sqrt(np.maximum((rel * rel).sum(-1) - along ** 2, 0.0))
    rho = max(min(shape) / 4.0, 0.75)
    return (x + np.clip((rho + 1.0 - dist) / 2.0, 0.0, 1.0)).astype(dtype)
