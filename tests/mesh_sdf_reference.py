"""NumPy fp64 restatement of afx_mesh_sdf_3d / afx_mesh_point_distance (include/afx.h): the distance of a point to a triangle as the
minimum of three segment terms and a plane term, the nearest triangle as the first index that attains the minimum, the generalised
winding number summed in triangle order, the sign.  Operation by operation as the header orders them (NumPy's element-wise ufuncs
round every product and sum on their own; a division by zero or an invalid operation raises: the definition has none), vectorised
over point-triangle pairs in chunks of points, all pairs: no culling, no bricks.  Meshes come from isosurface_reference.isosurface and from a few hand-made arrays."""
import numpy as np

import isosurface_reference as iso

PAIRS_PER_CHUNK = 200_000
FOUR_PI = 4.0 * np.pi


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _seg_d2(p, a, b):
    e, w = b - a, p - a
    den, num = _dot(e, e), _dot(w, e)
    t = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
    t = np.where(t < 0, 0.0, np.where(t > 1, 1.0, t))
    g = p - (a + t[..., None] * e)
    return _dot(g, g)


def pair_d2(p, a, b, c):
    """p [n, 1, 3] against a, b, c [1, T, 3] (fp64) -> d2 [n, T]"""
    d = _seg_d2(p, a, b)
    d1 = _seg_d2(p, b, c)
    d = np.where(d1 < d, d1, d)
    d2 = _seg_d2(p, c, a)
    d = np.where(d2 < d, d2, d)
    n = _cross(b - a, c - a)
    nn = _dot(n, n)
    e0 = _dot(_cross(b - a, p - a), n)
    e1 = _dot(_cross(c - b, p - b), n)
    e2 = _dot(_cross(a - c, p - c), n)
    h = _dot(p - a, n)
    ok = (nn > 0) & (e0 > 0) & (e1 > 0) & (e2 > 0)
    pl = (h * h) / np.where(nn > 0, nn, 1.0)
    return np.where(ok & (pl < d), pl, d)


def pair_winding_terms(p, a, b, c):
    A, B, C = a - p, b - p, c - p
    det = _dot(A, _cross(B, C))
    la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
    den = (((la * lb) * lc + _dot(A, B) * lc) + _dot(B, C) * la) + _dot(C, A) * lb
    return 2.0 * np.arctan2(det, den)


def valid_triangles(vertices, triangles):
    """-> (indices of the triangles that are not skipped, a, b, c as fp64 [1, T', 3])"""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    inside = ((t >= 0) & (t < len(v))).all(axis=1)
    finite = np.isfinite(v).all(axis=1)
    ok = inside.copy()
    ok[inside] = finite[t[inside]].all(axis=1)
    idx = np.flatnonzero(ok)
    v64 = v.astype(np.float64)
    a, b, c = (v64[t[idx, k]][None] if len(idx) else np.zeros((1, 0, 3)) for k in range(3))
    return idx, a, b, c


def grid_points(shape, affine=None):
    """World positions of the grid points in raster order, fp64 [N, 3], in the header's order of operations."""
    m, o = iso.affine_parts(affine)
    q = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1).reshape(-1, 3)
    return np.stack([((o[r] + m[r, 0] * q[:, 0]) + m[r, 1] * q[:, 1]) + m[r, 2] * q[:, 2] for r in range(3)], axis=1)


def _distance(points, idx, a, b, c):
    n = len(points)
    d2 = np.full(n, np.inf)
    nearest = np.full(n, -1, dtype=np.int64)
    if len(idx) and n:
        step = max(1, PAIRS_PER_CHUNK // len(idx))
        with np.errstate(divide="raise", invalid="raise"):
            for s in range(0, n, step):
                d = pair_d2(points[s:s + step, None, :], a, b, c)
                k = np.argmin(d, axis=1)                       # the first index that attains the minimum
                d2[s:s + step] = d[np.arange(len(k)), k]
                nearest[s:s + step] = idx[k]
    return d2, nearest


def _winding(points, idx, a, b, c):
    n = len(points)
    w = np.zeros(n)
    if len(idx) and n:
        step = max(1, PAIRS_PER_CHUNK // len(idx))
        with np.errstate(divide="raise", invalid="raise"):
            for s in range(0, n, step):
                terms = pair_winding_terms(points[s:s + step, None, :], a, b, c)
                w[s:s + step] = np.add.accumulate(terms, axis=1)[:, -1]      # one after the other, in triangle order
    return w / FOUR_PI


def point_distance(points, vertices, triangles):
    """-> (dist float32 [P], nearest int32 [P], d2 fp64 [P])"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    d2, nearest = _distance(p, *valid_triangles(vertices, triangles))
    return np.sqrt(d2).astype(np.float32), nearest.astype(np.int32), d2


def mesh_sdf(vertices, triangles, shape, affine=None):
    """-> dict(sdf float32 [shape], nearest int32 [shape], winding fp64 [shape], d2 fp64 [shape], valid, skipped)"""
    idx, a, b, c = valid_triangles(vertices, triangles)
    p = grid_points(shape, affine)
    d2, nearest = _distance(p, idx, a, b, c)
    w = _winding(p, idx, a, b, c)
    d = np.sqrt(d2)
    sdf = np.where((w >= 0.5) & (d > 0), -d, d).astype(np.float32)
    total = len(np.asarray(triangles).reshape(-1, 3))
    return dict(sdf=sdf.reshape(shape), nearest=nearest.astype(np.int32).reshape(shape), winding=w.reshape(shape), d2=d2.reshape(shape),
                valid=len(idx), skipped=total - len(idx))


def capped_mesh(f, level, affine=None, fill=-1.0):
    """(vertices float32 [V, 3], triangles int32 [T, 3]) of the closed surface engine.extract_isosurface(cap=True) gives"""
    m = iso.isosurface(iso.padded(f, fill), level, iso.shifted_affine(affine))
    return m["vertices"], m["triangles"].astype(np.int32)


def open_mesh(f, level, affine=None):
    m = iso.isosurface(f, level, affine)
    return m["vertices"], m["triangles"].astype(np.int32)


def sphere_sdf(n, points):
    """the analytic signed distance (negative inside) of iso.sphere_field(n)'s zero level at `points` (index coordinates)"""
    return np.linalg.norm(points - (n - 1) / 2.0, axis=-1) - 0.35 * n


def torus_sdf(n, points, major=None, minor=None):
    """... of iso.torus_field(n, major, minor)'s"""
    q = points - (n - 1) / 2.0
    ring = np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - (0.3 * n if major is None else major)
    return np.sqrt(ring ** 2 + q[..., 2] ** 2) - (0.12 * n if minor is None else minor)


def mesh_distance_scores(va, ta, vb, tb, q=95.0):
    """medpy's assd / hd / hd95 on two surfaces given as meshes: each mesh's vertices against the other's triangles; the mean of the
    two means, the maximum of the two maxima, the percentile of the concatenation.  NaN when either mesh is empty."""
    if min(len(va), len(ta), len(vb), len(tb)) == 0:
        return {"ASSD MESH": float("nan"), "HD MESH": float("nan"), "HD95 MESH": float("nan")}
    ab = point_distance(va, vb, tb)[0].astype(np.float64)
    ba = point_distance(vb, va, ta)[0].astype(np.float64)
    return {"ASSD MESH": float((ab.mean() + ba.mean()) / 2.0), "HD MESH": float(max(ab.max(), ba.max())),
            "HD95 MESH": float(np.percentile(np.concatenate([ab, ba]), q))}
