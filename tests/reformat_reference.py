"""The yardstick of the reformation tests (include/afx.h: afx_reformat_planes): a NumPy restatement of the definition, vectorised over the
P x Q samples and sequential over the slab index m, every scalar operation in the stated order (NumPy's elementwise + - * / and floor are
IEEE operations rounded one by one; nothing here goes through a dot product or a sum whose order NumPy chooses).  The lookup is step 4 of
afx_lumen_profile (tests/lumen_reference.py) with `fill` outside the box.  Plus the host pipeline of the sweep's CPR scores and the
measurements the phantom tests make on a longitudinal image."""
import numpy as np

import lumen_reference as lr

MEAN, MAX = 0, 1


def lookup(vol64, w, x0, x1, x2, fill):
    """Step 3: the volume (already float64) at world points; `fill` outside.  lumen_reference.lookup gives 0.0 outside, and its inside
    test is the definition's: the outside samples are found again with the same operations."""
    n = vol64.shape
    w = np.asarray(w, np.float64).reshape(3, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = np.ones(np.shape(x0), bool)
        for a in range(3):
            q = ((w[a, 0] * x0 + w[a, 1] * x1) + w[a, 2] * x2) + w[a, 3]
            inside &= (q >= 0.0) & (q <= float(n[a] - 1))
        return np.where(inside, lr.lookup(vol64, w, x0, x1, x2), float(fill)), inside


def reformat_planes(vol, world_to_index, planes, table, half_slab=0, mode=MEAN, fill=0.0, return_inside=False):
    """-> float64 [P, Q] of the definition in include/afx.h (with return_inside also bool [P, Q]: the m = 0 sample lies in the box)."""
    vol64 = np.asarray(vol).astype(np.float64)
    pl = np.asarray(planes, np.float64).reshape(-1, 9)
    tb = np.asarray(table, np.float64).reshape(-1, 4)
    h = int(half_slab)
    c, u, v = pl[:, None, 0:3], pl[:, None, 3:6], pl[:, None, 6:9]
    a, b, sa, sb = (tb[None, :, k] for k in range(4))
    out = acc = np.zeros((pl.shape[0], tb.shape[0]))
    inside0 = np.zeros(out.shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(-h, h + 1):
            alpha, beta = a + float(m) * sa, b + float(m) * sb
            x = [(c[:, :, r] + alpha * u[:, :, r]) + beta * v[:, :, r] for r in range(3)]
            f, inside = lookup(vol64, world_to_index, x[0], x[1], x[2], fill)
            if m == 0:
                inside0 = inside
            if mode == MEAN:
                acc = acc + f
            else:
                out = f if m == -h else np.where(f > out, f, out)
        if mode == MEAN:
            out = acc / float(2 * h + 1)
    return (out, inside0) if return_inside else out


def turn_angles(t, u):
    """The angle (radians) of the rotation that takes the frame (t, u, t x u) of point i to that of point i + 1: cos = (trace - 1) / 2 of
    F_{i+1} F_i^T.  It holds the bending of the line itself (curvature x spacing) and any twist about it.  -> float64 [P - 1]."""
    t, u = np.asarray(t, np.float64), np.asarray(u, np.float64)
    f = np.stack([t, u, np.cross(t, u)], axis=1)                     # [P, 3 vectors, 3 components]
    trace = np.einsum("pab,pab->p", f[1:], f[:-1])
    return np.arccos(np.clip((trace - 1.0) / 2.0, -1.0, 1.0))


def per_point_frames(points, half_window=3):
    """The per-point rule of afx_lumen_profile (steps 1 and 2) on one polyline -> (t, u)."""
    p = np.asarray(points, np.float64)
    n = len(p)
    k = np.arange(n)
    a, b = np.maximum(k - half_window, 0), np.minimum(k + half_window, n - 1)
    d = p[b] - p[a]
    t = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    e = np.eye(3)[np.argmin(np.abs(t), axis=1)]
    u = np.cross(t, e)
    return t, u / np.sqrt((u * u).sum(axis=1))[:, None]


def helix(n, radius=5.0, pitch=1.5, turns_rad=4.0 * np.pi):
    """n points of the helix (r cos phi, r sin phi, pitch phi), phi in [0, turns_rad] -> (points, arc length s, torsion tau)."""
    phi = np.linspace(0.0, turns_rad, n)
    pts = np.stack([radius * np.cos(phi), radius * np.sin(phi), pitch * phi], axis=1)
    norm = np.sqrt(radius * radius + pitch * pitch)
    return pts, phi * norm, pitch / (norm * norm)


def voxel_helix(radius=20.0, pitch=6.0, turns_rad=6.0 * np.pi):
    """The helix sampled at about unit arc length and rounded to voxel centres, neighbouring duplicates removed: the 26-connected path
    a skeleton would give (about 390 voxels)."""
    n = int(turns_rad * np.sqrt(radius * radius + pitch * pitch)) + 1
    pts = np.rint(helix(n, radius, pitch, turns_rad)[0])
    keep = np.concatenate([[True], np.any(pts[1:] != pts[:-1], axis=1)])
    return pts[keep]


def run_width(row, step, level=0.5):
    """The width of the run of samples >= level about the middle of one row of a longitudinal image, in world units (samples x step);
    0.0 when the middle sample is below the level."""
    row = np.asarray(row)
    mid = len(row) // 2
    if not row[mid] >= level:
        return 0.0
    lo = hi = mid
    while lo - 1 >= 0 and row[lo - 1] >= level:
        lo -= 1
    while hi + 1 < len(row) and row[hi + 1] >= level:
        hi += 1
    return float(hi - lo + 1) * float(step)


def pearson(a, b):
    """Pearson's correlation of two arrays over all elements in fp64; NaN when either is constant."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    da, db = a - a.mean(), b - b.mean()
    den = np.sqrt((da * da).sum() * (db * db).sum())
    return float((da * db).sum() / den) if den > 0 else float("nan")


def cpr_images_host(vol, points, index_to_world, angles, half_width, step, slab=0, mode=MEAN, half_window=3, fill=0.0):
    """engine.cpr_images on the host: the engine's own host geometry (frames, table, world_to_index - the arrays the device gets) and
    the restatement in place of the kernel -> (images float64 [A, P, K], flags)."""
    from nerf_for_angiography_amd import engine
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    t, u, v, flags = engine.rotation_minimising_frames(pts, half_window)
    table = engine.reformat_table_cpr(half_width, step, angles)
    out = reformat_planes(vol, engine.lumen_world_to_index(index_to_world), np.concatenate([pts, u, v], axis=1), table, slab, mode, fill)
    return np.ascontiguousarray(out.reshape(len(pts), len(angles), 2 * half_width + 1).transpose(1, 0, 2)), flags


def image_widths(images, step, level=0.5):
    """run_width of every row of every image -> float64 [A, P]."""
    return np.array([[run_width(row, step, level) for row in img] for img in images])


def waist(widths):
    """1 - min width / lower-median width of one image's rows (the lower median sorted[(n - 1) // 2], as the lumen summary's)."""
    w = np.sort(np.asarray(widths, np.float64))
    return 1.0 - w[0] / w[(len(w) - 1) // 2]


def graph_dict(g, shape):
    """The result of graph_reference.analyse as the dict engine.centreline_main_path reads (the fields of engine.centreline_graph)."""
    rows = g["branches"]
    return {"shape": tuple(shape), "path_voxels": np.array(g["path_voxels"], np.int64), "branch_size": np.array([r["n"] for r in rows], np.int64),
            "path_offset": np.array([r["offset"] for r in rows], np.int64), "is_cycle": np.array([r["cycle"] for r in rows], bool),
            "node_start": np.array([r["node_start"] for r in rows], np.int64), "node_end": np.array([r["node_end"] for r in rows], np.int64),
            "length": np.array([r["length"] for r in rows], np.float64), "total_length": float(g["record"]["length"])}
