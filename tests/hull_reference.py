"""NumPy restatement of afx_visual_hull (include/afx.h), operation by operation in fp64 and vectorised per view: the device must equal
it exactly.  Also the inverse of the forward ray model (`project`) and the helper that builds silhouette masks from 3-D points."""
import numpy as np

SQRT_HALF = float(np.sqrt(np.float64(0.5)))


def lattice_points(shape, index_to_world):
    """x_a = ((A[a][0] i + A[a][1] j) + A[a][2] k) + A[a][3] for every (i, j, k), k fastest -> float64 [n0 n1 n2, 3]."""
    a = np.asarray(index_to_world, np.float64).reshape(3, 4)
    n0, n1, n2 = (int(s) for s in shape)
    i, j, k = np.meshgrid(np.arange(n0, dtype=np.float64), np.arange(n1, dtype=np.float64), np.arange(n2, dtype=np.float64), indexing="ij")
    return np.stack([((a[r, 0] * i + a[r, 1] * j) + a[r, 2] * k) + a[r, 3] for r in range(3)], axis=-1).reshape(-1, 3)


def camera_coordinates(x, pose):
    """q = R^T (x - c) of the pose cam2world = [R | c], each component (R[0][n] e0 + R[1][n] e1) + R[2][n] e2 -> q [P, 3]."""
    m = np.asarray(pose, np.float64)
    r, c = m[:3, :3], m[:3, 3]
    e = np.asarray(x, np.float64) - c
    return np.stack([(r[0, n] * e[:, 0] + r[1, n] * e[:, 1]) + r[2, n] * e[:, 2] for n in range(3)], axis=-1)


def project(x, pose, f, width, height):
    """The pixel (u, w) a world point projects to and its depth d along the view axis (pixel centres at the integers); only where d > 0
    is the projection meaningful."""
    q = camera_coordinates(x, pose)
    d = -q[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = width / 2 + (f * q[:, 0]) / d
        w = height / 2 - (f * q[:, 1]) / d
    return u, w, d


def view_votes(x, rho, pose, f, width, height, margin, dist):
    """(seen, reject) bool [P] of one view; dist float64 [H, W]."""
    q = camera_coordinates(x, pose)
    q0, q1 = q[:, 0], q[:, 1]
    d = -q[:, 2]
    near = d - rho
    ok = near > 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = width / 2 + (f * q0) / d
        w = height / 2 - (f * q1) / d
        ell = np.sqrt(q0 * q0 + q1 * q1)
        r = ((f * rho) * (d + ell)) / (d * near) + margin
        dx = np.maximum(np.maximum(0.0, -u), u - (width - 1))
        dy = np.maximum(np.maximum(0.0, -w), w - (height - 1))
        delta = np.sqrt(dx * dx + dy * dy)
        seen = ok & (dx <= r) & (dy <= r)
        iu = np.clip(np.floor(u + 0.5), 0, width - 1)
        iw = np.clip(np.floor(w + 0.5), 0, height - 1)
        iu = np.where(seen, iu, 0).astype(np.int64)
        iw = np.where(seen, iw, 0).astype(np.int64)
        reject = seen & (np.asarray(dist, np.float64)[iw, iu] > (r + SQRT_HALF) + delta)
    return seen, reject


def hull_counts(x, rho, poses, focal, width, height, margin, dist):
    """seen, rejects uint16 [P]: the votes of all views over the points x float64 [P, 3]; focal: a number or one per view."""
    poses = np.asarray(poses, np.float64)
    f = np.broadcast_to(np.asarray(focal, np.float64), (poses.shape[0],))
    seen = np.zeros(x.shape[0], np.int64)
    rejects = np.zeros(x.shape[0], np.int64)
    for v in range(poses.shape[0]):
        s, r = view_votes(x, float(rho), poses[v], float(f[v]), int(width), int(height), float(margin), dist[v])
        seen += s
        rejects += r
    return seen.astype(np.uint16), rejects.astype(np.uint16)


def distance_stack(masks):
    """D_v = distance from each pixel to the nearest mask pixel (scipy's distance_transform_edt of the complement) -> float64 [V, H, W]."""
    from scipy.ndimage import distance_transform_edt
    masks = np.asarray(masks) != 0
    if not masks.reshape(masks.shape[0], -1).any(axis=1).all():
        raise ValueError("distance_stack: a view has an empty mask")
    return np.stack([distance_transform_edt(~m) for m in masks]).astype(np.float64)


def masks_from_points(points, poses, focal, width, height):
    """Silhouettes of a point cloud: pixel floor(proj + 0.5) of every point in front of the source that lands on the detector is marked
    -> (masks bool [V, H, W], inside bool [V, P]: the point landed on the detector of view v)."""
    poses = np.asarray(poses, np.float64)
    f = np.broadcast_to(np.asarray(focal, np.float64), (poses.shape[0],))
    masks = np.zeros((poses.shape[0], int(height), int(width)), bool)
    inside = np.zeros((poses.shape[0], points.shape[0]), bool)
    for v in range(poses.shape[0]):
        u, w, d = project(points, poses[v], float(f[v]), width, height)
        with np.errstate(invalid="ignore"):
            iu, iw = np.floor(u + 0.5), np.floor(w + 0.5)
            ok = (d > 0) & (iu >= 0) & (iu <= width - 1) & (iw >= 0) & (iw <= height - 1)
        masks[v, iw[ok].astype(np.int64), iu[ok].astype(np.int64)] = True
        inside[v] = ok
    return masks, inside


def box_lattice(half, n):
    """Cell centres of an n^3 grid over the box [-half, half]^3 and half the cell diagonal -> (index_to_world 12 doubles, rho)."""
    s = 2.0 * half / n
    o = -half + 0.5 * s
    a = np.array([s, 0, 0, o, 0, s, 0, o, 0, 0, s, o], np.float64)
    return a, 0.5 * float(np.sqrt((s * s + s * s) + s * s))
