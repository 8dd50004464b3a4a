"""NumPy restatement of afx_xray_project and afx_xray_backproject (include/afx.h) and of the SIRT iteration engine.sirt_reconstruct runs
with them, operation by operation in fp64: the loop over the samples of a ray and the loop over the views are sequential, everything else
is vectorised.  The device must equal it exactly.  Also the small scenes the tests share."""
import numpy as np


def world_to_index(index_to_world):
    """B = inv(A), offset -(B o), taken in fp64 as engine.lumen_world_to_index takes it -> 12 doubles."""
    a = np.asarray(index_to_world, np.float64).reshape(3, 4)
    w = np.linalg.inv(a[:, :3])
    return np.concatenate([w, -(w @ a[:, 3])[:, None]], axis=1).reshape(-1)


def view_records(poses, focal):
    """R row-major at [0..8], c at [9..11], f at [12] of 16 doubles per view, as engine.hull_view_records."""
    p = np.asarray(poses, np.float64)
    rec = np.zeros((p.shape[0], 16), np.float64)
    rec[:, 0:9] = p[:, :3, :3].reshape(-1, 9)
    rec[:, 9:12] = p[:, :3, 3]
    rec[:, 12] = np.broadcast_to(np.asarray(focal, np.float64), (p.shape[0],))
    return rec


def _lerp(p, q, phi):
    return p + phi * (q - p)


def project(volume, b12, records, width, height, near, far, n_samples, target=None, weight=None):
    """afx_xray_project -> float64 [V, H, W]: the line integrals y, or weight (target - y)."""
    vol = np.asarray(volume, np.float64)
    n0, n1, n2 = vol.shape
    b = np.asarray(b12, np.float64).reshape(3, 4)
    rec = np.asarray(records, np.float64)
    w_, h_, s_ = int(width), int(height), int(n_samples)
    iw, iu = np.meshgrid(np.arange(h_, dtype=np.float64), np.arange(w_, dtype=np.float64), indexing="ij")
    out = np.empty((rec.shape[0], h_, w_), np.float64)
    dt = (np.float64(far) - np.float64(near)) / np.float64(s_)
    for v in range(rec.shape[0]):
        r, c, f = rec[v, :9].reshape(3, 3), rec[v, 9:12], rec[v, 12]
        ca = (iu - w_ / 2) / f
        cb = -((iw - h_ / 2) / f)
        d = [(r[k, 0] * ca + r[k, 1] * cb) - r[k, 2] for k in range(3)]
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        acc = np.zeros((h_, w_), np.float64)
        for s in range(s_):
            t = np.float64(near) + (np.float64(s) + 0.5) * dt
            x = [c[k] + t * d[k] for k in range(3)]
            g = [((b[a, 0] * x[0] + b[a, 1] * x[1]) + b[a, 2] * x[2]) + b[a, 3] for a in range(3)]
            with np.errstate(invalid="ignore"):
                inside = ((g[0] >= 0) & (g[0] <= n0 - 1)) & ((g[1] >= 0) & (g[1] <= n1 - 1)) & ((g[2] >= 0) & (g[2] <= n2 - 1))
            if not inside.any():
                continue
            gi = [np.where(inside, g[a], 0.0) for a in range(3)]
            fl = [np.minimum(np.floor(gi[a]), n - 2) for a, n in enumerate((n0, n1, n2))]
            phi = [gi[a] - fl[a] for a in range(3)]
            i0, i1, i2 = (fl[a].astype(np.int64) for a in range(3))
            c00 = _lerp(vol[i0, i1, i2], vol[i0, i1, i2 + 1], phi[2])
            c01 = _lerp(vol[i0, i1 + 1, i2], vol[i0, i1 + 1, i2 + 1], phi[2])
            c10 = _lerp(vol[i0 + 1, i1, i2], vol[i0 + 1, i1, i2 + 1], phi[2])
            c11 = _lerp(vol[i0 + 1, i1 + 1, i2], vol[i0 + 1, i1 + 1, i2 + 1], phi[2])
            value = _lerp(_lerp(c00, c01, phi[1]), _lerp(c10, c11, phi[1]), phi[0])
            acc = np.where(inside, acc + value, acc)
        out[v] = (acc * dt) * length
    if target is not None:
        return np.asarray(weight, np.float64) * (np.asarray(target, np.float64) - out)
    return out


def lattice_points(shape, index_to_world):
    """x_a = ((A[a][0] i + A[a][1] j) + A[a][2] k) + A[a][3] for every (i, j, k), k fastest -> float64 [n0 n1 n2, 3]."""
    a = np.asarray(index_to_world, np.float64).reshape(3, 4)
    n0, n1, n2 = (int(s) for s in shape)
    i, j, k = np.meshgrid(np.arange(n0, dtype=np.float64), np.arange(n1, dtype=np.float64), np.arange(n2, dtype=np.float64), indexing="ij")
    return np.stack([((a[r, 0] * i + a[r, 1] * j) + a[r, 2] * k) + a[r, 3] for r in range(3)], axis=-1).reshape(-1, 3)


def backproject(images, records, shape, a12):
    """afx_xray_backproject's gather -> (acc float64, cnt uint16) of `shape`."""
    img = np.asarray(images, np.float64)
    rec = np.asarray(records, np.float64)
    _, h_, w_ = img.shape
    x = lattice_points(shape, a12)
    acc = np.zeros(x.shape[0], np.float64)
    cnt = np.zeros(x.shape[0], np.int64)
    for v in range(rec.shape[0]):
        r, c, f = rec[v, :9].reshape(3, 3), rec[v, 9:12], rec[v, 12]
        e = [x[:, k] - c[k] for k in range(3)]
        q = [(r[0, n] * e[0] + r[1, n] * e[1]) + r[2, n] * e[2] for n in range(3)]
        d = -q[2]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            front = d > 0.0
            u = w_ / 2 + (f * q[0]) / d
            w = h_ / 2 - (f * q[1]) / d
            seen = front & ((u >= 0) & (u <= w_ - 1)) & ((w >= 0) & (w <= h_ - 1))
        us, ws = np.where(seen, u, 0.0), np.where(seen, w, 0.0)
        fu, fw = np.minimum(np.floor(us), w_ - 2), np.minimum(np.floor(ws), h_ - 2)
        pu, pw = us - fu, ws - fw
        iu, iw = fu.astype(np.int64), fw.astype(np.int64)
        top = _lerp(img[v, iw, iu], img[v, iw, iu + 1], pu)
        bot = _lerp(img[v, iw + 1, iu], img[v, iw + 1, iu + 1], pu)
        acc = np.where(seen, acc + _lerp(top, bot, pw), acc)
        cnt += seen
    return acc.reshape(shape), cnt.astype(np.uint16).reshape(shape)


def update(x, acc, cnt, relax, nonneg, mask=None):
    """The fused SIRT update of afx_xray_backproject -> the new x."""
    cnt = np.asarray(cnt).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        upd = np.where(cnt > 0, acc / cnt, 0.0)
    y = np.asarray(x, np.float64) + np.float64(relax) * upd
    if nonneg:
        y = np.where(y > 0.0, y, 0.0)
    if mask is not None:
        y = np.where(np.asarray(mask) == 0, 0.0, y)
    return y


def sirt_weight(shape, b12, records, width, height, near, far, n_samples):
    """weight = where(l > 0, 1 / l, 0), l = the projection of a volume of ones."""
    ell = project(np.ones(shape, np.float64), b12, records, width, height, near, far, n_samples)
    with np.errstate(divide="ignore"):
        return np.where(ell > 0, 1.0 / ell, 0.0)


def sirt(line_integrals, shape, a12, records, width, height, near, far, n_samples, iterations, relax=1.0, mask=None, x0=None, nonneg=True):
    """engine.sirt_reconstruct -> (x, the weighted residual images of every iteration [iterations, V, H, W]): per iteration
    r = weight (b - project(x)), then x = update(x, backproject(r))."""
    b12 = world_to_index(a12)
    weight = sirt_weight(shape, b12, records, width, height, near, far, n_samples)
    x = np.zeros(shape, np.float64) if x0 is None else np.array(x0, np.float64)
    residuals = []
    for _ in range(int(iterations)):
        r = project(x, b12, records, width, height, near, far, n_samples, target=line_integrals, weight=weight)
        residuals.append(r)
        acc, cnt = backproject(r, records, shape, a12)
        x = update(x, acc, cnt, relax, nonneg, mask)
    return x, np.stack(residuals)


def residual_norms(residuals):
    """sqrt(sum r^2) of each iteration's weighted residual images, by NumPy (the engine's history is torch's sum of the same images)."""
    r = np.asarray(residuals, np.float64)
    return np.sqrt((r * r).reshape(r.shape[0], -1).sum(axis=1))


def look_at_pose(source, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """cam2world = [R | c] of a camera at `source` looking at `target` down its -z axis, y up -> float64 [4, 4] with orthonormal R."""
    c = np.asarray(source, np.float64)
    z = c - np.asarray(target, np.float64)
    z = z / np.sqrt((z * z).sum())
    x = np.cross(np.asarray(up, np.float64), z)
    x = x / np.sqrt((x * x).sum())
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, c
    return m


# ---- the 20 x 26 x 17 scene of the iteration tests ----
SCENE_SHAPE = (20, 26, 17)
SCENE_VIEW = dict(width=22, height=18, near=1440.0, far=1560.0, n_samples=40)
SCENE_FOCAL, SCENE_DISTANCE = 260.0, 1500.0


def scene():
    """The lattice spans +-30 world units with anisotropic spacing; the truth is three capsules of density 0.05; 5 views of 22 x 18 at
    source distance 1500, f = 260, near / far 1440 / 1560, S = 40; the mask is the truth dilated by two voxels ->
    dict(a12, truth, mask uint8, poses, records, line_integrals)."""
    n0, n1, n2 = SCENE_SHAPE
    s = [60.0 / (n - 1) for n in SCENE_SHAPE]
    a12 = np.array([s[0], 0, 0, -30.0, 0, s[1], 0, -30.0, 0, 0, s[2], -30.0], np.float64)
    x = lattice_points(SCENE_SHAPE, a12)
    caps = (((-18.0, -12.0, -10.0), (14.0, 8.0, 6.0), 5.0), ((14.0, 8.0, 6.0), (20.0, 22.0, -14.0), 4.0), ((14.0, 8.0, 6.0), (-4.0, 20.0, 18.0), 3.5))
    inside = np.zeros(x.shape[0], bool)
    for p, q, r in caps:
        p, q = np.asarray(p), np.asarray(q)
        t = np.clip(((x - p) @ (q - p)) / ((q - p) @ (q - p)), 0.0, 1.0)
        inside |= np.sqrt((((x - p) - t[:, None] * (q - p)) ** 2).sum(axis=1)) <= r
    truth = np.where(inside, 0.05, 0.0).reshape(SCENE_SHAPE)
    mask = inside.reshape(SCENE_SHAPE)
    for _ in range(2):      # dilated by two voxels (6 neighbours, twice)
        grown = mask.copy()
        for axis in range(3):
            grown[(slice(None),) * axis + (slice(1, None),)] |= mask[(slice(None),) * axis + (slice(None, -1),)]
            grown[(slice(None),) * axis + (slice(None, -1),)] |= mask[(slice(None),) * axis + (slice(1, None),)]
        mask = grown
    dirs = ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.05), (0.6, 0.5, 0.62), (-0.55, 0.45, 0.7))
    ups = ((0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0))
    poses = np.stack([look_at_pose(SCENE_DISTANCE * np.asarray(d) / np.sqrt(np.dot(d, d)), up=u) for d, u in zip(dirs, ups)])
    records = view_records(poses, SCENE_FOCAL)
    b = project(truth, world_to_index(a12), records, **SCENE_VIEW)
    return dict(a12=a12, truth=truth, mask=mask.astype(np.uint8), poses=poses, records=records, line_integrals=b)
