"""The 2D-3D chamfer registration restated in NumPy, operation by operation as include/afx.h states it (afx_pose_chamfer,
afx_pose_compose, afx_pose_select, afx_pose_lm_step): fp64, every operation rounded on its own, every comparison with a NaN false, the
sums in the order of the definition (thread t of 256 takes its points in ascending order, the 256 values meet in the adjacent-pair tree
of lumen_reference.tree_sum, the slices stay apart).  The device equals it exactly."""
import numpy as np

from lumen_reference import tree_sum

VIEW_DOUBLES = 16
SUM_DOUBLES = 32
STATE_DOUBLES = 64
BLOCK = 256
COST_ONLY = 1
LM_INIT, LM_UPDATE, LM_FINAL = 0, 1, 2
LAMBDA0 = 1e-3
# the state row of afx_pose_lm_step
ST_RECORD, ST_COST, ST_G, ST_H, ST_LAMBDA, ST_ACCEPTED, ST_REJECTED, ST_SINGULAR, ST_TRIAL = 0, 16, 17, 23, 44, 45, 46, 47, 48
H_INDEX = [(k, l) for k in range(6) for l in range(k, 6)]      # the upper triangle, row-major: slot 9 + n of the sums


def slice_length(n, n_slices):
    per = -(-int(n) // int(n_slices))
    return -(-per // BLOCK) * BLOCK


def compose(record, xi):
    """afx_pose_compose of one record [16] and one increment [6] = (a0, a1, a2, t0, t1, t2)."""
    rec = np.array(record, np.float64).reshape(VIEW_DOUBLES)
    x = np.asarray(xi, np.float64).reshape(6)
    if (x == 0.0).all():
        return rec.copy()
    a0, a1, a2, t = x[0], x[1], x[2], x[3:6]
    n = (a0 * a0 + a1 * a1) + a2 * a2
    s, den = 1.0 - n, 1.0 + n
    c = np.array([[(s + 2.0 * (a0 * a0)) / den, (2.0 * (a0 * a1) - 2.0 * a2) / den, (2.0 * (a0 * a2) + 2.0 * a1) / den],
                  [(2.0 * (a0 * a1) + 2.0 * a2) / den, (s + 2.0 * (a1 * a1)) / den, (2.0 * (a1 * a2) - 2.0 * a0) / den],
                  [(2.0 * (a0 * a2) - 2.0 * a1) / den, (2.0 * (a1 * a2) + 2.0 * a0) / den, (s + 2.0 * (a2 * a2)) / den]])
    r = rec[:9].reshape(3, 3)
    out = rec.copy()
    rn = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            rn[i, j] = (r[i, 0] * c[j, 0] + r[i, 1] * c[j, 1]) + r[i, 2] * c[j, 2]
    out[:9] = rn.reshape(-1)
    for i in range(3):
        out[9 + i] = rec[9 + i] - ((rn[i, 0] * t[0] + rn[i, 1] * t[1]) + rn[i, 2] * t[2])
    return out


def compose_outer(records, xis):
    """[R, 16] x [M, 6] -> [R, M, 16]: what afx_pose_compose gives with n_xi = M."""
    records, xis = np.asarray(records, np.float64).reshape(-1, VIEW_DOUBLES), np.asarray(xis, np.float64).reshape(-1, 6)
    return np.stack([np.stack([compose(r, x) for x in xis]) for r in records])


def residuals(field_v, points, radius, record, trunc):
    """Per point of one record: dict(r, kind (0 active, 1 satisfied, 2 saturated, 3 lost), J [N, 6] (zero rows where not active), u, w, d)."""
    fld = np.asarray(field_v, np.float64)
    h, wd = fld.shape
    rec = np.asarray(record, np.float64)
    rm, c, f = rec[:9].reshape(3, 3), rec[9:12], rec[12]
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = p.shape[0]
    rad = np.zeros(n) if radius is None else np.asarray(radius, np.float64).reshape(n)
    with np.errstate(all="ignore"):
        e = p - c
        q = [(rm[0, k] * e[:, 0] + rm[1, k] * e[:, 1]) + rm[2, k] * e[:, 2] for k in range(3)]
        d = -q[2]
        su, sw = (f * q[0]) / d, (f * q[1]) / d
        u, w = wd / 2 + su, h / 2 - sw
        ok = (d > 0.0) & (u >= 0.0) & (u <= wd - 1.0) & (w >= 0.0) & (w <= h - 1.0)
        uc, wc = np.where(ok, u, 0.0), np.where(ok, w, 0.0)
        fu, fw = np.minimum(np.floor(uc), wd - 2.0), np.minimum(np.floor(wc), h - 2.0)
        iu, iw = fu.astype(np.int64), fw.astype(np.int64)
        pu, pw = uc - fu, wc - fw
        f00, f01, f10, f11 = fld[iw, iu], fld[iw, iu + 1], fld[iw + 1, iu], fld[iw + 1, iu + 1]
        a, b = f01 - f00, f11 - f10
        top, bot = f00 + pu * a, f10 + pu * b
        gw = bot - top
        val = top + pw * gw
        gu = a + pw * (b - a)
        err = val + (f * rad) / d
        satisfied, saturated = ok & (err <= 0.0), ok & (err >= trunc)
        active = ok & ~(err <= 0.0) & ~(err >= trunc)
        r = np.where(active, err, np.where(satisfied, 0.0, trunc))
        kind = np.where(~ok, 3, np.where(satisfied, 1, np.where(saturated, 2, 0)))
        fd = f / d
        j3, j4 = gu * fd, -(gw * fd)
        j5 = (gu * su - gw * sw) / d
        j0 = 2.0 * (q[1] * j5 - q[2] * j4)
        j1 = 2.0 * (q[2] * j3 - q[0] * j5)
        j2 = 2.0 * (q[0] * j4 - q[1] * j3)
        jac = np.stack([j0, j1, j2, j3, j4, j5], axis=1)
        jac = np.where(active[:, None], jac, 0.0)
    return dict(r=r, kind=kind, J=jac, u=u, w=w, d=d)


def chamfer(field, points, radius, weight, records, rec_view, trunc, n_slices=1, flags=0):
    """(sums float64 [K, S, 32], counts int32 [K, S, 4]) of afx_pose_chamfer."""
    field = np.asarray(field, np.float64)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n, s_n = p.shape[0], int(n_slices)
    records = np.asarray(records, np.float64).reshape(-1, VIEW_DOUBLES)
    k_n = records.shape[0]
    wt = np.ones(n) if weight is None else np.asarray(weight, np.float64).reshape(n)
    length = slice_length(n, s_n)
    sums, counts = np.zeros((k_n, s_n, SUM_DOUBLES)), np.zeros((k_n, s_n, 4), np.int32)
    for k in range(k_n):
        v = int(rec_view[k])
        if v < 0 or v >= field.shape[0]:
            sums[k, :, 0], counts[k] = np.inf, -1
            continue
        res = residuals(field[v], p, radius, records[k], trunc)
        with np.errstate(all="ignore"):
            wr = wt * res["r"]
            terms = [wr * res["r"], wr, wt]
            if not flags & COST_ONLY:
                wj = wt[:, None] * res["J"]
                active = res["kind"] == 0
                terms += [np.where(active, wj[:, a] * res["r"], 0.0) for a in range(6)]
                terms += [np.where(active, wj[:, a] * res["J"][:, b], 0.0) for a, b in H_INDEX]
            terms = np.stack(terms, axis=1)                      # [N, 3 or 30]
            for s in range(s_n):
                lo, hi = s * length, min(n, (s + 1) * length)
                if lo >= hi:
                    continue
                rows = np.zeros((length, terms.shape[1]))
                rows[:hi - lo] = terms[lo:hi]
                rows = rows.reshape(-1, BLOCK, terms.shape[1])
                acc = np.zeros((BLOCK, terms.shape[1]))
                for row in rows:                                 # a padded +0.0 changes no accumulator: they start at +0.0
                    acc = acc + row
                sums[k, s, :terms.shape[1]] = tree_sum(acc.T)
                counts[k, s] = np.bincount(res["kind"][lo:hi], minlength=4)
    return sums, counts


def select(sums, n_views, n_candidates):
    """(selected int32 [V], cost float64 [V, M]) of afx_pose_select: sums [V M, S, 32], record v M + m."""
    sums = np.asarray(sums, np.float64).reshape(n_views, n_candidates, -1, SUM_DOUBLES)
    cost = np.zeros((n_views, n_candidates))
    for s in range(sums.shape[2]):
        cost = cost + sums[:, :, s, 0]
    sel = np.zeros(n_views, np.int32)
    for v in range(n_views):
        for m in range(1, n_candidates):
            if cost[v, m] < cost[v, sel[v]]:
                sel[v] = m
    return sel, cost


def solve(g, h_upper, lam, dof_mask):
    """(delta [6], singular) of (H + lam diag H) delta = -g by the unrolled Cholesky of afx_pose_lm_step."""
    a = np.zeros((6, 6))
    for n, (k, l) in enumerate(H_INDEX):
        a[k, l] = a[l, k] = h_upper[n]
    b = np.zeros(6)
    for k in range(6):
        if not (dof_mask >> k) & 1:
            a[k, :], a[:, k] = 0.0, 0.0
            a[k, k], b[k] = 1.0, 0.0
        else:
            a[k, k] = a[k, k] + lam * a[k, k]
            b[k] = -g[k]
    low = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            s = a[j, j]
            for p in range(j):
                s = s - low[j, p] * low[j, p]
            if not s > 0.0:
                return np.zeros(6), True
            low[j, j] = np.sqrt(s)
            for i in range(j + 1, 6):
                t = a[i, j]
                for p in range(j):
                    t = t - low[i, p] * low[j, p]
                low[i, j] = t / low[j, j]
        y = np.zeros(6)
        for i in range(6):
            t = b[i]
            for p in range(i):
                t = t - low[i, p] * y[p]
            y[i] = t / low[i, i]
        delta = np.zeros(6)
        for i in range(5, -1, -1):
            t = y[i]
            for p in range(i + 1, 6):
                t = t - low[p, i] * delta[p]
            delta[i] = t / low[i, i]
    return delta, False


def lm_step(state, sums, phase, dof_mask=63, lambda0=LAMBDA0, records_in=None):
    """afx_pose_lm_step on state [V, 64] in place; sums [V, S, 32].  -> trial_records [V, 16]."""
    sums = np.asarray(sums, np.float64).reshape(state.shape[0], -1, SUM_DOUBLES)
    trial = np.zeros((state.shape[0], VIEW_DOUBLES))
    for v in range(state.shape[0]):
        st = state[v]
        tot = np.zeros(30)
        with np.errstate(all="ignore"):
            for s in range(sums.shape[1]):
                tot = tot + sums[v, s, :30]
        if phase == LM_INIT:
            st[:] = 0.0
            st[ST_RECORD:ST_RECORD + 16] = records_in[v]
            st[ST_COST], st[ST_G:ST_G + 6], st[ST_H:ST_H + 21], st[ST_LAMBDA] = tot[0], tot[3:9], tot[9:30], lambda0
        elif tot[0] < st[ST_COST]:
            st[ST_RECORD:ST_RECORD + 16] = st[ST_TRIAL:ST_TRIAL + 16]
            st[ST_COST], st[ST_G:ST_G + 6], st[ST_H:ST_H + 21] = tot[0], tot[3:9], tot[9:30]
            st[ST_LAMBDA] = max(st[ST_LAMBDA] / 3.0, 1e-12)
            st[ST_ACCEPTED] += 1.0
        else:
            st[ST_LAMBDA] = min(4.0 * st[ST_LAMBDA], 1e12)
            st[ST_REJECTED] += 1.0
        if phase == LM_FINAL:
            st[ST_TRIAL:ST_TRIAL + 16] = st[ST_RECORD:ST_RECORD + 16]
        else:
            delta, singular = solve(st[ST_G:ST_G + 6], st[ST_H:ST_H + 21], st[ST_LAMBDA], dof_mask)
            if singular:
                st[ST_SINGULAR] += 1.0
            st[ST_TRIAL:ST_TRIAL + 16] = compose(st[ST_RECORD:ST_RECORD + 16], delta)
        trial[v] = st[ST_TRIAL:ST_TRIAL + 16]
    return trial


def register(field, points, radius, weight, records, iterations=20, trunc=8.0, dof_mask=63, offsets=None, n_slices=1, lambda0=LAMBDA0):
    """The sequence of engine.register_poses_record -> dict(state [V, 64], records [V, 16], selected [V], start [V, 16])."""
    records = np.asarray(records, np.float64).reshape(-1, VIEW_DOUBLES)
    nv = records.shape[0]
    views = np.arange(nv, dtype=np.int32)
    selected, start = np.zeros(nv, np.int32), records.copy()
    if offsets is not None:
        m = np.asarray(offsets).reshape(-1, 6).shape[0]
        cand = compose_outer(records, offsets)
        sums, _ = chamfer(field, points, radius, weight, cand.reshape(-1, VIEW_DOUBLES), np.repeat(views, m), trunc, n_slices, COST_ONLY)
        selected, _ = select(sums, nv, m)
        start = cand[np.arange(nv), selected]
    state = np.zeros((nv, STATE_DOUBLES))
    sums, _ = chamfer(field, points, radius, weight, start, views, trunc, n_slices, 0)
    trial = lm_step(state, sums, LM_INIT, dof_mask, lambda0, start)
    for it in range(iterations):
        sums, _ = chamfer(field, points, radius, weight, trial, views, trunc, n_slices, 0)
        trial = lm_step(state, sums, LM_UPDATE if it + 1 < iterations else LM_FINAL, dof_mask, lambda0)
    return dict(state=state, records=state[:, :16].copy(), selected=selected, start=start)


# ---- host-side helpers of the tests ----
def edt_brute(mask_on):
    """The exact Euclidean distance from every pixel to the nearest True pixel of a small image (inf without one)."""
    on = np.argwhere(mask_on)
    h, w = mask_on.shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if on.shape[0] == 0:
        return np.full((h, w), np.inf)
    d2 = ((yy[None] - on[:, 0, None, None]) ** 2 + (xx[None] - on[:, 1, None, None]) ** 2).min(axis=0)
    return np.sqrt(d2.astype(np.float64))


def signed_field(mask):
    """EDT(~mask) - EDT(mask): negative inside the silhouette, positive outside (engine.pose_views builds the same on the device)."""
    mask = np.asarray(mask, bool)
    return edt_brute(mask) - edt_brute(~mask)


def reprojection_error(points, rec_a, rec_b, width, height):
    """The mean pixel distance between the projections of the points under two records."""
    ra = residuals(np.zeros((height, width)), points, None, rec_a, 1.0)
    rb = residuals(np.zeros((height, width)), points, None, rec_b, 1.0)
    return float(np.mean(np.sqrt((ra["u"] - rb["u"]) ** 2 + (ra["w"] - rb["w"]) ** 2)))


# ---- the scene of the tests ----
def tree_points(n, n_branches, seed, radius_scale=1.0):
    """(points [n, 3], radius [n]) of viewmap_reference.wavy_tree: the first end and the radius of every segment."""
    import viewmap_reference as vr
    seg, _ = vr.wavy_tree(n, n_branches, seed)
    return np.ascontiguousarray(seg[:, 0:3]), np.ascontiguousarray(seg[:, 6] * radius_scale), seg


def oblique_views(n_views, width, seed=7, distance=60.0, focal_factor=2.4):
    """(poses [V, 4, 4], focal) of sources at `distance` from the scene's centre at seeded oblique angles."""
    from nerf_for_angiography_amd.phantomdata.proj_helpers import source_matrix
    rng = np.random.RandomState(seed)
    poses = [source_matrix(np.array([0.0, 0.0, distance]), rng.uniform(-180, 180), rng.uniform(-60, 60)) for _ in range(n_views)]
    return np.stack(poses), focal_factor * width


def silhouettes(segments, records, width, height):
    """bool [V, H, W]: the pixels some capsule of the tree covers (viewmap_reference.coverage), the masks of the scene."""
    import viewmap_reference as vr
    segments = np.array(segments)
    return np.stack([vr.coverage(segments, rec, width, height)[0].any(axis=0) for rec in records])


def perturbation(n_views, seed, rot_deg=0.5, shift=0.5):
    """Seeded increments [V, 6]: up to +-rot_deg about each camera axis (a = tan(theta / 2)) and +-shift world units along each."""
    rng = np.random.RandomState(seed)
    xi = np.zeros((n_views, 6))
    xi[:, :3] = np.tan(np.deg2rad(rng.uniform(-rot_deg, rot_deg, (n_views, 3))) / 2.0)
    xi[:, 3:] = rng.uniform(-shift, shift, (n_views, 3))
    return xi
