"""The grid ray march (k_march_count / k_march_write: march_range, march_keep, grid_cell) restated from its definition in NumPy float64,
with the margins of every step, the seeded problems of tests/test_march_cpu.py and tests/test_gpu_march.py, and - apart from the
reference, further down - an operation-by-operation fp32 emulation of the kernels.  Nothing here is shared with oracle/angio_oracle.py
or the kernels.

Definition (march64):
  slab interval   per axis with d != 0: t0 = (lo - o) / d, t1 = (hi - o) / d (true division), [min, max]; the ray's interval [lo, hi] is the
                  intersection.  An axis with d == 0 (either sign) constrains no t: the ray is inside that slab for all t when
                  lo <= o < hi and misses otherwise - half open, as the cells are (0 <= u < 1): the lower face grazes, the upper face
                  misses.  A miss is also hi < max(lo, 0).
  range           t_min = max(lo, 0, near), t_max = min(hi, far).
  steps           step k is [t_min + k dt, t_min + (k + 1) dt); it is the ray's iff its mid-point is < t_max.
  cell            u = (p - lo) / (hi - lo); inside iff 0 <= u < 1 on every axis; ijk = min(floor(u res), res - 1);
                  idx = (i ry + j) rz + k; bit = bits[idx >> 5] >> (idx & 31).
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

F32 = np.float32


@dataclass
class Problem:
    name: str
    origins: np.ndarray                      # [R, 3] float32
    dirs: np.ndarray                         # [R, 3] float32, not normalised unless the builder does
    scene: Optional[Tuple[float, ...]]       # scene box (lo, hi) or None
    near: Optional[float]
    far: Optional[float]
    dt: float
    grid_box: Optional[Tuple[float, ...]] = None
    grid_res: Optional[Tuple[int, int, int]] = None
    occ: Optional[np.ndarray] = None         # bool [rx, ry, rz] or None: no grid
    tags: Tuple[str, ...] = ()

    @property
    def n_rays(self):
        return self.origins.shape[0]


def pack_bits(occ: np.ndarray) -> np.ndarray:
    """bool cells, C order -> int32 words, bit (idx & 31) of word (idx >> 5); the last word zero-padded."""
    flat = np.asarray(occ, dtype=bool).reshape(-1)
    words = np.zeros((flat.size + 31) // 32, dtype=np.uint32)
    for idx in np.flatnonzero(flat):
        words[idx >> 5] |= np.uint32(1) << np.uint32(idx & 31)
    return words.view(np.int32)


# --------------------------------------------------------------------------------------------------------------------
# the reference: float64, from the definition
# --------------------------------------------------------------------------------------------------------------------

def ray_range64(o, d, scene, near, far):
    """(t_min, t_max) of one ray in float64, or None for a miss."""
    o = [float(v) for v in o]
    d = [float(v) for v in d]
    lo, hi = -math.inf, math.inf
    if scene is not None:
        for q in range(3):
            blo, bhi = float(scene[q]), float(scene[3 + q])
            if d[q] == 0.0:                       # +0.0 and -0.0
                if not (blo <= o[q] < bhi):
                    return None
                continue
            t0, t1 = (blo - o[q]) / d[q], (bhi - o[q]) / d[q]
            lo, hi = max(lo, min(t0, t1)), min(hi, max(t0, t1))
        if hi < max(lo, 0.0):
            return None
    t_min = max(lo, 0.0)
    if near is not None:
        t_min = max(t_min, float(near))
    t_max = hi if far is None else min(hi, float(far))
    if not math.isfinite(t_max):
        raise ValueError("march64: neither a box nor a far plane bounds the ray")
    return t_min, t_max


def cell64(pos, box, res):
    """pos [n, 3] float64 -> (idx int64 [n], inside bool [n], face [n, 3], outside_by [n], u [n, 3]).  `face`: world-space distance to
    the nearest plane lo + j cell, j = 0 .. res (cell faces and grid faces), per axis; `outside_by`: how far outside the grid box the
    point lies (0 inside), largest over the axes."""
    n = pos.shape[0]
    idx = np.zeros(n, dtype=np.int64)
    inside = np.ones(n, dtype=bool)
    face, us = np.full((n, 3), np.inf), np.zeros((n, 3))
    outside_by = np.zeros(n)
    for q in range(3):
        lo, hi, r = float(box[q]), float(box[3 + q]), int(res[q])
        u = (pos[:, q] - lo) / (hi - lo)
        inside &= (u >= 0.0) & (u < 1.0)
        c = np.minimum(np.floor(u * r), r - 1)
        idx = idx * r + np.maximum(c, 0).astype(np.int64)
        cell = (hi - lo) / r
        j = np.clip(np.rint(u * r), 0, r)
        face[:, q], us[:, q] = np.abs(pos[:, q] - (lo + j * cell)), u
        outside_by = np.maximum(outside_by, np.maximum(np.maximum(lo - pos[:, q], pos[:, q] - hi), 0.0))
    return idx, inside, face, outside_by, us


@dataclass
class March:
    """Candidate steps of every ray, ray-sorted: the steps whose mid-point is < t_max, and `beyond` more per ray behind them."""
    t_min: np.ndarray          # [R] float64 (nan: miss)
    t_max: np.ndarray
    ray: np.ndarray            # [m] int64
    k: np.ndarray              # [m] int64
    ts: np.ndarray             # [m] float64
    te: np.ndarray
    tm: np.ndarray             # mid-point parameter
    pos: np.ndarray            # [m, 3] mid-point position
    in_range: np.ndarray       # tm < t_max
    keep: np.ndarray           # in_range and (no grid, or inside an occupied cell)
    m_tmax: np.ndarray         # t_max - tm (signed)
    m_face: np.ndarray         # distance to the nearest cell / grid face plane (inf without a grid)
    face_axes: np.ndarray      # [m, 3] the same per axis
    u: np.ndarray              # [m, 3] grid coordinate (nan without a grid)
    outside_by: np.ndarray     # distance outside the grid box (0 inside or without a grid)
    n_rays: int

    def packed(self):
        """(ray_indices int32, t_starts, t_ends, mid-points - all float64 -, offsets int64 [R + 1]) of the kept steps."""
        s = self.keep
        counts = np.bincount(self.ray[s], minlength=self.n_rays)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return self.ray[s].astype(np.int32), self.ts[s], self.te[s], self.pos[s], offsets


def march64(p: Problem, beyond: int = 0) -> March:
    R = p.n_rays
    t_min, t_max = np.full(R, np.nan), np.full(R, np.nan)
    cols = {n: [] for n in ("ray", "k", "ts", "te", "tm", "pos", "in_range")}
    dt = float(p.dt)
    for r in range(R):
        o, d = p.origins[r].astype(np.float64), p.dirs[r].astype(np.float64)
        rng = ray_range64(o, d, p.scene, p.near, p.far)
        if rng is None:
            continue
        t_min[r], t_max[r] = rng
        n = max(0, int(math.ceil((rng[1] - rng[0]) / dt))) + 2
        k = np.arange(n, dtype=np.int64)
        ts, te = rng[0] + k * dt, rng[0] + (k + 1) * dt
        tm = 0.5 * (ts + te)
        count = int((tm < rng[1]).sum())
        assert count <= n - 1 and bool((tm[:count] < rng[1]).all())          # a prefix, and the estimate covers it
        m = count + beyond
        k = np.arange(m, dtype=np.int64)
        ts, te = rng[0] + k * dt, rng[0] + (k + 1) * dt
        tm = 0.5 * (ts + te)
        cols["ray"].append(np.full(m, r, dtype=np.int64)); cols["k"].append(k); cols["ts"].append(ts); cols["te"].append(te)
        cols["tm"].append(tm); cols["pos"].append(o[None, :] + d[None, :] * tm[:, None]); cols["in_range"].append(tm < rng[1])
    cat = lambda name, shape, dtype: np.concatenate(cols[name]) if cols[name] else np.zeros(shape, dtype=dtype)
    ray, k = cat("ray", 0, np.int64), cat("k", 0, np.int64)
    ts, te, tm = cat("ts", 0, np.float64), cat("te", 0, np.float64), cat("tm", 0, np.float64)
    pos, in_range = cat("pos", (0, 3), np.float64), cat("in_range", 0, bool)
    if p.occ is not None:
        idx, inside, face, outside_by, u = cell64(pos, p.grid_box, p.grid_res)
        words = pack_bits(p.occ).view(np.uint32)
        bit = ((words[idx >> 5] >> (idx & 31).astype(np.uint32)) & 1).astype(bool)
        keep = in_range & inside & bit
    else:
        face, outside_by, keep, u = np.full((ray.size, 3), np.inf), np.zeros(ray.size), in_range.copy(), np.full((ray.size, 3), np.nan)
    return March(t_min, t_max, ray, k, ts, te, tm, pos, in_range, keep, t_max[ray] - tm, face.min(1), face, u, outside_by, R)


# --------------------------------------------------------------------------------------------------------------------
# NOT the reference: the kernels' arithmetic, one rounded fp32 operation at a time (np.float32 arrays round every operation).
# It shows that the exact problems are exact, measures what fp32 costs on the general ones, and predicts the per-ray counts.
# (No fused multiply-add: the kernels round t_min + k dt and o + d m in two steps - add_rn, mul_rn in afx_kernels_grid.hip.)
# --------------------------------------------------------------------------------------------------------------------

def count32(t_min, t_max, dt):
    """march_range's step count: ceil((t_max - t_min) / dt), then the two mid-point corrections.  float32 arrays -> int64."""
    t_min, t_max, dt = np.asarray(t_min, F32), np.asarray(t_max, F32), F32(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        ns = np.ceil((t_max - t_min) / dt)
    ns = np.where(ns > 0, ns, F32(0))
    n = np.where(t_min >= F32(1e10), 0, np.minimum(ns, F32(2.0e9))).astype(np.int64)

    def mid(k):
        ts = t_min + k.astype(F32) * dt
        return (ts + (ts + dt)) * F32(0.5)

    while True:
        dec = (n > 0) & ~(mid(n - 1) < t_max)
        if not dec.any():
            break
        n = n - dec
    live = t_min < F32(1e10)
    for _ in range(2):
        live = live & (mid(n) < t_max)
        n = n + live
    return n


def range32(p: Problem):
    """(t_min, t_max) float32 [R] as march_range forms them: reciprocal, then products; 1e-12 in place of a zero component; 1e10 for a miss."""
    o, d = p.origins.astype(F32), p.dirs.astype(F32)
    R = o.shape[0]
    t_min, t_max = np.zeros(R, F32), np.full(R, 1e10, F32)
    if p.scene is not None:
        box = np.asarray(p.scene, F32)
        lo, hi = np.full(R, -np.inf, F32), np.full(R, np.inf, F32)
        for q in range(3):
            inv = F32(1.0) / np.where(d[:, q] == 0, F32(1e-12), d[:, q])
            t0, t1 = (box[q] - o[:, q]) * inv, (box[3 + q] - o[:, q]) * inv
            lo, hi = np.maximum(lo, np.minimum(t0, t1)), np.minimum(hi, np.maximum(t0, t1))
        miss = hi < np.maximum(lo, F32(0))
        t_min = np.where(miss, F32(1e10), np.maximum(lo, F32(0)))
        t_max = np.where(miss, F32(1e10), hi)
    if p.near is not None:
        t_min = np.maximum(t_min, F32(p.near))
    if p.far is not None:
        t_max = np.minimum(t_max, F32(p.far))
    return t_min.astype(F32), t_max.astype(F32)


def march32(p: Problem):
    """-> (ray_indices int32, t_starts, t_ends float32, mid-points float32 [n, 3], offsets int64, t_min float32 [R], decision points
    float32 [n, 3]).  Mid-points as k_march_write writes them, o + d (ts + te) / 2; the decision points are march_keep's
    o + d ((ts + te) 0.5)."""
    o, d = p.origins.astype(F32), p.dirs.astype(F32)
    t_min, t_max = range32(p)
    counts = count32(t_min, t_max, p.dt)
    dt = F32(p.dt)
    if p.occ is not None:
        words = pack_bits(p.occ).view(np.uint32)
        glo, ghi = np.asarray(p.grid_box[:3], F32), np.asarray(p.grid_box[3:], F32)
    ri, tss, tes, mids, dec, kept = [], [], [], [], [], np.zeros(p.n_rays, np.int64)
    for r in range(p.n_rays):
        k = np.arange(counts[r]).astype(F32)
        ts = t_min[r] + k * dt
        te = ts + dt
        m = (ts + te) * F32(0.5)
        pk = o[r][None, :] + d[r][None, :] * m[:, None]
        keep = np.ones(k.size, dtype=bool)
        if p.occ is not None:
            idx = np.zeros(k.size, dtype=np.int64)
            for q in range(3):
                u = (pk[:, q] - glo[q]) / (ghi[q] - glo[q])
                keep &= (u >= 0) & (u < 1)
                c = np.clip(np.floor(u * F32(p.grid_res[q])).astype(np.int64), 0, p.grid_res[q] - 1)
                idx = idx * p.grid_res[q] + c
            keep &= ((words[idx >> 5] >> (idx & 31).astype(np.uint32)) & 1).astype(bool)
        ts, te = ts[keep], te[keep]
        kept[r] = ts.size
        ri.append(np.full(ts.size, r, np.int32)); tss.append(ts); tes.append(te); dec.append(pk[keep])
        mids.append(o[r][None, :] + (d[r][None, :] * (ts + te)[:, None]) / F32(2.0))
    offsets = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    return (np.concatenate(ri), np.concatenate(tss).astype(F32), np.concatenate(tes).astype(F32), np.concatenate(mids).astype(F32).reshape(-1, 3),
            offsets, t_min, np.concatenate(dec).astype(F32).reshape(-1, 3))


# --------------------------------------------------------------------------------------------------------------------
# (a) exact problems: every number dyadic, so that no fp32 operation rounds
# --------------------------------------------------------------------------------------------------------------------

SCENE_A = (-64.0, -32.0, -64.0, 64.0, 96.0, 64.0)
GRID_INNER = (-32.0, 0.0, -32.0, 32.0, 64.0, 32.0)           # strictly inside the scene box
GRID_PARTIAL = (0.0, 32.0, 0.0, 128.0, 160.0, 128.0)         # overlaps the scene box partly
DIRS_A = [(0, 0, -1), (0, 0, 1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (-0.0, 0, 1), (1, -1, 0), (1, -1, 0.5), (-0.5, 1, 1)]
NEAR_FAR_A = [(None, None), (38.0, 150.0), (36.25, 100.5), (120.0, 60.0), (None, 20.0), (37.0, None), (None, 57.0)]


def exact_rays():
    """Rays from outside each of the six faces, from inside, from a face, along faces and edges, through corners.  [R, 3] float32 twice."""
    o, d = [], []
    targets = [(1.0, 10.0, 3.0), (0.5, 31.5, -7.0), (0.0, 32.0, 0.0)]      # inside the box; the last lies on cell faces of (16, 12, 20)
    for dv in DIRS_A:
        for tg in targets:
            for s in (0.0, 40.0, 200.0):                                      # inside, (mostly) inside, outside
                o.append(tuple(t - c * s for t, c in zip(tg, dv))); d.append(dv)
    special = [
        ((1, 10, 101), (0, 0, -1)), ((1, 10, 100), (0, 0, -1)), ((1, 10, 1), (0, 0, -1)), ((1, 1, 3), (0, -1, 0)), ((1, 10, 3), (-1, 0, 0)),
        # exactly on a face: entering, leaving
        ((1, 10, 64), (0, 0, -1)), ((1, 10, 64), (0, 0, 1)), ((-64, 10, 3), (1, 0, 0)), ((1, 96, 3), (0, -1, 0)), ((1, -32, 3), (0, -1, 0)),
        # on a face, zero component along it: the lower face grazes, the upper face misses
        ((1, 10, -64), (1, 0, 0)), ((1, 10, 64), (1, 0, 0)), ((1, -32, 3), (0, 0, 1)), ((1, 96, 3), (0, 0, 1)), ((-64, 10, 3), (0, 1, 0)),
        ((64, 10, 3), (0, 1, 0)), ((-100, 10, -64), (1, 0, 0)), ((-100, 10, 64), (1, 0, 0)), ((1, 10, -64), (-0.0, 1, 0)),
        # one grid's faces with a zero component (GRID_INNER): inside the scene box, on the grid's lower / upper face
        ((-50, 10, -32), (1, 0, 0)), ((-50, 10, 32), (1, 0, 0)), ((1, 0, 50), (0, 0, -1)), ((1, 64, 50), (0, 0, -1)),
        # exactly along an edge: lower-lower grazes, any upper face misses
        ((-100, -32, -64), (1, 0, 0)), ((-100, 96, 64), (1, 0, 0)), ((-100, -32, 64), (1, 0, 0)), ((-64, -100, -64), (0, 1, 0)),
        ((64, -100, 3), (0, 1, 0)), ((-64, -32, 100), (0, 0, -1)),
        # exactly through a corner or an edge: leaving through it from inside, touching it from outside
        ((24, 8, 44), (1, -1, 0.5)), ((-44, 56, 24), (-0.5, 1, 1)), ((24, 8, 3), (1, -1, 0)), ((-104, 8, 3), (1, -1, 0)),
        ((-104, 8, 44), (1, -1, 0.5)), ((-144, 48, -104), (1, -1, 0.5)), ((-24, -72, -104), (-0.5, 1, 1)),
        # misses: beside the box, behind the ray
        ((200, 10, 100), (0, 0, -1)), ((1, 10, 100), (0, 0, 1)), ((1, 200, 3), (1, -1, 0)),
    ]
    for ov, dv in special:
        o.append(ov); d.append(dv)
    return np.array(o, dtype=F32), np.array(d, dtype=F32)


def occupancy(kind: str, res, seed: int = 0):
    if kind == "all":
        return np.ones(res, dtype=bool)
    if kind == "none":
        return np.zeros(res, dtype=bool)
    if kind == "checker":
        i, j, k = np.indices(res)
        return ((i + j + k) % 2) == 0
    if kind == "fill30":
        return np.random.default_rng(1000 + seed).random(res) < 0.3
    raise ValueError(kind)


def exact_problems():
    """Grids x occupancies, each with two of the (near, far, dt) settings, over the rays of exact_rays()."""
    o, d = exact_rays()
    grids = [("nogrid", None, None, ("all",)),
             ("g111", SCENE_A, (1, 1, 1), ("all", "none")),
             ("g357", SCENE_A, (3, 5, 7), ("all", "none", "checker", "fill30")),
             ("g161220", SCENE_A, (16, 12, 20), ("all", "none", "checker", "fill30")),
             ("inner", GRID_INNER, (16, 12, 20), ("all", "checker", "fill30")),
             ("partial357", GRID_PARTIAL, (3, 5, 7), ("all", "checker", "fill30")),
             ("partial161220", GRID_PARTIAL, (16, 12, 20), ("all", "fill30"))]
    out, i = [], 0
    for gname, box, res, occs in grids:
        for kind in occs:
            for rep in range(2 if gname != "nogrid" else len(NEAR_FAR_A)):
                near, far = NEAR_FAR_A[i % len(NEAR_FAR_A)]
                dt = 0.5 if (near is not None and near != int(near)) else (2.0, 0.5)[(i // len(NEAR_FAR_A)) % 2]
                occ = None if box is None else occupancy(kind, res, seed=i)
                out.append(Problem(f"{gname}-{kind}-near{near}-far{far}-dt{dt}", o, d, SCENE_A, near, far, dt, box, res, occ, (gname, kind)))
                i += 1
    ties = [("inner", GRID_INNER, (16, 12, 20), "all", 38.0, 150.0, 2.0),            # mid-points on the grid's lower and upper face
            ("g161220", SCENE_A, (16, 12, 20), "checker", None, None, 2.0),          # mid-points on interior cell faces, every axis
            ("g161220", SCENE_A, (16, 12, 20), "all", 37.0, None, 2.0),              # last mid-point on t_max = the box's exit
            ("g357", SCENE_A, (3, 5, 7), "all", None, 57.0, 2.0),                    # last mid-point on t_max = far
            ("nogrid", None, None, "all", None, 57.0, 2.0)]
    for gname, box, res, kind, near, far, dt in ties:
        occ = None if box is None else occupancy(kind, res, seed=len(out))
        out.append(Problem(f"tie-{gname}-{kind}-near{near}-far{far}-dt{dt}", o, d, SCENE_A, near, far, dt, box, res, occ, (gname, kind)))
    return out


# --------------------------------------------------------------------------------------------------------------------
# (b) chunk and block edges: rays along -z with exactly the wanted number of steps in range
# --------------------------------------------------------------------------------------------------------------------

STEP_COUNTS_B = (0, 1, 63, 64, 65, 127, 128, 129, 257)
RAY_COUNTS_B = (1, 3, 4, 5, 1025)
KEPT_B = ("all", "none", "alternate", "first", "last")
RES_B = (1, 1, 512)
NEAR_B, FAR_B, DT_B = 86.0, 600.0, 2.0


def chunk_counts(n_rays: int):
    return [STEP_COUNTS_B[(i + n_rays + 7) % len(STEP_COUNTS_B)] for i in range(n_rays)]      # one ray: 257 steps, five passes


def chunk_clamped(n_rays: int):
    """Rays of chunk_problem whose box entry lies in front of `near`: every second one of those with 257 steps."""
    return [c == 257 and i % 2 == 1 for i, c in enumerate(chunk_counts(n_rays))]


def chunk_problem(n_rays: int, kept: str) -> Problem:
    """d = (0, 0, -1/8): the box is 1024 units of t deep, 512 steps of dt = 2, and step k of a ray has its mid-point in cell 511 - k of
    the (1, 1, 512) grid (z = 64 - 1/8 - k/4).  A ray that enters at t = e has c steps before far = 600 iff e = 600 - 2 c, and near = 86 is
    the entry of the rays with 257 steps.  The clamped ones among them (chunk_clamped) enter at t = 70 and start at near: 257 steps as well,
    step k in cell 503 - k."""
    counts = chunk_counts(n_rays)
    o = np.zeros((n_rays, 3), dtype=F32)
    for i, (c, clamped) in enumerate(zip(counts, chunk_clamped(n_rays))):
        e = NEAR_B - 16.0 if clamped else FAR_B - DT_B * c
        o[i] = (float(i % 101) - 50.0, float(i % 89) - 20.0, 64.0 + e / 8.0)
    d = np.tile(np.array([0.0, 0.0, -0.125], dtype=F32), (n_rays, 1))
    occ = np.zeros(RES_B, dtype=bool)
    for k in chunk_kept_steps(n_rays, kept):
        occ[0, 0, 511 - k] = True
    return Problem(f"chunk-r{n_rays}-{kept}", o, d, SCENE_A, NEAR_B, FAR_B, DT_B, SCENE_A, RES_B, occ, (kept,))


def chunk_kept_steps(n_rays: int, kept: str):
    """The steps k (of a ray that is not clamped) whose cell is occupied."""
    counts = chunk_counts(n_rays)
    return {"all": list(range(512)), "none": [], "alternate": list(range(0, 512, 2)), "first": [0],
            "last": sorted({c - 1 for c in counts if c > 0})}[kept]


# --------------------------------------------------------------------------------------------------------------------
# (c) general rays from every side
# --------------------------------------------------------------------------------------------------------------------

SCENE_C = (-100.0, -80.0, -100.0, 100.0, 120.0, 90.0)
GRID_C = (-70.0, -90.0, -60.0, 90.0, 70.0, 110.0)
RES_C = (16, 12, 20)
SETTINGS_C = ((2.5, 1300.0, 1700.0), (0.75, None, None), (7.0, 1450.0, 1520.0))
MARGIN_C = 4e-3            # m of the margin rule, world units (DESIGN: "The march against an independent reference")
UNDECIDED_CAP_C = 0.01


def general_rays(seed: int = 11):
    """384 rays from a sphere of radius 1500 about (0, 10, 0), aimed into 0.9 x the scene box; 32 from inside the box; 32 that miss."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(SCENE_C[:3]), np.array(SCENE_C[3:])
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    n = 384
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    src = np.array([0.0, 10.0, 0.0]) + 1500.0 * v
    aim = mid + 0.9 * half * rng.uniform(-1, 1, (n, 3))
    o_in = mid + 0.95 * half * rng.uniform(-1, 1, (32, 3))
    d_in = rng.standard_normal((32, 3))
    v2 = rng.standard_normal((32, 3))
    v2 /= np.linalg.norm(v2, axis=1, keepdims=True)
    o_miss = np.array([0.0, 10.0, 0.0]) + 1500.0 * v2
    w = rng.standard_normal((32, 3))
    w -= (w * v2).sum(1, keepdims=True) * v2                                   # aimed 400 units beside the centre
    aim_miss = mid + 400.0 * w / np.linalg.norm(w, axis=1, keepdims=True)
    o = np.concatenate([src, o_in, o_miss])
    d = np.concatenate([aim - src, d_in, aim_miss - o_miss])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F32), d.astype(F32)


def general_problems():
    o, d = general_rays()
    occ = occupancy("fill30", RES_C, seed=77)
    out = []
    for dt, near, far in SETTINGS_C:
        for use_grid in (False, True):
            out.append(Problem(f"general-dt{dt}-near{near}-far{far}-{'grid' if use_grid else 'nogrid'}", o, d, SCENE_C, near, far, dt,
                               GRID_C if use_grid else None, RES_C if use_grid else None, occ if use_grid else None))
    return out


def decide(m: March, margin: float):
    """Per candidate step of march64(p, beyond=...): +1 decided in, -1 decided out, 0 undecided.  Undecided: the mid-point within
    `margin` of t_max, or - where the range admits the step and there is a grid - the position within `margin` of a cell face or grid
    face plane, unless it lies farther than `margin` outside the grid box."""
    out = np.zeros(m.ray.size, dtype=np.int64)
    clear = np.abs(m.m_tmax) > margin
    out[clear & ~m.in_range] = -1
    inr = clear & m.in_range
    out[inr & (m.outside_by > margin)] = -1
    settled = inr & ~(m.outside_by > margin) & (m.m_face > margin)
    out[settled] = np.where(m.keep[settled], 1, -1)
    return out


# --------------------------------------------------------------------------------------------------------------------
# (d) the per-ray bound: (near, far, dt) triples and the t_min windows
# --------------------------------------------------------------------------------------------------------------------

NAMED_TRIPLES = ((1400.0, 1600.0, 200.0 / 300), (1400.0, 1600.0, 200.0 / 128), (10.0, 19.7, 9.7 / 37), (0.5, 3.25, 2.75 / 64),
                 (0.0, 130.0, 130.0 / 64.5), (1399.9, 1600.1, 2.5))


def half_step_triples(seed: int = 3):
    """(near, far, dt) with (far - near) / dt = N + 0.5 for N = 3 .. 400, as fp32 numbers."""
    rng = np.random.default_rng(seed)
    out = []
    for n in range(3, 401):
        near = float(F32(rng.uniform(0.0, 2000.0)))
        dt = float(F32(rng.uniform(0.01, 5.0)))
        out.append((near, float(F32(near + (n + 0.5) * dt)), dt))
    return out


def bound_triples():
    return [tuple(float(F32(v)) for v in t) for t in NAMED_TRIPLES] + half_step_triples()


def _ulps(x, lo, hi):
    """the fp32 numbers x + lo ulps .. x + hi ulps"""
    x = F32(x)
    out = [x]
    for _ in range(hi):
        out.append(np.nextafter(out[-1], F32(np.inf)))
    down = x
    for _ in range(-lo):
        down = np.nextafter(down, F32(-np.inf))
        out.append(down)
    return out


def tmin_windows(near: float, far: float, dt: float, n_random: int, seed: int = 0):
    """fp32 t_min values in [max(near, 0), far]: 0 .. 8 ulps above near, within 8 ulps of near + j dt / 2 (j = 0 .. 6), n_random random."""
    lo = F32(max(near, 0.0))
    vals = _ulps(lo, 0, 8)
    for j in range(7):
        vals += _ulps(F32(near + j * dt / 2.0), -8, 8)
    rng = np.random.default_rng([seed, int(F32(dt).view(np.uint32)), int(F32(near).view(np.uint32))])
    vals = np.concatenate([np.array(vals, dtype=F32), rng.uniform(float(lo), far, n_random).astype(F32)])
    return vals[(vals >= lo) & (vals <= F32(far))]


# --------------------------------------------------------------------------------------------------------------------
# comparing a packed march with the reference
# --------------------------------------------------------------------------------------------------------------------

def _match(m: March, dt: float, ri, ts):
    """Index into m's candidates of every given step, by k = round((t_start - t_min64) / dt); -1 where the reference has no such candidate
    (a missed ray, or a step farther behind t_max than m holds)."""
    ri = np.asarray(ri, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        k = np.rint((np.asarray(ts, dtype=np.float64) - m.t_min[ri]) / dt)
    k = np.where(np.isfinite(k), k, -1).astype(np.int64)
    big = int(m.k.max()) + 2 if m.k.size else 2
    keys = m.ray * big + m.k                                                      # ascending: ray-sorted, k ascending within a ray
    want = ri * big + np.clip(k, -1, big - 1)
    at = np.searchsorted(keys, want)
    at = np.where(at < keys.size, at, 0)
    found = (keys.size > 0) & (keys[at] == want) & (k >= 0)
    return np.where(found, at, -1)


def fp32_distance(p: Problem, m: March):
    """Largest distance of the fp32 emulation from the reference over its steps: (in t: t_starts and t_ends; in position: the written
    mid-points and march_keep's decision points)."""
    ri, ts, te, mid, _, _, dec = march32(p)
    at = _match(m, p.dt, ri, ts)
    ok = at >= 0
    if not ok.any():
        return 0.0, 0.0
    a = at[ok]
    d_t = max(np.abs(ts[ok] - m.ts[a]).max(), np.abs(te[ok] - m.te[a]).max())
    d_p = max(np.abs(mid[ok] - m.pos[a]).max(), np.abs(dec[ok] - m.pos[a]).max())
    return float(d_t), float(d_p)


def check_margin_rule(p: Problem, m: March, margin: float, bar: float, ri, ts, te, mid=None):
    """The margin rule of the general problems, on a packed march (ri, ts, te[, mid]) of p; m = march64(p, beyond >= 1).  Every decided-in
    step present, every decided-out step absent, floats of the present steps within `bar` of the fp64 values.
    -> {"candidates", "undecided", "share", "max_dt", "max_dpos"}; AssertionError otherwise."""
    status = decide(m, margin)
    at = _match(m, p.dt, ri, ts)
    stray = at < 0
    assert not stray.any(), (p.name, "steps the reference has no candidate for", int(stray.sum()), np.asarray(ri)[stray][:5], np.asarray(ts)[stray][:5])
    assert np.unique(at).size == at.size, (p.name, "a step appears twice")
    wrong = status[at] == -1
    assert not wrong.any(), (p.name, "decided-out steps present", int(wrong.sum()), m.ray[at[wrong]][:5], m.k[at[wrong]][:5])
    present = np.zeros(m.ray.size, dtype=bool)
    present[at] = True
    lost = (status == 1) & ~present
    assert not lost.any(), (p.name, "decided-in steps absent", int(lost.sum()), m.ray[lost][:5], m.k[lost][:5])
    max_dt = max(np.abs(np.asarray(ts, np.float64) - m.ts[at]).max(), np.abs(np.asarray(te, np.float64) - m.te[at]).max()) if at.size else 0.0
    max_dp = float(np.abs(np.asarray(mid, np.float64) - m.pos[at]).max()) if (mid is not None and at.size) else 0.0
    assert max_dt <= bar and max_dp <= bar, (p.name, "floats farther than the bar from the fp64 values", max_dt, max_dp, bar)
    cand = int(m.in_range.sum())
    und = int((status == 0).sum())
    return {"candidates": cand, "undecided": und, "share": und / max(cand, 1), "max_dt": float(max_dt), "max_dpos": max_dp}


@functools.lru_cache(maxsize=None)
def general_bar() -> float:
    """The bar of the general problems: 4 x the largest distance of the fp32 emulation from the reference, over t and position, over all
    of them (4: the kernels may differ from the emulation by an ulp per operation)."""
    return 4.0 * max(max(fp32_distance(p, march64(p, beyond=3))) for p in general_problems())
