"""A NumPy restatement of the occupancy-grid update (afx_grid_points, afx_grid_update, afx_grid_binarize, afx_grid_pack) and the seeded
problems the tests run it on.  Independent of the library and of oracle/angio_oracle.py: every fp32 operation is one NumPy float32 ufunc
call, rounded on its own, so the kernels must equal it on the bits (tests/test_gpu_grid_update.py); tests/test_grid_update_cpu.py asserts
what the problems claim."""
import math
from collections import namedtuple

import numpy as np

from test_grid_refresh_cpu import philox_u24

F32 = np.float32

GRIDS = [(1, 1, 1), (5, 3, 7), (257, 1, 1), (9, 7, 33), (16, 16, 16), (37, 29, 23)]
RAGGED = [r for r in GRIDS if (r[0] * r[1] * r[2]) % 32]
BOXES = [[-100.0, -80.0, -100.0, 100.0, 120.0, 90.0], [3.5, -7.25, 1400.0, 11.0, 2.5, 1600.5]]      # no extent is a power of two
DECAYS = [0.95, 0.5]
TINY = F32(2.0 ** -140)      # a denormal
TOP = F32(1.0 - 2.0 ** -24)      # the largest jitter below 1


def num_cells(res):
    return res[0] * res[1] * res[2]


def bits_of(a):
    """The bit patterns of an fp32 array: floats are compared as these, so that -0.0 != +0.0 and a NaN equals itself."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


# --- the restatement -------------------------------------------------------------------------------------------------------------------------

def _x_of(cells, jitter, res):
    c = np.asarray(cells, np.int64)
    r0, r1, r2 = (int(v) for v in res)
    ijk = np.stack([c // (r1 * r2), (c // r2) % r1, c % r2], 1).astype(F32)
    u = np.asarray(jitter)
    assert u.dtype == np.float32 and u.shape == ijk.shape
    s = ijk + u                                               # fl(ijk + u)
    return s / np.array([r0, r1, r2], F32)                    # fl(. / res)


def points(cells, jitter, aabb, res):
    """p = fl(fl(x fl(hi - lo)) + lo), x = fl(fl(ijk + u) / res), ijk from the flat index; four roundings, fp32 [n, 3]."""
    x = _x_of(cells, jitter, res)
    lo, hi = np.array(aabb[:3], F32), np.array(aabb[3:], F32)
    ext = hi - lo
    prod = x * ext
    out = prod + lo
    assert x.dtype == ext.dtype == prod.dtype == out.dtype == np.float32
    return out


def points_fused(cells, jitter, aabb, res):
    """What a contracted kernel computes: the fp64 product and sum of the same x and extent (the product of two fp32 numbers is exact in
    fp64), rounded to fp32 once."""
    x = _x_of(cells, jitter, res).astype(np.float64)
    lo, hi = np.array(aabb[:3], F32), np.array(aabb[3:], F32)
    return (x * (hi - lo).astype(np.float64) + lo.astype(np.float64)).astype(F32)


def philox_jitter(seed, stream, n):
    """u[i, a] = philox_u24(seed, stream, 3 i + a) / 2^24 (exact in fp32)."""
    return (philox_u24(seed, stream, 3 * n).astype(F32) * F32(2.0 ** -24)).reshape(n, 3)


def update(occs, cells, occ_new, decay):
    """Every selected cell drops to fl(occs_before[c] decay), once however often it is drawn, +0 when that is not above 0; then the maximum
    with every draw v > 0 of the cell.  Draws that are 0, -0.0, negative or NaN change nothing; unselected cells keep their bits."""
    before = np.asarray(occs)
    v = np.asarray(occ_new).reshape(-1)
    assert before.dtype == np.float32 and v.dtype == np.float32
    c = np.arange(v.size) if cells is None else np.asarray(cells, np.int64)
    assert c.shape == v.shape and (c.size == 0 or (c.min() >= 0 and c.max() < before.size))
    out = before.copy()
    d = before[c] * F32(decay)
    with np.errstate(invalid="ignore"):
        out[c] = np.where(d > 0, d, F32(0.0))
        take = v > 0
    np.maximum.at(out, c[take], v[take])
    return out


def mean64(occs):
    return math.fsum(np.asarray(occs, np.float64).tolist()) / np.asarray(occs).size


def threshold(occs, occ_thre):
    """(thr, mean): mean = fp32(exact fp64 sum / n), thr = mean if mean < fp32(occ_thre) else fp32(occ_thre)."""
    mean, t = F32(mean64(occs)), F32(occ_thre)
    return (mean if mean < t else t), mean


def pack(mask_bytes):
    """Bit b of word w = bytes[32 w + b] != 0; the bits past the last cell are 0.  -> uint32 [(n + 31) // 32]"""
    m = np.asarray(mask_bytes).reshape(-1) != 0
    full = np.zeros((m.size + 31) // 32 * 32, np.uint64)
    full[:m.size] = m
    return (full.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def binarize(occs, occ_thre):
    """(bytes, words): bytes = occs > thr (strict) as 0 / 1, words = pack(bytes)."""
    thr, _ = threshold(occs, occ_thre)
    b = (np.asarray(occs) > thr).astype(np.uint8)
    return b, pack(b)


def decision_counts(occs, occ_thre):
    """(on, off, ties) of the restatement: cells above the threshold, not above it, and exactly on it (ties are off)."""
    thr, _ = threshold(occs, occ_thre)
    o = np.asarray(occs)
    return int((o > thr).sum()), int((~(o > thr)).sum()), int((o == thr).sum())


# --- the problems ----------------------------------------------------------------------------------------------------------------------------

def jitter_problem(n, seed):
    """fp32 jitter [n, 3]: multiples of 2^-24 in [0, 1); row 1 (mod 5) is exactly 0 and row 2 (mod 5) is 1 - 2^-24 on every axis."""
    rng = np.random.default_rng(seed)
    u = (rng.integers(0, 1 << 24, (n, 3)).astype(F32) * F32(2.0 ** -24))
    u[1::5] = 0.0
    u[2::5] = TOP
    return u


def index_list(res, seed=0):
    """About n/2 draws (at least 7, an odd number: never a multiple of 256), unsorted, with duplicates, all in range."""
    n = num_cells(res)
    rng = np.random.default_rng(1000 + seed + n)
    length = max(7, (n // 2) | 1)
    c = rng.integers(0, n, length)
    c[length // 2:length // 2 + 3] = c[:3]      # duplicates for certain
    return c.astype(np.int64)


UpdateProblem = namedtuple("UpdateProblem", "res occs cells occ_new special")


def update_problem(res, seed=0):
    """occupancies, an unsorted index list of about n/2 draws and their values, with the special cells and draws of DESIGN 1.19 planted at
    increasing positions (so that the order of a cell's draws in the list is the one written here).  special: name -> cell."""
    n = num_cells(res)
    assert n >= 64
    rng = np.random.default_rng(2000 + seed + n)
    perm = rng.permutation(n)
    names = ["twice_down", "twice_up", "thrice_a", "thrice_b", "zero", "negative", "nan", "inf", "tiny_draw", "decayed_wins", "tiny_cell",
             "neg_zero_cell", "neg_zero_draw"]
    special = {k: int(perm[i]) for i, k in enumerate(names)}
    pool = perm[len(names):n - max(n // 8, 1)]      # the cells the random draws come from; the last n/8 of perm are never selected
    occs = (rng.random(n).astype(F32) * (rng.random(n) < 0.7)).astype(F32)
    occs[perm[n - max(n // 8, 1):]] += F32(0.25)      # unselected and non-zero
    length = (n // 2) | 1
    cells = pool[rng.integers(0, pool.size, length)]
    occ_new = (rng.random(length).astype(F32) * F32(0.8)).astype(F32)
    s = special
    planted = [(s["twice_down"], 0.7), (s["twice_up"], 0.2), (s["thrice_a"], 0.1), (s["thrice_b"], 0.9), (s["zero"], 0.0),
               (s["negative"], -0.3), (s["nan"], np.nan), (s["inf"], np.inf), (s["tiny_draw"], TINY), (s["decayed_wins"], 0.1),
               (s["tiny_cell"], 0.0), (s["neg_zero_cell"], 0.25), (s["neg_zero_draw"], -0.0), (s["thrice_a"], 0.9), (s["thrice_b"], 0.1),
               (s["twice_down"], 0.3), (s["twice_up"], 0.6), (s["decayed_wins"], 0.2), (s["thrice_a"], 0.5), (s["thrice_b"], 0.5)]
    pos = np.linspace(0, length - 1, len(planted)).astype(np.int64)
    assert np.unique(pos).size == len(planted)
    for p, (c, v) in zip(pos, planted):
        cells[p], occ_new[p] = c, F32(v)
    occs[s["zero"]], occs[s["negative"]], occs[s["nan"]], occs[s["inf"]] = 0.4, 0.3, 0.2, 0.1
    occs[s["tiny_draw"]] = 0.0
    occs[s["decayed_wins"]] = 0.9
    occs[s["tiny_cell"]] = TINY
    occs[s["neg_zero_cell"]] = -0.0
    occs[s["neg_zero_draw"]] = 0.35
    return UpdateProblem(res, occs, cells.astype(np.int64), occ_new, special)


def oracle_subproblem(p):
    """The update problem without what torch's index_reduce / clamp treat differently or the oracle does not define: the -0.0 cell and the
    NaN, negative, zero (either sign), +inf and 2^-140 draws.  -> (occs, cells, occ_new)"""
    v = p.occ_new
    with np.errstate(invalid="ignore"):
        keep = (v > 0) & np.isfinite(v) & (v != TINY) & (p.cells != p.special["neg_zero_cell"])
    return p.occs, p.cells[keep], v[keep]


def all_cells_draws(n, seed=0):
    """n draws for an update of cells 0 .. n-1: random values with exact zeros, one negative and one NaN among them."""
    rng = np.random.default_rng(3000 + seed + n)
    v = (rng.random(n).astype(F32) * (rng.random(n) < 0.8)).astype(F32)
    if n > 4:
        v[1], v[3] = -0.5, np.nan
    return v


def start_occs(n, seed=0):
    rng = np.random.default_rng(3500 + seed + n)
    return (rng.random(n).astype(F32) * (rng.random(n) < 0.7)).astype(F32)


EXACT_THRESHOLDS = [0.5, 0.125, 0.25]      # the mean (0.25) decides; the threshold decides; both are equal


def exact_binarize_problem(res, seed=0):
    """Multiples of 2^-6 with a total of exactly n / 4: every cell starts at 16/64 and whole units move between the two cells of random
    pairs (half of the pairs stay).  Every fp64 partial sum is then exact in any order and the mean is 0.25."""
    n = num_cells(res)
    assert n > 32
    rng = np.random.default_rng(4000 + seed + n)
    units = np.full(n, 16, np.int64)
    perm = rng.permutation(n)
    a, b = perm[:n // 2], perm[n // 2:2 * (n // 2)]
    t = rng.integers(-8, 9, n // 2) * (rng.random(n // 2) < 0.5)
    t[0], t[1] = 8, 0      # one cell at 8/64 = 0.125 (on the second threshold) and one tie for certain
    units[a] -= t
    units[b] += t
    return (units.astype(F32) * F32(2.0 ** -6)).astype(F32)


RANDOM_THRE = 1e-2
RANDOM_SEED = 0


def random_binarize_problem(res, seed=RANDOM_SEED):
    """U(0, 0.03) in fp32."""
    n = num_cells(res)
    rng = np.random.default_rng(5000 + seed + n)
    return (rng.random(n).astype(F32) * F32(0.03)).astype(F32)


def mean_margin(occs):
    """(margin, bound): the distance of the fp64 mean from the nearest boundary between two fp32 numbers' rounding intervals, and
    n 2^-52 mean - more than any order of an fp64 sum of n non-negative terms can move the mean."""
    m64 = mean64(occs)
    m32 = F32(m64)
    edges = [(float(m32) + float(np.nextafter(m32, F32(s)))) / 2.0 for s in (-np.inf, np.inf)]
    return min(abs(m64 - e) for e in edges), np.asarray(occs).size * 2.0 ** -52 * m64


def pack_problem(res, seed=0):
    """Bytes from {0, 1, 2, 255}."""
    n = num_cells(res)
    rng = np.random.default_rng(6000 + seed + n)
    return rng.choice(np.array([0, 1, 2, 255], np.uint8), n)
