"""The inputs of the many-chunk tests (tests/test_many_chunks_cpu.py, tests/test_gpu_many_chunks.py): the smallest problems at which the
two-level scans of the compaction, labelling and selection kernels hold MORE THAN 1024 PARTIALS, so that each of the 1024 threads of the
scanning workgroup walks a run of per = ceil(nb / 1024) > 1 of them (k_cc_scan, k_cg_scan_chunks, k_iso_scan, k_sel_offsets,
k_grid_occ_scan; the chunked init and mark launches of the thinning), and, kept apart, the cases at exactly 1024 and 1025 partials of
tests/test_gpu_scan_boundary.py and tests/test_scan_boundary_cpu.py.  Not a test module.

Every volume is sparse - three thin capsules from corner to corner, single-voxel specks at density 0.001, the first and the last voxel -
so that the host references stay at a second per call, yet nearly every chunk holds components, end points and one-voxel branches of its
own: every chunk's prefix takes part in the answer."""
import functools
import re
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent.parent / "nerf_for_angiography_amd" / "csrc"
SCAN_THREADS = 1024                 # threads of the one scanning workgroup, one run of partials each
# the chunk constants of the kernels, restated: (source file, value)
CHUNKS = {"CC_CHUNK": ("afx_kernels_metrics.hip", 2048), "SK_CHUNK": ("afx_kernels_metrics.hip", 2048),
          "CG_CHUNK": ("afx_kernels_graph.hip", 2048), "ISO_CHUNK": ("afx_kernels_mesh.hip", 1024),
          "SEL_PER_BLOCK": ("afx_kernels_grid.hip", 1024), "SEL_WORDS": ("afx_kernels_grid.hip", 256)}
CC_CHUNK, SK_CHUNK, CG_CHUNK, ISO_CHUNK, SEL_PER_BLOCK, SEL_WORDS = (CHUNKS[k][1] for k in ("CC_CHUNK", "SK_CHUNK", "CG_CHUNK", "ISO_CHUNK",
                                                                                          "SEL_PER_BLOCK", "SEL_WORDS"))

VOLUMES = {"129x128x128": (129, 128, 128),       # 1 032 chunks of 2048 (per = 2), 2 064 of 1024 (per = 3)
           "3x700x1001": (3, 700, 1001)}         # 1 027 chunks of 2048, the last one ragged; 2 053 of 1024: the last scanning thread's run is short
SPECK_DENSITY = 0.001
CAPSULE_RADIUS = 1.6
GRID_RES = (129, 256, 256)                       # 8 454 144 cells, 264 192 words, 1 032 workgroup totals
GRID_DENSITY = 0.02
GRID_FEW = 1500                                  # occupied cells of the second mask: fewer than either n_draw
GRID_DRAWS = (4096, GRID_RES[0] * GRID_RES[1] * GRID_RES[2] // 4)
SAMPLER_SIZES = (1_050_001, 2_100_001)           # 1 026 chunks (per = 2); 2 051 chunks (per = 3, the last run short)

# The cases of tests/test_gpu_scan_boundary.py, AT the boundary: exactly 1024 partials (per = 1, no scanning thread idle) and 1025 (per = 2,
# the threads from 513 on have empty runs).  Kept apart from VOLUMES and SAMPLER_SIZES, whose entries all exceed 1024 partials.
BOUNDARY_SHAPES = ((128, 128, 128), (4, 513, 1023))       # 1 024 chunks of 2048; 1 025, the last one ragged (no side may exceed 1024)
BOUNDARY_SAMPLER_SIZES = (1024 * 1024, 1024 * 1024 + 1)   # 1 024 and 1 025 blocks of SEL_PER_BLOCK keys
BOUNDARY_RAY_COUNTS = (1023, 1024, 1025, 2049)            # the offsets kernel scans one partial per ray: per = 1, 1, 2 and 3


def _ceil_div(a, b):
    return -(-int(a) // int(b))


def source_constant(name):
    """The value `constexpr int NAME = ...;` has in the kernel source (a product of integers and earlier constants of the same file)."""
    text = (CSRC / CHUNKS[name][0]).read_text()

    def value(n):
        m = re.search(r"constexpr\s+(?:int|unsigned|uint32_t)\s+" + n + r"\s*=\s*([^;]+);", text)
        assert m, f"{n} not found in {CHUNKS[name][0]}"
        out = 1
        for factor in m.group(1).split("*"):
            factor = factor.strip()
            out *= int(factor) if factor.isdigit() else value(factor)
        return out
    return value(name)


# ---- the number of partials the scanning workgroup sees
def partials_volume(n_voxels):
    """components, thinning, graph and pruning: one partial per 2048 voxels"""
    return _ceil_div(n_voxels, CC_CHUNK)


def partials_isosurface(n_points):
    return _ceil_div(n_points, ISO_CHUNK)


def partials_sampler(n_keys):
    return _ceil_div(n_keys, SEL_PER_BLOCK)


def partials_grid(n_cells):
    return _ceil_div(_ceil_div(n_cells, 32), SEL_WORDS)


def run_length(n_partials):
    """per: the partials each scanning thread walks serially"""
    return _ceil_div(n_partials, SCAN_THREADS)


# ---- the volumes
def capsule(shape, a, b, r):
    """The voxels within r of the segment a-b (open grids: no [N, 3] array of coordinates)."""
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = b - a
    t = np.clip(sum((g[q] - a[q]) * d[q] for q in range(3)) / float(d @ d), 0.0, 1.0)
    return sum((g[q] - a[q] - t * d[q]) ** 2 for q in range(3)) <= r * r


def volume(name):
    """The sparse boolean volume `name` of VOLUMES (read-only; built once per process)."""
    return sparse_volume(VOLUMES[name])


@functools.lru_cache(maxsize=None)
def sparse_volume(shape):
    """Capsules along three diagonals, specks, the first and the last voxel, in a volume of `shape` (read-only; built once per process)."""
    hi = [s - 1 for s in shape]
    m = np.random.default_rng(sum(shape)).random(shape) < SPECK_DENSITY
    for a, b in (((0, 0, 0), hi), ((0, hi[1], 0), (hi[0], 0, hi[2])), ((hi[0], 0, 0), (0, hi[1], hi[2]))):      # three of the four diagonals
        m |= capsule(shape, a, b, CAPSULE_RADIUS)
    m.flat[0] = m.flat[-1] = True
    m.setflags(write=False)
    return m


def chunk_occupancy(mask, chunk):
    """bool [chunks]: which chunks of `chunk` consecutive voxels hold foreground"""
    flat = np.zeros(_ceil_div(mask.size, chunk) * chunk, bool)
    flat[:mask.size] = mask.reshape(-1)
    return flat.reshape(-1, chunk).any(axis=1)


# ---- the occupancy grids
@functools.lru_cache(maxsize=None)
def grid_mask(kind):
    """bool [cells] of GRID_RES: "bernoulli" - density 0.02 (more occupied cells than either draw); "few" - GRID_FEW occupied cells spread
    over the whole grid, the first and the last cell among them (the "all of them, in index order" branch)."""
    n = GRID_RES[0] * GRID_RES[1] * GRID_RES[2]
    rng = np.random.default_rng(n)
    if kind == "bernoulli":
        m = rng.random(n) < GRID_DENSITY
    else:
        m = np.zeros(n, bool)
        m[rng.choice(n, GRID_FEW - 2, replace=False)] = True
        m[0] = m[-1] = True
    m.setflags(write=False)
    return m


# ---- the key arrays of the selection
def sampler_keys(n):
    """float32 [n]: log(u) / w keys as the sampler makes them, every 97th one -inf (a zero weight)."""
    rng = np.random.default_rng(n)
    keys = (np.log(np.maximum(rng.random(n), 1e-7)) / (rng.random(n) + 0.05)).astype(np.float32)
    keys[::97] = -np.inf
    return keys


def sampler_ks(n):
    return (1, 5625, n - 3, n)


def tie_keys(n):
    """float32 [n] of 5 values: every k cuts inside a tie class"""
    return np.random.default_rng(n + 5).integers(0, 5, n).astype(np.float32)


def descending_order(keys):
    """The stable descending sort of the keys: the indices by falling key, equal keys by rising index (no NaN among the keys)."""
    return np.argsort(-keys.astype(np.float64), kind="stable")       # (-(-inf) = +inf sorts last)


def topk_reference(keys, k, order=None):
    """The k largest keys, ties to the lowest index, in ascending index order (int64).  order: descending_order(keys), to share one sort."""
    order = descending_order(keys) if order is None else order
    return np.sort(order[:k]).astype(np.int64)
