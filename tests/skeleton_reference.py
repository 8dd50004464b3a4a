"""The yardstick of the skeleton tests (include/afx.h: afx_skeletonize_3d): a sequential NumPy / scipy.ndimage restatement of 8-subfield
parallel thinning to medial curves (Bertrand & Aktouf 1995) with Malandain & Bertrand's (26, 6)-simple points.  Components are counted
by scipy.ndimage.label on 3 x 3 x 3 cubes - no bit tricks, voxels deleted one after another in raster order.

Foreground is 26-connected, background 6-connected, everything beyond the array is background.  A pass:
  1. B = the foreground voxels that have a background 6-neighbour at the start of the pass;
  2. for s = 0..7, subfield s = (i0 & 1) * 4 + (i1 & 1) * 2 + (i2 & 1): every voxel of B in subfield s is deleted when, in the mask as it
     stands, it does not have exactly one foreground 26-neighbour (curve end points stay) and is simple.
Passes repeat until one deletes nothing; that last pass is counted (it is what establishes convergence).

Also here: the 26-component count, the 6-cavity count and the Euler characteristic of a mask, the shapes the tests thin, and the host
computation of the centreline scores."""
import numpy as np
from scipy import ndimage

S26 = np.ones((3, 3, 3), bool)
S6 = ndimage.generate_binary_structure(3, 1)
_D = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1)            # [3, 3, 3, 3]: the offset of every cube position
N26 = np.abs(_D).sum(-1) > 0                                                       # all but the centre
N18 = N26 & (np.abs(_D).sum(-1) <= 2)                                              # without the 8 corners
N6 = np.abs(_D).sum(-1) == 1                                                       # the 6 face neighbours


def cube_of(word):
    """The 3 x 3 x 3 bool cube of a 27-bit neighbourhood word: bit (d0 + 1) * 9 + (d1 + 1) * 3 + (d2 + 1)."""
    return ((int(word) >> np.arange(27)) & 1).astype(bool).reshape(3, 3, 3)


def word_of(cube):
    return int((np.asarray(cube, bool).ravel().astype(np.int64) << np.arange(27)).sum())


def is_simple(cube):
    """(26, 6)-simple: the foreground of the 26-neighbourhood (centre excluded) is exactly one 26-component, and the background of the
    18-neighbourhood holds exactly one 6-component (connectivity inside the 18-neighbourhood) that is 6-adjacent to the centre."""
    cube = np.asarray(cube, bool)
    if ndimage.label(cube & N26, structure=S26)[1] != 1:
        return False
    lab, _ = ndimage.label(~cube & N18, structure=S6)
    return len(set(lab[N6].tolist()) - {0}) == 1


def deletable(cube):
    """The rule of step 2 for a voxel of B: not a curve end point, and simple."""
    cube = np.asarray(cube, bool)
    return int((cube & N26).sum()) != 1 and is_simple(cube)


def border(mask):
    """B: foreground voxels with a background 6-neighbour (beyond the array is background)."""
    mask = np.asarray(mask, bool)
    return mask & ~ndimage.binary_erosion(mask, structure=S6, border_value=0)


def skeletonize(mask, max_passes=None):
    """-> (skeleton bool, record): record = {"passes", "deleted", "converged", "remaining", "deleted_last"} - the passes run (the
    one that deleted nothing included), voxels deleted in all, whether a pass deleted nothing, voxels left, voxels deleted by the
    last pass run.  max_passes stops early."""
    m = np.pad(np.asarray(mask) != 0, 1)
    passes = deleted = last = 0
    converged = False
    while not converged and (max_passes is None or passes < max_passes):
        cand = np.argwhere(border(m[1:-1, 1:-1, 1:-1]))                             # raster order
        sub = (cand[:, 0] & 1) * 4 + (cand[:, 1] & 1) * 2 + (cand[:, 2] & 1)
        last = 0
        for s in range(8):
            for i, j, k in cand[sub == s]:
                if deletable(m[i:i + 3, j:j + 3, k:k + 3]):
                    m[i + 1, j + 1, k + 1] = False
                    last += 1
        passes += 1
        deleted += last
        converged = last == 0
    out = m[1:-1, 1:-1, 1:-1].copy()
    return out, {"passes": passes, "deleted": deleted, "converged": int(converged), "remaining": int(out.sum()), "deleted_last": last}


def record_list(rec, n_in):
    """The 8-slot record afx_skeletonize_3d writes."""
    return [rec["passes"], rec["deleted"], rec["converged"], rec["remaining"], rec["deleted_last"], int(n_in), 0, 0]


def components26(mask):
    return int(ndimage.label(np.asarray(mask, bool), structure=S26)[1])


def cavities6(mask):
    """Bounded 6-components of the background: those of the mask padded by one layer, less the outer one."""
    return int(ndimage.label(~np.pad(np.asarray(mask, bool), 1), structure=S6)[1]) - 1


def euler26(mask):
    """The Euler characteristic of the union of the closed unit cubes (the 26-connected reading): vertices - edges + faces - cubes,
    each cell counted once.  Equals components - tunnels + cavities."""
    p = np.pad(np.asarray(mask, bool), 1)
    chi = 0
    for axes in ((), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):          # the axes along which the cell is degenerate
        x = p
        for a in axes:
            x = np.take(x, range(1, x.shape[a]), a) | np.take(x, range(0, x.shape[a] - 1), a)
        chi += (-1) ** (3 - len(axes)) * int(x.sum())
    return chi


def invariants(mask):
    return components26(mask), cavities6(mask), euler26(mask)


def n_neighbours(mask):
    """The number of foreground 26-neighbours of every voxel."""
    return ndimage.convolve(np.asarray(mask, bool).astype(np.int32), np.ones((3, 3, 3), np.int32), mode="constant") - np.asarray(mask, bool)


def end_points(mask):
    mask = np.asarray(mask, bool)
    return mask & (n_neighbours(mask) == 1)


def undeleted_candidates(mask):
    """How many border voxels of the mask the rule of step 2 would still delete (0 for a finished skeleton)."""
    m = np.pad(np.asarray(mask, bool), 1)
    return sum(deletable(m[i:i + 3, j:j + 3, k:k + 3]) for i, j, k in np.argwhere(border(m[1:-1, 1:-1, 1:-1])))


# ---- shapes
def bar():
    """A 5 x 5 x 18 bar (450 voxels) at [2:7, 3:8, 2:20] of a 9 x 11 x 22 volume: its centre line is [4, 5, 2:20]."""
    m = np.zeros((9, 11, 22), bool)
    m[2:7, 3:8, 2:20] = True
    return m


def _grid(shape):
    return np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")


def torus(shape=(11, 25, 25), big=8.0, small=2.6):
    i, j, k = _grid(shape)
    c = [(s - 1) / 2 for s in shape]
    return (np.sqrt((j - c[1]) ** 2 + (k - c[2]) ** 2) - big) ** 2 + (i - c[0]) ** 2 <= small ** 2


def shell(n=19, outer=8.2, inner=5.2):
    i, j, k = _grid((n, n, n))
    r = np.sqrt((i - n // 2) ** 2 + (j - n // 2) ** 2 + (k - n // 2) ** 2)
    return (r <= outer) & (r > inner)


def cube(n=16):
    return np.ones((n, n, n), bool)


def capsule(shape, a, b, r):
    """The voxels within r of the segment a-b."""
    p = np.stack(_grid(shape), -1)
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    t = np.clip(((p - a) @ (b - a)) / ((b - a) @ (b - a)), 0.0, 1.0)
    return np.linalg.norm(p - (a + t[..., None] * (b - a)), axis=-1) <= r


def capsule_tree(n=48, floaters=0, seed=0):
    """A trunk that splits twice: 4 capsule branches with radii 4.2 to 1.6 voxels at n = 48 (scaled with n), 4 true ends; `floaters`
    single voxels at seeded random places are added."""
    s = n / 48.0
    segs = [((6, 24, 24), (24, 24, 24), 4.2), ((24, 24, 24), (38, 12, 20), 2.8), ((24, 24, 24), (36, 36, 30), 2.2),
            ((36, 36, 30), (42, 42, 18), 1.6)]
    m = np.zeros((n, n, n), bool)
    for a, b, r in segs:
        m |= capsule(m.shape, np.asarray(a) * s, np.asarray(b) * s, r * s)
    if floaters:
        m.ravel()[np.random.default_rng(seed).choice(m.size, floaters, replace=False)] = True
    return m


def smooth_noise(shape, seed, sigma=1.5, fraction=0.4):
    """Gaussian-smoothed noise thresholded at its `1 - fraction` quantile: thicker pieces than plain noise, more passes."""
    x = ndimage.gaussian_filter(np.random.default_rng(seed).random(shape), sigma, mode="constant")
    return x >= np.quantile(x, 1.0 - fraction)


# ---- the centreline scores on the host
def cldice(vp, vl, sp=None, sl=None):
    """(clDice, Tprec, Tsens, S_P, S_L) of the masks V_P, V_L (Shit et al. 2021): Tprec = |S_P & V_L| / |S_P|, Tsens = |S_L & V_P| / |S_L|,
    clDice their harmonic mean (0 when both are 0)."""
    vp, vl = np.asarray(vp, bool), np.asarray(vl, bool)
    sp = skeletonize(vp)[0] if sp is None else sp
    sl = skeletonize(vl)[0] if sl is None else sl
    tprec = int((sp & vl).sum()) / int(sp.sum())
    tsens = int((sl & vp).sum()) / int(sl.sum())
    return (2.0 * tprec * tsens / (tprec + tsens) if tprec + tsens > 0 else 0.0), tprec, tsens, sp, sl
