"""Plain restatements of the voxel-volume lookup (vol_sample in csrc/afx_internal.h) and of the two kernels built on it (k_volume_grid /
afx_volume_grid, k_project_volume / afx_project_volume), and the seeded problems tests/test_volume_lookup_cpu.py and
tests/test_gpu_volume_lookup.py share.  NumPy float64 only: nothing here imports the library or scipy.  The CPU file ties the restatement
to scipy's RegularGridInterpolator and asserts the problems' preconditions; the GPU file assumes them.

Every volume here is non-cubic with its own point count, spacing and first point per axis, so a kernel that confuses strides, counts,
origins or spacings, or an axis order, cannot agree with it.  The `**mutation` knobs restate exactly those confusions; the CPU file counts
what each of them changes.

One difference to scipy is left alone: the kernel forms an axis' upper face as a0 + da (n - 1), which for a decimal spacing can differ
from the axis' last point by one fp64 ulp (3e-16 on the axes tried), so a point exactly on such a face may be inside for one and outside
for the other.  The exact-face probes below use dyadic axes, where the two are the same number, and the CPU file asserts that no other
sample point comes within 1e-9 of a face plane."""
import collections
import functools
import itertools

import numpy as np

AXES = "xyz"
PAIRS = (("x", "y"), ("x", "z"), ("y", "z"))
# name -> knobs of vol_sample.  Strides: vol[nx][ny][nz] has sx = ny nz and sy = nz.
MUTATIONS = collections.OrderedDict(
    [("sx = nx*nz", dict(sx=lambda nx, ny, nz: nx * nz)), ("sy = ny", dict(sy=lambda nx, ny, nz: ny)),
     ("strides swapped", dict(sx=lambda nx, ny, nz: nz, sy=lambda nx, ny, nz: ny * nz))]
    + [(f"{what} {a}<->{b}", dict(swap=(what, a, b))) for what in ("count", "origin", "spacing") for a, b in PAIRS]
    + [("upper face excluded", dict(open_upper=True)), ("i clamped to n-1", dict(clamp_top=True))])
FACE_MUTATIONS = ("upper face excluded", "i clamped to n-1")      # these change a result only ON an upper face


# ---- the operations ---------------------------------------------------------------------------------------------------------------
def _axis(p, a0, da, n, open_upper, clamp_top):
    """The kernel's rule along one axis -> (inside, i, t): inside iff a0 <= p <= a0 + da (n - 1); u = (p - a0) / da, i = int(u) clamped to
    0 .. n-2, t = u - i."""
    a1 = a0 + da * (n - 1)
    inside = (p >= a0) & ((p < a1) if open_upper else (p <= a1))
    u = (np.where(inside, p, a0) - a0) / da
    i = np.clip(np.trunc(u).astype(np.int64), 0, n - 1 if clamp_top else n - 2)
    return inside, i, u - i


def vol_sample(vol, origin, spacing, fill, points, sx=None, sy=None, swap=None, open_upper=False, clamp_top=False):
    """mu at points[..., 3] (float64) of the volume vol[nx, ny, nz] (fp32 values) whose axis a starts at origin[a] with spacing[a]: the
    8-voxel trilinear blend in the kernel's order (along z, then y, then x), `fill` where a coordinate is outside its axis.  float64.
    The knobs are mutations (MUTATIONS): sx / sy = another stride as a function of (nx, ny, nz); swap = (what, a, b) exchanges the count,
    origin or spacing of two axes; open_upper excludes the upper faces; clamp_top clamps i to n-1 instead of n-2.  A read a mutant makes
    outside the array, or behind the end of an axis, is undefined in a kernel: here it is NaN, so it counts as a change even under a
    zero weight."""
    vol = np.asarray(vol)
    assert vol.ndim == 3 and vol.dtype == np.float32
    flat = vol.astype(np.float64).ravel()
    n, org, spc = list(vol.shape), [float(x) for x in origin], [float(x) for x in spacing]
    if swap is not None:
        what, a, b = swap
        lst = {"count": n, "origin": org, "spacing": spc}[what]
        a, b = AXES.index(a), AXES.index(b)
        lst[a], lst[b] = lst[b], lst[a]
    stride_x = n[1] * n[2] if sx is None else sx(*n)
    stride_y = n[2] if sy is None else sy(*n)
    p = np.asarray(points, dtype=np.float64)
    (in_x, ix, tx), (in_y, iy, ty), (in_z, iz, tz) = (_axis(p[..., a], org[a], spc[a], n[a], open_upper, clamp_top) for a in range(3))
    inside = in_x & in_y & in_z

    def voxel(a, b, c):
        idx = (ix + a) * stride_x + (iy + b) * stride_y + (iz + c)
        ok = (idx >= 0) & (idx < flat.size) & (ix + a < n[0]) & (iy + b < n[1]) & (iz + c < n[2])
        return np.where(ok, flat[np.clip(idx, 0, flat.size - 1)], np.nan)
    c00 = voxel(0, 0, 0) * (1 - tz) + voxel(0, 0, 1) * tz
    c01 = voxel(0, 1, 0) * (1 - tz) + voxel(0, 1, 1) * tz
    c10 = voxel(1, 0, 0) * (1 - tz) + voxel(1, 0, 1) * tz
    c11 = voxel(1, 1, 0) * (1 - tz) + voxel(1, 1, 1) * tz
    mu = (c00 * (1 - ty) + c01 * ty) * (1 - tx) + (c10 * (1 - ty) + c11 * ty) * tx
    return np.where(inside, mu, np.float64(np.float32(fill)))


def lattice_axis(lo, hi, n):
    """np.linspace(lo, hi, n) rounded to fp32, as float64: m * ((hi - lo) / (n - 1)) + lo, the last point exactly hi."""
    t = np.arange(n, dtype=np.float64) * ((float(hi) - float(lo)) / (n - 1)) + float(lo)
    t[-1] = float(hi)
    return t.astype(np.float32).astype(np.float64)


def lattice_points(lo, hi, n, indexing="xy"):
    """The points of volume_grid -> [n, n, n, 3]: entry [i, j, k] is (t[j], t[i], t[k]), np.meshgrid's 'xy' order ('ij': (t[i], t[j], t[k]),
    a mutation)."""
    t = lattice_axis(lo, hi, n)
    first, second = (t[None, :, None], t[:, None, None]) if indexing == "xy" else (t[:, None, None], t[None, :, None])
    return np.stack(np.broadcast_arrays(first, second, t[None, None, :]), -1)


def volume_grid(vol, origin, spacing, fill, lo, hi, n, indexing="xy", **mutation):
    """afx_volume_grid: float32 [n, n, n], grid[i, j, k] = mu(t[j], t[i], t[k])."""
    return vol_sample(vol, origin, spacing, fill, lattice_points(lo, hi, n, indexing), **mutation).astype(np.float32)


def pose_rays(poses, w, h, focal, ids):
    """The kernel's fp64 ray generation for the rays `ids` of the [n_proj, h, w] table -> (o [R, 3], d [R, 3]): pixel (ii, jj) of pose M has
    c0 = (ii - w/2) / focal, c1 = -(jj - h/2) / focal, d = c0 M[:, 0] + c1 M[:, 1] - M[:, 2] (each product and sum rounded), o = M[:, 3]."""
    poses = np.asarray(poses, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64)
    proj, pix = ids // (w * h), ids % (w * h)
    jj, ii = pix // w, pix % w
    m = poses[proj]
    c0 = (ii.astype(np.float64) - w * 0.5) / float(focal)
    c1 = -(jj.astype(np.float64) - h * 0.5) / float(focal)
    d = (c0[:, None] * m[:, :3, 0] + c1[:, None] * m[:, :3, 1]) + (-m[:, :3, 2])
    return m[:, :3, 3].copy(), d


def sample_points(o, d, z):
    """[R, S, 3]: o + d z_s in fp64 (z is fp32)."""
    zs = np.asarray(z, dtype=np.float32).astype(np.float64)
    return np.asarray(o, np.float64)[:, None, :] + np.asarray(d, np.float64)[:, None, :] * zs[None, :, None]


def project(vol, origin, spacing, fill, o, d, z, type_ct, **mutation):
    """afx_project_volume -> float32 [R].  'ct': prod_s exp(-mu_s (dist_s |d|)) with dist_s = z[s+1] - z[s] formed in fp32 and the last one
    1e10; otherwise prod_s exp(-mu_s).  The product runs in sample order in fp64 and is rounded to fp32 once."""
    z = np.asarray(z, dtype=np.float32)
    d = np.asarray(d, dtype=np.float64)
    mu = vol_sample(vol, origin, spacing, fill, sample_points(o, d, z), **mutation)
    if type_ct:
        dist = np.append(z[1:] - z[:-1], np.float32(1e10)).astype(np.float64)
        nrm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        arg = -mu * (dist[None, :] * nrm[:, None])
    else:
        arg = -mu
    prod = np.ones(mu.shape[0])
    with np.errstate(under="ignore"):
        for s in range(mu.shape[1]):
            prod = prod * np.exp(arg[:, s])
        return prod.astype(np.float32)


def one_ulp(want):
    """One fp32 ulp of every reference value."""
    return np.spacing(np.abs(np.asarray(want, dtype=np.float32))).astype(np.float64)


# ---- the problems -----------------------------------------------------------------------------------------------------------------
Volume = collections.namedtuple("Volume", "name vol axes origin spacing fill")
Lattice = collections.namedtuple("Lattice", "lo hi n")


def _volume(name, vol, axes, fill):
    """origin / spacing as VoxelVolume derives them: every axis' first point and first difference."""
    return Volume(name, vol, axes, tuple(float(a[0]) for a in axes), tuple(float(a[1] - a[0]) for a in axes), float(fill))


def _dyadic_axes(shape, origin, spacing):
    return tuple(o + s * np.arange(n, dtype=np.float64) for n, o, s in zip(shape, origin, spacing))


A_SHAPE, A_ORIGIN, A_SPACING, A_FILL = (5, 7, 11), (-3.0, -1.5, -0.75), (0.5, 1.0, 0.25), -4096.0
A_LATTICE = Lattice(-4.0, 4.0, 33)


def a_field(u, v, w):
    """Problem A in voxel coordinates: multilinear, so the trilinear blend reproduces it exactly between the voxels too."""
    return 1 + 3 * u + 16 * v + 128 * w + u * v * w


@functools.lru_cache(maxsize=None)
def problem_a():
    i, j, k = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in A_SHAPE), indexing="ij")
    return _volume("A", a_field(i, j, k).astype(np.float32), _dyadic_axes(A_SHAPE, A_ORIGIN, A_SPACING), A_FILL)


def a_closed_form(points):
    """Problem A's answer in closed form (float64; every operation exact for dyadic coordinates): a_field inside the box, fill outside."""
    p = np.asarray(points, dtype=np.float64)
    uvw = [(p[..., a] - A_ORIGIN[a]) / A_SPACING[a] for a in range(3)]
    inside = np.logical_and.reduce([(c >= 0) & (c <= n - 1) for c, n in zip(uvw, A_SHAPE)])
    return np.where(inside, a_field(*uvw), A_FILL)


# shape -> (first point, spacing) per axis, fill, lattices.  Decimal, anisotropic, off-centre axes; the boxes of (2,2,2) and (6,9,4) do not
# contain the world origin.  Every lattice reaches outside the box on at least one side; the two-point ones have a corner inside it.
# The two long axes start near 0.  VoxelVolume takes an axis' spacing from its first difference, whose rounding error (an ulp of the first
# two points, relative to da) is multiplied by the cell index: for 64 points from -0.35 in steps of 0.07 that is at most 63 x 2^-54 / 0.07
# = 5e-14 cells, for 130 points from -0.12 in steps of 0.043 at most 129 x 2^-56 / 0.043 = 4e-14, and scipy's own (p - a[i]) / (a[i+1] -
# a[i]) adds an ulp of the far end over da, 2e-14.  Starting the 130 points at -3.2 instead brings 2.5e-13 of the maximum against scipy:
# more than the 1e-13 the CPU file holds the restatement to, though far below the fp32 results' 6e-8.
B_SPECS = collections.OrderedDict([
    ((2, 2, 2), ((0.217, -0.35, -0.4), (0.43, 0.625, 0.9), -1.5, (Lattice(0.2537, 0.9113, 2), Lattice(-0.3371, 0.8113, 33), Lattice(-0.5129, 0.7477, 50)))),
    ((2, 3, 5), ((-0.7, -0.55, -1.3), (0.9, 0.43, 0.625), 0.0, (Lattice(-0.4171, 0.2613, 2), Lattice(-1.4137, 1.3371, 33), Lattice(-1.1713, 0.9137, 50)))),
    ((6, 9, 4), ((1.3, 0.4, 0.85), (0.43, 0.625, 0.9), -2.0, (Lattice(1.7137, 3.5713, 2), Lattice(0.2371, 5.7113, 33), Lattice(0.7713, 4.1137, 50)))),
    ((64, 3, 2), ((-0.35, -0.3, -0.55), (0.07, 0.625, 0.9), 0.125, (Lattice(-0.2137, 0.3713, 2), Lattice(-0.5171, 4.2137, 33), Lattice(-0.6371, 1.0713, 50)))),
    ((3, 2, 130), ((-1.15, -0.45, -0.12), (0.9, 1.3, 0.043), -0.75, (Lattice(0.3713, 0.8137, 2), Lattice(-1.3137, 5.5171, 33), Lattice(-0.5171, 1.1137, 50)))),
])
B_SHAPES = list(B_SPECS)


@functools.lru_cache(maxsize=None)
def problem_b(shape, fill=None):
    """Seeded random fp32 values in [0.2, 2] on axes built the way the reference builds them from a CT grid: np.round(a0 + da arange(n), 3)."""
    first, spacing, spec_fill, _ = B_SPECS[shape]
    axes = tuple(np.round(a0 + da * np.arange(n), 3) for n, a0, da in zip(shape, first, spacing))
    rng = np.random.default_rng(1000 * shape[0] + 100 * shape[1] + shape[2])
    vol = (0.2 + 1.8 * rng.random(shape)).astype(np.float32)
    return _volume("B" + "x".join(map(str, shape)), vol, axes, spec_fill if fill is None else fill)


def lattices(shape):
    return B_SPECS[shape][3]


def lattice_cases():
    """Every (problem, lattice) pair: A with its own lattice, every B with n in (2, 33, 50)."""
    return [(problem_a(), A_LATTICE)] + [(problem_b(s), lat) for s in B_SHAPES for lat in lattices(s)]


# ---- exact point probes -------------------------------------------------------------------------------------------------------------
Probe = collections.namedtuple("Probe", "name point inside")
PROBE_SHAPES = {"A": (A_SHAPE, A_ORIGIN, A_SPACING), "2x3x5": ((2, 3, 5), (1.0, -2.5, 0.25), (0.5, 0.25, 2.0))}


@functools.lru_cache(maxsize=None)
def probe_volume(which):
    """Dyadic axes (problem A's, and a (2, 3, 5) box that does not contain the world origin), seeded values in [0.5, 2], fill 0: outside,
    exp(-mu) is exactly 1, and no vertex brings a pixel near it."""
    shape, origin, spacing = PROBE_SHAPES[which]
    rng = np.random.default_rng(17 + len(which))
    vol = (0.5 + 1.5 * rng.random(shape)).astype(np.float32)
    return _volume("probe" + which, vol, _dyadic_axes(shape, origin, spacing), 0.0)


@functools.lru_cache(maxsize=None)
def probes(which):
    """Exact fp64 points: the 8 corners, a point on each of the 12 edges and 6 faces, each face point moved one fp64 step outward and one
    inward, interior points of the first, the last and a middle cell, a voxel, and a point on a voxel plane between two cells."""
    shape, origin, spacing = PROBE_SHAPES[which]
    lo = np.array(origin)
    hi = lo + np.array(spacing) * (np.array(shape) - 1)
    ends = (lo, hi)

    def between(a, cell, frac):
        return origin[a] + spacing[a] * (cell + frac)
    out = []
    for c in itertools.product((0, 1), repeat=3):
        out.append(Probe("corner " + "".join("-+"[s] for s in c), tuple(ends[s][a] for a, s in enumerate(c)), True))
    fracs = (0.25, 0.5, 0.75, 0.375)
    for free in range(3):
        for m, (s1, s2) in enumerate(itertools.product((0, 1), repeat=2)):
            side = iter((s1, s2))
            p = [between(a, (shape[a] - 2) * m // 3, fracs[m]) if a == free else ends[next(side)][a] for a in range(3)]
            out.append(Probe(f"edge along {AXES[free]} {'-+'[s1]}{'-+'[s2]}", tuple(p), True))
    for fixed in range(3):
        for s in (0, 1):
            p = [ends[s][a] if a == fixed else between(a, (shape[a] - 2) // (1 + s), fracs[(a + s) % 3]) for a in range(3)]
            out.append(Probe(f"face {AXES[fixed]}{'-+'[s]}", tuple(p), True))
            for step, name, inside in ((1, "outward", False), (-1, "inward", True)):
                q = list(p)
                q[fixed] = float(np.nextafter(p[fixed], np.inf if (s == 1) == (step == 1) else -np.inf))
                out.append(Probe(f"face {AXES[fixed]}{'-+'[s]} one step {name}", tuple(q), inside))
    for name, cell in (("first", (0, 0, 0)), ("last", tuple(n - 2 for n in shape)), ("middle", tuple((n - 2) // 2 for n in shape))):
        out.append(Probe(f"{name} cell", tuple(between(a, cell[a], (0.25, 0.5, 0.75)[a]) for a in range(3)), True))
    out.append(Probe("a voxel", tuple(between(a, min(1, shape[a] - 1), 0.0) for a in range(3)), True))
    out.append(Probe("a voxel plane", (between(0, 0, 0.5), between(1, 1, 0.0), between(2, shape[2] - 2, 0.125)), True))
    return tuple(out)


def probe_poses(which):
    """One pose per probe, [P, 3, 4] float64: the camera sits at the probe.  With a 1 x 1 detector, one depth z = 0 and type_ct = False
    the pixel is exp(-mu(probe)): the sample point is o + d 0 = o, the double itself."""
    pts = np.array([p.point for p in probes(which)], dtype=np.float64)
    rot = np.array([[0.6, 0.0, 0.8], [0.0, 1.0, 0.0], [-0.8, 0.0, 0.6]])
    return np.concatenate([np.broadcast_to(rot, (len(pts), 3, 3)), pts[:, :, None]], -1)


# ---- ray bundles for the projector ----------------------------------------------------------------------------------------------------
RAY_SHAPES = [(6, 9, 4), (3, 2, 130)]
DETECTOR_W, DETECTOR_H, N_DEPTHS = 23, 19, 61      # 437 rays: a ragged second block of 256
Bundle = collections.namedtuple("Bundle", "poses w h focal z")
VIEW_DIRS = ((0.62, 0.48, 0.62), (-0.35, -0.81, -0.47))      # from the box centre to the two cameras: oblique, in different octants


def box_of(v):
    """(lo [3], hi [3]) with the kernel's upper face a0 + da (n - 1)."""
    lo = np.array(v.origin)
    return lo, lo + np.array(v.spacing) * (np.array(v.vol.shape) - 1)


@functools.lru_cache(maxsize=None)
def ray_bundle(shape):
    """Two cameras at 4 half-diagonals from the centre of problem_b(shape)'s box, looking at it, whose detector spans 1.25 half-diagonals
    to either side there (so the corner rays miss the box), and 61 fp32 depths from 2.7 to 5.3 half-diagonals: in front of the box
    and behind it for every ray."""
    lo, hi = box_of(problem_b(shape))
    centre, r = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    dist = 4.0 * r
    poses = []
    for v in VIEW_DIRS:
        back = np.array(v) / np.linalg.norm(v)
        right = np.cross([0.1, 0.2, 1.0], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        poses.append(np.stack([right, up, back, centre + dist * back], 1))
    focal = DETECTOR_W * 0.5 * dist / (1.25 * r)
    z = np.linspace(2.7 * r, 5.3 * r, N_DEPTHS).astype(np.float32)
    return Bundle(np.stack(poses), DETECTOR_W, DETECTOR_H, float(focal), z)


def bundle_rays(shape, as_fp32):
    """All 2 x 437 rays of the bundle as float64 arrays; as_fp32: rounded to fp32 first, which is what arrays mode hands the kernel."""
    b = ray_bundle(shape)
    o, d = pose_rays(b.poses, b.w, b.h, b.focal, np.arange(2 * b.w * b.h))
    if as_fp32:
        o, d = o.astype(np.float32).astype(np.float64), d.astype(np.float32).astype(np.float64)
    return o, d


def faces_crossed(o, d, lo, hi):
    """Slab test in fp64 -> (hit [R], entry face [R], exit face [R]) with faces numbered 2 axis + (1 for the upper one)."""
    with np.errstate(divide="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    near, far = np.minimum(t0, t1), np.maximum(t0, t1)
    a_in, a_out = near.argmax(1), far.argmin(1)
    rows = np.arange(o.shape[0])
    hit = near.max(1) < far.min(1)
    return hit, 2 * a_in + (t1[rows, a_in] < t0[rows, a_in]), 2 * a_out + (t1[rows, a_out] > t0[rows, a_out])


def face_margin(points, v):
    """The smallest distance (world units) of any coordinate of `points` [..., 3] to one of its axis' two face planes."""
    lo, hi = box_of(v)
    p = np.asarray(points, dtype=np.float64)
    return float(min(np.abs(p - lo).min(), np.abs(p - hi).min()))
