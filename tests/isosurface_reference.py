"""NumPy fp64 restatement of afx_isosurface_3d / afx_mesh_measures (include/afx.h): marching tetrahedra on the Kuhn split.

It shares no table and no case analysis with the kernels: a tetrahedron's triangles are built from the sets of inside and outside
corners, the winding of every triangle is decided geometrically (the normal of the triangle laid through the midpoints of its edges
against the direction from the inside corners to the outside ones, then the sign of det(m)), the vertex positions follow the header's
formula operation by operation, E and B are counted from the triangle list, the crossed faces from the list of all faces of the
triangulation, and `clipped_volume` is the volume of {interpolant >= iso} summed per tetrahedron, without any mesh."""
import itertools
import math

import numpy as np

DIRECTIONS = ((0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1))
PERMUTATIONS = tuple(itertools.permutations(range(3)))          # lexicographic: the order of the tetrahedra in a cube
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def tet_corners(p):
    """The four corner offsets of tetrahedron p: c0, c0 + e[p0], + e[p1], (1,1,1)."""
    c = [np.zeros(3, dtype=np.int64)]
    for axis in p:
        nxt = c[-1].copy()
        nxt[axis] += 1
        c.append(nxt)
    return c


def affine_parts(affine):
    a = np.asarray(IDENTITY if affine is None else affine, dtype=np.float64).reshape(3, 4)
    return a[:, :3].copy(), a[:, 3].copy()


def padded(f, fill):
    """cap=True of engine.extract_isosurface: one layer of `fill` around the volume; the affine moves by one index."""
    return np.pad(np.asarray(f, dtype=np.float32), 1, constant_values=np.float32(fill))


def shifted_affine(affine):
    m, o = affine_parts(affine)
    o2 = o - m @ np.ones(3)
    return tuple(np.concatenate([m, o2[:, None]], axis=1).reshape(-1))


def _cube_bases(shape):
    g = np.stack(np.meshgrid(*[np.arange(n - 1) for n in shape], indexing="ij"), axis=-1).reshape(-1, 3)
    return g.astype(np.int64)


def _lin(pts, shape):
    return (pts[..., 0] * shape[1] + pts[..., 1]) * shape[2] + pts[..., 2]


def isosurface(f, iso, affine=None):
    """-> dict(vertices float32 [V,3] in canonical order, triangles int64 [T,3] in the order of the header (cube, tetrahedron, the
    two triangles of a two-and-two cut), V, T, E, B, n22, euler)."""
    f = np.asarray(f, dtype=np.float32)
    iso = np.float32(iso)
    shape = f.shape
    m, o = affine_parts(affine)
    empty = dict(vertices=np.zeros((0, 3), np.float32), triangles=np.zeros((0, 3), np.int64), V=0, T=0, E=0, B=0, n22=0, euler=0)
    if min(shape) < 2:
        return empty
    inside = f >= iso
    f64 = f.astype(np.float64)
    # ---- vertices: one per crossed edge, ordered by linear_index(a) * 7 + d
    keys, pos = [], []
    for d, step in enumerate(DIRECTIONS):
        step = np.array(step)
        a = np.stack(np.meshgrid(*[np.arange(n - s) for n, s in zip(shape, step)], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
        b = a + step
        ia, ib = inside[tuple(a.T)], inside[tuple(b.T)]
        a, b = a[ia != ib], b[ia != ib]
        fa, fb = f64[tuple(a.T)], f64[tuple(b.T)]
        t = (np.float64(iso) - fa) / (fb - fa)
        q = a.astype(np.float64)
        for x in range(3):
            if step[x]:
                q[:, x] = q[:, x] + t
        w = np.empty_like(q)
        for r in range(3):
            w[:, r] = ((o[r] + m[r, 0] * q[:, 0]) + m[r, 1] * q[:, 1]) + m[r, 2] * q[:, 2]
        keys.append(_lin(a, shape) * 7 + d)
        pos.append(w.astype(np.float32))
    keys, pos = np.concatenate(keys), np.concatenate(pos)
    order = np.argsort(keys, kind="stable")
    keys, vertices = keys[order], pos[order]

    def vertex_id(p, q):
        """ids of the vertices on the edges p-q (arrays of grid points [k,3])"""
        lo = np.where((_lin(p, shape) < _lin(q, shape))[:, None], p, q)
        diff = np.abs(q - p)
        d = diff[:, 0] * 4 + diff[:, 1] * 2 + diff[:, 2] - 1
        k = _lin(lo, shape) * 7 + d
        idx = np.searchsorted(keys, k)
        assert np.array_equal(keys[idx], k)
        return idx

    # ---- triangles
    det_negative = np.linalg.det(m) < 0
    bases = _cube_bases(shape)
    cube_lin = _lin(bases, shape)
    tris, sort_key, n22 = [], [], 0
    for ip, p in enumerate(PERMUTATIONS):
        offs = tet_corners(p)
        corners = [bases + c for c in offs]
        ins = np.stack([inside[tuple(c.T)] for c in corners], axis=1)          # [cubes, 4]
        which = ins @ np.array([1, 2, 4, 8])
        for pattern in itertools.product((False, True), repeat=4):
            n_in = sum(pattern)
            if n_in in (0, 4):
                continue
            sel = np.flatnonzero(which == int(np.dot(pattern, [1, 2, 4, 8])))
            if not len(sel):
                continue
            in_c = [j for j in range(4) if pattern[j]]
            out_c = [j for j in range(4) if not pattern[j]]
            if n_in == 2:
                (A, B), (C, D) = in_c, out_c
                faces = [((A, C), (A, D), (B, D)), ((A, C), (B, D), (B, C))]
                n22 += len(sel)
            else:
                lone = in_c[0] if n_in == 1 else out_c[0]
                rest = [j for j in range(4) if j != lone]
                faces = [tuple((lone, j) for j in rest)]
            # the direction from inside to outside, in index space
            g = np.mean([offs[j] for j in out_c], axis=0) - np.mean([offs[j] for j in in_c], axis=0)
            for k, face in enumerate(faces):
                mid = [(offs[i] + offs[j]) / 2.0 for i, j in face]
                normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
                s = float(np.dot(normal, g))
                assert s != 0.0
                face = list(face)
                if (s < 0) != det_negative:
                    face[1], face[2] = face[2], face[1]
                ids = [vertex_id(corners[i][sel], corners[j][sel]) for i, j in face]
                tris.append(np.stack(ids, axis=1))
                sort_key.append((cube_lin[sel] * 6 + ip) * 2 + k)
    if not tris:
        res = dict(empty)
        res["vertices"], res["V"] = vertices, len(vertices)
        return res
    tris, sort_key = np.concatenate(tris), np.concatenate(sort_key)
    triangles = tris[np.argsort(sort_key, kind="stable")]
    # ---- E and B from the unique edges of the triangle list
    e = np.concatenate([triangles[:, [0, 1]], triangles[:, [1, 2]], triangles[:, [2, 0]]])
    V, T = len(vertices), len(triangles)
    und, mult = np.unique(e.min(axis=1) * V + e.max(axis=1), return_counts=True)
    E = len(und)
    return dict(vertices=vertices, triangles=triangles, V=V, T=T, E=E, B=int((mult == 1).sum()), n22=n22, euler=V - E + T,
                edge_multiplicities=sorted(set(mult.tolist())))


def crossed_faces(f, iso):
    """(crossed faces, crossed faces that belong to one tetrahedron only) of the triangulation: every face of every tetrahedron, as a set."""
    f = np.asarray(f, dtype=np.float32)
    shape = f.shape
    if min(shape) < 2:
        return 0, 0
    inside = (f >= np.float32(iso)).reshape(-1)
    bases = _cube_bases(shape)
    faces = []
    for p in PERMUTATIONS:
        lin = np.stack([_lin(bases + c, shape) for c in tet_corners(p)], axis=1)
        for skip in range(4):
            faces.append(np.sort(lin[:, [j for j in range(4) if j != skip]], axis=1))
    uniq, mult = np.unique(np.concatenate(faces), axis=0, return_counts=True)
    assert set(mult.tolist()) <= {1, 2}
    s = inside[uniq].sum(axis=1)
    crossed = (s > 0) & (s < 3)
    return int(crossed.sum()), int((crossed & (mult == 1)).sum())


def canonical_triangles(t):
    """every triangle rotated to start at its smallest id (the orientation kept), the list sorted"""
    t = np.asarray(t, dtype=np.int64).reshape(-1, 3)
    if len(t) == 0:
        return t
    r = np.argmin(t, axis=1)
    rot = np.stack([t[np.arange(len(t)), (r + k) % 3] for k in range(3)], axis=1)
    return rot[np.lexsort((rot[:, 2], rot[:, 1], rot[:, 0]))]


def rotated_triangles(t):
    """every triangle rotated to start at its smallest id, the order of the list kept"""
    t = np.asarray(t, dtype=np.int64).reshape(-1, 3)
    if len(t) == 0:
        return t
    r = np.argmin(t, axis=1)
    return np.stack([t[np.arange(len(t)), (r + k) % 3] for k in range(3)], axis=1)


def measure_terms(vertices, triangles, ref_point=(0.0, 0.0, 0.0)):
    """Per-triangle terms of afx_mesh_measures in fp64, operation by operation as the header orders them -> (area terms, volume terms)."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    u, w = b - a, c - a
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    r = np.asarray(ref_point, dtype=np.float64)
    e, g, h = a - r, b - r, c - r
    vol = ((e[:, 0] * (g[:, 1] * h[:, 2] - g[:, 2] * h[:, 1]) + e[:, 1] * (g[:, 2] * h[:, 0] - g[:, 0] * h[:, 2]))
           + e[:, 2] * (g[:, 0] * h[:, 1] - g[:, 1] * h[:, 0])) / 6.0
    return area, vol


def measures(vertices, triangles, ref_point=(0.0, 0.0, 0.0)):
    area, vol = measure_terms(vertices, triangles, ref_point)
    return {"area": math.fsum(area), "volume": math.fsum(vol), "area_abs": math.fsum(np.abs(area)), "volume_abs": math.fsum(np.abs(vol))}


def _tet_volume(p0, p1, p2, p3):
    return np.abs(np.einsum("ki,ki->k", p1 - p0, np.cross(p2 - p0, p3 - p0))) / 6.0


def clipped_volume(f, iso, affine=None):
    """The volume of {x : interpolant(x) >= iso} in world units, summed per tetrahedron in closed form - no mesh, no winding:
    a tetrahedron with one inside corner keeps the small tetrahedron at that corner, one with one outside corner loses the small
    tetrahedron there, one cut two and two keeps the wedge A, AC, AD - B, BC, BD (three tetrahedra; its quadrilaterals are planar).
    -> (volume by math.fsum, number of terms, sum of |terms|)."""
    f = np.asarray(f, dtype=np.float32)
    shape = f.shape
    m, _ = affine_parts(affine)
    scale = abs(float(np.linalg.det(m)))
    if min(shape) < 2:
        return 0.0, 0, 0.0
    g = f.astype(np.float64) - np.float64(np.float32(iso))
    inside = f >= np.float32(iso)
    bases = _cube_bases(shape)
    terms = []
    for p in PERMUTATIONS:
        corners = [bases + c for c in tet_corners(p)]
        ins = np.stack([inside[tuple(c.T)] for c in corners], axis=1)
        val = np.stack([g[tuple(c.T)] for c in corners], axis=1)
        pts = [c.astype(np.float64) for c in corners]
        n_in = ins.sum(axis=1)
        terms.append(np.full(int((n_in == 4).sum()), 1.0 / 6.0))

        def cut(sel, i, j):               # the point on the edge i-j where the interpolant is iso
            t = val[sel, i] / (val[sel, i] - val[sel, j])
            return pts[i][sel] + t[:, None] * (pts[j][sel] - pts[i][sel])

        for pattern in itertools.product((False, True), repeat=4):
            k = sum(pattern)
            if k in (0, 4):
                continue
            sel = np.all(ins == np.array(pattern), axis=1)
            if not sel.any():
                continue
            in_c = [j for j in range(4) if pattern[j]]
            out_c = [j for j in range(4) if not pattern[j]]
            if k == 1:
                L = in_c[0]
                terms.append(_tet_volume(pts[L][sel], *[cut(sel, L, j) for j in out_c]))
            elif k == 3:
                L = out_c[0]
                terms.append(np.full(int(sel.sum()), 1.0 / 6.0))
                terms.append(-_tet_volume(pts[L][sel], *[cut(sel, L, j) for j in in_c]))
            else:
                (A, B), (C, D) = in_c, out_c
                a1, a2, a3 = pts[A][sel], cut(sel, A, C), cut(sel, A, D)
                b1, b2, b3 = pts[B][sel], cut(sel, B, C), cut(sel, B, D)
                terms += [_tet_volume(a1, a2, a3, b1), _tet_volume(a2, a3, b1, b2), _tet_volume(a3, b1, b2, b3)]
    terms = np.concatenate(terms) * scale if terms else np.zeros(0)
    return math.fsum(terms), len(terms), math.fsum(np.abs(terms))


def sphere_field(n, centre=None, radius=None):
    """radius - distance: positive inside"""
    c = np.full(3, (n - 1) / 2.0) if centre is None else np.asarray(centre, dtype=np.float64)
    r = 0.35 * n if radius is None else radius
    i = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"), axis=-1)
    return (r - np.linalg.norm(i - c, axis=-1)).astype(np.float32)


def torus_field(n, major=None, minor=None):
    c = (n - 1) / 2.0
    R, r = (0.3 * n if major is None else major), (0.12 * n if minor is None else minor)
    i = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"), axis=-1) - c
    ring = np.sqrt(i[..., 0] ** 2 + i[..., 1] ** 2) - R
    return (r - np.sqrt(ring ** 2 + i[..., 2] ** 2)).astype(np.float32)


def two_spheres_field(n):
    a = sphere_field(n, centre=(0.28 * n, 0.5 * n, 0.5 * n), radius=0.17 * n)
    b = sphere_field(n, centre=(0.72 * n, 0.5 * n, 0.5 * n), radius=0.17 * n)
    return np.maximum(a, b)
