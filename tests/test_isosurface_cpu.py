"""Isosurface extraction without a GPU: the NumPy yardstick of the GPU tests (tests/isosurface_reference.py) on surfaces with a known
Euler characteristic, the closedness and orientation of a capped mesh, the rule the kernel counts E and B by (crossed faces + two-and-two
tetrahedra) against unique-edge counting, the STL and VTK writers round-tripped through a parser of this file's own, the sweep's
handling of the mesh metric names, and the argument checks and workspace queries of afx_isosurface_3d / afx_mesh_measures
(include/afx.h), which return before any HIP call."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import isosurface_reference as iso

AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
FAKE = C.c_void_p(0x10000)          # never dereferenced: every call below is refused before it reaches the device
# index (i0, i1, i2) -> (2 i1 - 3, i0 / 2 + 1, 1.5 i2 + 2): the density grid's exchange of the first two axes, anisotropic; det < 0
SWAPPED = (0.0, 2.0, 0.0, -3.0, 0.5, 0.0, 0.0, 1.0, 0.0, 0.0, 1.5, 2.0)


@pytest.fixture(scope="module")
def lib():
    from nerf_for_angiography_amd import _lib
    return _lib.load()


def _capped(f, level, affine=None, fill=-1.0):
    return iso.isosurface(iso.padded(f, fill), level, iso.shifted_affine(affine))


@pytest.mark.parametrize("name, field, chi", [("sphere", iso.sphere_field(16), 2), ("torus", iso.torus_field(20), 0),
                                              ("two spheres", iso.two_spheres_field(20), 4)], ids=lambda v: v if isinstance(v, str) else "")
def test_euler_characteristic_of_known_surfaces(name, field, chi):
    for affine in (None, SWAPPED):
        m = _capped(field, 0.0, affine)
        assert m["euler"] == chi and m["B"] == 0 and m["V"] > 0, (name, m["euler"], m["B"])
        vol = iso.measures(m["vertices"], m["triangles"])["volume"]
        clip, _, _ = iso.clipped_volume(iso.padded(field, -1.0), 0.0, iso.shifted_affine(affine))
        assert vol > 0 and abs(vol - clip) <= 1e-5 * clip, (name, vol, clip)         # outward normals whatever the sign of det(m)


def test_capped_mesh_is_closed_and_consistently_oriented():
    rng = np.random.default_rng(5)
    for shape, level in (((4, 5, 3), 0.5), ((6, 7, 5), 0.3), ((3, 3, 9), 0.8)):
        f = rng.random(shape).astype(np.float32)
        f[0, 0, 0] = f[1, 2, 1] = np.float32(level)                        # voxels exactly at the level: still closed
        m = _capped(f, level, SWAPPED)
        t = m["triangles"]
        directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
        keys, counts = np.unique(directed, axis=0, return_counts=True)
        assert (counts == 1).all()                                         # no directed edge twice ...
        back = {(int(b), int(a)) for a, b in keys}
        assert back == {(int(a), int(b)) for a, b in keys}                 # ... and each one met by its reverse: two triangles, opposite ways
        assert m["B"] == 0 and m["E"] * 2 == len(directed)


def test_edges_are_crossed_faces_plus_two_and_two_tetrahedra():
    rng = np.random.default_rng(6)
    for shape in ((2, 2, 2), (4, 5, 3), (6, 7, 5), (2, 9, 3)):
        for level in (0.5, 0.1, 0.9):
            f = rng.random(shape).astype(np.float32)
            m = iso.isosurface(f, level)
            faces, outer = iso.crossed_faces(f, level)
            assert m["E"] == faces + m["n22"] and m["B"] == outer, (shape, level)
            assert set(m.get("edge_multiplicities", [])) <= {1, 2}
    assert iso.isosurface(np.zeros((1, 5, 4), np.float32), 0.5)["V"] == 0 and iso.crossed_faces(np.zeros((1, 5, 4)), 0.5) == (0, 0)


# ---- the writers, read back by a parser that knows only the formats
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32) * np.float32(0.7) + np.float32(0.1)
TET_T = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)          # normals point out of the tetrahedron


def read_stl(path):
    raw = open(path, "rb").read()
    n, = struct.unpack_from("<I", raw, 80)
    assert len(raw) == 84 + 50 * n
    rec = np.frombuffer(raw, dtype=np.dtype([("normal", "<f4", 3), ("corners", "<f4", (3, 3)), ("attr", "<u2")]), offset=84)
    return raw[:80], rec["normal"].copy(), rec["corners"].copy(), rec["attr"].copy()


def read_vtk(path):
    raw = open(path, "rb").read()
    lines = raw.split(b"\n", 5)
    assert lines[0].startswith(b"# vtk DataFile Version") and lines[3] == b"DATASET POLYDATA"
    binary = {b"BINARY": True, b"ASCII": False}[lines[2]]
    kw, n, dtype = lines[4].split()
    assert kw == b"POINTS" and dtype == b"float"
    n, body = int(n), lines[5]
    if binary:
        pts = np.frombuffer(body, dtype=">f4", count=3 * n).reshape(n, 3).astype(np.float32)
        rest = body[12 * n:].lstrip(b"\n")
        head, cells = rest.split(b"\n", 1)
        kw, t, size = head.split()
        cells = np.frombuffer(cells, dtype=">i4", count=int(size)).reshape(int(t), 4)
    else:
        tok = body.split()
        pts = np.array([float(x) for x in tok[:3 * n]], dtype=np.float64).astype(np.float32).reshape(n, 3)
        kw, t, size = tok[3 * n:3 * n + 3]
        cells = np.array([int(x) for x in tok[3 * n + 3:3 * n + 3 + int(size)]]).reshape(int(t), 4)
    assert kw == b"POLYGONS" and int(size) == 4 * int(t) and (cells[:, 0] == 3).all()
    return pts, cells[:, 1:].astype(np.int64)


def test_stl_and_vtk_round_trip(tmp_path):
    from nerf_for_angiography_amd.visualization.mesh_io import write_mesh, write_stl, write_vtk_polydata
    centre = TET_V.mean(axis=0)
    p = write_stl(tmp_path / "tet.stl", TET_V, TET_T)
    head, normals, corners, attr = read_stl(p)
    assert np.array_equal(corners, TET_V[TET_T]) and (attr == 0).all() and not head.lstrip().lower().startswith(b"solid")
    for k in range(4):
        want = np.cross(corners[k, 1] - corners[k, 0], corners[k, 2] - corners[k, 0]).astype(np.float64)
        want /= np.linalg.norm(want)
        assert np.abs(normals[k] - want).max() <= 1e-6 and abs(np.linalg.norm(normals[k]) - 1.0) <= 1e-6
        assert np.dot(normals[k], corners[k].mean(axis=0) - centre) > 0                 # outward
    for binary in (True, False):
        p = write_vtk_polydata(tmp_path / f"tet{int(binary)}.vtk", TET_V, TET_T, binary=binary)
        pts, tri = read_vtk(p)
        assert np.array_equal(pts, TET_V) and np.array_equal(tri, TET_T)
    assert np.array_equal(read_vtk(write_mesh(tmp_path / "by_name.VTK", TET_V, TET_T))[1], TET_T)
    assert len(read_stl(write_mesh(tmp_path / "by_name.stl", TET_V, TET_T))[1]) == 4
    empty = write_stl(tmp_path / "empty.stl", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert len(read_stl(empty)[1]) == 0
    with pytest.raises(ValueError, match="stl or .vtk"):
        write_mesh(tmp_path / "mesh.obj", TET_V, TET_T)
    with pytest.raises(ValueError, match="outside"):
        write_stl(tmp_path / "bad.stl", TET_V, TET_T + 1)
    assert sorted(os.listdir(tmp_path)) == ["by_name.VTK", "by_name.stl", "empty.stl", "tet.stl", "tet0.vtk", "tet1.vtk"]


def test_a_failed_write_leaves_no_partial_file(tmp_path, monkeypatch):
    from nerf_for_angiography_amd.visualization import mesh_io
    target = tmp_path / "mesh.stl"
    mesh_io.write_stl(target, TET_V, TET_T)
    before = target.read_bytes()

    def fail(fd):
        raise OSError("disk full")
    monkeypatch.setattr(mesh_io.os, "fsync", fail)
    for writer, name in ((mesh_io.write_stl, "mesh.stl"), (mesh_io.write_vtk_polydata, "new.vtk")):
        with pytest.raises(OSError, match="disk full"):
            writer(tmp_path / name, TET_V * 2, TET_T)
    assert os.listdir(tmp_path) == ["mesh.stl"] and target.read_bytes() == before       # the old file as it was, nothing else


def test_sweep_accepts_the_mesh_metric_names():
    from nerf_for_angiography_amd.visualization.sweep import (CENTRELINE_METRICS, MESH_METRICS, _EXTRA_METRICS, _check_metrics,
                                                              grid_index_to_world)
    assert MESH_METRICS == ("VOLUME RATIO 3D", "AREA RATIO 3D", "EULER 3D")
    assert _EXTRA_METRICS[-3:] == MESH_METRICS and _EXTRA_METRICS[-6:-3] == CENTRELINE_METRICS       # appended: earlier columns keep their place
    volume = object()
    assert _check_metrics(["EULER 3D", "PSNR", "VOLUME RATIO 3D", "CLDICE 3D"], None, volume) == ["PSNR", "CLDICE 3D", "VOLUME RATIO 3D", "EULER 3D"]
    for name in MESH_METRICS:
        with pytest.raises(ValueError, match="need the ground-truth volume"):
            _check_metrics([name], None, None)
    a = np.array(grid_index_to_world(100.0, 5)).reshape(3, 4)
    assert np.linalg.det(a[:, :3]) < 0
    assert np.array_equal(a[:, :3] @ [1, 2, 4] + a[:, 3], [0.0, -50.0, 100.0])          # (i0, i1, i2) -> (t[i1], t[i0], t[i2])


def _iso_call(lib, shape=(4, 5, 6), iso_value=0.5, affine=iso.IDENTITY, max_v=0, max_t=0, f=FAKE, verts=None, tris=None, rec=FAKE, ws=FAKE,
              ws_bytes=1 << 40):
    aff = (C.c_double * 12)(*affine) if affine is not None else None
    return lib.afx_isosurface_3d(f, *shape, iso_value, aff, verts, max_v, tris, max_t, rec, ws, ws_bytes, None, None)


def test_isosurface_argument_checks_return_before_the_device(lib):
    nan, inf = float("nan"), float("inf")
    singular = (1.0, 2.0, 3.0, 0.0, 2.0, 4.0, 6.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    bad = [dict(f=None), dict(rec=None), dict(affine=None), dict(shape=(0, 5, 6)), dict(shape=(4, 1025, 6)), dict(shape=(4, 5, -1)),
           dict(iso_value=nan), dict(max_v=-1), dict(max_t=-1), dict(max_v=2 ** 31), dict(max_t=2 ** 31), dict(max_v=1), dict(max_t=1),
           dict(affine=singular), dict(affine=(0.0,) * 12), dict(affine=iso.IDENTITY[:3] + (nan,) + iso.IDENTITY[4:]),
           dict(affine=(inf,) + iso.IDENTITY[1:])]
    for kw in bad:
        assert _iso_call(lib, **kw) == AFX_E_INVALID, kw
    assert _iso_call(lib, ws=None) == AFX_E_WORKSPACE
    need = lib.afx_isosurface_3d_workspace_bytes(4, 5, 6)
    assert _iso_call(lib, ws_bytes=need - 1) == AFX_E_WORKSPACE
    got = C.c_size_t(0)
    aff = (C.c_double * 12)(*iso.IDENTITY)
    assert lib.afx_isosurface_3d(FAKE, 4, 5, 6, 0.5, aff, None, 0, None, 0, FAKE, None, 0, C.byref(got), None) == AFX_E_WORKSPACE
    assert got.value == need


def test_workspace_queries(lib):
    def region(nbytes):
        return -(-nbytes // 256) * 256
    for shape in ((1, 1, 1), (2, 2, 2), (33, 17, 65), (1024, 1024, 1024), (7, 1, 300)):
        n = shape[0] * shape[1] * shape[2]
        chunks = -(-n // 1024)
        want = region(n) + 2 * region(2 * n) + 5 * region(4 * chunks) + 2 * region(8 * chunks)
        assert lib.afx_isosurface_3d_workspace_bytes(*shape) == want, shape
    for shape in ((0, 4, 4), (4, 1025, 4), (4, 4, -3)):
        assert lib.afx_isosurface_3d_workspace_bytes(*shape) == 0
    assert lib.afx_mesh_measures_workspace_bytes() == 2 * 2048 * 8


def test_mesh_measures_argument_checks_return_before_the_device(lib):
    ref = (C.c_double * 3)(0.0, 0.0, 0.0)
    need = lib.afx_mesh_measures_workspace_bytes()

    def call(verts=FAKE, nv=4, tris=FAKE, nt=4, rec=FAKE, ref=ref, out=FAKE, ws=FAKE, ws_bytes=need):
        return lib.afx_mesh_measures(verts, nv, tris, nt, rec, ref, out, ws, ws_bytes, None, None)
    for kw in (dict(rec=None), dict(out=None), dict(verts=None), dict(tris=None), dict(nv=-1), dict(nt=2 ** 31),
               dict(ref=(C.c_double * 3)(0.0, float("nan"), 0.0))):
        assert call(**kw) == AFX_E_INVALID, kw
    assert call(ws=None) == AFX_E_WORKSPACE and call(ws_bytes=need - 1) == AFX_E_WORKSPACE


def test_host_tensors_are_refused():
    import torch
    from nerf_for_angiography_amd._lib import AfxError
    from nerf_for_angiography_amd.engine import extract_isosurface, isosurface_record, mesh_measures
    x = torch.zeros(4, 4, 4)
    for fn in (lambda: isosurface_record(x, 0.5), lambda: extract_isosurface(x, 0.5),
               lambda: mesh_measures(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))):
        with pytest.raises(AfxError, match="no CPU path"):
            fn()
