"""The mesh -> signed-distance-field path without a GPU: the NumPy yardstick of the GPU tests (tests/mesh_sdf_reference.py) against closed
forms, the STL / VTK readers of visualization/mesh_io.py round-tripped through its writers, the argument checks and workspace queries of
afx_mesh_sdf_3d / afx_mesh_point_distance (include/afx.h), which return before any HIP call, and the host-side plumbing around them."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import isosurface_reference as iso
import mesh_sdf_reference as ref

AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
FAKE = C.c_void_p(0x10000)          # never dereferenced: every call below is refused before it reaches the device


@pytest.fixture(scope="module")
def lib():
    from nerf_for_angiography_amd import _lib
    return _lib.load()


# ---- the reference against closed forms
def _thick_torus(n):
    return iso.torus_field(n, major=4.5, minor=3.0)          # (a tube thicker than the bound below, so that some grid points lie deep inside)


def _thick_torus_sdf(n, points):
    return ref.torus_sdf(n, points, major=4.5, minor=3.0)


@pytest.mark.parametrize("name, field, analytic, n", [("sphere", iso.sphere_field, ref.sphere_sdf, 12), ("torus", _thick_torus, _thick_torus_sdf, 17)],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_reference_against_the_analytic_distance(name, field, analytic, n):
    """The mesh is the zero level of the piecewise-linear interpolant of an exact distance function sampled at unit spacing; the
    interpolant differs from it by less than the variation of a 1-Lipschitz function over a cell, so the mesh lies within one cell
    diagonal (sqrt 3) of the true surface: |sdf - analytic| <= sqrt 3, and the signs agree wherever |analytic| exceeds it."""
    v, t = ref.capped_mesh(field(n), 0.0)
    shape = (9, 8, 7)
    affine = (1.5, 0.0, 0.0, -1.0, 0.0, 1.5, 0.0, 0.5, 0.0, 0.0, 2.0, 0.25)          # over the whole mesh and beyond, off the voxel lattice
    got = ref.mesh_sdf(v, t, shape, affine)
    want = analytic(n, ref.grid_points(shape, affine)).reshape(shape)
    diag = np.sqrt(3.0)
    assert np.abs(got["sdf"] - want).max() <= diag, name
    far = np.abs(want) > diag
    assert far.sum() > 50 and (want[far] < 0).any() and np.array_equal(got["sdf"][far] < 0, want[far] < 0), name
    assert np.abs(got["winding"] - np.round(got["winding"])).max() < 1e-9 and got["skipped"] == 0


def test_one_triangle_in_each_voronoi_region():
    """a = (0,0,0), b = (4,0,0), c = (0,4,0): every coordinate, every parameter t (a multiple of 1/4) and every intermediate is exact"""
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], dtype=np.float32)
    t = np.array([[0, 1, 2]], dtype=np.int32)
    points = np.array([[1, 1, 2],          # above the face: the plane term, 2
                       [-3, -4, 0],        # vertex a: 5
                       [7, -4, 0],         # vertex b: 5
                       [-4, 7, 0],         # vertex c: 5
                       [2, -3, 4],         # edge ab, foot (2, 0, 0): 5
                       [-3, 1, 4],         # edge ca, foot (0, 1, 0): 5
                       [4, 4, 1],          # edge bc, foot (2, 2, 0): 3
                       [1, 1, 0]],         # on the plane, inside: 0
                      dtype=np.float32)
    dist, nearest, d2 = ref.point_distance(points, v, t)
    assert np.array_equal(d2, [4, 25, 25, 25, 25, 25, 9, 0]) and np.array_equal(dist, [2, 5, 5, 5, 5, 5, 3, 0]) and (nearest == 0).all()
    # degenerate triangles: a line and a point give the distance to the segment and to the point; the reference runs with division by
    # zero and invalid operations raising, so nothing divides 0 by 0
    line = np.array([[0, 0, 0], [4, 0, 0], [2, 0, 0]], dtype=np.float32)
    dot = np.zeros((3, 3), dtype=np.float32)
    assert np.array_equal(ref.point_distance([[2, 3, 0], [7, 4, 0]], line, t)[0], [3, 5])
    assert np.array_equal(ref.point_distance([[0, 3, 4]], dot, t)[0], [5])
    # no valid triangle: +inf and -1; the open triangle seen from straight above its interior subtends less than a hemisphere
    empty = ref.mesh_sdf(v, np.zeros((0, 3), np.int32), (2, 2, 2))
    assert np.isposinf(empty["sdf"]).all() and (empty["nearest"] == -1).all() and (empty["winding"] == 0).all()
    one = ref.mesh_sdf(v, t, (1, 1, 1), (1.0, 0, 0, 1.0, 0, 1.0, 0, 1.0, 0, 0, 1.0, 0.0))      # the grid point (1, 1, 0): on the triangle
    assert one["sdf"][0, 0, 0] == 0 and not np.signbit(one["sdf"][0, 0, 0])                     # d = 0 gives +0.0 whatever the winding says
    skipped = ref.mesh_sdf(np.array([[0, 0, 0], [4, 0, 0], [np.nan, 3, 0]], np.float32), np.array([[0, 1, 2], [0, 1, 5]]), (2, 2, 2))
    assert skipped["valid"] == 0 and skipped["skipped"] == 2 and np.isposinf(skipped["sdf"]).all()


# ---- the readers
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32) * np.float32(0.7) + np.float32(0.1)
TET_T = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)


def test_stl_round_trip_and_welding(tmp_path):
    from nerf_for_angiography_amd.visualization.mesh_io import read_mesh, read_stl, write_stl
    v, t = ref.capped_mesh(iso.sphere_field(8), 0.0)
    path = write_stl(tmp_path / "sphere.stl", v, t)
    got_v, got_t = read_stl(path, weld=True)
    assert got_v.dtype == np.float32 and got_t.dtype == np.int32 and got_t.shape == t.shape
    assert got_v[got_t].tobytes() == v[t].tobytes()                                  # the same corners, triangle by triangle
    assert len(np.unique(got_v.view(np.dtype((np.void, 12))))) == len(got_v)         # welded: no position twice
    assert {p.tobytes() for p in got_v} == {p.tobytes() for p in v[np.unique(t)]}    # the vertex set of the input
    first = np.unique(got_t.reshape(-1), return_index=True)[1]
    assert np.array_equal(np.argsort(first), np.arange(len(got_v)))                  # numbered in the order of first appearance
    soup_v, soup_t = read_stl(path, weld=False)
    assert soup_v.shape == (3 * len(t), 3) and np.array_equal(soup_t.reshape(-1), np.arange(3 * len(t))) and soup_v[soup_t].tobytes() == v[t].tobytes()
    by_name = read_mesh(path)
    assert by_name[0].tobytes() == got_v.tobytes() and np.array_equal(by_name[1], got_t)
    tet = read_stl(write_stl(tmp_path / "tet.stl", TET_V, TET_T))
    assert len(tet[0]) == 4 and tet[0][tet[1]].tobytes() == TET_V[TET_T].tobytes() and np.array_equal(tet[1][0], [0, 1, 2])
    empty = read_stl(write_stl(tmp_path / "empty.stl", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


def test_ascii_stl(tmp_path):
    from nerf_for_angiography_amd.visualization.mesh_io import facet_normals, read_stl
    lines = ["solid tet"]
    for tri, n in zip(TET_T, facet_normals(TET_V, TET_T)):
        lines += [f"  facet normal {n[0]!r} {n[1]!r} {n[2]!r}", "    outer loop"]
        lines += [f"      vertex {float(TET_V[i][0])!r} {float(TET_V[i][1])!r} {float(TET_V[i][2])!r}" for i in tri]
        lines += ["    endloop", "  endfacet"]
    lines.append("endsolid tet")
    path = tmp_path / "tet_ascii.stl"
    path.write_text("\n".join(lines) + "\n")
    v, t = read_stl(path)
    assert v[t].tobytes() == TET_V[TET_T].tobytes() and len(v) == 4
    for cut in (len("\n".join(lines[:9])), len("\n".join(lines[:-1]))):               # inside a facet; before endsolid
        bad = tmp_path / "cut.stl"
        bad.write_text(path.read_text()[:cut])
        with pytest.raises(ValueError, match="truncated"):
            read_stl(bad)


def test_vtk_round_trip_is_bit_exact(tmp_path):
    from nerf_for_angiography_amd.visualization.mesh_io import read_mesh, read_vtk_polydata, write_vtk_polydata
    v, t = ref.capped_mesh(np.random.default_rng(3).random((4, 5, 3)).astype(np.float32), 0.5, iso.IDENTITY)
    for binary in (True, False):
        path = write_vtk_polydata(tmp_path / f"mesh{int(binary)}.vtk", v, t, binary=binary)
        got_v, got_t = read_vtk_polydata(path)
        assert got_v.dtype == np.float32 and got_t.dtype == np.int32
        assert got_v.tobytes() == v.tobytes() and got_t.tobytes() == t.tobytes(), binary
        again = read_mesh(path)
        assert again[0].tobytes() == v.tobytes() and again[1].tobytes() == t.tobytes()
    with pytest.raises(ValueError, match="stl or .vtk"):
        read_mesh(tmp_path / "mesh.obj")


def test_truncated_files_raise(tmp_path):
    from nerf_for_angiography_amd.visualization.mesh_io import read_stl, read_vtk_polydata, write_stl, write_vtk_polydata
    stl = open(write_stl(tmp_path / "a.stl", TET_V, TET_T), "rb").read()
    for cut in (len(stl) - 1, len(stl) - 50, 90, 40, 0):
        (tmp_path / "cut.stl").write_bytes(stl[:cut])
        with pytest.raises(ValueError):
            read_stl(tmp_path / "cut.stl")
    for binary in (True, False):
        vtk = open(write_vtk_polydata(tmp_path / "a.vtk", TET_V, TET_T, binary=binary), "rb").read()
        cuts = (len(vtk) - 8, len(vtk) - 30, 100, 60, 10) if binary else (len(vtk) - 4, len(vtk) - 30, 100, 60, 10)
        for cut in cuts:
            (tmp_path / "cut.vtk").write_bytes(vtk[:cut])
            with pytest.raises(ValueError):
                read_vtk_polydata(tmp_path / "cut.vtk")


# ---- the C ABI without a device
def _sdf_call(lib, verts=FAKE, nv=4, tris=FAKE, nt=4, shape=(4, 5, 6), affine=iso.IDENTITY, flags=0, out=FAKE, nearest=None, winding=None, rec=FAKE,
              ws=FAKE, ws_bytes=1 << 40, needed=None):
    aff = (C.c_double * 12)(*affine) if affine is not None else None
    return lib.afx_mesh_sdf_3d(verts, nv, tris, nt, *shape, aff, flags, out, nearest, winding, rec, ws, ws_bytes, needed, None)


def test_mesh_sdf_argument_checks_return_before_the_device(lib):
    nan, inf = float("nan"), float("inf")
    singular = (1.0, 2.0, 3.0, 0.0, 2.0, 4.0, 6.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    bad = [dict(out=None), dict(rec=None), dict(affine=None), dict(verts=None), dict(tris=None), dict(nv=-1), dict(nt=-1), dict(nv=2 ** 31),
           dict(nt=2 ** 31), dict(shape=(0, 5, 6)), dict(shape=(4, 1025, 6)), dict(shape=(4, 5, -1)), dict(affine=singular),
           dict(affine=(0.0,) * 12), dict(affine=iso.IDENTITY[:3] + (nan,) + iso.IDENTITY[4:]), dict(affine=(inf,) + iso.IDENTITY[1:]),
           dict(flags=4), dict(flags=1 << 31)]
    for kw in bad:
        assert _sdf_call(lib, **kw) == AFX_E_INVALID, kw
    assert b"afx_mesh_sdf_3d" in lib.afx_last_error()
    need = lib.afx_mesh_sdf_3d_workspace_bytes(4)
    assert _sdf_call(lib, ws=None) == AFX_E_WORKSPACE and _sdf_call(lib, ws_bytes=need - 1) == AFX_E_WORKSPACE
    got = C.c_size_t(0)
    assert _sdf_call(lib, ws=None, ws_bytes=0, needed=C.byref(got)) == AFX_E_WORKSPACE and got.value == need
    # an empty mesh is valid: with no arrays at all the call gets as far as the workspace check
    assert _sdf_call(lib, verts=None, nv=0, tris=None, nt=0, ws=None, flags=3) == AFX_E_WORKSPACE


def test_mesh_point_distance_argument_checks_return_before_the_device(lib):
    def call(points=FAKE, n=5, verts=FAKE, nv=4, tris=FAKE, nt=4, dist=FAKE, nearest=None, rec=FAKE):
        return lib.afx_mesh_point_distance(points, n, verts, nv, tris, nt, dist, nearest, rec, None)
    for kw in (dict(rec=None), dict(points=None), dict(dist=None), dict(n=-1), dict(n=2 ** 31), dict(verts=None), dict(tris=None), dict(nv=-1),
               dict(nt=-1), dict(nt=2 ** 31)):
        assert call(**kw) == AFX_E_INVALID, kw
    assert b"afx_mesh_point_distance" in lib.afx_last_error()


def test_workspace_query_and_constants(lib):
    from nerf_for_angiography_amd import engine

    def region(nbytes):
        return -(-nbytes // 256) * 256
    for t in (0, 1, 511, 512, 513, 300_000, 2 ** 31 - 1):
        assert lib.afx_mesh_sdf_3d_workspace_bytes(t) == region(9 * 8 * max(t, 1)) + region(4 * 8 * max(t, 1)), t
    assert lib.afx_mesh_sdf_3d_workspace_bytes(-1) == 0 and lib.afx_mesh_sdf_3d_workspace_bytes(2 ** 31) == 0
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "afx.h")).read()
    defines = {k: int(v.rstrip("u")) for k, v in re.findall(r"#define (AFX_MESH_SDF_[A-Z_]+) (\d+u?)", header)}
    assert defines == {"AFX_MESH_SDF_RECORD_SLOTS": engine.MESH_SDF_RECORD_SLOTS, "AFX_MESH_SDF_TILE": engine.MESH_SDF_TILE,
                       "AFX_MESH_SDF_BRUTE": engine.MESH_SDF_BRUTE, "AFX_MESH_SDF_CLOSED": engine.MESH_SDF_CLOSED}


def test_header_and_ctypes_table_agree_on_the_new_entry_points():
    from test_host_cpu import header_functions
    from nerf_for_angiography_amd import _lib
    new = {"afx_mesh_sdf_3d", "afx_mesh_sdf_3d_workspace_bytes", "afx_mesh_point_distance"}
    assert new <= set(header_functions()) and sorted(_lib.exported_symbols()) == header_functions()
    lib = _lib.load()
    assert all(getattr(lib, name) is not None for name in new)


def test_host_tensors_are_refused():
    import torch
    from nerf_for_angiography_amd._lib import AfxError
    from nerf_for_angiography_amd.engine import mesh_point_distance, mesh_point_distance_record, mesh_sdf_record, mesh_signed_distance
    v, t, p = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(2, 3)
    for fn in (lambda: mesh_signed_distance(v, t, (2, 2, 2)), lambda: mesh_sdf_record(v, t, (2, 2, 2)), lambda: mesh_point_distance(p, v, t),
               lambda: mesh_point_distance_record(p, v, t)):
        with pytest.raises(AfxError, match="no CPU path"):
            fn()


# ---- plumbing
def test_sweep_accepts_the_mesh_distance_names():
    from nerf_for_angiography_amd.visualization.sweep import MESH_DISTANCE_METRICS, MESH_METRICS, _check_metrics
    assert MESH_DISTANCE_METRICS == ("ASSD MESH", "HD MESH", "HD95 MESH")
    volume = object()
    assert _check_metrics(["HD MESH", "EULER 3D", "PSNR", "ASSD MESH"], None, volume) == ["PSNR", "EULER 3D", "ASSD MESH", "HD MESH"]
    assert _check_metrics(list(MESH_DISTANCE_METRICS) + list(MESH_METRICS), None, volume) == list(MESH_METRICS) + list(MESH_DISTANCE_METRICS)
    for name in MESH_DISTANCE_METRICS:
        with pytest.raises(ValueError, match="need the ground-truth volume"):
            _check_metrics([name], None, None)


def test_synthetic_dataset_without_a_phantom_is_unchanged():
    from nerf_for_angiography_amd.phantomdata.dataset import make_synthetic_dataset
    angles = [(90.0, 0.0), (60.0, 20.0)]
    kw = dict(img_size=8, depth_samples_per_ray=16, device="cpu", seed=3)
    old_p, old_r = make_synthetic_dataset(angles, **kw)
    new_p, new_r = make_synthetic_dataset(angles, phantom=None, **kw)
    assert old_p.equals(new_p) and old_r.equals(new_r)
    assert old_p.to_csv(sep=";") == new_p.to_csv(sep=";") and old_r.to_csv(sep=";") == new_r.to_csv(sep=";")          # byte for byte on disk
    sig = inspect.signature(make_synthetic_dataset).parameters
    assert sig["phantom"].default is None and sig["projection_type"].default == "ct"
    with pytest.raises(ValueError, match="VoxelVolume"):
        make_synthetic_dataset(angles, phantom=object(), **kw)
    with pytest.raises(ValueError, match="projection_type"):
        make_synthetic_dataset(angles, projection_type="mip", **kw)


def test_driver_flags():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser, check_args
    args = build_parser().parse_args(["--synthetic"])
    assert args.phantom_mesh is None and args.phantom_points == 201
    check_args(build_parser().parse_args(["--synthetic", "--phantom_mesh", "vessel.STL", "--phantom_points", "33"]))
    for argv, match in ((["--phantom_mesh", "vessel.stl"], "needs --synthetic"), (["--synthetic", "--phantom_mesh", "vessel.obj"], ".stl or .vtk"),
                        (["--synthetic", "--phantom_mesh", "vessel.vtk", "--phantom_points", "1"], "N >= 2")):
        with pytest.raises(ValueError, match=match):
            check_args(build_parser().parse_args(argv))
