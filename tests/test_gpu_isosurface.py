"""Isosurface extraction on the GPU (afx_isosurface_3d, afx_mesh_measures; engine.isosurface_record / extract_isosurface / mesh_measures,
visualization/sweep.py, visualization/mesh_io.py) against the NumPy restatement of tests/isosurface_reference.py.  The mesh is defined so
that every implementation gives the same one: vertices must EQUAL the reference bit for bit in the canonical order, the triangles as a
set (each rotated to start at its smallest id) and, beyond that, in the documented order; the record's counts are the reference's; a
second run gives the same bits.  There are no tolerances but for the two fp64 sums of afx_mesh_measures, whose bound is worked out from
the number of terms."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import isosurface_reference as iso
from test_isosurface_cpu import SWAPPED, read_stl, read_vtk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
# less than a wave, an empty mesh (an axis of one voxel), more than one workgroup and more than one scan chunk along the last and along
# the first axis, a non-multiple of everything, more chunks than one (36, 256 of 1024 points: the scan's threads take one chunk each)
SHAPES = [(2, 2, 2), (1, 5, 4), (2, 2, 300), (300, 2, 2), (3, 5, 4), (33, 17, 65), (65, 64, 63)]
LEVELS = (0.5, 0.05, 0.95)


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _extract(f, level, affine=None, cap=False, fill=0.0):
    """-> (vertices ndarray, triangles ndarray, info) of engine.extract_isosurface."""
    from nerf_for_angiography_amd.engine import extract_isosurface
    v, t, info = extract_isosurface(_dev(f, np.float32), level, affine, cap=cap, fill=fill)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.shape == (info["V"], 3) and t.shape == (info["T"], 3)
    return v.cpu().numpy(), t.cpu().numpy(), info


def _reference(f, level, affine=None, cap=False, fill=0.0):
    if cap:
        return iso.isosurface(iso.padded(f, fill), level, iso.shifted_affine(affine))
    return iso.isosurface(f, level, affine)


def _same_mesh(got, want, what):
    v, t, info = got
    assert {k: info[k] for k in ("V", "T", "E", "B", "n22", "euler")} == {k: want[k] for k in ("V", "T", "E", "B", "n22", "euler")}, what
    assert v.tobytes() == want["vertices"].tobytes(), what                                      # bit for bit, in the canonical order
    assert np.array_equal(iso.canonical_triangles(t), iso.canonical_triangles(want["triangles"])), what
    assert np.array_equal(iso.rotated_triangles(t), iso.rotated_triangles(want["triangles"])), what      # and in the documented order


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_fields_equal_the_reference(shape, level):
    rng = np.random.default_rng(shape[0] * 7919 + shape[1] * 31 + shape[2])
    f = rng.random(shape).astype(np.float32)
    # both affines with the cap off and on over the three levels of a shape; the cap's fill lies below every level
    first, second = (None, SWAPPED) if level != 0.05 else (SWAPPED, None)
    for affine, cap in ((first, False), (second, True)):
        what = (shape, level, "swapped" if affine else "identity", "capped" if cap else "open")
        got = _extract(f, level, affine, cap, fill=-1.0)
        _same_mesh(got, _reference(f, level, affine, cap, fill=-1.0), what)
        again = _extract(f, level, affine, cap, fill=-1.0)
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and again[2] == got[2], what
        if cap:
            assert got[2]["B"] == 0, what                                      # closed where the surface would leave the grid
        elif min(shape) == 1:
            assert got[2]["V"] == got[2]["T"] == got[2]["E"] == got[2]["B"] == 0, what      # no cube: an empty mesh, not an error


def test_exact_values_leave_a_closed_mesh():
    rng = np.random.default_rng(11)
    f = rng.integers(0, 3, (7, 6, 9)).astype(np.float32)                  # a third of the voxels exactly at the level
    for affine in (None, SWAPPED):
        got = _extract(f, 1.0, affine, cap=True, fill=0.0)
        _same_mesh(got, _reference(f, 1.0, affine, True, 0.0), affine)
        t = got[1].astype(np.int64)
        directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
        keys = directed[:, 0] * got[2]["V"] + directed[:, 1]
        assert len(np.unique(keys)) == len(keys) and got[2]["B"] == 0       # combinatorially closed: every directed edge once ...
        assert np.array_equal(np.sort(keys), np.sort(directed[:, 1] * got[2]["V"] + directed[:, 0]))      # ... and its reverse once
        assert np.isfinite(got[0]).all()
        area = iso.measure_terms(got[0], got[1])[0]
        assert (area == 0).any()                                            # degenerate triangles are allowed, and occur


def test_capacities_are_respected_and_counts_stay_true():
    from nerf_for_angiography_amd.engine import isosurface_record
    f = np.random.default_rng(12).random((9, 17, 33)).astype(np.float32)
    want = iso.isosurface(f, 0.5, SWAPPED)
    x = _dev(f)
    V, T = want["V"], want["T"]
    full = isosurface_record(x, 0.5, SWAPPED, V, T)
    assert full[2].cpu().tolist() == [V, T, want["E"], want["B"], want["n22"], 0, 0, 0]
    count = isosurface_record(x, 0.5, SWAPPED)[2].cpu().tolist()
    assert count == [V, T, want["E"], want["B"], want["n22"], 3, 0, 0]                       # the counting call: both bits, true counts
    guard = 64
    for cap_v, cap_t, status in ((V - 1, T, 1), (V, T - 1, 2), (V // 3, T // 2, 3), (1, 1, 3), (V + 5, T + 5, 0)):
        verts = torch.full((cap_v + guard, 3), -7.0, dtype=torch.float32, device=DEV)
        tris = torch.full((cap_t + guard, 3), -7, dtype=torch.int32, device=DEV)
        rec = isosurface_record(x, 0.5, SWAPPED, cap_v, cap_t, vertices=verts, triangles=tris)[2].cpu().tolist()
        assert rec == [V, T, want["E"], want["B"], want["n22"], status, 0, 0], (cap_v, cap_t)
        kv, kt = min(cap_v, V), min(cap_t, T)
        assert torch.equal(verts[:kv], full[0][:kv]) and torch.equal(tris[:kt], full[1][:kt])         # what fits is what a full call writes
        assert (verts[kv:] == -7.0).all() and (tris[kt:] == -7).all(), (cap_v, cap_t)                   # nothing beyond


def test_error_codes():
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd._lib import AfxError
    from nerf_for_angiography_amd.engine import extract_isosurface, isosurface_record
    lib = _lib.load()
    x = torch.rand(4, 5, 6, device=DEV)
    rec = torch.zeros(8, dtype=torch.int64, device=DEV)
    need = int(lib.afx_isosurface_3d_workspace_bytes(4, 5, 6))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    verts = torch.empty(8, 3, device=DEV)
    tris = torch.empty(8, 3, dtype=torch.int32, device=DEV)
    ident = (C.c_double * 12)(*iso.IDENTITY)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(f=p(x), shape=(4, 5, 6), level=0.5, aff=ident, v=p(verts), nv=8, t=p(tris), nt=8, r=p(rec), w=p(ws), wb=need):
        return lib.afx_isosurface_3d(f, *shape, level, aff, v, nv, t, nt, r, w, wb, None, None)
    assert call() == 0
    nan = float("nan")
    for kw in (dict(f=None), dict(r=None), dict(aff=None), dict(shape=(0, 5, 6)), dict(shape=(4, 5, 1025)), dict(level=nan), dict(nv=-1),
               dict(nt=2 ** 31), dict(v=None), dict(t=None), dict(aff=(C.c_double * 12)(*([0.0] * 12))),
               dict(aff=(C.c_double * 12)(1, 2, 3, 0, 2, 4, 6, 0, 0, 0, 1, 0)), dict(aff=(C.c_double * 12)(*((nan,) + iso.IDENTITY[1:])))):
        assert call(**kw) == AFX_E_INVALID, kw
    assert call(w=None) == AFX_E_WORKSPACE and call(wb=need - 1) == AFX_E_WORKSPACE
    torch.cuda.synchronize()
    with pytest.raises(AfxError):
        isosurface_record(torch.rand(4, 4, 1025, device=DEV), 0.5)
    with pytest.raises(AfxError, match="no CPU path"):
        extract_isosurface(torch.rand(4, 4, 4), 0.5)
    with pytest.raises(ValueError, match="must lie below iso"):
        extract_isosurface(x, 0.5, cap=True, fill=0.5)
    with pytest.raises(ValueError, match="12 numbers"):
        extract_isosurface(x, 0.5, index_to_world=[1.0] * 9)


def test_a_plane_has_its_exact_area():
    from nerf_for_angiography_amd.engine import mesh_measures
    for shape in ((6, 5, 7), (4, 33, 9)):
        f = np.broadcast_to(np.arange(shape[0], dtype=np.float32)[:, None, None], shape)
        v, t, info = _extract(f, 2.5)
        # the plane cuts all six tetrahedra of a cube: four into one triangle, two (those whose second step is along axis 0) into two
        assert info["T"] == 8 * (shape[1] - 1) * (shape[2] - 1) and info["euler"] == 1 and (v[:, 0] == 2.5).all()
        m = mesh_measures(_dev(v), _dev(t))
        assert m["area"] == float((shape[1] - 1) * (shape[2] - 1))           # every coordinate is dyadic: exact
        assert (np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])[:, 0] < 0).all()      # inside is i0 >= 2.5: the normals look down the axis


@functools.lru_cache(maxsize=None)
def _known(name):
    return {"sphere": iso.sphere_field, "torus": iso.torus_field, "two spheres": iso.two_spheres_field}[name](24)


@pytest.mark.parametrize("name, chi", [("sphere", 2), ("torus", 0), ("two spheres", 4)])
def test_euler_characteristic_of_known_surfaces(name, chi):
    from nerf_for_angiography_amd.engine import mesh_measures
    for affine in (None, SWAPPED):
        v, t, info = _extract(_known(name), 0.0, affine, cap=True, fill=-1.0)
        assert info["euler"] == chi and info["B"] == 0 and info["V"] > 0, (name, info)
        assert mesh_measures(_dev(v), _dev(t))["volume"] > 0, name              # outward normals whatever the sign of det(m)


def _sum_bound(n_terms, abs_sum):
    """A fixed-order fp64 sum of n terms errs by at most n 2^-53 times the sum of their magnitudes, and a term computed by a handful of
    fp64 operations by a few 2^-53 of its own: (T + 16) 2^-52 sum |term| covers both, for the device's sum and the reference's."""
    return (n_terms + 16) * 2.0 ** -52 * abs_sum


def test_measures_against_the_exact_sums():
    from nerf_for_angiography_amd.engine import isosurface_record, mesh_measures, mesh_measures_record
    rng = np.random.default_rng(13)
    f = rng.random((17, 18, 19)).astype(np.float32)
    for affine, cap in ((None, False), (SWAPPED, True)):
        v, t, info = _extract(f, 0.5, affine, cap, fill=0.0)
        ref = tuple(float(c) for c in (v.min(axis=0).astype(np.float64) + v.max(axis=0).astype(np.float64)) / 2)
        got = mesh_measures(_dev(v), _dev(t), ref)
        area, vol = iso.measure_terms(v, t, ref)
        for key, terms in (("area", area), ("volume", vol)):
            want, bound = math.fsum(terms), _sum_bound(len(terms), math.fsum(np.abs(terms)))
            print(f"{key}: got {got[key]!r} want {want!r} diff {abs(got[key] - want):.3e} bound {bound:.3e} (T = {len(terms)})")
            assert abs(got[key] - want) <= bound, (key, cap)
        assert mesh_measures(_dev(v), _dev(t)) == got                           # the default reference point is the one computed above
        if cap:
            # a general field: the fp32 rounding of the vertices (at most 2^-24 of the largest coordinate, per coordinate) moves the enclosed
            # volume by at most the area times that displacement to first order; twice that covers the second order.  A missing or
            # turned triangle changes the volume by its own term, orders of magnitude more.
            clip, n_clip, clip_abs = iso.clipped_volume(iso.padded(f, 0.0), 0.5, iso.shifted_affine(affine))
            slack = 2.0 * math.sqrt(3.0) * 2.0 ** -24 * float(np.abs(v).max()) * got["area"]
            print(f"volume {got['volume']!r} clipped {clip!r} diff {abs(got['volume'] - clip):.3e} slack {slack:.3e}")
            assert got["volume"] > 0 and abs(got["volume"] - clip) <= slack + _sum_bound(len(vol) + n_clip, math.fsum(np.abs(vol)) + clip_abs)
    # extract-then-measure without a host round trip: V and T come from the record on the device, the buffers are larger than the mesh
    x = _dev(f)
    verts, tris, rec = isosurface_record(x, 0.5, SWAPPED, 7 * f.size, 12 * f.size)
    out = mesh_measures_record(verts, tris, rec, (1.0, 2.0, 3.0)).cpu().tolist()
    v, t, _ = _extract(f, 0.5, SWAPPED)
    area, vol = iso.measure_terms(v, t, (1.0, 2.0, 3.0))
    assert abs(out[0] - math.fsum(area)) <= _sum_bound(len(area), math.fsum(np.abs(area)))
    assert abs(out[1] - math.fsum(vol)) <= _sum_bound(len(vol), math.fsum(np.abs(vol)))
    again = mesh_measures_record(verts, tris, rec, (1.0, 2.0, 3.0)).cpu().tolist()
    assert again == out                                                         # a fixed order: the same bits


def test_capped_volume_equals_the_clipped_volume():
    """On a field whose crossings fall on quarters of the edges (values -3, -1, 1, 3 at the level 0) under an affine with dyadic entries
    every vertex is exact in fp32, so the mesh encloses exactly the region the interpolant clips: the two fp64 sums agree to their own
    rounding.  Any missing triangle, or one wound the wrong way, breaks this by its whole term."""
    from nerf_for_angiography_amd.engine import mesh_measures
    rng = np.random.default_rng(14)
    f = rng.choice(np.array([-3.0, -1.0, 1.0, 3.0], dtype=np.float32), size=(9, 12, 10))
    for affine in (None, SWAPPED):
        v, t, info = _extract(f, 0.0, affine, cap=True, fill=-3.0)
        assert info["B"] == 0 and info["T"] > 1000
        ref = (1.0, 2.0, 3.0)
        got = mesh_measures(_dev(v), _dev(t), ref)
        _, vol = iso.measure_terms(v, t, ref)
        clip, n_clip, clip_abs = iso.clipped_volume(iso.padded(f, -3.0), 0.0, iso.shifted_affine(affine))
        bound = _sum_bound(len(vol) + n_clip, math.fsum(np.abs(vol)) + clip_abs)
        print(f"volume {got['volume']!r} clipped {clip!r} diff {abs(got['volume'] - clip):.3e} bound {bound:.3e}")
        assert got["volume"] > 0 and abs(got["volume"] - clip) <= bound


def test_worst_case_capacities_replay_from_a_graph():
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.engine import isosurface_record
    shape = (33, 17, 65)
    n = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng(15)
    a, b = _dev(rng.random(shape).astype(np.float32)), _dev(iso.torus_field(65)[16:49, 24:41, :].copy() + np.float32(0.5))
    eager = {name: isosurface_record(x, 0.5, SWAPPED, 7 * n, 12 * n) for name, x in (("a", a), ("b", b))}
    static_x = a.clone()
    ws = torch.empty(int(_lib.load().afx_isosurface_3d_workspace_bytes(*shape)), dtype=torch.uint8, device=DEV)
    verts = torch.zeros(7 * n, 3, dtype=torch.float32, device=DEV)
    tris = torch.zeros(12 * n, 3, dtype=torch.int32, device=DEV)
    rec = torch.zeros(8, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            isosurface_record(static_x, 0.5, SWAPPED, 7 * n, 12 * n, vertices=verts, triangles=tris, record=rec, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    for name, x in (("b", b), ("a", a)):
        static_x.copy_(x)
        for t in (verts, tris, rec, ws):
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        ev, et, er = eager[name]
        V, T = int(er[0]), int(er[1])
        assert V > 0 and torch.equal(rec, er) and torch.equal(verts[:V], ev[:V]) and torch.equal(tris[:T], et[:T]), name
        assert (verts[V:] == 7).all() and (tris[T:] == 7).all()


def test_reconstruction_mesh_of_a_sphere():
    from nerf_for_angiography_amd.phantomdata.helpers import VoxelVolume
    from nerf_for_angiography_amd.visualization.sweep import ground_truth_grid, reconstruction_mesh, reconstruction_mesh_metrics
    axis = np.linspace(-100.0, 100.0, 21)
    centre, radius = np.array([10.0, -20.0, 5.0]), 55.0
    r = np.linalg.norm(np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1) - centre, axis=-1)
    vol = VoxelVolume(axis, axis, axis, np.clip((radius - r) / 40.0 + 0.5, 0.0, 1.0), fill_value=0.0, device=DEV)
    n = 25
    step = 200.0 / (n - 1)
    gt = ground_truth_grid(vol, 100.0, n)
    grids = (gt.clone(), gt)                                   # the stand-in for a model: a reconstruction equal to the truth
    v, t, info, pred, ref = reconstruction_mesh(None, vol, 100.0, n, threshold=0.5, grids=grids)
    assert pred is grids[0] and ref is gt and info["euler"] == 2 and info["B"] == 0 and info["threshold"] == 0.5
    dist = np.linalg.norm(v.cpu().numpy().astype(np.float64) - centre, axis=1)      # world coordinates: (x, y, z), not the grid's (i0, i1, i2)
    assert np.abs(dist - radius).max() < step, (dist.min(), dist.max())
    # the radius is off by less than 2 (two linear interpolations of a distance, at spacings 10 and 8.3: h^2 / (8 r) per axis and pass):
    # the volume by less than 3 * 2 / 55, the area by less than 2 * 2 / 55, and a polyhedron inscribed at this step loses a few per cent more
    assert abs(info["volume"] / (4.0 / 3.0 * math.pi * radius ** 3) - 1.0) < 0.15 and abs(info["area"] / (4.0 * math.pi * radius ** 2) - 1.0) < 0.15
    lcc = reconstruction_mesh(None, vol, 100.0, n, threshold=0.5, largest_component=True, grids=grids)
    assert lcc[2]["euler"] == 2 and 0.8 < lcc[2]["volume"] / info["volume"] < 1.2
    scores, _, _ = reconstruction_mesh_metrics(None, vol, 100.0, n, threshold=0.5, grids=grids)
    assert scores["volume_ratio"] == 1.0 and scores["area_ratio"] == 1.0 and scores["euler"] == scores["euler_gt"] == 2
    assert scores["n_triangles"] == info["T"] and scores["volume"] == info["volume"] and scores["voxel_size"] == step
    with pytest.raises(ValueError, match="pred or gt"):
        reconstruction_mesh_metrics(None, vol, 100.0, n, threshold=2.0, grids=grids)


def test_sweep_mesh_columns(golden):
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from nerf_for_angiography_amd.visualization.sweep import CENTRELINE_METRICS, MESH_METRICS, evaluation_sweep, reconstruction_mesh_metrics
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    n = 25
    scores, pred, ref = reconstruction_mesh_metrics(m, vol, 100.0, n)
    assert scores["threshold"] == float(torch.mean(ref)) and scores["volume"] > 0 and scores["volume_gt"] > 0
    df, _ = evaluation_sweep(m, gt, angles, *geo, metrics=["EULER 3D", "PSNR", "AREA RATIO 3D", "TSENS 3D", "VOLUME RATIO 3D"], volume=vol,
                             volume_outside=100.0, volume_points=n)
    assert list(df.columns) == BASE + ["PSNR", "TSENS 3D"] + list(MESH_METRICS)
    assert list(df.columns).index(CENTRELINE_METRICS[2]) < list(df.columns).index(MESH_METRICS[0])
    for col, key in zip(MESH_METRICS, ("volume_ratio", "area_ratio", "euler")):
        assert df[col].nunique() == 1 and df[col][0] == scores[key], col                       # one value per column, repeated on every row


DRIVER = ["--synthetic", "--img_size", "16", "--num_layers", "4", "--num_hidden_units", "64", "--sample_size", "8", "--depth_samples", "32",
          "--n_iters", "4", "--display_every", "2", "--out_bias_init", "0.0"]      # (sigma ~ 0.5 everywhere: the 0.5 level is a real surface)


def test_driver_saves_the_mesh(tmp_path):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import check_args, build_parser, main
    plain = main(DRIVER + ["--log_dir", str(tmp_path / "a")])
    assert "mesh_info" not in plain
    for k, name in enumerate(("vessel.stl", "vessel.vtk")):
        out = main(DRIVER + ["--log_dir", str(tmp_path / f"b{k}"), "--save_mesh", str(tmp_path / name), "--mesh_threshold", "0.5"])
        info = out["mesh_info"]
        assert torch.equal(out["model"].flat_params, plain["model"].flat_params)               # the flag changes nothing else
        assert info["T"] > 0 and info["B"] == 0 and info["path"] == str(tmp_path / name)
        if name.endswith(".stl"):
            assert len(read_stl(info["path"])[1]) == info["T"]
        else:
            pts, tri = read_vtk(info["path"])
            assert len(pts) == info["V"] and len(tri) == info["T"] and tri.max() == info["V"] - 1
    with pytest.raises(ValueError, match=".stl or .vtk"):
        check_args(build_parser().parse_args(DRIVER + ["--save_mesh", "vessel.obj"]))
