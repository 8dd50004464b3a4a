"""The signed distance field of a triangle mesh on the GPU (afx_mesh_sdf_3d, afx_mesh_point_distance; engine.mesh_signed_distance /
mesh_point_distance and their *_record forms, phantomdata.helpers.voxel_volume_from_mesh, the synthetic dataset and the driver on a mesh
phantom, the mesh-distance columns of the evaluation sweep) against the NumPy restatement of tests/mesh_sdf_reference.py.  The distance
and the nearest triangle are defined operation by operation: they must EQUAL the reference bit for bit, with the culling and without;
the sign must equal the reference's at every point (the tests first make sure that the reference's winding number is nowhere near one
half); the winding number itself goes through the library's atan2 and a sum of up to 4 000 terms of about 1e-15 of rounding each: 1e-10.

On a closed mesh the winding number is an integer at every point OFF the surface, and that is what the tests require of the reference
(within 1e-6) before they compare signs.  A grid point ON the surface - the identity grid puts over a hundred on the vertices of the
integer-valued field - has a fractional winding number by nature (one half on a flat piece) and no sign to decide: its distance is 0 and
the result +0.0 by definition, which is asserted instead.  Every point's value, sign included, is compared with the reference."""
import functools

import numpy as np
import pytest
import torch

import isosurface_reference as iso
import mesh_sdf_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDENTITY = None
# index (i0, i1, i2) -> anisotropic steps and a shear, laid over the meshes below (which live in about [-1, 9]^3); det > 0.  The steps are
# chosen off the half-integer lattice the vertices of the integer-valued field lie on: a grid point ON the surface has a fractional
# winding number (one half on a flat piece), and one a rounding error off it has the sign a rounding error gives it.  The identity does
# put grid points on that surface, at distance exactly 0: there the result is +0.0 whatever the winding number says.
SHEARED = (0.913, 0.257, 0.0, -1.531, 0.0, 1.117, 0.303, -1.013, 0.211, 0.0, 0.613, -0.507)
# the first two axes exchanged (the density grid's layout), anisotropic; det < 0
FLIPPED = (0.0, 1.307, 0.0, -1.011, 0.709, 0.0, 0.0, -0.503, 0.0, 0.0, 0.811, 0.253)
AFFINES = {"identity": IDENTITY, "sheared": SHEARED, "flipped": FLIPPED}
# one point; a flat grid; exactly one brick; a one-point-thick partial brick along the slow and along the fast axis; several partial
# bricks on every axis; a long thin grid that leaves the mesh far behind
SHAPES = [(1, 1, 1), (2, 3, 1), (8, 8, 8), (9, 8, 8), (8, 8, 9), (17, 9, 10), (3, 5, 70)]


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "random":
        return ref.capped_mesh(np.random.default_rng(21).random((7, 6, 9)).astype(np.float32), 0.5)
    if name == "exact":          # the field of test_gpu_isosurface.py::test_exact_values_leave_a_closed_mesh: degenerate triangles, a grid point at distance 0
        return ref.capped_mesh(np.random.default_rng(11).integers(0, 3, (7, 6, 9)).astype(np.float32), 1.0, fill=0.0)
    if name == "torus":
        return ref.capped_mesh(iso.torus_field(17), 0.0)
    if name == "open":           # the uncapped random field: the surface ends where it leaves the grid
        return ref.open_mesh(np.random.default_rng(21).random((7, 6, 9)).astype(np.float32), 0.5)
    if name == "small":          # a closed surface of about 4 index units across
        v, t = ref.capped_mesh(iso.sphere_field(8), 0.0)
        return (v * np.float32(0.5)).astype(np.float32), t
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name, shape, affine_name):
    v, t = _mesh(name)
    return ref.mesh_sdf(v, t, shape, AFFINES[affine_name])


def _gpu(v, t, shape, affine, **kw):
    """-> (sdf, nearest, winding or None, record) as arrays"""
    from nerf_for_angiography_amd.engine import mesh_signed_distance
    winding = kw.pop("return_winding", False)
    out = mesh_signed_distance(_dev(v, np.float32), _dev(t, np.int32), shape, affine, return_nearest=True, return_winding=winding,
                               return_record=True, **kw)
    sdf, nearest = out[0], out[1]
    assert sdf.dtype == torch.float32 and nearest.dtype == torch.int32 and tuple(sdf.shape) == tuple(shape) == tuple(nearest.shape)
    return sdf.cpu().numpy(), nearest.cpu().numpy(), out[2].cpu().numpy() if winding else None, out[-1]


def _same_distance(got, want, what):
    """|sdf| and the nearest index equal the reference bit for bit"""
    assert np.abs(got[0]).tobytes() == np.abs(want["sdf"]).tobytes(), what
    assert np.array_equal(got[1], want["nearest"]), what


@pytest.mark.parametrize("affine_name", list(AFFINES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", ["random", "exact", "torus", "open"])
def test_distance_nearest_and_sign_equal_the_reference(name, shape, affine_name):
    v, t = _mesh(name)
    affine = AFFINES[affine_name]
    want = _reference(name, shape, affine_name)
    n = int(np.prod(shape))
    what = (name, shape, affine_name)
    culled = _gpu(v, t, shape, affine, return_winding=True)
    brute = _gpu(v, t, shape, affine, brute=True)
    _same_distance(culled, want, what)
    _same_distance(brute, want, what)
    assert culled[3]["valid_triangles"] == len(t) and culled[3]["skipped_triangles"] == 0 and culled[3]["clear_bricks"] == 0
    assert brute[3]["pairs_evaluated"] == n * len(t) and culled[3]["pairs_evaluated"] <= n * len(t), what
    w = want["winding"]
    off = want["d2"] > 0          # a point ON the surface (d = 0) has a fractional winding number and no sign to decide: +0.0 by definition
    assert off.all() or (name == "exact" and affine_name == "identity"), what
    assert not np.signbit(want["sdf"][~off]).any() and not np.signbit(culled[0][~off]).any(), what
    if name == "open":
        assert (np.abs(w - 0.5) >= 1e-6).all(), what               # no point of the reference sits on the fence: every sign is compared
    else:
        assert (np.abs(w - np.round(w))[off] < 1e-6).all(), what   # a closed mesh: an integer off the surface, so no point is left out
    assert np.abs(culled[2] - w).max() <= 1e-10, (what, np.abs(culled[2] - w).max())
    assert culled[0].tobytes() == want["sdf"].tobytes() and brute[0].tobytes() == want["sdf"].tobytes(), what      # distance and sign
    if name == "exact" and affine_name == "identity" and shape == (8, 8, 8):
        assert (~off).sum() > 50                                                                       # d = 0 does occur
    if name != "open":
        closed = _gpu(v, t, shape, affine, closed=True)
        assert closed[0].tobytes() == culled[0].tobytes() and np.array_equal(closed[1], culled[1]), what


def test_triangle_counts_around_the_lds_tile():
    from nerf_for_angiography_amd.engine import MESH_SDF_TILE as K
    v, t = _mesh("torus")
    assert len(t) >= 2 * K + 1
    shape = (9, 8, 8)
    for count in (0, 1, K - 1, K, K + 1, 2 * K + 1):
        # (cut from the middle of the list too, so that the bricks see different neighbourhoods)
        tris = t[:count] if count <= K else np.concatenate([t[:K], t[-(count - K):]])
        want = ref.mesh_sdf(v, tris, shape, SHEARED)
        for brute in (False, True):
            got = _gpu(v, tris, shape, SHEARED, brute=brute)
            _same_distance(got, want, (count, brute))
            assert got[3]["valid_triangles"] == count
        if count == 0:
            assert np.isposinf(got[0]).all() and (got[1] == -1).all()
        # (the record's pair count is what the culling left of N T: never more, and all of it without culling)
    # without vertices either
    empty = _gpu(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), (2, 3, 1), None, closed=True)
    assert np.isposinf(empty[0]).all() and (empty[1] == -1).all() and empty[3]["valid_triangles"] == 0


def test_culling_is_exercised_and_exact():
    v, t = _mesh("small")
    shape = (24, 24, 24)
    n = 24 ** 3
    # inside the brick of the points 8..15 on every axis: the mesh spans about [0.3, 3.2] after the scaling, moved to about [10.3, 13.2]
    inside = (v + np.float32(10.0)).astype(np.float32)
    assert inside.min() > 8.5 and inside.max() < 14.5
    far = (v + np.float32(1000.0)).astype(np.float32)
    for name, verts in (("inside one brick", inside), ("far outside", far)):
        culled = _gpu(verts, t, shape, None)
        brute = _gpu(verts, t, shape, None, brute=True)
        assert culled[0].tobytes() == brute[0].tobytes() and np.array_equal(culled[1], brute[1]), name
        assert brute[3]["pairs_evaluated"] == n * len(t)
        assert 0 < culled[3]["pairs_evaluated"] < n * len(t), name            # a condition on the mechanism, not a timing
        closed = _gpu(verts, t, shape, None, closed=True)
        assert closed[0].tobytes() == culled[0].tobytes() and np.array_equal(closed[1], culled[1]), name
        if name == "far outside":
            assert closed[3]["clear_bricks"] == 27 and (culled[0] > 0).all()   # every brick is clear
        else:
            assert 1 <= closed[3]["clear_bricks"] < 27 and (culled[0] < 0).any() and (culled[0] > 0).any()
    # against the reference where the host can afford it: the bricks around the mesh (N T stays below 10^7)
    sub = (12, 12, 12)
    off = (1.0, 0.0, 0.0, 6.0, 0.0, 1.0, 0.0, 6.0, 0.0, 0.0, 1.0, 6.0)
    want = ref.mesh_sdf(inside, t, sub, off)
    got = _gpu(inside, t, sub, off)
    assert got[0].tobytes() == want["sdf"].tobytes() and np.array_equal(got[1], want["nearest"])
    whole = _gpu(inside, t, shape, None)
    assert whole[0][6:18, 6:18, 6:18].tobytes() == want["sdf"].tobytes()


def test_ties_go_to_the_smallest_index():
    v, t = _mesh("exact")
    twice = np.concatenate([t, t])
    once = _gpu(v, t, (9, 8, 8), SHEARED)
    for brute in (False, True):
        got = _gpu(v, twice, (9, 8, 8), SHEARED, brute=brute)
        assert (got[1] < len(t)).all() and np.array_equal(got[1], once[1]) and np.abs(got[0]).tobytes() == np.abs(once[0]).tobytes()
        assert got[3]["valid_triangles"] == 2 * len(t)


def test_rejected_triangles_are_skipped_and_counted():
    from nerf_for_angiography_amd.engine import mesh_point_distance_record
    v, t = _mesh("random")
    rng = np.random.default_rng(5)
    v = v.copy()
    t = t.copy()
    v[rng.choice(len(v), 7, replace=False), rng.integers(0, 3, 7)] = (np.nan, np.inf, -np.inf, np.nan, np.nan, np.inf, np.nan)
    rows = rng.choice(len(t), 9, replace=False)
    t[rows, rng.integers(0, 3, 9)] = (-1, len(v), len(v) + 5, 2 ** 31 - 1, -2 ** 31, -7, len(v), -1, len(v) + 1)
    keep, _, _, _ = ref.valid_triangles(v, t)
    assert 0 < len(keep) < len(t) - 9                                           # the non-finite vertices take their triangles along
    clean = t[keep]
    shape = (9, 8, 9)
    for brute in (False, True):
        got = _gpu(v, t, shape, SHEARED, brute=brute)
        want = _gpu(np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0), clean, shape, SHEARED, brute=brute)
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], keep[want[1]]), brute
        assert got[3]["valid_triangles"] == len(keep) and got[3]["skipped_triangles"] == len(t) - len(keep)
    host = ref.mesh_sdf(v, t, shape, SHEARED)
    assert got[0].tobytes() == host["sdf"].tobytes() and np.array_equal(got[1], host["nearest"])
    pts = _dev(ref.grid_points((3, 3, 3), SHEARED), np.float32)
    dist, rec = mesh_point_distance_record(pts, _dev(v, np.float32), _dev(t, np.int32))
    assert rec.cpu().tolist()[:4] == [len(keep), len(t) - len(keep), 0, 27 * len(keep)]
    assert dist.cpu().numpy().tobytes() == ref.point_distance(pts.cpu().numpy(), v, t)[0].tobytes()


def test_point_distance_equals_the_reference():
    from nerf_for_angiography_amd.engine import mesh_point_distance
    va, ta = _mesh("random")
    vb, tb = _mesh("torus")
    vd, td = _dev(vb, np.float32), _dev(tb, np.int32)
    for count in (1, 63, 64, 65, 257, len(va)):          # around a wave, beyond one workgroup, the vertices of one mesh against the other
        pts = va[:count]
        want = ref.point_distance(pts, vb, tb)
        dist, nearest = mesh_point_distance(_dev(pts, np.float32), vd, td, return_nearest=True)
        assert dist.dtype == torch.float32 and nearest.dtype == torch.int32 and dist.shape == (count,)
        assert dist.cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(nearest.cpu().numpy(), want[1]), count
    alone = mesh_point_distance(_dev(va[:5], np.float32), vd, td)
    assert torch.equal(alone, dist[:5])
    none = mesh_point_distance(_dev(va[:5], np.float32), vd, td[:0], return_nearest=True)
    assert torch.isposinf(none[0]).all() and (none[1] == -1).all()
    assert mesh_point_distance(_dev(va[:0], np.float32), vd, td).shape == (0,)


def test_determinism_and_graph_replay():
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.engine import MESH_SDF_CLOSED, mesh_point_distance_record, mesh_sdf_record
    v, t = _mesh("torus")
    shape = (17, 9, 10)
    first = _gpu(v, t, shape, FLIPPED, return_winding=True)
    again = _gpu(v, t, shape, FLIPPED, return_winding=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], again[:3])) and first[3] == again[3]
    vd, td = _dev(v, np.float32), _dev(t, np.int32)
    pts = _dev(_mesh("random")[0], np.float32)
    eager_sdf, eager_rec = mesh_sdf_record(vd, td, shape, FLIPPED, MESH_SDF_CLOSED)
    eager_dist, eager_prec = mesh_point_distance_record(pts, vd, td)
    n = int(np.prod(shape))
    sdf = torch.zeros(shape, dtype=torch.float32, device=DEV)
    nearest = torch.zeros(shape, dtype=torch.int32, device=DEV)
    rec = torch.zeros(8, dtype=torch.int64, device=DEV)
    ws = torch.zeros(int(_lib.load().afx_mesh_sdf_3d_workspace_bytes(len(t))), dtype=torch.uint8, device=DEV)
    dist = torch.zeros(len(pts), dtype=torch.float32, device=DEV)
    pnear = torch.zeros(len(pts), dtype=torch.int32, device=DEV)
    prec = torch.zeros(8, dtype=torch.int64, device=DEV)
    static_v = vd.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            mesh_sdf_record(static_v, td, shape, FLIPPED, MESH_SDF_CLOSED, sdf=sdf, nearest=nearest, record=rec, workspace=ws)
            mesh_point_distance_record(pts, static_v, td, dist=dist, nearest=pnear, record=prec)
    torch.cuda.current_stream().wait_stream(side)
    for buf in (sdf, nearest, rec, ws, dist, pnear, prec):
        buf.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sdf, eager_sdf) and torch.equal(rec, eager_rec) and torch.equal(dist, eager_dist) and torch.equal(prec, eager_prec)
    assert np.array_equal(nearest.cpu().numpy(), first[1]) and sdf.cpu().numpy().tobytes() == first[0].tobytes() and n == sdf.numel()
    static_v.copy_(vd + 0.25)                                   # the replay reads the buffers as they are now
    graph.replay()
    torch.cuda.synchronize()
    moved = mesh_sdf_record(vd + 0.25, td, shape, FLIPPED, MESH_SDF_CLOSED)
    assert torch.equal(sdf, moved[0]) and torch.equal(rec, moved[1]) and not torch.equal(sdf, eager_sdf)


def test_library_refusals_on_the_device():
    from nerf_for_angiography_amd._lib import AfxError
    from nerf_for_angiography_amd.engine import mesh_sdf_record, mesh_signed_distance
    v, t = (_dev(x, d) for x, d in zip(_mesh("small"), (np.float32, np.int32)))
    with pytest.raises(AfxError, match="1..1024"):
        mesh_signed_distance(v, t, (4, 4, 1025))
    with pytest.raises(AfxError, match="singular"):
        mesh_signed_distance(v, t, (4, 4, 4), [1.0, 2.0, 3.0, 0.0, 2.0, 4.0, 6.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    with pytest.raises(AfxError, match="flag"):
        mesh_sdf_record(v, t, (4, 4, 4), flags=8)
    with pytest.raises(AfxError, match="workspace"):
        mesh_sdf_record(v, t, (4, 4, 4), workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="12 numbers"):
        mesh_signed_distance(v, t, (4, 4, 4), [1.0] * 9)


# ---- through the layers
PHANTOM_POINTS = 17          # 17 x 17 x 8 points against 3 760 triangles on the host: below 10^7 pairs


@functools.lru_cache(maxsize=None)
def _torus_phantom():
    from nerf_for_angiography_amd.phantomdata.helpers import voxel_volume_from_mesh
    v, t = _mesh("torus")
    vol, sdf = voxel_volume_from_mesh(v, t, n=PHANTOM_POINTS, margin=0.1, vol_scale=10.0, closed=True, device=DEV, return_sdf=True)
    return vol, sdf


def test_voxel_volume_from_mesh():
    from nerf_for_angiography_amd.phantomdata.helpers import rev_sigmoid, voxel_volume_from_mesh
    v, t = _mesh("torus")
    vol, sdf = _torus_phantom()
    shape = tuple(vol.values.shape)
    assert max(shape) == PHANTOM_POINTS and min(shape) >= 2                         # n points along the longest side ...
    steps = vol.spacing
    assert np.allclose(steps, steps[0], rtol=1e-12)                                 # ... the same spacing on every axis
    scaled = v.astype(np.float64) * 10.0
    mid = (scaled.min(axis=0) + scaled.max(axis=0)) / 2
    moved = (scaled - mid).astype(np.float32)
    longest = (scaled.max(axis=0) - scaled.min(axis=0)).max()
    assert abs(steps[0] - 1.2 * longest / (PHANTOM_POINTS - 1)) <= 1e-9 * longest
    for k in range(3):                                                              # the grid covers the box grown by the margin, centred on it
        assert vol.axes[k][0] <= moved[:, k].min() - 0.1 * longest + 1e-6 and vol.axes[k][-1] >= moved[:, k].max() + 0.1 * longest - 1e-6
        assert abs(vol.axes[k][0] + vol.axes[k][-1]) <= 1e-6
    affine = (steps[0], 0.0, 0.0, vol.origin[0], 0.0, steps[1], 0.0, vol.origin[1], 0.0, 0.0, steps[2], vol.origin[2])
    want = ref.mesh_sdf(moved, t, shape, affine)
    assert sdf.cpu().numpy().tobytes() == want["sdf"].tobytes()                     # the field bit for bit ...
    values = vol.values.cpu().numpy()
    assert np.abs(values - rev_sigmoid(want["sdf"].astype(np.float64), 2)).max() <= 1e-6      # ... its transfer to 1e-6 (exp's last place)
    assert vol.fill_value == float(values.min()) and values.max() > 0.9 and values.min() < 0.1
    plain = voxel_volume_from_mesh(torch.from_numpy(v), torch.from_numpy(t), n=PHANTOM_POINTS, margin=0.1, vol_scale=10.0, device=DEV)
    assert torch.equal(plain.values, vol.values)                                    # tensors or arrays, closed or not
    with pytest.raises(ValueError, match="n >= 2"):
        voxel_volume_from_mesh(v, t, n=1, device=DEV)


def test_synthetic_dataset_on_a_mesh_phantom(tmp_path):
    from nerf_for_angiography_amd.phantomdata import dataset as ds
    from nerf_for_angiography_amd.phantomdata.helpers import get_depth_values, get_ray_values, ray_tracing
    vol, _ = _torus_phantom()
    angles = [(90.0, 0.0), (70.0, 15.0)]
    size, samples = 16, 32
    proj_df, ray_df = ds.make_synthetic_dataset(angles, img_size=size, depth_samples_per_ray=samples, device=DEV, phantom=vol,
                                                projection_type="sdf")
    assert list(proj_df.columns) == ds.PROJ_COLUMNS and list(ray_df.columns) == ds.RAY_COLUMNS
    assert len(proj_df) == 2 and len(ray_df) == 2 * size * size
    for k, (theta, phi) in enumerate(angles):
        o, d, _, ii, jj = get_ray_values(theta, phi, 0.0, np.array([0.0, 0.0, 1500.0]), size, size, 13.0 * size, DEV)
        z = get_depth_values(1400.0, 1600.0, samples, DEV, stratified=False)
        want = ray_tracing(vol, None, o, d, z, size, size, ii, jj, None, DEV, type="sdf").cpu().numpy().astype(np.float64)
        got = ray_df[ray_df["image_id"] == k]["pixel_value"].to_numpy().reshape(size, size)
        assert np.array_equal(got, want) and want.std() > 0, k
    ds.save_dataset(proj_df, ray_df, str(tmp_path / "mesh"), "torus", binary=True)
    back_p, back_r, _, _ = ds.load_data("mesh", "torus", False, True, size, None, data_root=str(tmp_path))      # load_data's schema accepts the frames
    assert list(back_p.columns) == ds.PROJ_COLUMNS and list(back_r.columns) == ds.RAY_COLUMNS and len(back_r) == len(ray_df)
    assert np.allclose(np.array(back_p["image_data"].tolist()), np.array(proj_df["image_data"].tolist()))


def test_driver_trains_on_a_mesh_phantom(tmp_path):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    from nerf_for_angiography_amd.visualization.mesh_io import write_mesh
    v, t = _mesh("torus")
    for name in ("vessel.stl", "vessel.vtk"):
        path = write_mesh(tmp_path / name, v, t)
        out = main(["--synthetic", "--phantom_mesh", str(path), "--phantom_points", "33", "--img_size", "16", "--num_layers", "4",
                    "--num_hidden_units", "64", "--sample_size", "8", "--depth_samples", "32", "--n_iters", "20", "--display_every", "10",
                    "--log_dir", str(tmp_path / name.replace(".", "_"))])
        losses = [rec["train_loss"] for rec in out["history"]]
        assert len(losses) >= 2 and np.isfinite(losses).all(), (name, losses)


SWEEP_POINTS = 17


def test_sweep_mesh_distance_columns(golden):
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from nerf_for_angiography_amd.visualization import sweep
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    n = SWEEP_POINTS
    scores, pred, truth = sweep.reconstruction_mesh_distance_metrics(m, vol, 100.0, n)
    v, t, info, _, _ = sweep.reconstruction_mesh(m, vol, 100.0, n, grids=(pred, truth))
    vg, tg, info_gt = sweep._grid_mesh(truth, info["threshold"], 100.0, n)
    assert info["T"] > 0 and info_gt["T"] > 0 and scores["threshold"] == info["threshold"] == float(torch.mean(truth))
    assert scores["n_vertices"] == info["V"] and scores["n_vertices_gt"] == info_gt["V"]
    want = ref.mesh_distance_scores(v.cpu().numpy(), t.cpu().numpy(), vg.cpu().numpy(), tg.cpu().numpy(), 95.0)
    for name, key in zip(sweep.MESH_DISTANCE_METRICS, ("assd", "hd", "hd_percentile")):
        assert want[name] > 0 and abs(scores[key] - want[name]) <= 1e-6 * want[name], (name, scores[key], want[name])
    df, _ = sweep.evaluation_sweep(m, gt, angles, *geo, metrics=["HD95 MESH", "PSNR", "ASSD MESH", "EULER 3D", "HD MESH"], volume=vol,
                                   volume_outside=100.0, volume_points=n)
    assert list(df.columns) == BASE + ["PSNR", "EULER 3D"] + list(sweep.MESH_DISTANCE_METRICS)
    for col, key in zip(sweep.MESH_DISTANCE_METRICS, ("assd", "hd", "hd_percentile")):
        assert df[col].nunique() == 1 and df[col][0] == scores[key], col            # one value per column, repeated on every row
    same, _, _ = sweep.reconstruction_mesh_distance_metrics(None, vol, 100.0, n, grids=(truth.clone(), truth))
    assert same["assd"] == 0.0 and same["hd"] == 0.0 and same["hd_percentile"] == 0.0          # the truth against itself
    none, _, _ = sweep.reconstruction_mesh_distance_metrics(None, vol, 100.0, n, threshold=2.0, grids=(truth.clone(), truth))
    assert all(np.isnan(none[k]) for k in ("assd", "hd", "hd_percentile")) and none["n_vertices"] == 0      # empty meshes: NaN, as the voxel scores
