"""afx_view_map on the CPU: the library's symbol and its argument refusals, the host-side pieces of the engine, the sweep and the driver,
and properties of the NumPy restatement tests/viewmap_reference.py (include/afx.h: afx_view_map).  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import viewmap_reference as vr
from nerf_for_angiography_amd import _lib, engine

AFX_E_INVALID = -1
FAKE = C.c_void_p(0x1000)      # never dereferenced: every refusal below comes before the device is touched


def test_library_exports_the_symbol():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "afx.h")).read()
    assert "afx_view_map" in _lib.exported_symbols() and lib.afx_view_map is not None and " afx_view_map(" in header
    assert "#define AFX_VIEWMAP_SEGMENT_DOUBLES 8" in header and engine.VIEWMAP_SEGMENT_DOUBLES == vr.SEGMENT_DOUBLES == 8
    assert "#define AFX_VIEWMAP_BRUTE 1u" in header and engine.VIEWMAP_BRUTE == 1
    assert "#define AFX_VIEWMAP_TREE_SLOTS 4" in header and engine.VIEWMAP_TREE_SLOTS == 4


def _call(lib, **kw):
    a = dict(segments=FAKE, seg_branch=FAKE, n=5, b=2, views=FAKE, v=3, w=8, h=8, flags=0, count=FAKE, area=FAKE, shared=FAKE, tree=FAKE,
             proj=FAKE, length=FAKE)
    a.update(kw)
    rc = lib.afx_view_map(a["segments"], a["seg_branch"], a["n"], a["b"], a["views"], a["v"], a["w"], a["h"], a["flags"], a["count"], a["area"],
                          a["shared"], a["tree"], a["proj"], a["length"], None)
    return rc, lib.afx_last_error().decode()


REFUSALS = [
    (dict(segments=None), "segments"), (dict(seg_branch=None), "seg_branch"), (dict(views=None), "views"),
    (dict(count=None), "together"), (dict(area=None), "together"), (dict(shared=None), "together"), (dict(tree=None), "together"),
    (dict(count=None, area=None, shared=None, tree=None, proj=None, length=None), "no output"),
    (dict(v=0), "n_views"), (dict(v=65536), "n_views"), (dict(n=0), "n_segments"), (dict(n=-4), "n_segments"), (dict(n=(1 << 30) + 1), "n_segments"),
    (dict(b=0), "n_branches"), (dict(b=65536), "n_branches"), (dict(w=0), "width"), (dict(h=0), "height"), (dict(w=-3), "width"),
    (dict(w=16385), "width"), (dict(flags=6), "flags"),
]


@pytest.mark.parametrize("kw, word", REFUSALS, ids=[f"{'-'.join(k)}:{w}:{n}" for n, (k, w) in enumerate(REFUSALS)])
def test_view_map_refuses(kw, word):
    rc, msg = _call(_lib.load(), **kw)
    assert rc == AFX_E_INVALID and msg.startswith("afx_view_map: ") and word in msg, msg


def test_engine_has_no_cpu_path():
    seg, br = vr.wavy_tree(5, 2, 0)
    rec = engine.hull_view_records(*vr.scene_views(1, 8, 8, 2))
    with pytest.raises(engine.AfxError, match="no CPU path"):
        engine.view_map((torch.from_numpy(seg), torch.from_numpy(br)), torch.from_numpy(rec), 8, 8)
    with pytest.raises(engine.AfxError, match="no CPU path"):
        engine.view_map_record(torch.from_numpy(seg), torch.from_numpy(br), torch.from_numpy(rec), 8, 8)
    with pytest.raises(ValueError, match="no segment"):
        engine.view_map((np.zeros((0, 8)), np.zeros(0, np.int32)), rec, 8, 8)


# ---- the host-side pieces ----
def test_view_map_segments_on_short_branches():
    """A one-point branch is one degenerate segment, a two-point branch one segment with the mean radius, a branch without points has
    none; ids are 1-based and non-decreasing."""
    pts = np.array([[0.0, 0, 0], [1.0, 2, 3], [4.0, 5, 6], [7.0, 8, 9], [7.0, 8, 10], [7.0, 9, 10]])
    radius = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0])
    seg, br = engine.view_map_segments(pts, [0, 1, 3, 3, 6], radius)
    assert seg.dtype == np.float64 and seg.shape == (4, 8) and br.dtype == np.int32 and br.tolist() == [1, 2, 4, 4]
    assert seg[0].tolist() == [0, 0, 0, 0, 0, 0, 1.0, 0] and seg[1].tolist() == [1, 2, 3, 4, 5, 6, 3.0, 0]
    assert seg[2].tolist() == [7, 8, 9, 7, 8, 10, 12.0, 0] and seg[3].tolist() == [7, 8, 10, 7, 9, 10, 24.0, 0]
    assert engine.view_map_segments(pts, [0, 6], 0.5)[0][:, 6].tolist() == [0.5] * 5
    with pytest.raises(ValueError, match="offsets"):
        engine.view_map_segments(pts, [0, 4, 3, 6], radius)
    with pytest.raises(ValueError, match="radius"):
        engine.view_map_segments(pts, [0, 6], radius[:3])


def test_view_angles_records_are_the_sweeps_poses():
    from nerf_for_angiography_amd.visualization import sweep
    angles = sweep.sweep_angles(40, 20)
    rec = engine.view_angles_records(angles, (0.0, 0.0, 1500.0), 312.0, translation=(1.0, -2.0, 3.0))
    poses = sweep._poses(angles, (0.0, 0.0, 1500.0), (1.0, -2.0, 3.0), "cpu").numpy()
    assert np.array_equal(rec, engine.hull_view_records(poses, 312.0)) and rec.shape == (9, 16)


def _vmap(fs, ov, n_invisible=None):
    fs, ov = np.asarray(fs, np.float64), np.asarray(ov, np.float64)
    vm = dict(foreshortening=fs, overlap=ov, tree_foreshortening=fs[:, 0], tree_overlap=ov[:, 0])
    if n_invisible is not None:
        vm["n_invisible"] = np.asarray(n_invisible)
    return vm


def test_optimal_views_ordering_ties_and_nan():
    nan = float("nan")
    vm = _vmap([[0.5, 0.1], [0.2, 0.1], [0.2, 0.3], [0.1, 0.0], [0.0, 0.2]], [[0.0, 0.0], [0.0, nan], [0.0, 0.1], [nan, 0.5], [0.2, 0.0]])
    idx, score = engine.optimal_views(vm, k=5)                  # whole tree: 0.5, 0.2, 0.2, NaN, 0.2 -> the tie by index, the NaN last
    assert idx.tolist() == [1, 2, 4, 0, 3] and idx.dtype == np.int64 and score[:4].tolist() == [0.2, 0.2, 0.2, 0.5] and np.isnan(score[4])
    idx, score = engine.optimal_views(vm, branch=2, overlap_weight=2.0, k=3)      # 0.1, NaN, 0.5, 1.0, 0.2
    assert idx.tolist() == [0, 4, 2] and score.tolist() == [0.1, 0.2, 0.5]
    assert engine.optimal_views(vm, branch=2, overlap_weight=0.0, k=9)[0].tolist() == [3, 0, 4, 2, 1]      # 0 x NaN is NaN: still last
    assert engine.optimal_views(vm, k=0)[0].size == 0
    hidden = _vmap([[0.5], [0.1], [0.3]], [[0.0], [0.0], [0.0]], n_invisible=[0, 2, 0])      # a view that loses part of the tree is last
    idx, score = engine.optimal_views(hidden, k=3)
    assert idx.tolist() == [2, 0, 1] and np.isnan(score[2])
    with pytest.raises(ValueError, match="branch"):
        engine.optimal_views(vm, branch=3)


def test_sweep_names_and_checks():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.VIEW_METRICS == ("FORESHORTENING ERR 3D", "OVERLAP ERR 3D", "VIEW REGRET 3D")
    for names, _, _ in sweep._VOLUME_FAMILIES:                  # a tuple of its own, in no family
        assert not set(sweep.VIEW_METRICS) & set(names)
    with pytest.raises(ValueError, match="ground-truth volume"):
        sweep._check_metrics(["PSNR", "VIEW REGRET 3D"], None, None)
    with pytest.raises(ValueError, match="ground-truth volume"):
        sweep.evaluation_sweep(None, None, sweep.sweep_angles(40, 20), 8, 8, 100.0, (0, 0, 1500.0), 1400.0, 1600.0, 8, metrics=["OVERLAP ERR 3D"])
    got = sweep._check_metrics(["VIEW REGRET 3D", "CORR 3D SIRT", "PSNR", "FORESHORTENING ERR 3D"], None, object(), sirt_views=({}, None))
    assert got == ["PSNR", "CORR 3D SIRT", "FORESHORTENING ERR 3D", "VIEW REGRET 3D"]


def test_view_scores_arithmetic():
    from nerf_for_angiography_amd.visualization import sweep
    nan = float("nan")
    truth = dict(tree_foreshortening=np.array([0.5, 0.1, 0.3]), tree_overlap=np.array([0.0, 0.25, 0.0]), n_invisible=np.zeros(3, np.int32))
    same = sweep.view_scores(truth, truth)
    assert (same["foreshortening_err"], same["overlap_err"], same["view_regret"], same["best_view"], same["best_view_gt"]) == (0.0, 0.0, 0.0, 2, 2)
    pred = dict(tree_foreshortening=np.array([0.25, 0.5, 0.5]), tree_overlap=np.array([0.0, nan, 0.5]), n_invisible=np.zeros(3, np.int32))
    got = sweep.view_scores(pred, truth)                        # the prediction prefers view 0, where the truth scores 0.5 against its best 0.3
    assert got["foreshortening_err"] == (0.25 + 0.4 + 0.2) / 3 and got["overlap_err"] == 0.25 and got["view_regret"] == 0.5 - 0.3
    assert got["best_view"] == 0 and got["best_view_gt"] == 2


def _args(*extra):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser
    return build_parser().parse_args(["--synthetic", *extra])


def test_driver_checks_the_view_map_flag():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import check_args
    assert _args().save_view_map is None and _args().view_map_step == 5.0
    check_args(_args("--save_view_map", "views.csv", "--view_map_step", "10"))
    with pytest.raises(ValueError, match="--save_view_map"):
        check_args(_args("--save_view_map", "views.txt"))
    with pytest.raises(ValueError, match="--view_map_step"):
        check_args(_args("--save_view_map", "views.csv", "--view_map_step", "0"))
    with pytest.raises(ValueError, match="--mesh_threshold"):
        check_args(_args("--save_view_map", "views.csv", "--mesh_threshold", "0"))


# ---- properties of the restatement ----
def _look_at(source, f=500.0):
    """A view record whose source looks at the origin: the camera's -z axis points from the source to the origin."""
    c = np.asarray(source, np.float64)
    z = c / np.linalg.norm(c)
    x = np.cross([0.0, 1.0, 0.0] if abs(z[1]) < 0.9 else [1.0, 0.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    rec = np.zeros(16)
    rec[0:9] = np.stack([x, y, z], axis=1).reshape(-1)
    rec[9:12], rec[12] = c, f
    return rec


def _record_at(c, f=500.0):
    """A view record with the identity rotation and its source at c (the foreshortening reads the source alone)."""
    rec = np.zeros(16)
    rec[[0, 4, 8]], rec[9:12], rec[12] = 1.0, np.asarray(c, np.float64), f
    return rec


def _segment(p0, p1, r):
    return np.array([[*p0, *p1, r, 0.0]], np.float64)


def test_foreshortening_of_a_segment_across_and_along_the_ray():
    """A segment at right angles to the ray through its midpoint has foreshortening 0 to 1e-15 (one rounding of a quantity of size 1);
    a segment along that ray has 1 to 1e-12.  'Along the ray' is a statement about the input, so the second half is asked of inputs of
    which it is true: source, p0 and p1 on one line exactly, c + m k with small integers (then every product is exact, (le le) / n2 is
    l2 itself and the result is 1).  Of a segment that is on the ray only up to the rounding of its coordinates the formula gives less:
    perp2 is a cancellation residue of about 1e-16 l2 and perp its square root, 1e-8 l - printed below, measured 1.6e-8, not asserted."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(50):
        c = rng.uniform(-50, 50, 3)
        mid = rng.uniform(-5, 5, 3)
        ray = (mid - c) / np.linalg.norm(mid - c)
        across = np.cross(ray, rng.standard_normal(3))
        across *= rng.uniform(0.1, 3.0) / np.linalg.norm(across)
        rec = _look_at(c)[None]
        proj, length = vr.foreshortening(_segment(mid - across, mid + across, 0.3), [1], rec)
        assert abs(1.0 - proj[0, 0] / length[0]) <= 1e-15
        half = ray * rng.uniform(0.1, 3.0)
        proj, length = vr.foreshortening(_segment(mid - half, mid + half, 0.3), [1], rec)
        worst = max(worst, abs(proj[0, 0] / length[0]))
    print(f"a segment on the ray up to rounding: 1 - foreshortening <= {worst:.3g}")
    for k in ((0, 0, 1), (1, 0, 0), (1, 2, 2), (3, -4, 12), (-2, 3, 6), (1, 1, 1), (7, -5, 3)):
        for c in ((0, 0, 0), (11, -3, 40), (-250, 125, 60)):
            for m0, m1 in ((1, 2), (3, 10), (-7, -2), (5, 4)):
                k, c = np.asarray(k, np.float64), np.asarray(c, np.float64)
                proj, length = vr.foreshortening(_segment(c + m0 * k, c + m1 * k, 0.3), [1], _record_at(c)[None])
                assert abs((1.0 - proj[0, 0] / length[0]) - 1.0) <= 1e-12, (k, c, m0, m1)
    proj, length = vr.foreshortening(_segment((1.0, 2, 3), (1.0, 2, 3), 0.3), [1], _look_at((0.0, 0, 40))[None])
    assert proj[0, 0] == 0.0 and length[0] == 0.0               # a point has no length to foreshorten


@pytest.fixture(scope="module")
def skew():
    """Two skew branches at different depths: one along x at z = 0, one along y at z = 6; their common perpendicular is the z axis."""
    pts = np.array([[-8.0, 0, 0], [0.0, 0, 0], [8.0, 0, 0], [0, -8.0, 6], [0, 0.0, 6], [0, 8.0, 6]])
    seg, br = engine.view_map_segments(pts, [0, 3, 6], 0.6)
    rec = np.stack([_look_at((0.0, 0.0, 300.0), 900.0), _look_at((0.0, 300.0, 0.0), 900.0), _look_at((0.0, 0.0, 4.0), 40.0)])
    return seg, br, rec, vr.view_map(seg, br, rec, 64, 48)


def test_skew_branches_share_pixels_only_along_their_common_perpendicular(skew):
    seg, br, rec, vm = skew
    assert (vm["shared"][0] > 0).all() and vm["tree"][0, 1] > 0       # along z: one lies over the other
    assert (vm["shared"][1] == 0).all() and vm["tree"][1, 1] == 0     # from the side: 6 apart in depth, 18 pixels apart on the detector
    assert (vm["area"][:2] > 0).all()


def test_counts_are_consistent(skew):
    seg, br, rec, vm = skew
    cases = [vm] + [vr.view_map(*vr.wavy_tree(n, b, 5), engine.hull_view_records(*vr.scene_views(3, 17, 33, 0)), 17, 33) for n, b in ((40, 4), (9, 9))]
    for m in cases:
        nb = m["area"].shape[1]
        assert int(m["count"].max()) <= nb
        for v in range(m["tree"].shape[0]):
            union, multi = int(m["tree"][v, 0]), int(m["tree"][v, 1])
            assert union == int((m["count"][v] >= 1).sum()) and multi == int((m["count"][v] >= 2).sum())
            assert union >= int(m["area"][v].max()) and int(m["area"][v].sum()) >= union
            assert int(m["area"][v].sum()) == int(m["count"][v].sum())
            assert (multi == 0) == bool((m["shared"][v] == 0).all()) and (m["shared"][v] <= m["area"][v]).all()


def test_a_segment_with_one_end_behind_the_source_is_invisible(skew):
    seg, br, rec, vm = skew
    # view 2: the source at z = 4 looks down at the origin: branch 2 (z = 6) lies behind it, branch 1 in front
    assert vm["tree"][2, 2] == 2 and vm["area"][2, 1] == 0 and vm["area"][2, 0] > 0
    half = _segment((0.0, 0, 1), (0.0, 0.5, 9), 0.5)             # one end in front of that source, one behind
    one = vr.view_map(half, [1], rec[2:3], 64, 48)
    assert one["tree"][0].tolist() == [0, 0, 1, 0] and int(one["count"].max()) == 0


def test_nan_covers_nothing():
    seg = _segment((0.0, 0, 0), (1.0, 0, 0), float("nan"))
    vm = vr.view_map(seg, [1], _look_at((0.0, 0.0, 50.0))[None], 16, 16)
    assert vm["tree"][0].tolist() == [0, 0, 0, 0] and vm["area"][0, 0] == 0
