"""Lumen cross-sections without a GPU: the NumPy restatement of the definition (tests/lumen_reference.py) against the geometry of two tube
phantoms, its exact invariances, the per-branch summary, the sweep's handling of the lumen metric names, the driver's flag, and the argument
checks of afx_lumen_profile (include/afx.h), which return before any HIP call."""
import ctypes as C
import math

import numpy as np
import pytest

import lumen_reference as lr

AFX_E_INVALID = -1
FAKE = C.c_void_p(0x10000)          # never dereferenced: every call below is refused, or returns, before it reaches the device


@pytest.fixture(scope="module")
def lib():
    from nerf_for_angiography_amd import _lib
    return _lib.load()


def _restate(vol, pts, index_to_world=None, iso=0.5, n_rays=64, step=0.5, max_steps=64, half_window=3):
    from nerf_for_angiography_amd import engine
    cs, coef = engine.lumen_ray_table(n_rays)
    p = len(pts)
    return lr.lumen_profile(vol, engine.lumen_world_to_index(index_to_world), pts, np.zeros(p, np.int32), np.full(p, p - 1, np.int32),
                            half_window, n_rays, cs, coef, iso, step, max_steps)


@pytest.fixture(scope="module")
def tubes():
    """{name: (volume, points, s, (profile, flags, radii))} of the phantoms, computed once."""
    out = {}
    for name, n, rho, half in (("rho5", 33, 5.0, 8), ("rho3", 33, 3.0, 8), ("stenosis", 48, lr.stenosis_radius, 16)):
        vol, pts, s = lr.oblique_tube(n, rho, half)
        out[name] = (vol, pts, s, _restate(vol, pts))
    return out


def test_the_library_exports_the_new_symbol(lib):
    from nerf_for_angiography_amd import _lib
    assert hasattr(lib, "afx_lumen_profile") and "afx_lumen_profile" in _lib.exported_symbols()


def test_lumen_profile_argument_validation(lib):
    good_w = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]

    def call(vol=FAKE, shape=(4, 5, 6), W=good_w, pts=FAKE, sf=FAKE, sl=FAKE, P=3, h=3, R=8, cs=None, coef=0.25, iso=0.5, step=0.5, M=8,
             prof=FAKE, flags=FAKE, radii=None):
        w = None if W is None else (C.c_double * 12)(*W)
        table = None if cs is False else (C.c_double * 128)(*(cs if cs is not None else [0.5] * 128))
        return lib.afx_lumen_profile(vol, 0, *shape, w, pts, sf, sl, P, h, R, table, coef, iso, step, M, prof, flags, radii, None)

    def refused(word, **kw):
        assert call(**kw) == AFX_E_INVALID and word in lib.afx_last_error(), (kw, lib.afx_last_error())

    refused(b"vol", vol=None)
    refused(b"world_to_index", W=None)
    refused(b"ray_cs", cs=False)
    for name, word in (("pts", b"points"), ("sf", b"seg_first"), ("sl", b"seg_last"), ("prof", b"profile"), ("flags", b"flags")):
        refused(word, **{name: None})
        assert b"null" in lib.afx_last_error()
    for bad in ((1, 5, 6), (4, 1, 6), (4, 5, 1), (0, 5, 6), (-3, 5, 6)):
        refused(b"n0, n1, n2", shape=bad)
    for bad in ((1 << 11, 1 << 10, 1 << 10), (46341, 46341, 2), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1)):
        refused(b"2^31", shape=bad)
    for bad in (-1, 1 << 31):
        refused(b"n_points", P=bad)
    for bad in (0, 4, 12, 63, 128, -8):
        refused(b"n_rays", R=bad)
    for bad in (0, -1):
        refused(b"half_window", h=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(b"iso", iso=bad)
        refused(b"world_to_index", W=good_w[:7] + [bad] + good_w[8:])
        refused(b"ray_cs", cs=[0.5] * 15 + [bad] + [0.5] * 112)              # within the 2 R = 16 entries that are read
        refused(b"area_coef", coef=bad)
        refused(b"step", step=bad)
    assert call(cs=[0.5] * 16 + [float("nan")] * 112, P=0) == 0             # beyond 2 R nothing is looked at
    for bad in (0.0, -0.5):
        refused(b"step", step=bad)
    for bad in (0, -1, 4097):
        refused(b"max_steps", M=bad)
    assert call(P=0) == 0 and call(P=0, pts=None, sf=None, sl=None, prof=None, flags=None) == 0      # nothing to launch
    assert call(P=0, R=64, M=4096, shape=(2, 2, 2)) == 0
    refused(b"n_rays", P=0, R=7)                                            # the checks come before the early return


def test_host_tensors_are_refused():
    import torch
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd._lib import AfxError
    vol, pts, seg = torch.ones(4, 5, 6), torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(AfxError):
        engine.lumen_profile(vol, pts, seg, seg + 2)
    with pytest.raises(AfxError):
        engine.lumen_profile_record(vol, pts, seg, seg, engine.lumen_world_to_index(None), 0.5, 8, 0.5, 8)
    with pytest.raises(AfxError):
        engine.centreline_lumen_profile({}, vol, None, 0.5)
    with pytest.raises(ValueError, match="n_rays"):
        engine.lumen_ray_table(12)


def test_host_side_tables():
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd.visualization.sweep import grid_index_to_world
    assert engine.lumen_world_to_index(None).tolist() == [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    a = np.asarray(grid_index_to_world(100.0, 25)).reshape(3, 4)
    w = engine.lumen_world_to_index(a).reshape(3, 4)
    idx = np.array([3.0, 7.0, 11.0])
    assert np.allclose(w[:, :3] @ (a[:, :3] @ idx + a[:, 3]) + w[:, 3], idx, rtol=0, atol=1e-12)
    assert np.array_equal(engine.lumen_world_to_index(2.0 * a).reshape(3, 4)[:, :3], w[:, :3] / 2.0)      # a power of two scales exactly
    assert engine.lumen_default_step(a) == 0.5 * (200.0 / 24) and engine.lumen_default_step(None) == 0.5
    cs, coef = engine.lumen_ray_table(8)
    assert cs.shape == (16,) and cs[0] == 1.0 and cs[1] == 0.0 and cs[4] == math.cos(math.pi / 2) and coef == 0.5 * np.sin(2 * np.pi / 8)
    seg_first, seg_last, branch, arc = engine.centreline_segments(np.array([[0, 0, 0], [3, 4, 0], [3, 4, 12], [9, 9, 9.0]]), [0, 3, 4])
    assert seg_first.tolist() == [0, 0, 0, 3] and seg_last.tolist() == [2, 2, 2, 3] and branch.tolist() == [1, 1, 1, 2]
    assert arc.tolist() == [0.0, 5.0, 17.0, 0.0]


def test_metric_columns_with_the_lumen_names():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.LUMEN_METRICS == ("LUMEN AREA ERR 3D", "MLA RATIO 3D", "STENOSIS ERR 3D")
    assert sweep._ALL_VOLUME_METRICS == sweep._VOLUME_METRICS + sweep.VESSELNESS_METRICS + sweep.LUMEN_METRICS
    assert not set(sweep.LUMEN_METRICS) & set(sweep.METRICS + sweep._VOLUME_METRICS + sweep.VESSELNESS_METRICS)
    got = sweep._check_metrics(["STENOSIS ERR 3D", "SCALE RATIO 3D", "LUMEN AREA ERR 3D", "PSNR", "MLA RATIO 3D", "BRANCHES 3D"], None, object())
    assert got == ["PSNR", "BRANCHES 3D", "SCALE RATIO 3D"] + list(sweep.LUMEN_METRICS)
    assert sweep._check_metrics(None, None, object()) == ["PSNR", "DOT 2D"]          # the defaults do not grow
    for name in sweep.LUMEN_METRICS:
        with pytest.raises(ValueError, match="volume"):
            sweep._check_metrics([name], None, None)


def test_lumen_scores_bookkeeping():
    from nerf_for_angiography_amd.visualization.sweep import lumen_scores
    nan = float("nan")
    gt = {"area": np.array([4.0, 2.0, 8.0, 0.0, 5.0]), "flags": np.array([0, 0, 0, 2, 0])}
    pr = {"area": np.array([5.0, 1.0, 0.0, 3.0, 5.0]), "flags": np.array([0, 0, 256, 0, 0])}
    s = lumen_scores(pr, gt, {"area_stenosis": np.array([0.5, nan, 0.25])}, {"area_stenosis": np.array([0.25, 0.75, nan])})
    assert (s["n_points"], s["n_valid_gt"], s["n_valid_both"], s["centreline_coverage"]) == (5, 4, 3, 0.75)
    assert s["lumen_area_err"] == np.mean(np.array([0.25, 0.5, 0.0])) and (s["mla"], s["mla_gt"], s["mla_ratio"]) == (1.0, 2.0, 0.5)
    assert (s["max_stenosis"], s["max_stenosis_gt"], s["stenosis_err"]) == (0.5, 0.75, 0.25)
    none = {"area": np.zeros(2), "flags": np.array([2, 2])}
    e = lumen_scores(none, none, {"area_stenosis": np.array([nan])}, {"area_stenosis": np.array([nan])})
    assert e["n_valid_gt"] == 0 and all(math.isnan(e[k]) for k in ("centreline_coverage", "lumen_area_err", "mla", "mla_ratio", "max_stenosis",
                                                                    "stenosis_err"))


@pytest.mark.parametrize("name,rho,bar", (("rho5", 5.0, 0.03), ("rho3", 3.0, 0.04)))
def test_the_area_of_an_oblique_tube(tubes, name, rho, bar):
    vol, pts, s, (profile, flags, radii) = tubes[name]
    rel = profile[:, 0] / (math.pi * rho * rho) - 1.0
    print(f"{name}: area / (pi rho^2) - 1 in [{rel.min():+.4f}, {rel.max():+.4f}], P = {len(pts)}")
    assert len(pts) == 17 and (flags == 0).all()                                    # every point valid, no open ray
    assert np.abs(rel).max() <= bar
    assert (profile[:, 2] <= profile[:, 1]).all() and (profile[:, 1] <= profile[:, 3]).all() and (profile[:, 4] <= profile[:, 5]).all()
    assert (profile[:, 6] >= 0.5).all() and (profile[:, 7] == 0).all()
    assert np.array_equal(profile[:, 2], radii.min(axis=1)) and np.array_equal(profile[:, 3], radii.max(axis=1))


def test_the_stenosis_of_a_narrowing_tube(tubes):
    from nerf_for_angiography_amd.engine import lumen_branch_summary
    vol, pts, s, (profile, flags, radii) = tubes["stenosis"]
    assert len(pts) == 33 and (flags == 0).all()
    true = np.sort(math.pi * lr.stenosis_radius(s) ** 2)
    want = 1.0 - true[0] / true[(len(true) - 1) // 2]
    summary = lumen_branch_summary({"area": profile[:, 0], "flags": flags, "branch": np.ones(33, np.int64)})
    got = float(summary["area_stenosis"][0])
    print(f"area stenosis {got:.4f}, sampled true {want:.4f}")
    assert abs(got - want) <= 0.02
    assert summary["diameter_stenosis"][0] == 1.0 - np.sqrt(summary["area_min"][0] / summary["area_ref"][0])
    ref = lr.branch_summary(profile[:, 0], flags, np.ones(33, np.int64))
    for key in ref:
        assert np.array_equal(summary[key], ref[key], equal_nan=True), key


def test_scaling_the_world_scales_areas_by_four_exactly(tubes):
    vol, pts, s, (profile, flags, radii) = tubes["rho3"]
    two = np.array([[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 2.0, 0]])
    p2, f2, r2 = _restate(vol, 2.0 * pts, index_to_world=two, step=1.0)
    assert np.array_equal(f2, flags) and np.array_equal(r2, 2.0 * radii)
    assert np.array_equal(p2[:, 0], 4.0 * profile[:, 0]) and np.array_equal(p2[:, 1:6], 2.0 * profile[:, 1:6])
    assert np.array_equal(p2[:, 6], profile[:, 6])


def test_scaling_the_density_changes_no_bit(tubes):
    vol, pts, s, (profile, flags, radii) = tubes["rho3"]
    p8, f8, r8 = _restate(vol * np.float32(0.125), pts, iso=0.5 * 0.125)
    assert np.array_equal(f8, flags) and np.array_equal(r8, radii) and np.array_equal(p8[:, :6], profile[:, :6])
    assert np.array_equal(p8[:, 6], 0.125 * profile[:, 6])


def test_flags_of_the_restatement():
    vol = np.ones((6, 6, 6), np.float32)
    pts = np.array([[2.0, 2, 2], [2, 2, 3], [2, 2, 3], [2, 2, 3], [9, 9, 9]])
    seg_first, seg_last = np.array([0, 0, 2, 2, 4], np.int32), np.array([1, 1, 3, 3, 4], np.int32)
    from nerf_for_angiography_amd import engine
    cs, coef = engine.lumen_ray_table(8)
    profile, flags, radii = lr.lumen_profile(vol, engine.lumen_world_to_index(None), pts, seg_first, seg_last, 1, 8, cs, coef, 0.5, 0.5, 2)
    assert flags.tolist() == [8 << 8, 8 << 8, lr.NO_TANGENT, lr.NO_TANGENT, lr.NO_TANGENT | lr.CENTRE_OUTSIDE]      # open; n2 == 0; one point, outside
    assert (radii[:2] == 1.0).all() and (radii[2:] == 0).all() and (profile[2:, :6] == 0).all() and profile[:, 6].tolist() == [1, 1, 1, 1, 0]
    assert np.array_equal(profile[0, :6], [coef * 8.0, 1.0, 1.0, 1.0, 2.0, 2.0])
    assert lr.tree_sum(np.array([[1e16, 1.0, -1e16, 1.0]])).tolist() == [0.0]       # (a + b) + (c + d), not a running sum (which gives 1.0)


def test_branch_summary():
    from nerf_for_angiography_amd.engine import lumen_branch_summary
    area = np.array([5.0, 3.0, 9.0, 3.0, 7.0, 1.0,   4.0, 2.0, 8.0, 6.0, 0.5,   1.0, 2.0, 3.0, 4.0])
    flags = np.array([0, 0, 0, 0, 0, 2,              0, 0, 0, 0, 256,           0, 0, 0, 0])
    branch = np.array([1] * 6 + [2] * 5 + [3] * 4)
    s = lumen_branch_summary({"area": area, "flags": flags, "branch": branch}, min_points=4)
    assert s["branch"].tolist() == [1, 2, 3] and s["n_valid"].tolist() == [5, 4, 4]
    assert s["area_ref"].tolist() == [5.0, 4.0, 2.0]                               # odd count: the median; even: the LOWER of the two
    assert s["area_min"].tolist() == [3.0, 2.0, 1.0] and s["argmin"].tolist() == [1, 1, 0]      # the first minimum; flagged points left out
    assert s["area_stenosis"].tolist() == [1 - 3.0 / 5.0, 0.5, 0.5] and s["diameter_stenosis"].tolist() == [1 - np.sqrt(3.0 / 5.0)] + [1 - np.sqrt(0.5)] * 2
    s5 = lumen_branch_summary({"area": area, "flags": flags, "branch": branch})
    assert s5["n_valid"].tolist() == [5, 4, 4] and s5["argmin"].tolist() == [1, -1, -1]
    assert not np.isnan(s5["area_stenosis"][0]) and np.isnan(s5["area_stenosis"][1:]).all() and np.isnan(s5["area_ref"][1:]).all()
    ref = lr.branch_summary(area, flags, branch, 4)
    for key in ref:
        assert np.array_equal(s[key], ref[key], equal_nan=True), key
    by_seg = lumen_branch_summary({"area": area, "flags": flags, "seg_first": np.array([0] * 6 + [6] * 5 + [11] * 4)}, min_points=4)
    assert by_seg["branch"].tolist() == [1, 2, 3] and np.array_equal(by_seg["area_stenosis"], s["area_stenosis"])


def test_driver_checks_the_lumen_flag():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser, check_args
    base = ["--synthetic", "--img_size", "16", "--n_iters", "4"]
    assert build_parser().parse_args(base).save_lumen is None
    check_args(build_parser().parse_args(base + ["--save_lumen", "lumen.csv"]))
    with pytest.raises(ValueError, match=".csv"):
        check_args(build_parser().parse_args(base + ["--save_lumen", "x.txt"]))
