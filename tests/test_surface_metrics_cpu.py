"""The surface-distance scores without a GPU: the NumPy / SciPy restatement the GPU tests measure against (tests/surface_reference.py)
checked against spelled-out versions of its own rules and a case with a closed form, evaluation_sweep's handling of the new metric
names, and the argument checks and workspace queries of afx_distance_transform_edt_3d / afx_surface_metrics_3d (include/afx.h), which
return before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import surface_reference as sr

AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
FAKE = C.c_void_p(0x10000)          # never dereferenced: every call below is refused before it reaches the device


@pytest.mark.parametrize("shape", [(8, 7, 6), (5, 7, 3), (1, 1, 6), (1, 6, 1), (6, 1, 1), (2, 3, 8)])
@pytest.mark.parametrize("p", [0.5, 0.9, 0.99])
def test_restated_edt_equals_brute_force(shape, p):
    rng = np.random.default_rng(int(p * 100) + 7 * shape[0] + shape[2])
    fg = rng.random(shape) < p
    fg[tuple(rng.integers(0, s) for s in shape)] = False                 # at least one zero voxel
    want = sr.edt_brute(fg)
    got = sr.edt(fg)
    assert got.dtype == np.float64
    assert np.array_equal(got, np.sqrt(want.astype(np.float64)))          # bit for bit
    assert np.array_equal(np.rint(got * got).astype(np.int64), want)
    corner = np.ones(shape, bool)
    corner[0, 0, 0] = False
    assert np.array_equal(sr.edt(corner), np.sqrt(sr.edt_brute(corner).astype(np.float64)))
    assert not sr.edt(np.zeros(shape, bool)).any()


def test_surface_rule_equals_the_neighbour_form():
    rng = np.random.default_rng(3)
    for shape, p in (((9, 8, 7), 0.6), ((4, 5, 6), 1.0), ((1, 5, 6), 0.8), ((7, 1, 1), 0.7), ((6, 6, 6), 0.95)):
        m = rng.random(shape) < p
        assert np.array_equal(sr.surface(m), sr.surface_by_neighbours(m)), shape
    full = np.ones((4, 5, 6), bool)
    assert sr.surface(full).sum() == 4 * 5 * 6 - 2 * 3 * 4                # touching the faces: everything but the interior
    blob = sr.tube_and_ball((24, 20, 28)) >= 0.5
    assert np.array_equal(sr.surface(blob), sr.surface_by_neighbours(blob)) and 0 < sr.surface(blob).sum() < blob.sum()


def test_shifted_box_has_the_closed_form():
    """A 5 x 5 x 6 box against itself moved 3 voxels along its long side."""
    a = sr.box((9, 9, 16), (2, 2, 2), (7, 7, 8))
    b = sr.box((9, 9, 16), (2, 2, 5), (7, 7, 11))
    m = sr.surface_metrics(a, b, 0.5, 0.5)
    assert m["hd"] == 3.0 and m["hd_percentile"] == 3.0 and m["dice_vessel"] == 0.5
    assert m["assd"] == pytest.approx(7.0 / 6.0, abs=1e-14)
    assert (m["n_pred"], m["n_gt"], m["n_overlap"], m["n_surface_pred"], m["n_surface_gt"]) == (150, 150, 75, 114, 114)
    same = sr.surface_metrics(a, a, 0.5, 0.5)
    assert same["hd"] == same["assd"] == same["hd_percentile"] == 0.0 and same["dice_vessel"] == 1.0
    with pytest.raises(ValueError):
        sr.surface_metrics(a, b, 2.0, 0.5)


def test_engine_lerp_is_numpys():
    from nerf_for_angiography_amd.engine import _lerp
    rng = np.random.default_rng(11)
    for n in (2, 3, 7, 20):
        d = np.sqrt(rng.integers(0, 50, n).astype(np.float64))
        for q in (0.0, 5.0, 30.0, 50.0, 95.0, 99.9, 100.0):
            v = (n - 1) * np.true_divide(q, 100)
            lo = int(np.floor(v))
            s = np.sort(d)
            assert _lerp(float(s[lo]), float(s[min(lo + 1, n - 1)]), float(v - lo)) == float(np.percentile(d, q)), (n, q)


def test_metric_columns_with_the_surface_names():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.SURFACE_METRICS == ("DICE 3D VESSEL", "ASSD 3D", "HD 3D", "HD95 3D")
    assert sweep.METRICS == ("PSNR", "SSIM", "LPIPS", "DISTS", "DICE 2D", "DOT 2D", "DICE 3D", "DOT 3D")
    got = sweep._check_metrics(["HD95 3D", "DOT 3D", "ASSD 3D", "PSNR", "DICE 3D VESSEL", "SSIM", "HD 3D"], None, object())
    assert got == ["PSNR", "SSIM", "DOT 3D", "DICE 3D VESSEL", "ASSD 3D", "HD 3D", "HD95 3D"]
    assert sweep._check_metrics("ASSD 3D", None, object()) == ["ASSD 3D"]
    assert sweep._check_metrics(None, None, object()) == ["PSNR", "DOT 2D"]          # the defaults do not grow
    for name in sweep.SURFACE_METRICS:
        with pytest.raises(ValueError, match="volume"):
            sweep._check_metrics([name], None, None)
    with pytest.raises(ValueError, match="unknown"):
        sweep._check_metrics(["HD 3D", "HD99 3D"], None, object())
    with pytest.raises(NotImplementedError, match="pretrained"):
        sweep._check_metrics(["HD 3D", "LPIPS"], None, object())
    with pytest.raises(ValueError, match="binary_targets"):
        sweep._check_metrics(["HD 3D", "DICE 2D"], None, object())


class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"evaluation_sweep touched the model ({name}) before rejecting its arguments")


def test_evaluation_sweep_refuses_surface_metrics_before_gpu_work():
    from nerf_for_angiography_amd.visualization.sweep import evaluation_sweep
    args = dict(model=_NoModel(), targets=None, angles=np.zeros((4, 2)), img_width=8, img_height=8, focal_length=100.0,
                src_pt=np.array([0, 0, 1500.0]), near_thresh=1400.0, far_thresh=1600.0, depth_samples_per_ray=16)
    with pytest.raises(ValueError, match="volume"):
        evaluation_sweep(metrics=["PSNR", "ASSD 3D"], **args)
    with pytest.raises(ValueError, match="unknown"):
        evaluation_sweep(metrics=["ASSD"], volume=object(), **args)
    with pytest.raises(AssertionError, match="touched the model"):       # a request it can serve goes on to the model
        evaluation_sweep(metrics=["HD95 3D"], volume=object(), **args)


def test_host_tensors_are_refused():
    import torch
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd._lib import AfxError
    with pytest.raises(AfxError):
        engine.distance_transform_edt_3d(torch.ones(4, 5, 6))
    with pytest.raises(AfxError):
        engine.surface_metrics_3d(torch.ones(4, 5, 6), torch.ones(4, 5, 6), 0.5, 0.5)
    with pytest.raises(AfxError):
        engine.surface_metrics_record(np.ones((4, 5, 6), np.float32), torch.ones(4, 5, 6), 0.5, 0.5)


def _rup(b):
    return (b + 255) // 256 * 256


@pytest.fixture(scope="module")
def lib():
    from nerf_for_angiography_amd import _lib
    return _lib.load()


BAD_SHAPES = ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1025, 4, 4), (4, 1025, 4), (4, 4, 1025), (1 << 20, 1, 1))


def test_workspace_queries(lib):
    for shape in ((1, 1, 1), (5, 7, 3), (33, 17, 65), (201, 201, 201), (1024, 1, 1), (1, 1024, 1024)):
        n = shape[0] * shape[1] * shape[2]
        assert lib.afx_distance_transform_edt_3d_workspace_bytes(*shape) == _rup(2 * n), shape
        want = 2 * _rup(n) + _rup(2 * n) + 2 * _rup(4 * n) + 2 * 2048 * 8 + 3 * 2048 * 4 + 256
        assert lib.afx_surface_metrics_3d_workspace_bytes(*shape) == want, shape
    for bad in BAD_SHAPES:
        assert lib.afx_distance_transform_edt_3d_workspace_bytes(*bad) == 0, bad
        assert lib.afx_surface_metrics_3d_workspace_bytes(*bad) == 0, bad


def test_edt_3d_argument_validation(lib):
    def call(fg=FAKE, shape=(4, 5, 6), d2=FAKE, dist=FAKE, ws=FAKE, nbytes=1 << 40, needed=None):
        return lib.afx_distance_transform_edt_3d(fg, *shape, d2, dist, ws, nbytes, needed, None)
    assert call(fg=None) == AFX_E_INVALID and call(d2=None) == AFX_E_INVALID
    for bad in BAD_SHAPES:
        assert call(shape=bad) == AFX_E_INVALID, bad
    need = C.c_size_t(0)
    assert call(nbytes=8, needed=C.byref(need)) == AFX_E_WORKSPACE
    assert need.value == lib.afx_distance_transform_edt_3d_workspace_bytes(4, 5, 6) == 256
    assert call(ws=None) == AFX_E_WORKSPACE and b"workspace" in lib.afx_last_error()


def test_surface_metrics_argument_validation(lib):
    def call(pred=FAKE, gt=FAKE, shape=(4, 5, 6), thr=(0.5, 0.5), q=95.0, rec=FAKE, ws=FAKE, nbytes=1 << 40, needed=None):
        return lib.afx_surface_metrics_3d(pred, gt, *shape, thr[0], thr[1], q, rec, ws, nbytes, needed, None)
    assert call(pred=None) == AFX_E_INVALID and call(gt=None) == AFX_E_INVALID and call(rec=None) == AFX_E_INVALID
    for bad in BAD_SHAPES:
        assert call(shape=bad) == AFX_E_INVALID, bad
    for q in (-0.1, 100.5, float("nan"), float("inf")):
        assert call(q=q) == AFX_E_INVALID, q
    assert call(thr=(float("nan"), 0.5)) == AFX_E_INVALID and call(thr=(0.5, float("nan"))) == AFX_E_INVALID
    need = C.c_size_t(0)
    assert call(nbytes=1024, needed=C.byref(need)) == AFX_E_WORKSPACE
    assert need.value == lib.afx_surface_metrics_3d_workspace_bytes(4, 5, 6)
    assert call(ws=None) == AFX_E_WORKSPACE
