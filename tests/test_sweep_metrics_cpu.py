"""The evaluation sweep's SSIM and 3-D metrics without a GPU: sanity checks of the NumPy restatement the GPU tests measure afx_ssim against
(tests/ssim_reference.py), the workspace query and argument validation of afx_ssim and afx_volume_grid (include/afx.h), which return
before any HIP call, and evaluation_sweep's refusal of requests it cannot serve, which comes before any GPU work."""
import ctypes as C

import numpy as np
import pytest

import ssim_reference as sr

AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
FAKE = C.c_void_p(0x10000)          # never dereferenced: every call below is refused before it reaches the device


def test_identical_images_give_one():
    x = sr.vessel_views(1, 40, 52, seed=2)[0]
    assert sr.ssim(x, x) == pytest.approx(1.0, abs=1e-12)
    rnd = np.random.default_rng(0).random((23, 31))
    assert sr.ssim(rnd, rnd) == pytest.approx(1.0, abs=1e-12)


@pytest.mark.parametrize("a,b", [(1.0, 1.0), (0.9, 0.2), (0.0, 0.5), (0.31, 0.97)])
def test_constant_images_give_the_closed_form(a, b):
    got = sr.ssim(np.full((17, 29), a), np.full((17, 29), b))
    want = (2 * a * b + sr.C1) / (a * a + b * b + sr.C1)           # no variance: the c2 factors cancel
    assert got == pytest.approx(want, abs=1e-12)


def test_symmetric_and_below_one():
    rng = np.random.default_rng(4)
    x, y = rng.random((30, 41)), rng.random((30, 41))
    assert sr.ssim(x, y) == pytest.approx(sr.ssim(y, x), abs=1e-14)
    assert sr.ssim(x, y) < 0.5
    v = sr.vessel_views(2, 33, 33, seed=9)
    assert sr.ssim(v[0], v[1]) == pytest.approx(sr.ssim(v[1], v[0]), abs=1e-14)


def test_window_and_crop():
    g = sr.gaussian_1d()
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15 and np.argmax(g) == 5 and np.allclose(g, g[::-1])
    assert sr.ssim_map(np.zeros((11, 11)), np.zeros((11, 11))).shape == (1, 1)
    assert sr.ssim_map(np.zeros((13, 37)), np.zeros((13, 37))).shape == (3, 27)
    with pytest.raises(ValueError):
        sr.ssim(np.zeros((10, 20)), np.zeros((10, 20)))


def _rup(b):
    return (b + 255) // 256 * 256


def _tiles(h, w):
    return -(-(h - 10) // 16) * -(-(w - 10) // 64)


@pytest.fixture(scope="module")
def lib():
    from nerf_for_angiography_amd import _lib
    return _lib.load()


def test_ssim_workspace_query_follows_its_formula(lib):
    for n, h, w in ((1, 11, 11), (4, 13, 37), (1369, 100, 100), (25, 512, 512), (3, 27, 75), (2, 26, 74), (1, 11, 16384)):
        assert lib.afx_ssim_workspace_bytes(n, h, w) == _rup(8 * n * _tiles(h, w)), (n, h, w)
    assert lib.afx_ssim_workspace_bytes(1369, 100, 100) == _rup(1369 * 12 * 8)
    for bad in ((0, 16, 16), (-1, 16, 16), (1, 10, 16), (1, 16, 10), (1, 0, 0), (1, 65536, 65536), (1 << 20, 512, 512)):
        assert lib.afx_ssim_workspace_bytes(*bad) == 0, bad


def test_ssim_argument_validation(lib):
    def call(x=FAKE, y=FAKE, n=2, h=16, w=16, out=FAKE, ws=FAKE, nbytes=1 << 40, needed=None):
        return lib.afx_ssim(x, y, n, h, w, out, ws, nbytes, needed, None)
    assert call(x=None) == AFX_E_INVALID and call(y=None) == AFX_E_INVALID and call(out=None) == AFX_E_INVALID
    for n, h, w in ((0, 16, 16), (-2, 16, 16), (2, 10, 16), (2, 16, 10), (2, -11, 16), (1, 65536, 65536), (1 << 20, 512, 512)):
        assert call(n=n, h=h, w=w) == AFX_E_INVALID, (n, h, w)
    need = C.c_size_t(0)
    assert call(nbytes=8, needed=C.byref(need)) == AFX_E_WORKSPACE
    assert need.value == lib.afx_ssim_workspace_bytes(2, 16, 16) == 256
    assert call(ws=None) == AFX_E_WORKSPACE
    from nerf_for_angiography_amd import _lib
    assert b"workspace" in _lib.load().afx_last_error()


def test_volume_grid_argument_validation(lib):
    def call(vol=FAKE, shape=(4, 5, 6), origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), lo=-1.0, hi=1.0, n=8, out=FAKE):
        org = (C.c_double * 3)(*origin) if origin is not None else None
        spc = (C.c_double * 3)(*spacing) if spacing is not None else None
        return lib.afx_volume_grid(vol, *shape, org, spc, 0.0, lo, hi, n, out, None)
    assert call(vol=None) == AFX_E_INVALID and call(out=None) == AFX_E_INVALID
    assert call(origin=None) == AFX_E_INVALID and call(spacing=None) == AFX_E_INVALID
    for shape in ((1, 5, 6), (4, 1, 6), (4, 5, 1), (0, 5, 6)):
        assert call(shape=shape) == AFX_E_INVALID, shape
    for spacing in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan"))):
        assert call(spacing=spacing) == AFX_E_INVALID, spacing
    for n in (1, 0, -5, (1 << 20) + 1, 1 << 30):
        assert call(n=n) == AFX_E_INVALID, n
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (-float("inf"), 1.0), (0.0, float("inf"))):
        assert call(lo=lo, hi=hi) == AFX_E_INVALID, (lo, hi)


class _NoModel:
    """Stands in for the model: touching it (flat_params, rendering) would be GPU work, which the argument checks must come before."""

    def __getattr__(self, name):
        raise AssertionError(f"evaluation_sweep touched the model ({name}) before rejecting its arguments")


def _sweep(**kw):
    from nerf_for_angiography_amd.visualization.sweep import evaluation_sweep
    args = dict(model=_NoModel(), targets=None, angles=np.zeros((4, 2)), img_width=8, img_height=8, focal_length=100.0,
                src_pt=np.array([0, 0, 1500.0]), near_thresh=1400.0, far_thresh=1600.0, depth_samples_per_ray=16)
    args.update(kw)
    return evaluation_sweep(**args)


def test_evaluation_sweep_refuses_before_gpu_work():
    for nets in (["LPIPS"], ["PSNR", "DISTS"], ["SSIM", "LPIPS", "DICE 3D"]):
        with pytest.raises(NotImplementedError, match="pretrained"):
            _sweep(metrics=nets)
    with pytest.raises(ValueError, match="volume"):
        _sweep(metrics=["PSNR", "DICE 3D"])
    with pytest.raises(ValueError, match="volume"):
        _sweep(metrics=["DOT 3D"], binary_targets=object())
    with pytest.raises(ValueError, match="binary_targets"):
        _sweep(metrics=["SSIM", "DICE 2D"], volume=object())
    with pytest.raises(ValueError, match="unknown"):
        _sweep(metrics=["PSNR", "MS-SSIM"])
    with pytest.raises(AssertionError, match="touched the model"):      # a request it can serve goes on to the model
        _sweep(metrics=["PSNR", "SSIM"])


def test_metric_columns_in_the_reference_order():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.METRICS == ("PSNR", "SSIM", "LPIPS", "DISTS", "DICE 2D", "DOT 2D", "DICE 3D", "DOT 3D")
    assert sweep._check_metrics(None, None, None) == ["PSNR", "DOT 2D"]
    assert sweep._check_metrics(None, object(), None) == ["PSNR", "DOT 2D", "DICE 2D"]
    got = sweep._check_metrics(["DOT 3D", "DICE 2D", "SSIM", "PSNR", "DOT 2D", "DICE 3D"], object(), object())
    assert got == ["PSNR", "SSIM", "DICE 2D", "DOT 2D", "DICE 3D", "DOT 3D"]
    assert sweep._check_metrics("SSIM", None, None) == ["SSIM"]


def test_host_tensors_are_refused():
    import torch
    from nerf_for_angiography_amd.engine import ssim, volume_grid
    from nerf_for_angiography_amd._lib import AfxError
    with pytest.raises(AfxError):
        ssim(torch.zeros(2, 16, 16), torch.zeros(2, 16, 16))
    with pytest.raises(AfxError):
        volume_grid(torch.zeros(4, 4, 4), (0, 0, 0), (1, 1, 1), 0.0, -1.0, 1.0, 5)
