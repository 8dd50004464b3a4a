"""The projection ray-sampling weights without a GPU: sanity checks of the NumPy / SciPy restatement the GPU tests measure the HIP
kernels against (tests/vesselness_reference.py), and the argument validation and workspace queries of afx_frangi,
afx_distance_transform_edt and afx_sampling_weights (include/afx.h), which return before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import vesselness_reference as vr

AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
FAKE = C.c_void_p(0x10000)          # never dereferenced: every call below is refused before it reaches the device


def test_dark_line_responds_on_the_line_and_not_far_from_it():
    img = vr.dark_line_image(64, 64, row=32, width=3)
    f = vr.frangi(img)
    assert f.max() > 0
    inner = f[:, 8:56]
    assert np.all(np.argmax(inner, axis=0) >= 31) and np.all(np.argmax(inner, axis=0) <= 33)
    assert np.all(inner[31:34] > 0.5 * f.max())
    assert np.abs(f[12]).max() <= 1e-6 * f.max() and np.abs(f[52]).max() <= 1e-6 * f.max()       # 20 px off the line


def test_transpose_transposes_the_output():
    img = vr.dark_line_image(48, 64, row=20, width=3)
    assert np.array_equal(vr.frangi(img.T.copy()), vr.frangi(img).T)
    # a general image: the separable Gaussian passes swap order under a transpose, so the sums round differently - the
    # outputs agree to rounding and in their zero pattern
    v = vr.vessel_image(40, 56, seed=3)
    f, t = vr.frangi(v), vr.frangi(v.T.copy()).T
    assert np.abs(f - t).max() <= 1e-11 * f.max()
    assert np.array_equal(f == 0, t == 0)


def test_black_ridges_false_on_the_inverse_equals_the_default():
    v = vr.vessel_image(50, 70, seed=5)
    assert np.array_equal(vr.frangi(1 - v, black_ridges=False), vr.frangi(v))
    assert np.array_equal(vr.frangi(1 - v, sigmas=(2, 4), black_ridges=False), vr.frangi(v, sigmas=(2, 4)))


def test_weights_are_normalised_and_positive():
    w = vr.sampling_weights(vr.vessel_image(64, 64, seed=1), binary=False)
    assert w.min() == 1e-10 and abs(w.max() - (1 + 1e-10)) < 1e-15
    with pytest.raises(ValueError):
        vr.sampling_weights(np.ones((16, 16)))


def _rup(b):
    return (b + 255) // 256 * 256


@pytest.fixture(scope="module")
def lib():
    from nerf_for_angiography_amd import _lib
    return _lib.load()


def _sig(vals):
    return (C.c_double * max(len(vals), 1))(*vals)


def test_workspace_queries_follow_their_formula(lib):
    for n, h, w, s in ((1, 2, 2, 1), (5, 64, 64, 5), (1369, 100, 100, 5), (25, 512, 512, 5), (3, 96, 128, 3), (2, 3, 517, 16)):
        planes = 2 * _rup(n * s * h * w * 8)
        assert lib.afx_frangi_workspace_bytes(n, h, w, s) == planes
        assert lib.afx_distance_transform_edt_workspace_bytes(n, h, w) == _rup(n * h * w * 4)
        fixed = _rup(8 * n) + 2 * _rup(16 * n) + _rup(4 * n * h * w)
        assert lib.afx_sampling_weights_workspace_bytes(0, n, h, w, s) == fixed + planes
        assert lib.afx_sampling_weights_workspace_bytes(1, n, h, w, s) == fixed
    assert lib.afx_distance_transform_edt_workspace_bytes(1, 1, 1) == 256
    for bad in ((0, 8, 8, 5), (1, 1, 8, 5), (1, 8, 0, 5), (1, 8, 8, 0), (1, 8, 8, 17), (-1, 8, 8, 5), (1, 16385, 8, 5), (65536, 8, 8, 1)):
        assert lib.afx_frangi_workspace_bytes(*bad) == 0, bad
        assert lib.afx_sampling_weights_workspace_bytes(0, *bad) == 0, bad
    assert lib.afx_distance_transform_edt_workspace_bytes(0, 4, 4) == 0
    assert lib.afx_sampling_weights_workspace_bytes(2, 1, 8, 8, 5) == 0          # unknown strategy


def _frangi(lib, img=FAKE, n=2, h=16, w=16, sig=(1.0, 3.0), beta=0.5, gamma=15.0, out=FAKE, ws=FAKE, nbytes=1 << 40, needed=None):
    return lib.afx_frangi(img, n, h, w, _sig(sig), len(sig), beta, gamma, 1, out, ws, nbytes, needed, None)


def test_frangi_argument_validation(lib):
    assert _frangi(lib, img=None) == AFX_E_INVALID
    assert _frangi(lib, out=None) == AFX_E_INVALID
    for n, h, w in ((0, 16, 16), (-3, 16, 16), (2, 0, 16), (2, 16, -1), (2, 1, 16), (2, 16, 1)):
        assert _frangi(lib, n=n, h=h, w=w) == AFX_E_INVALID, (n, h, w)
    for sig in ((0.0,), (1.0, -2.0), (float("nan"),), (300.0,), ()):
        assert _frangi(lib, sig=sig) == AFX_E_INVALID, sig
    assert lib.afx_frangi(FAKE, 2, 16, 16, None, 2, 0.5, 15.0, 1, FAKE, FAKE, 1 << 40, None, None) == AFX_E_INVALID
    assert _frangi(lib, beta=0.0) == AFX_E_INVALID and _frangi(lib, gamma=-1.0) == AFX_E_INVALID
    need = C.c_size_t(0)
    assert _frangi(lib, nbytes=1000, needed=C.byref(need)) == AFX_E_WORKSPACE
    assert need.value == lib.afx_frangi_workspace_bytes(2, 16, 16, 2) == 2 * _rup(2 * 2 * 16 * 16 * 8)
    assert _frangi(lib, ws=None) == AFX_E_WORKSPACE
    from nerf_for_angiography_amd import _lib
    assert b"workspace" in _lib.load().afx_last_error()


def test_edt_and_weights_argument_validation(lib):
    edt = lambda x=FAKE, n=1, h=8, w=8, out=FAKE, nbytes=1 << 40, needed=None: lib.afx_distance_transform_edt(x, n, h, w, out, FAKE, nbytes, needed, None)
    assert edt(x=None) == AFX_E_INVALID and edt(out=None) == AFX_E_INVALID
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, -1, 8)):
        assert edt(n=n, h=h, w=w) == AFX_E_INVALID
    need = C.c_size_t(0)
    assert edt(n=3, h=3, w=517, nbytes=10, needed=C.byref(need)) == AFX_E_WORKSPACE and need.value == _rup(3 * 3 * 517 * 4)

    def sw(img=FAKE, n=2, h=8, w=8, strategy=0, sig=(1.0,), out=FAKE, nbytes=1 << 40, needed=None):
        return lib.afx_sampling_weights(img, n, h, w, strategy, 1, _sig(sig), len(sig), 0.5, 15.0, out, None, FAKE, nbytes, needed, None)
    assert sw(img=None) == AFX_E_INVALID and sw(out=None) == AFX_E_INVALID
    assert sw(strategy=7) == AFX_E_INVALID
    assert sw(n=0) == AFX_E_INVALID and sw(h=1) == AFX_E_INVALID and sw(sig=(-1.0,)) == AFX_E_INVALID and sw(sig=()) == AFX_E_INVALID
    assert sw(h=1, strategy=1, sig=(), nbytes=0) == AFX_E_WORKSPACE               # segmentation: no Hessian, no sigmas - past validation
    need = C.c_size_t(0)
    assert sw(nbytes=64, needed=C.byref(need)) == AFX_E_WORKSPACE
    assert need.value == lib.afx_sampling_weights_workspace_bytes(0, 2, 8, 8, 1)
    assert sw(strategy=1, sig=(), nbytes=64, needed=C.byref(need)) == AFX_E_WORKSPACE
    assert need.value == lib.afx_sampling_weights_workspace_bytes(1, 2, 8, 8, 0)


def test_host_frangi_still_refused_and_cpu_synthetic_frangi_refused():
    from nerf_for_angiography_amd.phantomdata import dataset as ds
    with pytest.raises(NotImplementedError):
        ds.sampling_weights(np.ones((4, 4)), "frangi")
    with pytest.raises(NotImplementedError):
        ds.make_synthetic_dataset([(90.0, 0.0)], img_size=8, depth_samples_per_ray=20, sampling_strategy="frangi", device="cpu")
