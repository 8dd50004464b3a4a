"""Host-side checks of the input-gradient entry points (afx_mlp_backward_inputs, afx_render_backward_inputs) and their workspace
queries: every refusal below is decided before anything touches device memory, so no GPU is needed.  The existing backward entry
points keep refusing exactly as before."""
import ctypes as C

import pytest

from nerf_for_angiography_amd import _lib
from nerf_for_angiography_amd.engine import Engine

AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
FAKE = C.c_void_p(1 << 20)      # a non-null pointer the host checks never dereference


def _err(lib):
    return lib.afx_last_error().decode()


def _args(n_rays=64, n_samples=70, ray_mode=_lib.RAYS_ARRAYS, depth_mode=_lib.DEPTH_UNIFORM_MID, ws_bytes=1 << 40):
    a = _lib.RenderArgs()
    a.n_rays, a.n_samples, a.ray_mode, a.depth_mode = n_rays, n_samples, ray_mode, depth_mode
    a.t_near, a.t_far = 1.0, 2.0
    a.pixel = a.workspace = FAKE.value
    a.workspace_bytes = ws_bytes
    if ray_mode == _lib.RAYS_ARRAYS:
        a.origins = a.dirs = FAKE.value
    else:
        a.poses, a.width, a.height, a.focal = FAKE.value, 8, 8, 10.0
    return a


@pytest.fixture(scope="module")
def eng():
    return Engine(128, 4)


def test_queries_order(eng):
    lib = eng.lib
    for enc in ("none", "barf"):
        e = Engine(64, 2, enc=enc, n_freq=4 if enc != "none" else 0)
        for prec in ("f32", "bf16x3", "bf16", "f16", "f16s8"):
            p = _lib.PREC[prec]
            for n_rays, s in ((0, 100000), (5625, 300), (4096, 64)):
                lo = int(lib.afx_query(e.h, _lib.Q_BWD_INPUTS_WORKSPACE_MIN, n_rays, s, p))
                hi = int(lib.afx_query(e.h, _lib.Q_BWD_INPUTS_WORKSPACE_FULL, n_rays, s, p))
                assert 0 < lo and lo <= hi, (enc, prec, n_rays, s, lo, hi)
                # rays mode adds the per-ray and per-group head to what the points of the same count need
                if n_rays:
                    pts = int(lib.afx_query(e.h, _lib.Q_BWD_INPUTS_WORKSPACE_FULL, 0, n_rays * ((s + 31) // 32 * 32), p))
                    assert hi > pts
    assert int(lib.afx_query(eng.h, _lib.Q_BWD_INPUTS_WORKSPACE_MIN, 0, 1000, 9)) == -1


def test_mlp_inputs_refusals(eng):
    lib, h = eng.lib, eng.h
    f = lib.afx_mlp_backward_inputs
    ws = 1 << 40
    for args in ((None, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE), (FAKE, FAKE, None, FAKE), (FAKE, FAKE, FAKE, None)):
        prepared, pts, d_out, d_pts = args
        assert f(h, 0, prepared, pts, 100, d_out, FAKE, d_pts, FAKE, ws, None) == AFX_E_INVALID
        assert "null argument" in _err(lib)
    assert f(h, 0, FAKE, FAKE, 100, FAKE, FAKE, FAKE, None, ws, None) == AFX_E_INVALID
    assert f(h, 7, FAKE, FAKE, 100, FAKE, None, FAKE, FAKE, ws, None) == AFX_E_INVALID
    assert "unknown precision" in _err(lib)
    assert f(h, 0, FAKE, FAKE, 1 << 31, FAKE, None, FAKE, FAKE, ws, None) == AFX_E_INVALID
    assert f(h, 0, FAKE, FAKE, 0, FAKE, None, FAKE, FAKE, ws, None) == 0      # nothing to do
    for prec in ("f32", "bf16", "f16s8"):
        need = int(lib.afx_query(h, _lib.Q_BWD_INPUTS_WORKSPACE_MIN, 0, 100000, _lib.PREC[prec]))
        assert f(h, _lib.PREC[prec], FAKE, FAKE, 100000, FAKE, None, FAKE, FAKE, need - 1, None) == AFX_E_WORKSPACE
        assert f"< {need} bytes" in _err(lib) and "AFX_Q_BWD_INPUTS_WORKSPACE_MIN" in _err(lib)


def test_render_inputs_refusals(eng):
    lib, h = eng.lib, eng.h
    f = lib.afx_render_backward_inputs
    a = _args()
    assert f(h, 0, None, C.byref(a), FAKE, None, FAKE, FAKE, None) == AFX_E_INVALID
    assert f(h, 0, FAKE, C.byref(a), None, None, FAKE, FAKE, None) == AFX_E_INVALID
    assert f(h, 0, FAKE, C.byref(a), FAKE, None, None, None, None) == AFX_E_INVALID
    assert "nothing requested" in _err(lib)
    # rays generated from poses inside the kernel have no input to differentiate
    p = _args(ray_mode=_lib.RAYS_POSE)
    for d_o, d_d in ((FAKE, None), (None, FAKE), (FAKE, FAKE)):
        assert f(h, 0, FAKE, C.byref(p), FAKE, FAKE, d_o, d_d, None) == AFX_E_INVALID
        assert "AFX_RAYS_POSE" in _err(lib)
    # what afx_render_backward refuses is refused here too
    bad = _args(n_samples=1)
    assert f(h, 0, FAKE, C.byref(bad), FAKE, None, FAKE, FAKE, None) == AFX_E_INVALID
    assert "n_samples" in _err(lib)
    nows = _args()
    nows.workspace = None
    assert f(h, 0, FAKE, C.byref(nows), FAKE, None, FAKE, FAKE, None) == AFX_E_WORKSPACE
    for prec in ("f32", "bf16", "f16", "f16s8"):
        for n_rays, s in ((64, 70), (5625, 300)):
            need = int(lib.afx_query(h, _lib.Q_BWD_INPUTS_WORKSPACE_MIN, n_rays, s, _lib.PREC[prec]))
            short = _args(n_rays=n_rays, n_samples=s, ws_bytes=need - 1)
            assert f(h, _lib.PREC[prec], FAKE, C.byref(short), FAKE, None, FAKE, FAKE, None) == AFX_E_WORKSPACE
            assert f"< {need} bytes" in _err(lib)
    assert f(h, 0, FAKE, C.byref(_args(n_rays=0)), FAKE, None, FAKE, FAKE, None) == 0      # no rays: nothing to do


def test_existing_entry_points_refuse_as_before(eng):
    lib, h = eng.lib, eng.h
    a = _args()
    assert lib.afx_render_backward(h, 0, FAKE, C.byref(a), FAKE, None, None) == AFX_E_INVALID
    assert _err(lib) == "afx_render_backward: null argument"
    assert lib.afx_mlp_backward(h, 0, FAKE, FAKE, 100, FAKE, None, FAKE, 1 << 30, None) == AFX_E_INVALID
    assert _err(lib) == "afx_mlp_backward: null argument"
    nows = _args()
    nows.workspace = None
    assert lib.afx_render_backward(h, 0, FAKE, C.byref(nows), FAKE, FAKE, None) == AFX_E_WORKSPACE
    assert _err(lib) == "afx_render_backward: workspace required"
    # the queries that were there keep their numbers' relation: the input-gradient ones are new values of the same function
    assert int(lib.afx_query(h, 8, 0, 0, 0)) == -1
    assert "unknown query 8" in _err(lib)
