"""Host side of the single-evaluation grid iteration (no GPU needed): the exported symbols, the workspace bound of
afx_march_train_step_mse_single_eval, and its refusals - each with its error code and message."""
import ctypes as C

import pytest

AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
NEAR, FAR, SPR = 1400.0, 1600.0, 300


def _load():
    from nerf_for_angiography_amd import _lib
    return _lib, _lib.load()


def _train_args(_lib, n_rays=64, has_far=1, ws_bytes=1 << 40):
    """Arguments that pass every check before the device is touched: fake (never dereferenced) pointers, a huge stated workspace."""
    mt = _lib.MarchTrainArgs()
    m = mt.march
    m.n_rays, m.has_aabb, m.step = n_rays, 1, (FAR - NEAR) / SPR
    for i, v in enumerate((-100.0, -100, -100, 100, 100, 100)):
        m.scene_aabb[i] = v
    m.has_near, m.near_plane, m.has_far, m.far_plane = 1, NEAR, has_far, FAR
    m.origins, m.dirs = 4096, 4096
    mt.early_stop_eps, mt.alpha_thre, mt.inv_n = 1e-2, 1e-4, 1.0 / n_rays
    mt.target, mt.pixel, mt.grad_flat, mt.workspace, mt.workspace_bytes = 4096, 4096, 4096, 4096, ws_bytes
    return mt


def _call(lib, eng, prec, mt):
    counts = (C.c_int64 * 3)()
    skip = (C.c_float * 1)()
    return lib.afx_march_train_step_mse_single_eval(eng.h, prec, 4096, C.byref(mt), counts, skip, None)


def test_symbols_are_exported():
    _lib, lib = _load()
    for name in ("afx_march_train_step_mse_single_eval", "afx_march_single_eval_workspace_bytes"):
        assert hasattr(lib, name), name
    from nerf_for_angiography_amd.engine import Engine
    assert callable(Engine.march_train_step_mse_single_eval) and callable(Engine.march_single_eval_workspace_bytes)


def test_workspace_bound_covers_the_layout_and_is_monotone():
    """The bound holds at least the stash of one chunk over every candidate row plus the per-candidate arrays, equals what the call asks for
    (workspace_needed), and grows with rays and steps; the reference's batch fits at 4x128 and 8x256."""
    _lib, lib = _load()
    from nerf_for_angiography_amd.engine import Engine
    p = _lib.PREC["f16s8"]
    for width, layers in ((128, 4), (256, 8)):
        e = Engine(width, layers)
        steps = int(lib.afx_march_max_steps(C.byref(_train_args(_lib).march)))
        assert steps >= SPR
        b = int(lib.afx_march_single_eval_workspace_bytes(e.h, p, 5625, steps))
        rows = (5625 * ((steps + 31) // 32) * 32 + 255) // 256 * 256
        assert b >= 2 * (layers + 1) * rows * width + rows * (4 * 4 + 4) + 5625 * steps * 13
        prev = 0
        for n_rays in (1, 7, 64, 1000, 5625):
            cur = int(lib.afx_march_single_eval_workspace_bytes(e.h, p, n_rays, steps))
            assert cur > prev
            prev = cur
        prev = 0
        for s in (0, 1, 31, 32, 33, 100, steps):
            cur = int(lib.afx_march_single_eval_workspace_bytes(e.h, p, 1000, s))
            assert cur >= prev
            prev = cur
        mt = _train_args(_lib, n_rays=5625, ws_bytes=1000)
        assert _call(lib, e, p, mt) == AFX_E_WORKSPACE
        assert mt.workspace_needed == b and b"afx_march_single_eval_workspace_bytes" in lib.afx_last_error()


def test_refusals():
    """Each unsupported configuration returns its error code and says why - before the device is touched."""
    _lib, lib = _load()
    from nerf_for_angiography_amd.engine import Engine
    p = _lib.PREC["f16s8"]
    e = Engine(128, 4)
    for prec in ("f32", "bf16", "f16"):
        assert _call(lib, e, _lib.PREC[prec], _train_args(_lib)) == AFX_E_INVALID
        assert b"AFX_PREC_F16S8 only" in lib.afx_last_error()
    assert int(lib.afx_march_single_eval_workspace_bytes(e.h, _lib.PREC["f16"], 64, 300)) == -1
    assert _call(lib, Engine(128, 4, act="tanh"), p, _train_args(_lib)) == AFX_E_INVALID
    assert b"ReLU" in lib.afx_last_error()
    for enc, n_freq in (("barf", 5), ("fourier", 5)):
        assert _call(lib, Engine(128, 4, enc=enc, n_freq=n_freq), p, _train_args(_lib)) == AFX_E_INVALID
        assert b"no input encoding" in lib.afx_last_error()
    assert _call(lib, e, p, _train_args(_lib, has_far=0)) == AFX_E_INVALID
    assert b"far plane" in lib.afx_last_error()
    assert _call(lib, Engine(256, 8), p, _train_args(_lib, n_rays=200000)) == AFX_E_INVALID
    assert b"sample limit" in lib.afx_last_error()
    assert int(lib.afx_march_single_eval_workspace_bytes(Engine(256, 8).h, p, 200000, 302)) == -1
    mt = _train_args(_lib)
    skip = (C.c_float * 1)()
    assert lib.afx_march_train_step_mse_single_eval(e.h, p, 4096, C.byref(mt), None, skip, None) == AFX_E_INVALID
    assert b"null" in lib.afx_last_error()
    mt = _train_args(_lib, ws_bytes=1 << 20)
    assert _call(lib, e, p, mt) == AFX_E_WORKSPACE and mt.workspace_needed > (1 << 20)


def test_python_layers_refuse_encodings_and_the_driver_refuses_other_modes():
    """render.march_train_step_mse(single_eval=True) / GridTrainGraph(single_eval=True) refuse an encoded model, and the driver refuses
    --single-eval outside --march grid at f16s8 without an encoding - before any GPU work."""
    from nerf_for_angiography_amd import render
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main

    class _Model:
        fused = True
        precision = "f16s8"
        use_pos_enc = "barf"

        def __init__(self):
            self.engine = None

    with pytest.raises(NotImplementedError, match="no input encoding"):
        render.march_train_step_mse(_Model(), None, None, None, None, SPR, NEAR, FAR, 1e-2, 1e-4, None, single_eval=True)
    base = ["--synthetic", "--img_size", "20", "--number_angles", "1", "--limited_size", "90", "--n_iters", "2", "--sample_size", "4",
            "--depth_samples", "32", "--num_layers", "2", "--num_hidden_units", "64", "--single-eval"]
    for extra in (["--march", "dense"], ["--march", "grid_ops"], ["--march", "grid", "--precision", "f16"],
                  ["--march", "grid", "--pos_enc", "barf"]):
        with pytest.raises(ValueError, match="--single-eval"):
            main(base + extra)
