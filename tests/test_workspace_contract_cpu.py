"""The host side of the caller-workspace contract (no GPU needed): the guard-band harness of tests/workspace_contract.py checked on host
tensors, the table of tests/test_gpu_workspace_contract.py checked against include/afx.h, and the alignment rule - every entry point that
takes a workspace refuses a base that is no multiple of 16 bytes with its workspace error code, before it touches a device.  The
pointers are never-dereferenced integers, as in tests/test_host_cpu.py: 4096 for every valid one."""
import ctypes as C
import os
import re

import pytest
import torch

import workspace_contract as wc
from conftest import ROOT

AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
P = 4096                        # a valid (aligned, never dereferenced) pointer
AMPLE = 1 << 40
MISALIGNED = (P + 8, P + 1)


# ---------------------------------------------------------------- the harness
@pytest.mark.parametrize("nbytes", [1, 256, 1000])
@pytest.mark.parametrize("fill", [0x00, 0xFF, "random"])
def test_guard_check_sees_one_byte_on_either_side_and_nothing_inside(nbytes, fill):
    whole, interior = wc.arena(nbytes, fill)
    assert whole.numel() == nbytes + 2 * wc.GUARD and interior.numel() == nbytes and interior.data_ptr() == whole.data_ptr() + wc.GUARD
    assert wc.GUARD % 256 == 0
    before = whole.clone()
    assert wc.guards_intact(whole, nbytes, before)
    for at, intact in ((wc.GUARD - 1, False), (wc.GUARD + nbytes, False), (wc.GUARD, True), (wc.GUARD + nbytes - 1, True),
                       (0, False), (whole.numel() - 1, False)):
        hit = before.clone()
        hit[at] ^= 0x5A
        assert wc.guards_intact(hit, nbytes, before) == intact, (at, intact)


def test_fills_and_typed_arenas():
    assert wc.FILLS == (0x00, 0xFF, "random", "stale")
    zero, ones = wc.arena(64, 0x00)[0], wc.arena(64, 0xFF)[0]
    assert int(zero.sum()) == 0 and bool((ones == 0xFF).all())
    a, b, c = wc.arena(4096, "random")[0], wc.arena(4096, "random")[0], wc.arena(4096, "random", seed=1)[0]
    assert torch.equal(a, b) and not torch.equal(a, c) and len(torch.unique(a)) > 200        # seeded, and bytes of every kind
    whole, t = wc.typed_arena((3, 5), torch.float64, 0xFF)
    assert t.shape == (3, 5) and t.dtype == torch.float64 and bool(torch.isnan(t).all()) and t.data_ptr() == whole.data_ptr() + wc.GUARD
    whole, t = wc.typed_arena((7,), torch.int32, 0xFF)
    assert bool((t == -1).all())
    before = whole.clone()
    t[-1] = 3                                                # the last element of the interior: no guard is touched
    assert wc.guards_intact(whole, 28, before)
    whole, t = wc.typed_arena((0, 3), torch.float32, "random")
    assert t.numel() == 0 and whole.numel() == 2 * wc.GUARD
    nan = torch.tensor([float("nan"), 0.0])
    assert wc.same_bits(nan, nan.clone()) and not wc.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not wc.same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.float64))


# ---------------------------------------------------------------- the table against the header
def _header():
    txt = open(os.path.join(ROOT, "include", "afx.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def functions_with_a_workspace_parameter():
    """Every function of include/afx.h whose prototype has a parameter named `workspace`."""
    return sorted(name for name, params in re.findall(r"\b(afx_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", _header()) if re.search(r"\bworkspace\b", params))


def functions_with_a_workspace_field():
    """Every function of include/afx.h that takes a pointer to an args struct with a `workspace` field."""
    structs = [name for body, name in re.findall(r"typedef struct \w+ \{(.*?)\}\s*(\w+);", _header(), flags=re.S) if re.search(r"\bworkspace\b", body)]
    out = set()
    for name, params in re.findall(r"\b(afx_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", _header()):
        if any(re.search(rf"\b{s}\s*\*", params) for s in structs):
            out.add(name)
    return sorted(out)


def test_the_contract_table_names_every_workspace_taking_function():
    import test_gpu_workspace_contract as gpu
    table = set(gpu.TABLE)
    by_parameter = functions_with_a_workspace_parameter()
    assert len(by_parameter) >= 20 and "afx_frangi" in by_parameter and "afx_topk_indices" in by_parameter
    assert not set(by_parameter) - table, sorted(set(by_parameter) - table)
    by_field = functions_with_a_workspace_field()
    assert "afx_grid_refresh" in by_field and "afx_march_render" in by_field and "afx_hier_train_step_mse" in by_field
    # the args-struct functions: in the table, or among those another test pins (named there with that test), or takers of afx_render_args
    # that never look at its workspace
    known = table | set(gpu.COVERED_ELSEWHERE) | set(gpu.WORKSPACE_FIELD_UNUSED)
    assert not set(by_field) - known, sorted(set(by_field) - known)
    declared = set(re.findall(r"\b(afx_[a-z0-9_]+)\s*\(", _header()))
    assert known <= declared, sorted(known - declared)       # no stale names
    for name, entry in gpu.TABLE.items():
        assert entry is not None and callable(entry), name     # every table entry has a case that runs it


# ---------------------------------------------------------------- alignment: refused on the host
def _lib_and_lib():
    from nerf_for_angiography_amd import _lib
    return _lib, _lib.load()


def _misaligned_calls():
    """name -> f(workspace pointer) -> rc, every other argument valid: fake pointers, shapes the call takes, an ample workspace_bytes."""
    from nerf_for_angiography_amd.engine import Engine
    from test_grid_refresh_cpu import _grid
    from test_grid_render_cpu import _args as render_args
    from test_grid_single_eval_cpu import _train_args
    from test_input_grads_cpu import _args as dense_args
    _lib, lib = _lib_and_lib()
    sig = (C.c_double * 2)(1.0, 2.0)
    aff = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    ref = (C.c_double * 3)(0, 0, 0)
    g = _grid(_lib)
    e = Engine(128, 4)
    s8, f32 = _lib.PREC["f16s8"], _lib.PREC["f32"]
    counts, skip = (C.c_int64 * 3)(), (C.c_float * 1)()

    def dense(ws, **kw):
        a = dense_args(**kw)
        a.workspace = ws
        return a

    def grid_step(ws):
        mt = _train_args(_lib)
        mt.workspace = ws
        return mt

    def march_render(ws, pose):
        a = render_args(_lib, pose=pose)
        a.workspace = ws
        return lib.afx_march_render(e.h, _lib.PREC["f16"], P, C.byref(a), None)

    def refresh(ws):
        a = _lib.GridRefreshArgs()
        a.grid = g
        a.occs = a.binary = a.bits = P
        a.n_draw, a.all_cells, a.occ_thre, a.ema_decay = 1024, 0, 0.01, 0.95
        a.workspace, a.workspace_bytes = ws, AMPLE
        return lib.afx_grid_refresh(e.h, s8, P, C.byref(a), None)

    def hier(ws):
        a = dense(ws, n_rays=9, n_samples=35, depth_mode=_lib.DEPTH_SHARED_Z)
        a.z = P
        return lib.afx_hier_train_step_mse(e.h, s8, P, C.byref(a), 7, P, P, 1.0, None, P, None)

    return {
        "afx_frangi": lambda ws: lib.afx_frangi(P, 3, 37, 53, sig, 2, 0.5, 15.0, 1, P, ws, AMPLE, None, None),
        "afx_distance_transform_edt": lambda ws: lib.afx_distance_transform_edt(P, 3, 37, 53, P, ws, AMPLE, None, None),
        "afx_sampling_weights": lambda ws: lib.afx_sampling_weights(P, 3, 37, 53, _lib.SAMPLING["frangi"], 1, sig, 2, 0.5, 15.0, P, P, ws, AMPLE, None, None),
        "afx_ssim": lambda ws: lib.afx_ssim(P, P, 3, 37, 53, P, ws, AMPLE, None, None),
        "afx_distance_transform_edt_3d": lambda ws: lib.afx_distance_transform_edt_3d(P, 9, 7, 5, P, P, ws, AMPLE, None, None),
        "afx_surface_metrics_3d": lambda ws: lib.afx_surface_metrics_3d(P, P, 9, 7, 5, 0.5, 0.5, 95.0, P, ws, AMPLE, None, None),
        "afx_label_components_3d": lambda ws: lib.afx_label_components_3d(P, 9, 7, 5, 3, P, P, P, ws, AMPLE, None, None),
        "afx_skeletonize_3d": lambda ws: lib.afx_skeletonize_3d(P, 9, 7, 5, 4, 0, P, P, ws, AMPLE, None),
        "afx_isosurface_3d": lambda ws: lib.afx_isosurface_3d(P, 9, 7, 5, 0.5, aff, P, 8, P, 8, P, ws, AMPLE, None, None),
        "afx_mesh_measures": lambda ws: lib.afx_mesh_measures(P, 8, P, 8, P, ref, P, ws, AMPLE, None, None),
        "afx_mesh_sdf_3d": lambda ws: lib.afx_mesh_sdf_3d(P, 8, P, 8, 9, 7, 5, aff, 0, P, None, None, P, ws, AMPLE, None, None),
        "afx_centreline_graph": lambda ws: lib.afx_centreline_graph(P, P, 9, 7, 5, None, P, P, P, P, 8, P, ws, AMPLE, None, None),
        "afx_prune_spurs": lambda ws: lib.afx_prune_spurs(P, P, 9, 7, 5, 1.0, 2, 0, P, P, ws, AMPLE, None, None),
        "afx_frangi_3d": lambda ws: lib.afx_frangi_3d(P, 1, 9, 7, 5, sig, 2, 0.5, 0.5, 0.0, 0, P, P, ws, AMPLE, None, None),
        "afx_topk_indices": lambda ws: lib.afx_topk_indices(P, 3000, 10, P, ws, AMPLE, None),
        "afx_sample_batches": lambda ws: lib.afx_sample_batches(P, 3000, 0, 0, 4, 10, P, ws, AMPLE, None),
        "afx_sample_batches_dev": lambda ws: lib.afx_sample_batches_dev(P, 3000, 0, P, 4, 10, P, ws, AMPLE, None),
        "afx_grid_select_cells": lambda ws: lib.afx_grid_select_cells(C.byref(g), P, 16, 0, 0, None, P, P, ws, AMPLE, None),
        "afx_grid_refresh": refresh,
        "afx_march_train_step_mse": lambda ws: lib.afx_march_train_step_mse(e.h, s8, P, C.byref(grid_step(ws)), None),
        "afx_march_train_step_mse_capturable": lambda ws: lib.afx_march_train_step_mse_capturable(e.h, s8, P, C.byref(grid_step(ws)), counts, skip, None),
        "afx_march_train_step_mse_single_eval": lambda ws: lib.afx_march_train_step_mse_single_eval(e.h, s8, P, C.byref(grid_step(ws)), counts, skip, None),
        "afx_march_render[arrays]": lambda ws: march_render(ws, False),
        "afx_march_render[pose]": lambda ws: march_render(ws, True),
        "afx_hier_train_step_mse": hier,
        "afx_train_step_packed_mse": lambda ws: lib.afx_train_step_packed_mse(e.h, s8, P, P, P, 64, P, P, 100, P, P, P, 1.0, P, P, ws, AMPLE, None),
        "afx_mlp_backward": lambda ws: lib.afx_mlp_backward(e.h, f32, P, P, 1000, P, P, ws, AMPLE, None),
        "afx_mlp_backward_inputs[f32]": lambda ws: lib.afx_mlp_backward_inputs(e.h, f32, P, P, 1000, P, P, P, ws, AMPLE, None),
        "afx_mlp_backward_inputs[f16]": lambda ws: lib.afx_mlp_backward_inputs(e.h, _lib.PREC["f16"], P, P, 1000, P, P, P, ws, AMPLE, None),
        "afx_render_backward_inputs[f32]": lambda ws: lib.afx_render_backward_inputs(e.h, f32, P, C.byref(dense(ws)), P, P, P, P, None),
        "afx_render_backward_inputs[f16]": lambda ws: lib.afx_render_backward_inputs(e.h, _lib.PREC["f16"], P, C.byref(dense(ws)), P, P, P, P, None),
        "afx_render_forward": lambda ws: lib.afx_render_forward(e.h, f32, P, C.byref(dense(ws)), None),
        "afx_render_backward": lambda ws: lib.afx_render_backward(e.h, f32, P, C.byref(dense(ws)), P, P, None),
        "afx_train_step_mse": lambda ws: lib.afx_train_step_mse(e.h, s8, P, C.byref(dense(ws)), P, 1.0, P, None),
    }


def test_every_entry_point_refuses_a_misaligned_workspace_before_it_touches_a_device():
    import test_gpu_workspace_contract as gpu
    _, lib = _lib_and_lib()
    calls = _misaligned_calls()
    covered = {name.split("[")[0] for name in calls}
    takers = (set(gpu.TABLE) | set(gpu.COVERED_ELSEWHERE)) - {"afx_tv_denoise_3d"}
    assert covered == takers, (sorted(takers - covered), sorted(covered - takers))
    for name, call in calls.items():
        for ws in MISALIGNED:
            rc = call(ws)
            msg = lib.afx_last_error()
            assert rc == AFX_E_WORKSPACE, (name, ws, rc, msg)
            assert name.split("[")[0].encode() in msg and b"aligned to 16 bytes" in msg, (name, ws, msg)


def test_null_and_short_workspaces_keep_their_codes():
    """The helper's other two refusals, on an entry point of an analysis unit (its default message) and on one of the API unit."""
    _, lib = _lib_and_lib()
    need = int(lib.afx_label_components_3d_workspace_bytes(9, 7, 5))
    call = lambda ws, nbytes: lib.afx_label_components_3d(P, 9, 7, 5, 3, P, P, P, ws, nbytes, None, None)
    assert call(None, AMPLE) == AFX_E_WORKSPACE and b"workspace" in lib.afx_last_error()
    assert call(P, need - 1) == AFX_E_WORKSPACE and f"{need - 1} < {need} bytes".encode() in lib.afx_last_error()
    assert call(P + 8, need - 1) == AFX_E_WORKSPACE and b"<" in lib.afx_last_error()       # too small is said before misaligned
    need = int(lib.afx_topk_workspace_bytes(3000))
    assert lib.afx_topk_indices(P, 3000, 10, P, P, need - 1, None) == AFX_E_WORKSPACE and f"< {need} bytes".encode() in lib.afx_last_error()
    assert lib.afx_topk_indices(P, 3000, 10, P, None, need, None) == AFX_E_INVALID


def test_tv_keeps_its_own_rule():
    """afx_tv_denoise_3d: 8 bytes, AFX_E_INVALID, its own message (include/afx.h)."""
    _, lib = _lib_and_lib()
    rc = lib.afx_tv_denoise_3d(P, 9, 7, 5, 0.3, 1.0 / 6.0, 2, 0, None, P, P + 1, AMPLE, None)
    assert rc == AFX_E_INVALID and b"aligned to 8 bytes" in lib.afx_last_error()
    rc = lib.afx_tv_denoise_3d(P, 9, 7, 5, 0.3, 1.0 / 6.0, 2, 0, None, P, P + 4, AMPLE, None)
    assert rc == AFX_E_INVALID and b"aligned to 8 bytes" in lib.afx_last_error()
    need = int(lib.afx_tv_denoise_3d_workspace_bytes(9, 7, 5))
    rc = lib.afx_tv_denoise_3d(P, 9, 7, 5, 0.3, 1.0 / 6.0, 2, 0, None, P, P, need - 1, None)
    assert rc == AFX_E_INVALID and b"workspace_bytes" in lib.afx_last_error()
