"""Host side of the forward-only grid render (no GPU needed): the exported symbols, the ctypes mirror of afx_march_render_args, the workspace
bound, every refusal of afx_march_render - each with its error code and message, before the device is touched - and the refusals of the Python
layers."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
NEAR, FAR, SPR = 1400.0, 1600.0, 400
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    from nerf_for_angiography_amd import _lib
    return _lib, _lib.load()


def _args(_lib, n_rays=64, pose=False, ws_bytes=1 << 40):
    """Arguments that pass every check before the device is touched: fake (never dereferenced) pointers, a huge stated workspace."""
    a = _lib.MarchRenderArgs()
    m = a.march
    m.has_aabb, m.step = 1, (FAR - NEAR) / SPR
    for i, v in enumerate((-100.0, -100, -100, 100, 100, 100)):
        m.scene_aabb[i] = v
    m.has_near, m.near_plane, m.has_far, m.far_plane = 1, NEAR, 1, FAR
    if pose:
        a.ray_mode, a.poses, a.width, a.height, a.focal, a.n_rays = _lib.RAYS_POSE, 4096, 100, 100, 1300.0, n_rays
    else:
        a.ray_mode, m.origins, m.dirs, m.n_rays = _lib.RAYS_ARRAYS, 4096, 4096, n_rays
    a.early_stop_eps, a.alpha_thre = 1e-2, 1e-3
    a.pixel, a.workspace, a.workspace_bytes = 4096, 4096, ws_bytes
    return a


def _call(lib, eng, prec, a):
    return lib.afx_march_render(eng.h, prec, 4096, C.byref(a), None)


def test_symbols_are_declared_and_exported():
    _lib, lib = _load()
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    for name in ("afx_march_render", "afx_march_render_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.exported_symbols() and f"{name}(" in header, name
    from nerf_for_angiography_amd.engine import Engine
    from nerf_for_angiography_amd import render
    assert callable(Engine.march_render) and callable(render.march_render) and callable(render.march_render_projection)


def test_ctypes_struct_matches_the_header(tmp_path):
    """Offsets of every field of afx_march_render_args and its size, as a C compiler lays them out from include/afx.h."""
    _lib, _ = _load()
    cc = shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/llvm/bin/clang"
    if not os.path.exists(cc) and not shutil.which(cc):
        pytest.fail("no C compiler to lay out include/afx.h with")
    fields = [f[0] for f in _lib.MarchRenderArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"afx.h\"\nint main(void) {\n"
                   + "".join(f'  printf("%zu\\n", offsetof(afx_march_render_args, {f}));\n' for f in fields)
                   + '  printf("%zu\\n", sizeof(afx_march_render_args));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [getattr(_lib.MarchRenderArgs, f).offset for f in fields] + [C.sizeof(_lib.MarchRenderArgs)]
    assert got == want


def test_workspace_bound_grows_with_rays_and_steps():
    _lib, lib = _load()
    for mode in (_lib.RAYS_ARRAYS, _lib.RAYS_POSE):
        prev = 0
        for n_rays in (1, 7, 64, 10000):
            cur = int(lib.afx_march_render_workspace_bytes(mode, n_rays, 402))
            assert cur >= n_rays * 402 * 24 and cur > prev
            prev = cur
    assert int(lib.afx_march_render_workspace_bytes(_lib.RAYS_POSE, 100, 402)) > int(lib.afx_march_render_workspace_bytes(_lib.RAYS_ARRAYS, 100, 402))
    assert int(lib.afx_march_render_workspace_bytes(7, 100, 402)) == -1
    assert int(lib.afx_march_render_workspace_bytes(_lib.RAYS_ARRAYS, 1 << 22, 600)) == -1 and b"2^31" in lib.afx_last_error()


def test_refusals():
    """Each refusal returns its code and says why - before the device is touched."""
    _lib, lib = _load()
    from nerf_for_angiography_amd.engine import Engine
    e = Engine(128, 4)
    p = _lib.PREC["f16"]
    assert lib.afx_march_render(e.h, p, 4096, None, None) == AFX_E_INVALID and b"null" in lib.afx_last_error()
    assert lib.afx_march_render(e.h, p, None, C.byref(_args(_lib)), None) == AFX_E_INVALID and b"null" in lib.afx_last_error()
    a = _args(_lib)
    a.pixel = None
    assert _call(lib, e, p, a) == AFX_E_INVALID and b"pixel" in lib.afx_last_error()
    a = _args(_lib)
    a.march.origins = None
    assert _call(lib, e, p, a) == AFX_E_INVALID and b"origins" in lib.afx_last_error()
    a = _args(_lib)
    a.workspace = None
    assert _call(lib, e, p, a) == AFX_E_INVALID and b"workspace" in lib.afx_last_error()
    assert _call(lib, e, 9, _args(_lib)) == AFX_E_INVALID and b"precision" in lib.afx_last_error()
    a = _args(_lib)
    a.ray_mode = 5
    assert _call(lib, e, p, a) == AFX_E_INVALID and b"ray_mode" in lib.afx_last_error()
    for field, bad in (("poses", None), ("width", 0), ("height", 0), ("focal", 0.0)):
        a = _args(_lib, pose=True)
        setattr(a, field, bad)
        assert _call(lib, e, p, a) == AFX_E_INVALID and b"pose mode needs" in lib.afx_last_error(), field
    a = _args(_lib)
    a.march.has_far = 0
    assert _call(lib, e, p, a) == AFX_E_INVALID and b"far plane" in lib.afx_last_error()
    for pose in (False, True):      # 2^23 rays x 402 steps: beyond afx_mlp_infer's 2^31 - 256 points
        assert _call(lib, e, p, _args(_lib, n_rays=1 << 23, pose=pose)) == AFX_E_INVALID and b"2^31" in lib.afx_last_error()
    for pose in (False, True):
        a = _args(_lib, n_rays=5000, pose=pose, ws_bytes=1000)
        a.n_candidates = 7
        assert _call(lib, e, p, a) == AFX_E_WORKSPACE and b"afx_march_render_workspace_bytes" in lib.afx_last_error()
        steps = int(lib.afx_march_max_steps(C.byref(a.march)))
        assert steps >= SPR and a.workspace_needed == int(lib.afx_march_render_workspace_bytes(a.ray_mode, 5000, steps))
        assert a.n_candidates == 0
    assert _call(lib, e, p, _args(_lib, n_rays=0)) == 0      # zero rays: nothing to do


class _FakeModel:
    fused = fused_forward = True
    precision = "f16"
    flat_params = torch.zeros(4)

    def parameters(self):
        return iter(())


def test_python_layers_refuse_cpu_tensors_autograd_and_unfused_models():
    from nerf_for_angiography_amd import render
    from nerf_for_angiography_amd._lib import AfxError
    from nerf_for_angiography_amd.model.CPPN import CPPN
    o, d = torch.zeros(4, 3), torch.zeros(4, 3)
    poses = torch.zeros(1, 3, 4, dtype=torch.float64)
    with pytest.raises(AfxError, match="GPU"):
        render.march_render(_FakeModel(), None, None, o, d, SPR, NEAR, FAR)
    with pytest.raises(AfxError, match="GPU"):
        render.march_render_projection(_FakeModel(), None, None, poses, 2, 2, 10.0, SPR, NEAR, FAR)
    md = dict(num_early_layers=2, num_late_layers=0, num_filters=64, num_input_channels=3, num_output_channels=1,
              num_input_channels_views=0, use_bias=True, pos_enc="none", pos_enc_basis=5, act_func="relu", fourier_sigma=5, num_img=1,
              device=torch.device("cpu"), precision="f16")
    model = CPPN(md)
    with pytest.raises(RuntimeError, match="march_train_step_mse"):      # autograd is recording and the model trains
        render.march_render(model, None, None, o, d, SPR, NEAR, FAR)
    with pytest.raises(RuntimeError, match="forward only"):
        render.march_render_projection(model, None, None, poses, 2, 2, 10.0, SPR, NEAR, FAR)
    with torch.no_grad(), pytest.raises(AfxError, match="GPU"):            # ... and under no_grad the host model is refused
        render.march_render(model, None, None, o, d, SPR, NEAR, FAR)
    unfused = CPPN(dict(md, act_func="tanh", pos_enc="barf"))
    with torch.no_grad(), pytest.raises(NotImplementedError, match="outside the fused kernels"):
        render.march_render(unfused, None, None, o, d, SPR, NEAR, FAR)
