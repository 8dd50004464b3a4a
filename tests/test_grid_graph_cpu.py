"""Host side of the graph-capturable grid iteration (no GPU needed): the per-ray step bound of afx_march_max_steps against the CPU oracle's
march, the workspace bound, and the refusals of afx_march_train_step_mse_capturable."""
import ctypes as C

import pytest
import torch

from oracle import angio_oracle as orc


def _load():
    from nerf_for_angiography_amd import _lib
    return _lib, _lib.load()


def _march_args(_lib, near, far, step, aabb=(-100.0, -100, -100, 100, 100, 100)):
    m = _lib.MarchArgs()
    m.n_rays, m.has_aabb, m.step = 1, 1, float(step)
    for i, v in enumerate(aabb):
        m.scene_aabb[i] = v
    m.has_near, m.near_plane, m.has_far, m.far_plane = 1, float(near), 1, float(far)
    return m


@pytest.mark.parametrize("near,far,n_samples", [(1400.0, 1600.0, 300), (1400.0, 1600.0, 128), (10.0, 19.7, 37), (0.5, 3.25, 64)])
def test_step_bound_covers_the_oracle_march(near, far, n_samples):
    """All cells occupied: the oracle march of random rays never has more steps per ray than the bound, and an axis-aligned ray through
    a box that holds all of [near, far] has exactly that many."""
    _lib, lib = _load()
    step = (far - near) / n_samples
    bound = int(lib.afx_march_max_steps(C.byref(_march_args(_lib, near, far, step))))
    assert bound >= n_samples
    centre = 0.5 * (near + far)
    box = torch.tensor([-far, -far, -far, far, far, far]) * 2
    # axis-aligned: from the origin along -z, the box extends far beyond [near, far]
    o = torch.tensor([[0.0, 0.0, 0.0]])
    d = torch.tensor([[0.0, 0.0, -1.0]])
    ri, _, _ = orc.march_grid(o, d, box, near, far, step)
    assert ri.numel() == bound
    g = torch.Generator().manual_seed(n_samples)
    o = torch.tensor([[0.0, 0.0, centre]]) + torch.randn(64, 3, generator=g) * 0.1 * (far - near)
    d = torch.nn.functional.normalize(torch.randn(64, 3, generator=g) * 0.2 + torch.tensor([0, 0, -1.0]), dim=-1)
    half = 0.3 * (far - near)
    ri, _, _ = orc.march_grid(o, d, torch.tensor([-half, -half, -half, half, half, half]), near, far, step)
    per_ray = torch.bincount(ri, minlength=64)
    assert int(per_ray.max()) <= bound
    ri, _, _ = orc.march_grid(o, d, None, near, far, step)      # no box: every ray spans [near, far]
    assert int(torch.bincount(ri, minlength=64).max()) <= bound and ri.numel() <= 64 * bound


def test_workspace_bound_and_refusals():
    """The workspace is fixed by (rays, steps per ray); the reference's batch fits the one-chunk plane at 4x128 and 8x256; a worst case beyond
    the packed step's sample limit is refused with a message naming it; the call refuses without a far plane, at other precisions and with
    null counters."""
    _lib, lib = _load()
    from nerf_for_angiography_amd.engine import Engine
    e4, e8 = Engine(128, 4), Engine(256, 8)
    p = _lib.PREC["f16s8"]
    b4 = int(lib.afx_march_train_workspace_bytes(e4.h, p, 5625, 302))
    b8 = int(lib.afx_march_train_workspace_bytes(e8.h, p, 5625, 302))
    assert 1.5e9 < b4 < 3e9 and 7e9 < b8 < 10e9 and b4 < b8
    assert int(lib.afx_march_train_workspace_bytes(e4.h, p, 5625, 100)) < b4
    assert int(lib.afx_march_train_workspace_bytes(e8.h, p, 200000, 302)) == -1 and b"sample limit" in lib.afx_last_error()
    assert int(lib.afx_march_train_workspace_bytes(e4.h, _lib.PREC["f16"], 5625, 302)) == -1
    m = _march_args(_lib, 1400.0, 1600.0, 200.0 / 300)
    m.has_far = 0
    assert int(lib.afx_march_max_steps(C.byref(m))) == -1 and b"far" in lib.afx_last_error()
    mt = _lib.MarchTrainArgs()
    mt.march = _march_args(_lib, 1400.0, 1600.0, 200.0 / 300)
    counts = (C.c_int64 * 3)()
    skip = (C.c_float * 1)()
    assert lib.afx_march_train_step_mse_capturable(e4.h, p, 4096, C.byref(mt), None, skip, None) == -1 and b"null" in lib.afx_last_error()
    assert lib.afx_march_train_step_mse_capturable(e4.h, _lib.PREC["f16"], 4096, C.byref(mt), counts, skip, None) == -1


def test_graph_helper_refuses_a_multi_rank_hook_and_other_optimizers():
    """GridTrainGraph refuses what it cannot capture - a multi-rank gradient all-reduce, an optimizer without a device-side skip - before it
    touches a GPU."""
    from nerf_for_angiography_amd import render
    from nerf_for_angiography_amd._lib import AfxError

    class _Hook:
        world = 2

        def __call__(self, g):
            pass

    class _Model:
        fused = True
        precision = "f16s8"

    saved = render._grad_hook
    render._grad_hook = _Hook()
    try:
        with pytest.raises(AfxError, match="multi-rank"):
            render.GridTrainGraph(_Model(), None, None, None, 16, 300, 1400.0, 1600.0, 1e-2, 1e-4)
    finally:
        render._grad_hook = saved
    model = torch.nn.Linear(2, 2)
    model.fused, model.precision, model._coef_trainable = True, "f16s8", (lambda: False)
    with pytest.raises(ValueError, match="fused=True, capturable=True"):
        render.GridTrainGraph(model, torch.optim.SGD(model.parameters(), lr=0.1), None, None, 16, 300, 1400.0, 1600.0, 1e-2, 1e-4)
