"""The SIRT operators on the CPU: the library's two symbols and their argument refusals, the host-side checks of the sweep and the driver,
and properties of the NumPy restatement tests/sirt_reference.py (include/afx.h: afx_xray_project, afx_xray_backproject).  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sirt_reference as sr
from nerf_for_angiography_amd import _lib, engine

AFX_E_INVALID = -1
FAKE = C.c_void_p(0x1000)      # never dereferenced: every refusal below comes before the device is touched
SYMBOLS = ("afx_xray_project", "afx_xray_backproject")
IDENTITY = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


def _bad12(value):
    a = list(IDENTITY)
    a[5] = value
    return (C.c_double * 12)(*a)


def test_library_exports_the_two_symbols():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "afx.h")).read()
    for name in SYMBOLS:
        assert name in _lib.exported_symbols()
        assert getattr(lib, name) is not None
        assert f"int {name}(" in header


def _project(lib, **kw):
    a = dict(volume=FAKE, n0=4, n1=5, n2=6, b=IDENTITY, views=FAKE, n_views=3, width=8, height=7, near=1.0, far=2.0, n_samples=5, target=None,
             weight=None, out=FAKE)
    a.update(kw)
    rc = lib.afx_xray_project(a["volume"], a["n0"], a["n1"], a["n2"], a["b"], a["views"], a["n_views"], a["width"], a["height"], a["near"],
                              a["far"], a["n_samples"], a["target"], a["weight"], a["out"], None)
    return rc, lib.afx_last_error().decode()


def _backproject(lib, **kw):
    a = dict(images=FAKE, views=FAKE, n_views=3, width=8, height=7, n0=4, n1=5, n2=6, a=IDENTITY, acc=FAKE, seen=FAKE, x=None, relax=1.0,
             nonneg=1, mask=None)
    a.update(kw)
    rc = lib.afx_xray_backproject(a["images"], a["views"], a["n_views"], a["width"], a["height"], a["n0"], a["n1"], a["n2"], a["a"], a["acc"],
                                  a["seen"], a["x"], a["relax"], a["nonneg"], a["mask"], None)
    return rc, lib.afx_last_error().decode()


PROJECT_REFUSALS = [
    (dict(volume=None), "volume"), (dict(b=None), "world_to_index"), (dict(views=None), "views"), (dict(out=None), "out"),
    (dict(n_views=0), "n_views"), (dict(n_views=65536), "n_views"),
    (dict(n0=1), "n0"), (dict(n1=1), "n1"), (dict(n2=0), "n2"), (dict(n0=2048, n1=1024, n2=1024), "2^31"),
    (dict(width=1), "width"), (dict(height=1), "height"), (dict(n_samples=0), "n_samples"),
    (dict(far=1.0), "far"), (dict(near=3.0), "far"), (dict(near=float("nan")), "near"), (dict(far=float("inf")), "far"),
    (dict(b=_bad12(float("nan"))), "world_to_index"), (dict(b=_bad12(float("inf"))), "world_to_index"),
    (dict(target=FAKE), "weight"), (dict(weight=FAKE), "target"),
]
BACKPROJECT_REFUSALS = [
    (dict(images=None), "images"), (dict(views=None), "views"), (dict(a=None), "index_to_world"),
    (dict(acc=None, seen=None), "no output"), (dict(mask=FAKE), "x_inout"),
    (dict(n_views=0), "n_views"), (dict(n_views=70000), "n_views"),
    (dict(n0=1), "n0"), (dict(n1=-3), "n1"), (dict(n2=1), "n2"), (dict(n0=2048, n1=1024, n2=1024), "2^31"),
    (dict(width=1), "width"), (dict(height=0), "height"),
    (dict(a=_bad12(float("nan"))), "index_to_world"), (dict(relax=float("nan"), x=FAKE), "relax"), (dict(relax=float("inf")), "relax"),
]


@pytest.mark.parametrize("kw, word", PROJECT_REFUSALS, ids=[f"{'-'.join(k)}:{w}" for k, w in PROJECT_REFUSALS])
def test_project_refuses(kw, word):
    rc, msg = _project(_lib.load(), **kw)
    assert rc == AFX_E_INVALID and msg.startswith("afx_xray_project: ") and word in msg, msg


@pytest.mark.parametrize("kw, word", BACKPROJECT_REFUSALS, ids=[f"{'-'.join(k)}:{w}" for k, w in BACKPROJECT_REFUSALS])
def test_backproject_refuses(kw, word):
    rc, msg = _backproject(_lib.load(), **kw)
    assert rc == AFX_E_INVALID and msg.startswith("afx_xray_backproject: ") and word in msg, msg


def test_engine_has_no_cpu_path():
    poses = np.stack([sr.look_at_pose((0.0, 0.0, 50.0))])
    with pytest.raises(engine.AfxError, match="no CPU path"):
        engine.xray_views(poses, 30.0, 8, 8, 40.0, 60.0, 4, device="cpu")
    views = dict(records=torch.from_numpy(engine.hull_view_records(poses, 30.0)), n_views=1, width=8, height=8, near=40.0, far=60.0, n_samples=4)
    with pytest.raises(engine.AfxError, match="no CPU path"):
        engine.xray_project(torch.zeros(4, 4, 4, dtype=torch.float64), views)
    with pytest.raises(engine.AfxError, match="no CPU path"):
        engine.xray_backproject(torch.zeros(1, 8, 8, dtype=torch.float64), views, (4, 4, 4))
    with pytest.raises(engine.AfxError, match="no CPU path"):
        engine.sirt_reconstruct(views, torch.zeros(1, 8, 8, dtype=torch.float64), (4, 4, 4))
    with pytest.raises(ValueError, match="width and height"):
        engine.xray_views(poses, 30.0, 1, 8, 40.0, 60.0, 4)
    with pytest.raises(ValueError, match="far > near"):
        engine.xray_views(poses, 30.0, 8, 8, 60.0, 60.0, 4)
    with pytest.raises(ValueError, match="n_samples"):
        engine.xray_views(poses, 30.0, 8, 8, 40.0, 60.0, 0)


def test_line_integrals():
    i = torch.tensor([[1.0, 0.5, 1e-9, 2.0, 0.0]], dtype=torch.float32)
    got = engine.line_integrals(i)
    assert got.dtype == torch.float64
    want = -np.log(np.clip(i.numpy().astype(np.float64), 1e-6, 1.0))
    assert np.allclose(got.numpy(), want, rtol=1e-15, atol=0) and got[0, 0] == 0 and got[0, 3] == 0 and got.min() >= 0
    with pytest.raises(ValueError, match="eps"):
        engine.line_integrals(i, eps=0.0)


def test_sweep_names_and_checks():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.SIRT_METRICS == ("DICE 3D SIRT", "DICE GAIN 3D", "CORR 3D SIRT")
    others = [sweep.METRICS, sweep._ALL_VOLUME_METRICS, sweep.HULL_METRICS] + [f[0] for f in sweep._VOLUME_FAMILIES if f[0] is not sweep.SIRT_METRICS]
    for names in others:
        assert not set(sweep.SIRT_METRICS) & set(names)
    with pytest.raises(ValueError, match="sirt_views"):
        sweep._check_metrics(["PSNR", "DICE 3D SIRT"], None, object())
    with pytest.raises(ValueError, match="sirt_views"):
        sweep._check_metrics(["CORR 3D SIRT"], None, object(), hull_views={})
    with pytest.raises(ValueError, match="ground-truth volume"):
        sweep._check_metrics(["DICE GAIN 3D"], None, None, sirt_views=({}, None))
    got = sweep._check_metrics(["CORR 3D SIRT", "HULL RATIO 3D", "PSNR", "DICE 3D SIRT"], None, object(), hull_views={}, sirt_views=({}, None))
    assert got == ["PSNR", "HULL RATIO 3D", "DICE 3D SIRT", "CORR 3D SIRT"]
    s = sweep.sirt_scores(n_sirt=300, n_pred=150, n_gt=100, n_sirt_gt=90, n_pred_gt=75, n=4, sx=10.0, sg=4.0, sxx=30.0, sgg=6.0, sxg=13.0)
    # x = (1, 2, 3, 4), g = (0, 1, 1, 2): cov 4 * 13 - 40 = 12, var 20 and 8
    assert s == dict(dice_sirt=0.45, dice_model=0.6, dice_gain=0.6 - 0.45, corr_sirt=12.0 / float(np.sqrt(160.0)))
    assert all(np.isnan(v) for v in sweep.sirt_scores(0, 0, 0, 0, 0, 8, 0.0, 0.0, 0.0, 0.0, 0.0).values())


def _args(*extra):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser
    return build_parser().parse_args(["--synthetic", *extra])


def test_driver_checks_save_sirt():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import check_args
    check_args(_args("--binary", "True", "--save_sirt", "sirt.npy"))
    check_args(_args("--save_sirt", "sirt.npy"))                                  # (the default data is CT-type)
    check_args(_args("--binary", "True", "--march", "grid", "--grid_init", "hull", "--save_sirt", "sirt.NPY", "--sirt_iterations", "5"))
    with pytest.raises(ValueError, match="--binary True or CT-type"):
        check_args(_args("--data_name", "sdf", "--save_sirt", "sirt.npy"))
    with pytest.raises(ValueError, match="--save_sirt: PATH"):
        check_args(_args("--binary", "True", "--save_sirt", "sirt.vtk"))
    with pytest.raises(ValueError, match="--sirt_iterations"):
        check_args(_args("--binary", "True", "--save_sirt", "sirt.npy", "--sirt_iterations", "0"))
    with pytest.raises(ValueError, match="--sirt_relax"):
        check_args(_args("--binary", "True", "--save_sirt", "sirt.npy", "--sirt_relax", "2.5"))


# ---- properties of the restatement ----
def test_backprojecting_ones_counts_the_views():
    """All-ones images: every lerp of ones is exactly 1 (1 + phi (1 - 1)), so acc == cnt exactly - on a lattice some of whose points are
    unseen by some views, by all, or lie behind a source."""
    a12 = np.array([2.0, 0.3, 0, -9.0, 0, 1.5, 0.2, -8.0, 0.1, 0, 2.5, -7.0])
    poses = np.stack([sr.look_at_pose((0.0, 0.0, 60.0)), sr.look_at_pose((50.0, 5.0, 8.0)), sr.look_at_pose((3.0, -2.0, 4.0), target=(3.0, -2.0, -30.0))])
    rec = sr.view_records(poses, (40.0, 70.0, 25.0))
    acc, cnt = sr.backproject(np.ones((3, 9, 11)), rec, (9, 12, 7), a12)
    assert np.array_equal(acc, cnt.astype(np.float64))
    assert set(np.unique(cnt)) == {0, 1, 2, 3}


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_projecting_ones_gives_the_chord(axis):
    """A ones volume on a unit lattice, the central rays of a far source on a lattice axis: y = the chord, n_axis - 1, to 1e-12 (the samples
    are 0.125 apart and none lies on a face)."""
    shape = (6, 8, 5)
    centre = [(n - 1) / 2.0 for n in shape]
    a12 = np.array([1, 0, 0, -centre[0], 0, 1, 0, -centre[1], 0, 0, 1, -centre[2]], np.float64)
    src = np.zeros(3)
    src[axis] = 1000.0
    pose = sr.look_at_pose(src, up=(0.0, 1.0, 0.0) if axis != 1 else (0.0, 0.0, 1.0))
    # even detector: pixel (W / 2, H / 2) is the central ray, exactly along the axis
    y = sr.project(np.ones(shape), sr.world_to_index(a12), sr.view_records(pose[None], 2000.0), 4, 4, 992.0, 1008.0, 128)
    assert abs(y[0, 2, 2] - (shape[axis] - 1)) <= 1e-12, y[0, 2, 2]
    assert np.abs(y - (shape[axis] - 1)).max() <= 1e-5      # the neighbours are oblique by 5e-4: longer by 1e-7 at most, inside all the way


@pytest.fixture(scope="module")
def scene():
    return sr.scene()


@pytest.mark.parametrize("masked", [False, True], ids=["no mask", "mask"])
def test_residual_falls_strictly(scene, masked):
    """20 iterations at relax = 1 on the 20 x 26 x 17 scene: the norm of the weighted residual falls in every iteration and ends below half
    of the first (measured: 0.177 without the mask, 0.170 with it - profiles/r22_sirt.md)."""
    x, res = sr.sirt(scene["line_integrals"], sr.SCENE_SHAPE, scene["a12"], scene["records"], iterations=20, relax=1.0,
                     mask=scene["mask"] if masked else None, **sr.SCENE_VIEW)
    norms = sr.residual_norms(res)
    print(f"residual norms: first {norms[0]:.6g}, last {norms[-1]:.6g}, ratio {norms[-1] / norms[0]:.4f}")
    assert np.all(np.diff(norms) < 0)
    assert norms[-1] < 0.5 * norms[0]
    assert x.min() >= 0 and x.max() > 0
    if masked:
        assert not x[scene["mask"] == 0].any()


def test_mask_changes_only_masked_voxels_to_zero(scene):
    """One update from the same volume and the same backprojection, with and without the mask: equal where the mask is set, zero elsewhere."""
    rng = np.random.RandomState(3)
    x0 = rng.uniform(-0.02, 0.05, sr.SCENE_SHAPE)
    acc, cnt = sr.backproject(scene["line_integrals"], scene["records"], sr.SCENE_SHAPE, scene["a12"])
    for nonneg in (False, True):
        free = sr.update(x0, acc, cnt, 1.9, nonneg)
        held = sr.update(x0, acc, cnt, 1.9, nonneg, scene["mask"])
        on = scene["mask"] != 0
        assert np.array_equal(held[on], free[on]) and not held[~on].any() and free[~on].any()
        assert (free.min() < 0) != nonneg
