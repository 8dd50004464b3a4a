"""afx_tv_denoise_3d on the CPU: the library's two symbols and the argument refusals, the host-side checks of the engine, the sweep and the
driver, and properties of the NumPy restatement tests/tv_reference.py (include/afx.h: afx_tv_denoise_3d).  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import sirt_reference as sr
import tv_reference as tv
from nerf_for_angiography_amd import _lib, engine

AFX_E_INVALID = -1
FAKE = C.c_void_p(0x1000)      # never dereferenced: every refusal below comes before the device is touched
SYMBOLS = ("afx_tv_denoise_3d", "afx_tv_denoise_3d_workspace_bytes")


def test_library_exports_the_two_symbols():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "afx.h")).read()
    for name in SYMBOLS:
        assert name in _lib.exported_symbols()
        assert getattr(lib, name) is not None
        assert f" {name}(" in header
    assert lib.afx_tv_denoise_3d_workspace_bytes(20, 26, 17) == 6 * 8 * 20 * 26 * 17
    assert lib.afx_tv_denoise_3d_workspace_bytes(1, 1, 1) == 48
    for bad in ((0, 4, 4), (4, -1, 4), (2048, 1024, 1024), (65536, 65536, 1)):
        assert lib.afx_tv_denoise_3d_workspace_bytes(*bad) == 0


def _denoise(lib, **kw):
    a = dict(x=FAKE, n0=4, n1=5, n2=6, weight=0.1, tau=1.0 / 6.0, iterations=3, nonneg=0, mask=None, out=FAKE, workspace=FAKE,
             workspace_bytes=6 * 8 * 120)
    a.update(kw)
    rc = lib.afx_tv_denoise_3d(a["x"], a["n0"], a["n1"], a["n2"], a["weight"], a["tau"], a["iterations"], a["nonneg"], a["mask"], a["out"],
                               a["workspace"], a["workspace_bytes"], None)
    return rc, lib.afx_last_error().decode()


REFUSALS = [
    (dict(x=None), "x"), (dict(out=None), "out"),
    (dict(n0=0), "n0"), (dict(n1=-2), "n1"), (dict(n2=0), "n2"), (dict(n0=2048, n1=1024, n2=1024), "2^31"), (dict(n0=65536, n1=65536, n2=1), "2^31"),
    (dict(weight=0.0), "weight"), (dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"), (dict(weight=float("inf")), "weight"),
    (dict(tau=0.0), "tau"), (dict(tau=float("nan")), "tau"), (dict(tau=float("inf")), "tau"),
    (dict(iterations=-1), "iterations"),
    (dict(workspace=None), "workspace"), (dict(workspace=C.c_void_p(0x1004)), "workspace"), (dict(workspace_bytes=6 * 8 * 120 - 1), "workspace_bytes"),
]


@pytest.mark.parametrize("kw, word", REFUSALS, ids=[f"{'-'.join(k)}:{w}:{n}" for n, (k, w) in enumerate(REFUSALS)])
def test_denoise_refuses(kw, word):
    rc, msg = _denoise(_lib.load(), **kw)
    assert rc == AFX_E_INVALID and msg.startswith("afx_tv_denoise_3d: ") and word in msg, msg


def test_engine_has_no_cpu_path():
    x = torch.zeros(4, 5, 6, dtype=torch.float64)
    with pytest.raises(engine.AfxError, match="no CPU path"):
        engine.tv_denoise_3d(x, 0.1)
    with pytest.raises(ValueError, match=r"\[n0, n1, n2\]"):
        engine.tv_denoise_3d(torch.zeros(4, 5, dtype=torch.float64), 0.1)
    poses = np.stack([sr.look_at_pose((0.0, 0.0, 50.0))])
    views = dict(records=torch.from_numpy(engine.hull_view_records(poses, 30.0)), n_views=1, width=8, height=8, near=40.0, far=60.0, n_samples=4)
    with pytest.raises(engine.AfxError, match="no CPU path"):
        engine.sirt_reconstruct(views, torch.zeros(1, 8, 8, dtype=torch.float64), (4, 4, 4), tv_weight=1e-3)


def test_total_variation_equals_the_restatement():
    """engine.total_variation_3d is plain torch and runs anywhere: the restatement's figure to rounding of the sum."""
    rng = np.random.default_rng(5)
    for shape in ((1, 1, 1), (1, 7, 5), (9, 1, 17), (6, 5, 4)):
        u = rng.standard_normal(shape)
        got = engine.total_variation_3d(torch.from_numpy(u))
        assert got.dim() == 0 and got.dtype == torch.float64
        assert abs(float(got) - tv.total_variation(u)) <= 1e-13 * max(1.0, tv.total_variation(u))
    assert float(engine.total_variation_3d(torch.full((3, 4, 5), 2.5))) == 0.0
    ramp = torch.arange(5, dtype=torch.float64).repeat(3, 4, 1)      # differs along k only: 4 unit steps in each of 12 rows
    assert float(engine.total_variation_3d(ramp)) == 48.0


def test_sweep_names_and_checks():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.SIRT_TV_METRICS == ("DICE 3D SIRT-TV", "TV GAIN 3D", "CORR 3D SIRT-TV")
    families = [f[0] for f in sweep._VOLUME_FAMILIES]
    assert families[-2] is sweep.SIRT_METRICS and families[-1] is sweep.SIRT_TV_METRICS
    others = [sweep.METRICS, sweep._ALL_VOLUME_METRICS, sweep.HULL_METRICS, sweep.SIRT_METRICS] + families[:-1]
    for names in others:
        assert not set(sweep.SIRT_TV_METRICS) & set(names)
    with pytest.raises(ValueError, match="sirt_views"):
        sweep._check_metrics(["PSNR", "DICE 3D SIRT-TV"], None, object(), sirt_tv_weight=1e-3)
    with pytest.raises(ValueError, match="ground-truth volume"):
        sweep._check_metrics(["TV GAIN 3D"], None, None, sirt_views=({}, None), sirt_tv_weight=1e-3)
    with pytest.raises(ValueError, match="sirt_tv_weight"):
        sweep._check_metrics(["CORR 3D SIRT-TV"], None, object(), sirt_views=({}, None))
    got = sweep._check_metrics(["TV GAIN 3D", "CORR 3D SIRT", "HULL RATIO 3D", "PSNR", "DICE 3D SIRT-TV"], None, object(), hull_views={},
                               sirt_views=({}, None), sirt_tv_weight=1e-3)
    assert got == ["PSNR", "HULL RATIO 3D", "CORR 3D SIRT", "DICE 3D SIRT-TV", "TV GAIN 3D"]
    # the plain SIRT columns ask for no weight, as before
    assert sweep._check_metrics(["DICE 3D SIRT"], None, object(), sirt_views=({}, None)) == ["DICE 3D SIRT"]


def _args(*extra):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser
    return build_parser().parse_args(["--synthetic", *extra])


def test_driver_checks_the_tv_flags():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import check_args
    assert _args().sirt_tv_weight == 0.0 and _args().sirt_tv_iterations == 10
    check_args(_args())
    check_args(_args("--binary", "True", "--save_sirt", "sirt.npy", "--sirt_tv_weight", "3e-4", "--sirt_tv_iterations", "5"))
    check_args(_args("--binary", "True", "--save_sirt", "sirt.npy", "--sirt_tv_weight", "0"))
    with pytest.raises(ValueError, match="--sirt_tv_weight: needs --save_sirt"):
        check_args(_args("--binary", "True", "--sirt_tv_weight", "3e-4"))
    with pytest.raises(ValueError, match="--sirt_tv_weight"):
        check_args(_args("--binary", "True", "--save_sirt", "sirt.npy", "--sirt_tv_weight", "-1"))
    with pytest.raises(ValueError, match="--sirt_tv_weight"):
        check_args(_args("--binary", "True", "--save_sirt", "sirt.npy", "--sirt_tv_weight", "nan"))
    with pytest.raises(ValueError, match="--sirt_tv_iterations"):
        check_args(_args("--binary", "True", "--save_sirt", "sirt.npy", "--sirt_tv_weight", "3e-4", "--sirt_tv_iterations", "-1"))


# ---- properties of the restatement ----
def test_zero_iterations_return_x():
    x = np.random.default_rng(2).standard_normal((5, 6, 7))
    x[1, 2, 3] = -0.0
    out = tv.tv_denoise(x, 0.3, 0)
    assert np.array_equal(out, x) and np.array_equal(np.signbit(out), np.signbit(x)) and out is not x


@pytest.mark.parametrize("iterations", [1, 2, 15])
def test_a_constant_volume_is_returned_exactly(iterations):
    x = np.full((5, 4, 6), 0.7310585786300049)
    assert np.array_equal(tv.tv_denoise(x, 0.05, iterations), x)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 7, 5), (9, 1, 17)])
def test_thin_shapes_stay_finite(shape):
    x = np.random.default_rng(4).standard_normal(shape)
    out = tv.tv_denoise(x, 0.2, 15)
    assert out.shape == shape and np.isfinite(out).all()
    if shape == (1, 1, 1):
        assert np.array_equal(out, x)


@pytest.fixture(scope="module")
def scene():
    return sr.scene()


@pytest.fixture(scope="module")
def noisy(scene):
    """The denoising recipe: the scene's truth plus Gaussian noise of sigma 0.01, w = 0.004, denoised at 0, 1, 10 and 50 iterations."""
    x = scene["truth"] + 0.01 * np.random.default_rng(7).standard_normal(sr.SCENE_SHAPE)
    return x, {n: tv.tv_denoise(x, 0.004, n) for n in (0, 1, 10, 50)}


def test_the_mean_is_kept(noisy):
    """The divergence telescopes to zero over the volume and |p| <= w, so the sum of out equals the sum of x to rounding: within
    1e-13 w N."""
    x, outs = noisy
    n = x.size
    for iterations, out in outs.items():
        drift = math.fsum(out.ravel()) - math.fsum(x.ravel())
        print(f"{iterations} iterations: fsum(out) - fsum(x) = {drift:.3g} (bound {1e-13 * 0.004 * n:.3g})")
        assert abs(drift) <= 1e-13 * 0.004 * n


def test_the_denoising_recipe(scene, noisy):
    x, outs = noisy
    truth = scene["truth"]
    rmse = lambda u: float(np.sqrt(((u - truth) ** 2).mean()))
    tvs = [tv.total_variation(outs[n]) for n in (0, 1, 10, 50)]
    energies = [tv.rof_energy(outs[n], x, 0.004) for n in (0, 1, 10, 50)]
    print(f"TV {tvs}, ROF energy {energies}, RMSE {rmse(x):.5f} -> {rmse(outs[50]):.5f} (ratio {rmse(outs[50]) / rmse(x):.3f})")
    assert all(b <= a for a, b in zip(tvs, tvs[1:]))
    assert all(b < a for a, b in zip(energies, energies[1:]))
    assert rmse(outs[50]) < 0.5 * rmse(x)


def test_nonneg_and_mask(scene, noisy):
    x, outs = noisy
    out = tv.tv_denoise(x, 0.004, 10, nonneg=True, mask=scene["mask"])
    on = scene["mask"] != 0
    assert (outs[10] < 0).any() and out.min() >= 0 and not out[~on].any()
    assert np.array_equal(out[on], np.where(outs[10] > 0, outs[10], 0.0)[on])


def test_sirt_tv_beats_sirt_on_noisy_views(scene):
    """5 views, line integrals plus noise of 10 % of the largest, 30 iterations at relax 1, nonneg, no mask, weight 3e-4, 10 inner
    iterations: the RMSE against the truth is below 0.95 of plain SIRT's (measured: 0.889)."""
    b = scene["line_integrals"]
    b = b + 0.1 * b.max() * np.random.default_rng(1).standard_normal(b.shape)
    plain, _ = sr.sirt(b, sr.SCENE_SHAPE, scene["a12"], scene["records"], iterations=30, relax=1.0, **sr.SCENE_VIEW)
    with_tv = tv.sirt_tv(b, sr.SCENE_SHAPE, scene["a12"], scene["records"], iterations=30, tv_weight=3e-4, tv_iterations=10, relax=1.0,
                         **sr.SCENE_VIEW)
    rmse = lambda u: float(np.sqrt(((u - scene["truth"]) ** 2).mean()))
    print(f"RMSE SIRT {rmse(plain):.6f}, SIRT-TV {rmse(with_tv):.6f}, ratio {rmse(with_tv) / rmse(plain):.4f}")
    assert rmse(with_tv) < 0.95 * rmse(plain)
