"""afx_tv_denoise_3d, engine.tv_denoise_3d and SIRT-TV (engine.sirt_reconstruct(tv_weight=...)) against the NumPy restatement
tests/tv_reference.py: every comparison is on the fp64 bits.  Also the sweep's SIRT-TV columns (run with -m gpu on an MI355X)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import sirt_reference as sr
import tv_reference as tv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _engine():
    from nerf_for_angiography_amd import engine
    return engine


def _tile():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "afx.h")).read()
    return tuple(int(re.search(rf"#define AFX_TV_TILE_{a} (\d+)", header).group(1)) for a in range(3))


T0, T1, T2 = _tile()
# a single voxel, a single plane along axes 0 and 1; the scene; per axis one extent below, at and above the tile and one above two tiles,
# the other two extents above their tiles, so that every workgroup border is crossed by a halo and the last tile of every axis is ragged;
# and a volume of several tiles along every axis at once
SHAPES = [(1, 1, 1), (1, 7, 5), (9, 1, 17), sr.SCENE_SHAPE]
SHAPES += [(n, T1 + 1, T2 + 1) for n in (T0 - 1, T0, T0 + 1, 2 * T0 + 1)]
SHAPES += [(T0 + 1, n, T2 + 1) for n in (T1 - 1, T1, 2 * T1 + 1)]
SHAPES += [(T0 + 1, T1 + 1, n) for n in (T2 - 1, T2, 2 * T2 + 1)]
SHAPES += [(3 * T0 + 1, 2 * T1 + 3, 2 * T2 + 5)]
ITERATIONS = (0, 1, 2, 15)      # none; the first, which reads no p; both ping-pong parities; many
# nonneg, mask, out is x
OPTIONS = ((False, False, False), (True, False, False), (False, True, False), (True, True, True))


def _same_bits(device_tensor, array):
    """fp64 bits equal (the sign of zero included)."""
    return np.array_equal(device_tensor.cpu().numpy().view(np.int64), np.ascontiguousarray(array, dtype=np.float64).view(np.int64))


@functools.lru_cache(maxsize=None)
def _scene():
    return sr.scene()


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """name -> (volume, weight): random normal; exact ties and -0.0; one NaN; on the scene's shape the noisy scene as well."""
    rng = np.random.default_rng(shape[0] * 10007 + shape[1] * 101 + shape[2])
    out = {"normal": (rng.standard_normal(shape), 0.3)}
    ties = rng.choice(np.array([-1.0, -0.0, 0.0, 0.0, 1.0, 2.0]), size=shape)      # many equal neighbours: g = 0 and m = 0 exactly
    out["ties"] = (ties, 0.5)
    holed = rng.standard_normal(shape)
    holed[tuple(s // 2 for s in shape)] = np.nan
    out["nan"] = (holed, 0.3)
    if shape == sr.SCENE_SHAPE:
        out["noisy scene"] = (_scene()["truth"] + 0.01 * np.random.default_rng(7).standard_normal(shape), 0.004)
    mask = (rng.uniform(size=shape) < 0.6).astype(np.uint8)
    return out, mask


@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_device_equals_the_restatement(shape, iterations):
    eng = _engine()
    inputs, mask = _inputs(shape)
    dev_mask = torch.from_numpy(mask).to(DEV)
    for name, (x, weight) in inputs.items():
        for nonneg, masked, alias in OPTIONS:
            want = tv.tv_denoise(x, weight, iterations, nonneg=nonneg, mask=mask if masked else None)
            xd = torch.from_numpy(x).to(DEV)
            got = eng.tv_denoise_3d(xd, weight, iterations, nonneg=nonneg, mask=dev_mask if masked else None, out=xd if alias else None)
            torch.cuda.synchronize()                          # the launches end, whatever the volume holds
            assert (got is xd) == alias and tuple(got.shape) == shape and got.dtype == torch.float64
            what = (name, nonneg, masked, alias)
            if name == "nan":
                assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), what
            else:
                assert torch.equal(got.cpu(), torch.from_numpy(want)), what
                assert _same_bits(got, want), what
            if not alias:
                assert _same_bits(xd, x) or name == "nan", what      # x is only read
            if iterations == 0 and not nonneg and not masked and name != "nan":
                assert _same_bits(got, x)


def test_a_nan_stays_with_its_neighbours():
    """An iteration carries a NaN two steps further (u -> g and m -> p -> div): after two iterations and the last div nothing beyond
    four steps from it is touched."""
    shape = (3 * T0 + 1, 2 * T1 + 3, 2 * T2 + 5)
    x, weight = _inputs(shape)[0]["nan"]
    got = _engine().tv_denoise_3d(torch.from_numpy(x).to(DEV), weight, 2).cpu().numpy()
    centre = np.array([s // 2 for s in shape])
    far = np.abs(np.indices(shape) - centre[:, None, None, None]).sum(axis=0) > 4
    assert np.isnan(got).any() and np.isfinite(got[far]).all()


def test_two_runs_are_equal():
    eng = _engine()
    x = torch.from_numpy(_inputs(sr.SCENE_SHAPE)[0]["noisy scene"][0]).to(DEV)
    one, two = eng.tv_denoise_3d(x, 0.004, 50), eng.tv_denoise_3d(x, 0.004, 50)
    assert torch.equal(one.view(torch.int64), two.view(torch.int64)) and not torch.equal(one, x)
    want = tv.tv_denoise(x.cpu().numpy(), 0.004, 50)
    assert _same_bits(one, want)
    got_tv, want_tv = float(eng.total_variation_3d(one)), tv.total_variation(want)
    print(f"total variation {float(eng.total_variation_3d(x)):.4f} -> {got_tv:.4f}")
    assert abs(got_tv - want_tv) <= 1e-12 * want_tv


def test_a_captured_call_replays_the_eager_bits():
    """Buffers passed in, nothing allocated: one capture, replayed on two different inputs, gives what the eager call gives."""
    eng = _engine()
    shape = (2 * T0 + 1, T1 + 1, 2 * T2 + 1)
    rng = np.random.default_rng(11)
    a, b = torch.from_numpy(rng.standard_normal(shape)).to(DEV), torch.from_numpy(rng.standard_normal(shape) * 3.0).to(DEV)
    mask = torch.from_numpy((rng.uniform(size=shape) < 0.7).astype(np.uint8)).to(DEV)
    x, out = torch.zeros(shape, dtype=torch.float64, device=DEV), torch.zeros(shape, dtype=torch.float64, device=DEV)
    work = eng.tv_denoise_3d_workspace(shape, DEV)
    assert work.numel() == 6 * 8 * x.numel()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            eng.tv_denoise_3d(x, 0.2, 5, nonneg=True, mask=mask, out=out, workspace=work)
    torch.cuda.current_stream().wait_stream(side)
    for source in (a, b):
        x.copy_(source)
        work.fill_(0xFF)                                  # whatever the workspace holds: the first iteration reads none of it
        graph.replay()
        torch.cuda.synchronize()
        eager = eng.tv_denoise_3d(source, 0.2, 5, nonneg=True, mask=mask)
        assert torch.equal(out.view(torch.int64), eager.view(torch.int64))
        assert _same_bits(out, tv.tv_denoise(source.cpu().numpy(), 0.2, 5, nonneg=True, mask=mask.cpu().numpy()))


def test_bad_buffers_are_refused():
    eng = _engine()
    x = torch.zeros(4, 5, 6, dtype=torch.float64, device=DEV)
    with pytest.raises(eng.AfxError, match="workspace_bytes"):
        eng.tv_denoise_3d(x, 0.1, 3, workspace=torch.empty(6 * 8 * 120 - 8, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="out"):
        eng.tv_denoise_3d(x, 0.1, 3, out=torch.zeros(4, 5, 6, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="mask"):
        eng.tv_denoise_3d(x, 0.1, 3, mask=torch.ones(4, 5, 7, dtype=torch.uint8, device=DEV))
    with pytest.raises(eng.AfxError, match="weight"):
        eng.tv_denoise_3d(x, 0.0, 3)
    assert _same_bits(eng.tv_denoise_3d(x + 1.5, 0.1, 0, workspace=None), np.full((4, 5, 6), 1.5))      # no workspace needed


# ---- SIRT-TV ----
def _views(eng, scene):
    return eng.xray_views(scene["poses"], sr.SCENE_FOCAL, device=DEV, **sr.SCENE_VIEW)


@pytest.mark.parametrize("masked", [False, True], ids=["no mask", "mask"])
def test_sirt_tv_equals_the_restatement(masked):
    eng, scene = _engine(), _scene()
    mask = scene["mask"] if masked else None
    want = tv.sirt_tv(scene["line_integrals"], sr.SCENE_SHAPE, scene["a12"], scene["records"], iterations=4, tv_weight=3e-4, tv_iterations=3,
                      relax=1.0, mask=mask, **sr.SCENE_VIEW)
    got = eng.sirt_reconstruct(_views(eng, scene), torch.from_numpy(scene["line_integrals"]).to(DEV), sr.SCENE_SHAPE, scene["a12"], iterations=4,
                               relax=1.0, mask=None if mask is None else torch.from_numpy(mask).to(DEV), tv_weight=3e-4, tv_iterations=3)
    plain, _ = sr.sirt(scene["line_integrals"], sr.SCENE_SHAPE, scene["a12"], scene["records"], iterations=4, relax=1.0, mask=mask, **sr.SCENE_VIEW)
    assert _same_bits(got, want) and not np.array_equal(want, plain)
    if masked:
        assert not want[scene["mask"] == 0].any()


def test_without_a_weight_sirt_is_what_it_was():
    """tv_weight=None: the volume and the history of the two launches per iteration, bit for bit."""
    eng, scene = _engine(), _scene()
    views = _views(eng, scene)
    b, mask = torch.from_numpy(scene["line_integrals"]).to(DEV), torch.from_numpy(scene["mask"]).to(DEV)
    x, history = eng.sirt_reconstruct(views, b, sr.SCENE_SHAPE, scene["a12"], iterations=5, relax=1.0, mask=mask, return_history=True, tv_weight=None)
    want, residuals = sr.sirt(scene["line_integrals"], sr.SCENE_SHAPE, scene["a12"], scene["records"], iterations=5, relax=1.0, mask=scene["mask"],
                              **sr.SCENE_VIEW)
    assert _same_bits(x, want)
    norms = torch.stack([eng.sirt_residual_norm(torch.from_numpy(r).to(DEV)) for r in residuals]).cpu()
    assert torch.equal(history.view(torch.int64), norms.view(torch.int64))
    ell = eng.xray_project(torch.ones(sr.SCENE_SHAPE, dtype=torch.float64, device=DEV), views, scene["a12"])
    weight = torch.where(ell > 0, 1.0 / ell, torch.zeros_like(ell))
    y = torch.zeros(sr.SCENE_SHAPE, dtype=torch.float64, device=DEV)
    for _ in range(5):
        r = eng.xray_project(y, views, scene["a12"], target=b, weight=weight)
        eng.xray_backproject(r, views, sr.SCENE_SHAPE, scene["a12"], x_inout=y, relax=1.0, nonneg=True, mask=mask)
    assert torch.equal(x.view(torch.int64), y.view(torch.int64))
    assert torch.equal(eng.sirt_reconstruct(views, b, sr.SCENE_SHAPE, scene["a12"], iterations=5, relax=1.0, mask=mask).view(torch.int64),
                       x.view(torch.int64))


@pytest.mark.parametrize("masked", [False, True], ids=["no mask", "mask"])
def test_sirt_tv_beats_sirt_on_noisy_views(masked):
    """The recipe of test_tv_cpu.py on the device, 30 iterations: the RMSE against the truth is below 0.95 of plain SIRT's without the
    mask (measured on the host: 0.889) and below plain SIRT's with the scene's mask (0.92 - 0.94)."""
    eng, scene = _engine(), _scene()
    b = scene["line_integrals"]
    b = torch.from_numpy(b + 0.1 * b.max() * np.random.default_rng(1).standard_normal(b.shape)).to(DEV)
    mask = torch.from_numpy(scene["mask"]).to(DEV) if masked else None
    views = _views(eng, scene)
    kw = dict(iterations=30, relax=1.0, mask=mask, nonneg=True)
    plain = eng.sirt_reconstruct(views, b, sr.SCENE_SHAPE, scene["a12"], **kw)
    with_tv = eng.sirt_reconstruct(views, b, sr.SCENE_SHAPE, scene["a12"], tv_weight=3e-4, tv_iterations=10, **kw)
    truth = torch.from_numpy(scene["truth"]).to(DEV)
    rmse = lambda u: float(torch.sqrt(((u - truth) ** 2).mean()))
    ratio = rmse(with_tv) / rmse(plain)
    print(f"{'mask' if masked else 'no mask'}: RMSE SIRT {rmse(plain):.6f}, SIRT-TV {rmse(with_tv):.6f}, ratio {ratio:.4f}; "
          f"TV {float(eng.total_variation_3d(plain)):.4f} -> {float(eng.total_variation_3d(with_tv)):.4f}")
    assert ratio < (1.0 if masked else 0.95)


# ---- the sweep's columns ----
def test_sweep_columns_equal_the_stand_alone_scores(golden, monkeypatch):
    """On the G10 setup of test_gpu_sweep_shared.py: the three columns are reconstruction_sirt_metrics' scores at the weight; asked for
    together with the plain SIRT columns, plain SIRT runs once and SIRT-TV once."""
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from test_gpu_sweep_shared import N, OUTSIDE, _same
    from nerf_for_angiography_amd.visualization import sweep
    eng = _engine()
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    w, h, focal, src, near, far, s = geo
    poses = sweep._poses(angles, src, (0.0, 0.0, 0.0), DEV)
    views = eng.xray_views(poses, focal, w, h, near, far, s)
    images = eng.line_integrals(gt.reshape(len(angles), h, w))
    weight = 0.02
    keys = ("dice_sirt_tv", "tv_gain", "corr_sirt_tv")
    alone = sweep.reconstruction_sirt_metrics(m, vol, OUTSIDE, N, views, images, iterations=8, tv_weight=weight, tv_iterations=4)
    plain = sweep.reconstruction_sirt_metrics(m, vol, OUTSIDE, N, views, images, iterations=8)
    print(f"SIRT-TV alone: { {k: alone[0][k] for k in keys + ('dice_sirt', 'corr_sirt', 'n_sirt_tv', 'n_sirt', 'n_gt')} }")
    assert tuple(alone[1].shape) == (N, N, N) and alone[1].dtype == torch.float64 and float(alone[1].min()) >= 0 and float(alone[1].max()) > 0
    assert not torch.equal(alone[1], plain[1])
    assert all(np.isfinite(alone[0][k]) for k in keys) and alone[0]["tv_gain"] == alone[0]["dice_sirt_tv"] - alone[0]["dice_sirt"]
    assert all(_same(alone[0][k], plain[0][k]) for k in plain[0])      # the plain scores are those of the plain call
    want = eng.sirt_reconstruct(views, images, (N, N, N), sweep.grid_index_to_world(OUTSIDE, N), iterations=8, tv_weight=weight, tv_iterations=4)
    assert torch.equal(alone[1].view(torch.int64), want.view(torch.int64))
    runs = []
    real = eng.sirt_reconstruct
    def counting(*args, **kw):
        runs.append(kw.get("tv_weight"))
        return real(*args, **kw)
    monkeypatch.setattr(eng, "sirt_reconstruct", counting)
    df, _ = sweep.evaluation_sweep(m, gt, angles, *geo, metrics=["CORR 3D SIRT-TV", "PSNR", "DICE 3D SIRT", "TV GAIN 3D", "DICE GAIN 3D",
                                                                 "DICE 3D SIRT-TV", "CORR 3D SIRT"],
                                   volume=vol, volume_outside=OUTSIDE, volume_points=N, sirt_views=(views, images), sirt_iterations=8,
                                   sirt_tv_weight=weight, sirt_tv_iterations=4)
    monkeypatch.undo()
    assert sorted(runs, key=str) == sorted([None, weight], key=str), runs      # plain SIRT once, SIRT-TV once
    assert list(df.columns) == BASE + ["PSNR"] + list(sweep.SIRT_METRICS) + list(sweep.SIRT_TV_METRICS)
    for col, key in zip(sweep.SIRT_TV_METRICS, keys):
        assert len(df[col]) == len(angles) and all(_same(v, alone[0][key]) for v in df[col].tolist()), (col, df[col][0], alone[0][key])
    for col, key in zip(sweep.SIRT_METRICS, ("dice_sirt", "dice_gain", "corr_sirt")):
        assert all(_same(v, plain[0][key]) for v in df[col].tolist()), (col, df[col][0], plain[0][key])
    with pytest.raises(ValueError, match="sirt_tv_weight"):
        sweep.evaluation_sweep(m, gt, angles, *geo, metrics=["DICE 3D SIRT-TV"], volume=vol, sirt_views=(views, images))
