"""The exact 3-D distance transform and the surface-distance scores on the GPU (afx_distance_transform_edt_3d, afx_surface_metrics_3d;
engine.distance_transform_edt_3d / engine.surface_metrics_3d, visualization/sweep.py) against the NumPy / SciPy restatement of
tests/surface_reference.py: squared distances and distances bit for bit, counts, hd, the percentile and the vessel Dice exactly, assd to
the rounding bound of a sum taken in another order."""
import numpy as np
import pytest
import torch

import surface_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NONE = 0xffffffff

# small volumes at which the tiling can go wrong: fewer lines than a tile, sizes that are no multiple of it, single lines along each axis,
# lines longer than a workgroup or a tile (and, from 513 voxels, the narrower tile), more than one tile and block
SHAPES = [(5, 7, 3), (33, 17, 65), (1, 1, 40), (1, 40, 1), (40, 1, 1), (3, 2, 300), (2, 300, 3), (300, 2, 3), (2, 520, 35), (1024, 1, 3),
          (64, 64, 64)]


def _gpu_edt(fg):
    from nerf_for_angiography_amd.engine import distance_transform_edt_3d
    dist, d2 = distance_transform_edt_3d(torch.from_numpy(np.ascontiguousarray(fg)).to(DEV), return_squared=True)
    assert dist.dtype == torch.float64 and d2.dtype == torch.int64 and dist.shape == d2.shape == fg.shape
    return dist.cpu().numpy(), d2.cpu().numpy()


def _check_edt(fg, what):
    dist, d2 = _gpu_edt(fg)
    if fg.all():                                       # no zero voxel (SciPy's values mean nothing there): the mark and +inf
        assert (d2 == NONE).all() and np.isposinf(dist).all(), what
    else:
        want = sr.edt(fg)
        assert np.array_equal(d2, np.rint(want * want).astype(np.int64)), (what, np.abs(d2 - want * want).max())
        assert np.array_equal(dist.view(np.int64), want.view(np.int64)), what            # bit for bit
    again, d2_again = _gpu_edt(fg)
    assert np.array_equal(again.view(np.int64), dist.view(np.int64)) and np.array_equal(d2_again, d2), what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edt_3d_is_exact(shape):
    rng = np.random.default_rng(shape[0] * 7919 + shape[1] * 31 + shape[2])
    for p in (0.5, 0.99, 0.999):
        _check_edt(rng.random(shape) < p, f"p = {p}")
    for corner in ((0, 0, 0), (shape[0] - 1, shape[1] - 1, shape[2] - 1), (0, shape[1] - 1, 0)):
        fg = np.ones(shape, bool)                      # one zero voxel in a corner: the search crosses whole lines without an early exit
        fg[corner] = False
        _check_edt(fg, f"zero voxel at {corner}")
    _check_edt(np.zeros(shape, bool), "all zero")
    _check_edt(np.ones(shape, bool), "no zero voxel")


def test_edt_3d_takes_any_dtype_and_refuses_bad_input():
    from nerf_for_angiography_amd.engine import distance_transform_edt_3d
    from nerf_for_angiography_amd._lib import AfxError
    rng = np.random.default_rng(5)
    x = rng.random((9, 6, 11)) * (rng.random((9, 6, 11)) < 0.8)
    want = sr.edt(x)
    for t in (torch.from_numpy(x), torch.from_numpy(x.astype(np.float32)), torch.from_numpy(x != 0), torch.from_numpy(np.ceil(x * 100).astype(np.int64))):
        assert np.array_equal(distance_transform_edt_3d(t.to(DEV)).cpu().numpy(), want)
    sliced = torch.from_numpy(x).to(DEV).permute(2, 0, 1)                 # not contiguous
    assert np.array_equal(distance_transform_edt_3d(sliced).cpu().numpy(), sr.edt(x.transpose(2, 0, 1)))
    with pytest.raises(ValueError):
        distance_transform_edt_3d(torch.ones(4, 4, device=DEV))
    with pytest.raises(AfxError):
        distance_transform_edt_3d(torch.ones(1025, 1, 2, device=DEV))


def test_edt_3d_replays_from_a_graph():
    from nerf_for_angiography_amd.engine import distance_transform_edt_3d
    rng = np.random.default_rng(9)
    a = torch.from_numpy(rng.random((33, 17, 65)) < 0.97).to(DEV)
    b = torch.from_numpy(rng.random((33, 17, 65)) < 0.9).to(DEV)
    static_x = a.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        distance_transform_edt_3d(static_x, return_squared=True)         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dist, d2 = distance_transform_edt_3d(static_x, return_squared=True)
    for x in (b, a):
        static_x.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        want, want2 = distance_transform_edt_3d(x, return_squared=True)
        assert torch.equal(dist, want) and torch.equal(d2, want2)
        assert np.array_equal(dist.cpu().numpy(), sr.edt(x.cpu().numpy()))


def _gpu_metrics(pred, gt, thr_pred, thr_gt, q=95.0):
    from nerf_for_angiography_amd.engine import surface_metrics_3d
    return surface_metrics_3d(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), thr_pred, thr_gt, q)


def _compare_scores(got, want):
    """The device's scores against the restatement's: everything exactly but assd, which is a sum taken in another order."""
    for key in ("n_pred", "n_gt", "n_overlap", "n_surface_pred", "n_surface_gt", "hd", "hd_percentile", "dice_vessel"):
        assert got[key] == want[key], (key, got[key], want[key])
    bound = sr.assd_bound(want["n_surface_pred"], want["n_surface_gt"])
    assert abs(got["assd"] - want["assd"]) <= bound * want["assd"], (got["assd"], want["assd"], bound)


def _check_scores(pred, gt, thr_pred, thr_gt, q=95.0):
    got = _gpu_metrics(pred, gt, thr_pred, thr_gt, q)
    want = sr.surface_metrics(pred, gt, thr_pred, thr_gt, q)
    print(f"surface metrics q = {q}: got {got}\n want {want}")
    _compare_scores(got, want)
    assert _gpu_metrics(pred, gt, thr_pred, thr_gt, q) == got                          # the same bits on a second run
    return got


def test_surface_metrics_of_two_offset_phantoms():
    shape = (24, 20, 28)
    a, b = sr.tube_and_ball(shape), sr.tube_and_ball(shape, offset=(1.5, -1.0, 2.0))
    for q in (95.0, 50.0, 0.0, 100.0, 37.3):
        got = _check_scores(a, b, 0.5, 0.5, q)
    assert 0.0 < got["dice_vessel"] < 1.0 and got["hd"] >= got["hd_percentile"] > 0.0 and got["assd"] > 0.0
    _check_scores(a, b, 0.3, 0.8)                      # a threshold per volume
    back = _check_scores(b, a, 0.5, 0.5)
    fwd = _check_scores(a, b, 0.5, 0.5)
    assert back["hd"] == fwd["hd"] and back["hd_percentile"] == fwd["hd_percentile"] and back["n_pred"] == fwd["n_gt"]


def test_surface_metrics_of_identical_masks():
    a = sr.tube_and_ball((24, 20, 28))
    got = _check_scores(a, a.copy(), 0.5, 0.5)
    assert got["hd"] == got["assd"] == got["hd_percentile"] == 0.0 and got["dice_vessel"] == 1.0


def test_surface_metrics_of_the_shifted_box():
    a = sr.box((9, 9, 16), (2, 2, 2), (7, 7, 8))
    b = sr.box((9, 9, 16), (2, 2, 5), (7, 7, 11))
    got = _check_scores(a, b, 0.5, 0.5)
    assert got["hd"] == 3.0 and got["hd_percentile"] == 3.0 and got["dice_vessel"] == 0.5
    assert abs(got["assd"] - 7.0 / 6.0) <= 1e-14


def test_surface_metrics_of_masks_on_the_grid_faces():
    full = np.ones((7, 9, 11), np.float32)             # every face voxel is surface: nothing lies beyond the grid
    slab = sr.box((7, 9, 11), (0, 0, 0), (7, 9, 4))
    _check_scores(full, slab, 0.5, 0.5)
    _check_scores(slab, full, 0.5, 0.5, q=80.0)
    flat = np.ones((1, 6, 70), np.float32)             # one voxel thick: every voxel is surface
    _check_scores(flat, sr.box((1, 6, 70), (0, 2, 10), (1, 5, 66)), 0.5, 0.5)


def test_surface_metrics_of_single_voxels():
    """M = 2 (and 3): np.percentile's interpolation runs with a fractional weight between the two order statistics."""
    a = np.zeros((5, 6, 7), np.float32)
    b = np.zeros((5, 6, 7), np.float32)
    a[1, 2, 3] = 1.0
    b[3, 4, 3] = 1.0
    got = _check_scores(a, b, 0.5, 0.5)
    assert got["n_surface_pred"] == got["n_surface_gt"] == 1 and got["hd"] == np.sqrt(8.0)
    b[0, 0, 0] = 1.0                                   # distances sqrt(8) (twice) and sqrt(14): the two order statistics differ
    for q in (95.0, 60.0, 50.0, 10.0):
        _check_scores(a, b, 0.5, 0.5, q)


def test_surface_metrics_refuse_an_empty_volume():
    a, b = sr.tube_and_ball((12, 10, 14)), sr.tube_and_ball((12, 10, 14), offset=(1, 0, 0))
    with pytest.raises(ValueError, match="pred"):
        _gpu_metrics(a, b, 2.0, 0.5)
    with pytest.raises(ValueError, match="gt"):
        _gpu_metrics(a, b, 0.5, 2.0)
    with pytest.raises(ValueError, match="pred or gt"):
        _gpu_metrics(a, b, 2.0, 2.0)
    from nerf_for_angiography_amd.engine import surface_metrics_record
    rec = surface_metrics_record(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), 0.5, 2.0).cpu().numpy()
    assert rec[12] == 2 and rec[0] > 0 and rec[1] == 0 and rec[4] == 0
    assert np.isnan(rec.view(np.float64)[[5, 6, 11]]).all() and (rec[7:11] == NONE).all()
    with pytest.raises(ValueError):
        _gpu_metrics(a, b[:, :, :5].copy(), 0.5, 0.5)


def test_surface_metrics_record_replays_from_a_graph():
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.engine import surface_metrics_record
    shape = (24, 20, 28)
    a = torch.from_numpy(sr.tube_and_ball(shape)).to(DEV)
    b = torch.from_numpy(sr.tube_and_ball(shape, offset=(1.5, -1.0, 2.0))).to(DEV)
    want = surface_metrics_record(a, b, 0.5, 0.5)
    ws = torch.empty(int(_lib.load().afx_surface_metrics_3d_workspace_bytes(*shape)), dtype=torch.uint8, device=DEV)
    rec = torch.zeros(16, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            surface_metrics_record(a, b, 0.5, 0.5, record=rec, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        rec.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rec, want)


def test_evaluation_sweep_with_the_surface_columns(golden):
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from nerf_for_angiography_amd.visualization.sweep import SURFACE_METRICS, evaluation_sweep, reconstruction_surface_metrics
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    scores, pred, ref = reconstruction_surface_metrics(m, vol, 100.0, 33)
    assert pred.shape == ref.shape == (33, 33, 33)
    thr = float(torch.mean(ref))
    want = sr.surface_metrics(pred.cpu().numpy(), ref.cpu().numpy(), thr, thr)
    voxel = 2.0 * 100.0 / 32
    assert scores["voxel_size"] == voxel and scores["threshold"] == thr
    assert scores["dice_vessel"] == want["dice_vessel"] and scores["hd"] == want["hd"] * voxel
    assert scores["hd_percentile"] == want["hd_percentile"] * voxel
    assert abs(scores["assd"] - want["assd"] * voxel) <= sr.assd_bound(want["n_surface_pred"], want["n_surface_gt"]) * want["assd"] * voxel
    df, _ = evaluation_sweep(m, gt, angles, *geo, metrics=["HD95 3D", "PSNR", "HD 3D", "DOT 3D", "ASSD 3D", "DICE 3D VESSEL"], volume=vol,
                             volume_outside=100.0, volume_points=33)
    assert list(df.columns) == BASE + ["PSNR", "DOT 3D"] + list(SURFACE_METRICS)
    for col, key in zip(SURFACE_METRICS, ("dice_vessel", "assd", "hd", "hd_percentile")):
        assert df[col].nunique() == 1 and df[col][0] == scores[key], col                   # one score, repeated on every row
    coarse, _, _ = reconstruction_surface_metrics(m, vol, 100.0, 33, threshold=thr * 0.5, q=50.0)
    assert coarse["threshold"] == thr * 0.5 and coarse["q"] == 50.0 and coarse["n_pred"] >= scores["n_pred"]
