"""The 3-D Frangi vesselness on the GPU (afx_frangi_3d; engine.frangi_3d / frangi_3d_record, sweep.reconstruction_vesselness_metrics) against
the NumPy / SciPy restatement of tests/frangi3d_reference.py: to 1e-12 of each volume's maximum (or twice the restatement's own
sensitivity to one-ulp changes of its input, where that is larger) with the same zero pattern and the same selected scales."""
import functools
import math

import numpy as np
import pytest
import torch

import frangi3d_reference as fr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _line_volume():
    """2 x 2 x 64: the minimum sides with a long contiguous axis - two bumps along axis 2 with a different weight on each of the 4 lines."""
    i2 = np.arange(64, dtype=np.float64)
    def bump(c, w):
        d2 = (i2 - c) ** 2
        return np.where(d2 <= 9 * w * w, np.exp(-d2 / (2 * w * w)), 0.0)
    a = np.array([[1.0, 0.6], [0.3, 0.8]])[:, :, None]
    b = np.array([[0.2, 0.9], [0.7, 0.1]])[:, :, None]
    return a * bump(20, 2.0)[None, None] + b * bump(45, 3.0)[None, None]


# name: (volume maker, sigmas).  The smallest shapes that still exercise each failure mode:
CASES = {
    "24x20x17": (lambda: fr.shapes_phantom((24, 20, 17), seed=3)[0], (1, 2, 3)),      # three distinct sides: any axis mix-up shows
    "5x6x7": (lambda: fr.shapes_phantom((5, 6, 7), seed=4)[0], (2,)),               # radius 8 > every side: the reflection wraps, every voxel an edge
    "2x2x64": (_line_volume, (1, 2)),                                                # the minimum sides
    # lines longer than a workgroup, N no multiple of 256.  Over a faint noise floor: around compact shapes on an exact-zero background a
    # single small scale leaves a rim of almost-zero smoothed values (products of three kernel tails) that would exceed the left-out cap
    "40x33x300": (lambda: fr.shapes_phantom((40, 33, 300), seed=5)[0] + 0.02 * np.random.default_rng(6).random((40, 33, 300)), (1.5,)),
    "16x16x16 noise": (lambda: np.random.default_rng(16).random((16, 16, 16)), (1, 2)),      # every ordering and sign of the eigenvalues
}


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    """(input as `dtype`, vesselness, scale index, parts, bar) of the restatement, computed once and shared."""
    make, sigmas = CASES[name]
    x = np.ascontiguousarray(make().astype(dtype))
    x64 = x.astype(np.float64)
    v, idx, parts = fr.frangi_3d(x64, sigmas, return_scale=True, return_parts=True)
    rng = np.random.default_rng(0)
    # the restatement's own largest relative change under random one-ulp (fp64) perturbations of its input sets the bar when above 1e-12
    sens = max(np.abs(fr.frangi_3d(np.where(rng.random(x.shape) < 0.5, np.nextafter(x64, 2.0), x64), sigmas) - v).max() for _ in range(4)) / v.max()
    bar = max(1e-12, 2 * sens)
    for a in (v, idx):
        a.setflags(write=False)
    return x, v, idx, parts, bar, sens


def _compare(name, dtype, got, got_idx):
    x, v, idx, parts, bar, sens = _reference(name, dtype)
    assert got.shape == v.shape and got.dtype == np.float64 and v.max() > 0, name
    err = np.abs(got - v).max()
    lam = parts["lambda_max"]
    floor = 1e-9 * lam.max()
    left_out = (lam > 0) & (lam < floor)                # an exactly zero Hessian gives an exact zero on both sides: compared as well
    flips = int((((got == 0) != (v == 0)) & ~left_out).sum())
    top = np.sort(parts["per_scale"], axis=0)
    clear = np.ones(v.shape, bool) if top.shape[0] == 1 else (top[-1] - top[-2]) > bar * v.max()
    print(f"{name} {np.dtype(dtype).name}: |gpu - ref| / max = {err / v.max():.3e} (bar {bar:.3e}, restatement sensitivity {sens:.3e}), "
          f"left out {int(left_out.sum())} of {v.size}, zero-pattern differences {flips}, scale-index differences "
          f"{int(((got_idx != idx) & clear).sum())} on {int(clear.sum())} clear voxels")
    assert left_out.mean() <= 1e-3, (name, left_out.mean())            # on the restatement alone
    assert err <= bar * v.max(), (name, err / v.max(), bar)
    assert flips == 0, (name, flips)
    assert got_idx.dtype == np.uint8 and np.array_equal(got_idx[clear], idx[clear]), name


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_restatement(name, dtype):
    from nerf_for_angiography_amd.engine import frangi_3d
    x = _reference(name, dtype)[0]
    v, idx = frangi_3d(torch.from_numpy(x).to(DEV), CASES[name][1], return_scale=True)
    assert v.dtype == torch.float64 and idx.dtype == torch.uint8 and v.shape == idx.shape == x.shape
    _compare(name, dtype, v.cpu().numpy(), idx.cpu().numpy())


def test_options():
    from nerf_for_angiography_amd.engine import frangi_3d
    x = _reference("24x20x17", np.float64)[0]
    xd = torch.from_numpy(x).to(DEV)
    for kw in (dict(alpha=0.7, beta=0.3, gamma=0.05), dict(sigmas=(0.8, 2.5), alpha=0.25), dict(sigmas=(3, 1), gamma=0.2)):
        sig = kw.get("sigmas", (1, 2, 3))
        ref, ref_idx, parts = fr.frangi_3d(x, return_scale=True, return_parts=True, **kw)
        got, got_idx = frangi_3d(xd, return_scale=True, **kw)
        err = float(np.abs(got.cpu().numpy() - ref).max() / ref.max())
        print(kw, "relative to the maximum:", err)
        assert err <= 1e-12 and np.array_equal(got.cpu().numpy() == 0, ref == 0), kw
        top = np.sort(parts["per_scale"], axis=0)
        clear = (top[-1] - top[-2]) > 1e-12 * ref.max()
        assert np.array_equal(got_idx.cpu().numpy()[clear], ref_idx[clear]) and len(sig) == parts["per_scale"].shape[0], kw
    assert torch.equal(frangi_3d(xd), frangi_3d(xd, return_scale=True)[0]) and isinstance(frangi_3d(xd), torch.Tensor)
    xq = torch.round(xd * 2.0 ** 20) / 2.0 ** 20            # multiples of 2^-20 in [0, 1.05]: 1 - xq and 1 - (1 - xq) are exact
    assert torch.equal(frangi_3d(1 - xq, black_ridges=True), frangi_3d(xq))
    flat = frangi_3d(torch.full((6, 7, 8), 0.37, device=DEV))
    assert flat.shape == (6, 7, 8) and not bool(flat.any())
    strided = xd.permute(2, 0, 1)                                                     # a non-contiguous view is taken as the volume it shows
    assert torch.equal(frangi_3d(strided), frangi_3d(strided.contiguous()))


def test_deterministic_and_graph_capturable():
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.engine import frangi_3d_record
    lib = _lib.load()
    a = torch.from_numpy(_reference("24x20x17", np.float32)[0]).to(DEV)
    b = torch.flip(a, dims=[0, 2]).contiguous()
    eager = {k: frangi_3d_record(t) for k, t in (("a", a), ("b", b))}
    again = frangi_3d_record(a)
    assert torch.equal(again[0], eager["a"][0]) and torch.equal(again[1], eager["a"][1])
    static_x = a.clone()
    out = torch.zeros(a.shape, dtype=torch.float64, device=DEV)
    idx = torch.zeros(a.shape, dtype=torch.uint8, device=DEV)
    ws = torch.empty(int(lib.afx_frangi_3d_workspace_bytes(*a.shape, 3)), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            frangi_3d_record(static_x, out=out, scale_index=idx, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    for k, t in (("b", b), ("a", a)):
        static_x.copy_(t)
        for buf in (out, idx, ws):
            buf.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[k][0]) and torch.equal(idx, eager[k][1]), k


def test_refusals():
    from nerf_for_angiography_amd._lib import AfxError
    from nerf_for_angiography_amd.engine import frangi_3d, frangi_3d_record
    with pytest.raises(AfxError):
        frangi_3d(torch.ones(4, 5, 6))
    for shape in ((4, 5), (2, 4, 5, 6)):
        with pytest.raises(ValueError):
            frangi_3d(torch.ones(shape, device=DEV))
    for shape in ((1, 5, 6), (4, 1, 6), (4, 5, 1)):
        with pytest.raises((AfxError, ValueError)):
            frangi_3d(torch.ones(shape, device=DEV))
    with pytest.raises(ValueError):
        frangi_3d(torch.ones(4, 5, 6, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        frangi_3d(torch.ones(4, 5, 6, device=DEV), gamma=0.0)
    with pytest.raises(AfxError):
        frangi_3d(torch.ones(4, 5, 6, device=DEV), sigmas=())
    with pytest.raises(AfxError, match="workspace"):
        frangi_3d_record(torch.ones(4, 5, 6, device=DEV), workspace=torch.empty(64, dtype=torch.uint8, device=DEV))


def _tube_pair(n=33):
    """(prediction, truth) float32 [n, n, n]: the truth two Gaussian tubes of widths 1.2 and 2 voxels with exact-zero background, the
    prediction the truth plus one floater in an empty corner - a Gaussian blob of 3 voxels radius (w = 3, cut at 3 w) and 0.7 of the
    vessels' peak density; and the blob's centre.  Why this blob: at the centre of a blob the three eigenvalues are equal, ra = rb = 1, and
    v = (1 - e^-2) e^-2 (1 - exp(-2 S / max S)) <= 0.117 - below v_min = 0.1 only when the blob's S is clearly below the scale's largest,
    which holds for a floater that is broader and fainter than the vessels (here v = 0.079 at the centre).  On the shell r ~ sqrt(w^2 + s^2)
    of any blob the radial curvature vanishes and the voxels look tubular; the filter removes a blob's core, not all of it."""
    i = np.arange(n, dtype=np.float64)
    i0, i1, i2 = np.meshgrid(i, i, i, indexing="ij")

    def prof(d2, w):
        return np.where(d2 <= 9 * w * w, np.exp(-d2 / (2 * w * w)), 0.0)

    gt = np.maximum(prof((i0 - 9) ** 2 + (i1 - 10) ** 2, 1.2), prof((i0 - 23) ** 2 + (i2 - 12) ** 2, 2.0))
    c = (8, 26, 26)
    blob = 0.7 * prof((i0 - c[0]) ** 2 + (i1 - c[1]) ** 2 + (i2 - c[2]) ** 2, 3.0)
    return np.maximum(gt, blob).astype(np.float32), gt.astype(np.float32), c


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_reconstruction_vesselness_metrics():
    from nerf_for_angiography_amd.visualization.sweep import reconstruction_vesselness_metrics
    pred, gt, c = _tube_pair()
    grids = (torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))
    sigmas, v_min = (1, 2, 3), 0.1
    scores, p, g, mask = reconstruction_vesselness_metrics(None, None, 100.0, 33, grids=grids)
    assert p is grids[0] and g is grids[1] and mask.dtype == torch.bool and mask.shape == (33, 33, 33)
    thr = float(torch.mean(grids[1]))
    a, b = pred >= np.float32(thr), gt >= np.float32(thr)
    vp, ip = fr.frangi_3d(pred, sigmas, return_scale=True)
    vg, ig = fr.frangi_3d(gt, sigmas, return_scale=True)
    for v in (vp, vg):                                                     # no voxel of the restatement sits on the v_min boundary
        assert np.abs(v - v_min).min() > 1e-9
    ta, tb = a & (vp >= v_min), b & (vg >= v_min)
    sg = np.array(sigmas, dtype=np.float64)
    mean_a, mean_b = sg[ip[ta]].sum() / ta.sum(), sg[ig[tb]].sum() / tb.sum()
    want = {"tubular_fraction": int(ta.sum()) / int(a.sum()), "tubular_fraction_gt": int(tb.sum()) / int(b.sum()),
            "dice_tubular": 2.0 * int((ta & tb).sum()) / (int(ta.sum()) + int(tb.sum())), "scale_ratio": float(mean_a / mean_b),
            "mean_scale": float(mean_a), "mean_scale_gt": float(mean_b), "n_pred": int(a.sum()), "n_gt": int(b.sum()), "n_tubular": int(ta.sum()),
            "n_tubular_gt": int(tb.sum()), "n_tubular_both": int((ta & tb).sum()), "sigmas": (1.0, 2.0, 3.0), "v_min": 0.1, "threshold": thr}
    print(f"vesselness scores: got {scores}\n want {want}")
    assert scores.keys() == want.keys()
    for key in want:
        assert _same(scores[key], want[key]), (key, scores[key], want[key])
    assert np.array_equal(mask.cpu().numpy(), ta)
    assert scores["tubular_fraction"] < scores["tubular_fraction_gt"] and scores["n_tubular_gt"] > 0
    assert a[c] and not bool(mask[c])                                      # the blob passes the threshold and fails the filter
    # another threshold, scale list and v_min; an empty tubular mask gives NaN, an empty thresholded mask raises
    other = reconstruction_vesselness_metrics(None, None, 100.0, 33, threshold=0.5, sigmas=(1.5, 2.5), v_min=0.3, grids=grids)[0]
    a5 = pred >= np.float32(0.5)
    v5 = fr.frangi_3d(pred, (1.5, 2.5))
    assert other["threshold"] == 0.5 and other["n_pred"] == int(a5.sum()) and other["n_tubular"] == int((a5 & (v5 >= 0.3)).sum())
    none = reconstruction_vesselness_metrics(None, None, 100.0, 33, v_min=2.0, grids=grids)[0]
    assert none["n_tubular"] == 0 and none["tubular_fraction"] == 0.0 and math.isnan(none["dice_tubular"]) and math.isnan(none["scale_ratio"])
    with pytest.raises(ValueError, match="threshold"):
        reconstruction_vesselness_metrics(None, None, 100.0, 33, threshold=5.0, grids=grids)


def test_sweep_vesselness_columns(golden):
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from nerf_for_angiography_amd.visualization.sweep import GRAPH_METRICS, VESSELNESS_METRICS, evaluation_sweep, reconstruction_vesselness_metrics
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    n = 17
    scores = reconstruction_vesselness_metrics(m, vol, 100.0, n)[0]
    df, _ = evaluation_sweep(m, gt, angles, *geo, metrics=["SCALE RATIO 3D", "PSNR", "TUBULAR FRACTION 3D", "BRANCHES 3D", "DICE 3D TUBULAR"],
                             volume=vol, volume_outside=100.0, volume_points=n)
    assert list(df.columns) == BASE + ["PSNR", "BRANCHES 3D"] + list(VESSELNESS_METRICS)
    assert list(df.columns).index(GRAPH_METRICS[0]) < list(df.columns).index(VESSELNESS_METRICS[0])
    print({k: scores[k] for k in ("tubular_fraction", "dice_tubular", "scale_ratio")})
    for col, key in zip(VESSELNESS_METRICS, ("tubular_fraction", "dice_tubular", "scale_ratio")):
        assert all(_same(float(v), float(scores[key])) for v in df[col]), col          # one value per column, repeated on every row
    assert 0.0 <= scores["tubular_fraction"] <= 1.0
