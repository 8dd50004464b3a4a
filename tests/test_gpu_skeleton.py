"""3-D thinning to medial curves on the GPU (afx_skeletonize_3d; engine.skeletonize_3d / skeleton_record, visualization/sweep.py) against
the sequential restatement of tests/skeleton_reference.py.  Two voxels of one subfield are never 26-neighbours, so the parallel result
is the sequential one: skeleton and record must EQUAL the reference - there are no tolerances - and a second run gives the same bits."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import skeleton_reference as sk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the shapes the definition is easy to get wrong on: a single voxel, no interior, single lines and planes along each axis, odd extents
SHAPES = [(1, 1, 1), (2, 2, 2), (1, 1, 9), (1, 8, 9), (7, 1, 33), (5, 65, 9), (9, 17, 33), (33, 9, 17), (17, 18, 19)]
# the kernels tile the volume by its LINEAR index: a wave holds 64 consecutive voxels, a workgroup of the subfield launches 256 list
# entries, a workgroup of the init and mark launches a chunk of 2048 voxels.  One less, exactly and one more than each, with the long
# extent along every axis in turn.
SHAPES += [(1, 7, 9), (9, 7, 1), (4, 4, 4), (1, 5, 13), (13, 1, 5), (5, 13, 1),
           (3, 5, 17), (17, 3, 5), (4, 8, 8), (1, 1, 257), (1, 257, 1), (257, 1, 1),
           (1, 23, 89), (89, 1, 23), (23, 89, 1), (2, 1, 1024), (1, 1024, 2), (1024, 2, 1), (16, 8, 16), (1, 3, 683), (3, 683, 1), (683, 1, 3)]


def _gpu(mask, **kw):
    """-> (skeleton bool ndarray, record dict) of engine.skeletonize_3d."""
    from nerf_for_angiography_amd.engine import skeletonize_3d
    s, rec = skeletonize_3d(torch.from_numpy(np.ascontiguousarray(mask)).to(DEV), return_record=True, **kw)
    assert s.dtype == torch.bool and s.shape == mask.shape
    return s.cpu().numpy(), rec


def _want_record(rec, mask):
    return dict(rec, input=int(np.count_nonzero(mask)))


def _check(mask, what=""):
    want, rec = sk.skeletonize(mask)
    got, grec = _gpu(mask)
    assert grec == _want_record(rec, mask), (what, grec, rec)
    assert np.array_equal(got, want), (what, int((got != want).sum()))
    return want, rec


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_noise_equals_the_reference(shape):
    rng = np.random.default_rng(shape[0] * 7919 + shape[1] * 31 + shape[2])
    masks = [(f"p = {p}", rng.random(shape) < p) for p in (0.3, 0.5, 0.9)]
    masks += [("smoothed", sk.smooth_noise(shape, shape[1] + 3)), ("all one", np.ones(shape, bool)), ("all zero", np.zeros(shape, bool))]
    for what, mask in masks:
        _check(mask, what)


@functools.lru_cache(maxsize=None)
def _shape(name):
    """(mask, reference skeleton, reference record), computed once per session."""
    m = {"bar": sk.bar, "torus": sk.torus, "shell": sk.shell, "cube": sk.cube, "tree": lambda: sk.capsule_tree(48)}[name]()
    return (m, *sk.skeletonize(m))


def test_structured_shapes():
    got = {}
    for name in ("bar", "torus", "shell", "cube", "tree"):
        m, want, rec = _shape(name)
        s, grec = _gpu(m)
        assert np.array_equal(s, want) and grec == _want_record(rec, m), (name, grec, rec)
        assert sk.invariants(s) == sk.invariants(m) and not (s & ~m).any(), name
        got[name] = (s, grec)
    s, rec = got["bar"]                                                            # the centre line of [2:7, 3:8, 2:20] and a 2-voxel fork
    assert rec["passes"] == 3 and s.sum() == 16 and s[4, 5, 4:18].all() and sk.end_points(s).sum() == 3
    s, rec = got["torus"]                                                          # one closed loop
    assert rec["passes"] == 4 and sk.components26(s) == 1 and (sk.n_neighbours(s)[s] == 2).all()
    s, rec = got["shell"]                                                          # still a closed surface: the cavity is kept
    assert rec["passes"] == 3 and sk.cavities6(s) == 1 and not s[9, 9, 9] and sk.end_points(s).sum() == 0
    s, rec = got["cube"]
    assert rec["passes"] == 9 and np.argwhere(s).tolist() == [[d, d, d] for d in range(1, 16)]
    s, rec = got["tree"]
    assert rec["passes"] == 5 and sk.n_neighbours(s)[s].max() <= 4 and sk.end_points(s).sum() >= 4


def test_invariants_without_the_reference():
    m = sk.capsule_tree(64, floaters=30, seed=1)
    s, rec = _gpu(m)
    assert rec["converged"] == 1 and rec["input"] == m.sum() and rec["remaining"] == s.sum() == m.sum() - rec["deleted"]
    assert not (s & ~m).any()
    assert sk.invariants(s) == sk.invariants(m) and sk.components26(m) >= 25       # the tree and its floaters, none lost, none joined
    again, rec2 = _gpu(s)
    assert np.array_equal(again, s) and rec2["passes"] == 1 and rec2["deleted"] == 0
    assert sk.undeleted_candidates(s) == 0                                         # no border voxel left that the rule would delete
    assert s.sum() < 0.05 * m.sum()


def _record(mask, max_passes, sync_every, in_place=False):
    from nerf_for_angiography_amd.engine import skeleton_record
    x = torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(DEV)
    skel, rec = skeleton_record(x, max_passes, sync_every, skel=x if in_place else None)
    assert skel.dtype == torch.uint8 and rec.dtype == torch.int64 and rec.shape == (8,) and (skel.data_ptr() == x.data_ptr()) == in_place
    if not in_place:
        assert torch.equal(x.cpu(), torch.from_numpy(mask.astype(np.uint8)))       # the input is left alone
    return skel.cpu().numpy(), rec.cpu().tolist()


def test_record_early_stop_in_place_and_repeat():
    from nerf_for_angiography_amd import _lib
    mask = sk.smooth_noise((17, 18, 19), 3)
    want, rec = sk.skeletonize(mask)
    need = rec["passes"]
    assert need >= 5
    full = sk.record_list(rec, mask.sum())
    for sync in (0, 1, 3, need, need + 5):                                         # more passes than needed change nothing
        s, r = _record(mask, need + 5, sync)
        assert r == full and np.array_equal(s, want.astype(np.uint8)), (sync, r, full)
    s, r = _record(mask, need, 0)                                                  # exactly enough: the last pass finds nothing
    assert r == full and np.array_equal(s, want.astype(np.uint8))
    for k in (1, 2, need - 1):
        part, prec = sk.skeletonize(mask, max_passes=k)
        assert prec["converged"] == 0
        for sync in (0, 2):
            s, r = _record(mask, k, sync)
            assert r == sk.record_list(prec, mask.sum()) and np.array_equal(s, part.astype(np.uint8)), (k, sync, r)
        assert b"max_passes" in _lib.load().afx_last_error()                       # the synchronised form says that it stopped early
    s1, r1 = _record(mask, need + 2, 4, in_place=True)
    s2, r2 = _record(mask, need + 2, 0, in_place=True)
    assert r1 == r2 == full and np.array_equal(s1, s2) and np.array_equal(s1, want.astype(np.uint8))
    got, grec = _gpu(mask, max_passes=2)
    assert grec["converged"] == 0 and grec["passes"] == 2 and np.array_equal(got, sk.skeletonize(mask, max_passes=2)[0])


def test_input_handling():
    from nerf_for_angiography_amd.engine import skeletonize_3d
    from nerf_for_angiography_amd._lib import AfxError
    rng = np.random.default_rng(5)
    x = rng.random((9, 6, 11)) * (rng.random((9, 6, 11)) < 0.6)
    want = sk.skeletonize(x != 0)[0]
    for t in (torch.from_numpy(x != 0), torch.from_numpy(x.astype(np.float32)), torch.from_numpy(x), torch.from_numpy(np.ceil(x * 100).astype(np.int64))):
        got = skeletonize_3d(t.to(DEV))
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)
    view = torch.from_numpy(x).to(DEV).permute(2, 0, 1)                            # not contiguous
    assert not view.is_contiguous()
    assert np.array_equal(skeletonize_3d(view).cpu().numpy(), sk.skeletonize(x.transpose(2, 0, 1) != 0)[0])
    with pytest.raises(ValueError):
        skeletonize_3d(torch.ones(4, 4, device=DEV))
    with pytest.raises(AfxError):
        skeletonize_3d(torch.ones(1025, 1, 2, device=DEV))
    with pytest.raises(AfxError):
        skeletonize_3d(torch.ones(4, 4, 4, device=DEV), max_passes=0)


def test_fixed_pass_form_replays_from_a_graph():
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.engine import skeleton_record
    shape = (17, 18, 19)
    a = torch.from_numpy(sk.smooth_noise(shape, 3).astype(np.uint8)).to(DEV)
    b = torch.from_numpy((np.random.default_rng(9).random(shape) < 0.5).astype(np.uint8)).to(DEV)
    passes = 12
    eager = {}
    for name, x in (("a", a), ("b", b)):
        eager[name] = skeleton_record(x, passes, 0)
        want, rec = sk.skeletonize(x.cpu().numpy())
        assert rec["passes"] <= passes and np.array_equal(eager[name][0].cpu().numpy(), want.astype(np.uint8))
    static_x = a.clone()
    ws = torch.empty(int(_lib.load().afx_skeletonize_3d_workspace_bytes(*shape)), dtype=torch.uint8, device=DEV)
    skel = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    rec = torch.zeros(8, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            skeleton_record(static_x, passes, 0, skel=skel, record=rec, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    for name, x in (("b", b), ("a", a)):
        static_x.copy_(x)
        for t in (skel, rec, ws):
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(skel, eager[name][0]) and torch.equal(rec, eager[name][1]), name


def _host_centreline(pred, gt, thr, voxel, largest):
    vp, vl = pred >= np.float32(thr), gt >= np.float32(thr)
    body = vp
    if largest:
        lab, k = ndimage.label(vp, structure=sk.S26)
        body = lab == 1 + int(np.argmax(np.bincount(lab.ravel())[1:]))             # argmax: the first of equal sizes, as the filter
    sp, rec_p = sk.skeletonize(body)
    sl, rec_l = sk.skeletonize(vl)
    cl, tprec, tsens, _, _ = sk.cldice(vp, vl, sp, sl)
    return {"cldice": cl, "tprec": tprec, "tsens": tsens, "n_skeleton": int(sp.sum()), "n_skeleton_gt": int(sl.sum()),
            "n_end_points": int(sk.end_points(sp).sum()), "n_end_points_gt": int(sk.end_points(sl).sum()),
            "mean_radius": float(ndimage.distance_transform_edt(body)[sp].sum()) / int(sp.sum()) * voxel,
            "mean_radius_gt": float(ndimage.distance_transform_edt(vl)[sl].sum()) / int(sl.sum()) * voxel,
            "n_pred": int(vp.sum()), "n_gt": int(vl.sum()), "passes": rec_p["passes"], "passes_gt": rec_l["passes"], "voxel_size": voxel,
            "threshold": thr}, sp, sl


def _same_scores(got, want):
    assert got.keys() == want.keys()
    for key in want:
        if key in ("mean_radius", "mean_radius_gt"):       # an fp64 mean of bit-exact distances: only the order of the sum differs
            assert abs(got[key] - want[key]) <= 1e-9 * want[key], (key, got[key], want[key])
        else:                                              # the counts, and the three scores from the same formula
            assert got[key] == want[key], (key, got[key], want[key])


def test_sweep_centreline_scores_and_columns(golden):
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from nerf_for_angiography_amd.visualization.sweep import (CENTRELINE_METRICS, TOPOLOGY_METRICS, evaluation_sweep,
                                                              reconstruction_centreline_metrics)
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    n = 25
    voxel = 2.0 * 100.0 / (n - 1)
    scores, pred, ref, sp, sl = reconstruction_centreline_metrics(m, vol, 100.0, n)
    assert pred.shape == ref.shape == sp.shape == sl.shape == (n, n, n) and sp.dtype == sl.dtype == torch.bool
    thr = float(torch.mean(ref))
    want, want_sp, want_sl = _host_centreline(pred.cpu().numpy(), ref.cpu().numpy(), thr, voxel, False)
    print(f"centreline: got {scores}\n want {want}")
    _same_scores(scores, want)
    assert np.array_equal(sp.cpu().numpy(), want_sp) and np.array_equal(sl.cpu().numpy(), want_sl)
    assert 0.0 <= scores["cldice"] <= 1.0 and scores["n_skeleton"] > 0 and scores["mean_radius_gt"] > 0.0
    only, _, _, sp1, _ = reconstruction_centreline_metrics(m, vol, 100.0, n, threshold=thr * 0.5, largest_component=True)
    want1, want_sp1, _ = _host_centreline(pred.cpu().numpy(), ref.cpu().numpy(), thr * 0.5, voxel, True)
    _same_scores(only, want1)
    assert np.array_equal(sp1.cpu().numpy(), want_sp1) and sk.components26(want_sp1) == 1
    with pytest.raises(ValueError, match="pred or gt"):
        reconstruction_centreline_metrics(m, vol, 100.0, n, threshold=1e30)
    df, _ = evaluation_sweep(m, gt, angles, *geo, metrics=["TSENS 3D", "PSNR", "CLDICE 3D", "COMPONENTS 3D", "TPREC 3D", "HD 3D"], volume=vol,
                             volume_outside=100.0, volume_points=n)
    assert list(df.columns) == BASE + ["PSNR", "HD 3D", "COMPONENTS 3D"] + list(CENTRELINE_METRICS)
    assert list(df.columns).index(TOPOLOGY_METRICS[0]) < list(df.columns).index(CENTRELINE_METRICS[0])
    for col, key in zip(CENTRELINE_METRICS, ("cldice", "tprec", "tsens")):
        assert df[col].nunique() == 1 and df[col][0] == scores[key], col                       # one value per column, repeated on every row
