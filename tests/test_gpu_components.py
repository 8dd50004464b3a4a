"""3-D connected-component labelling on the GPU (afx_label_components_3d, afx_filter_components_3d; engine.label_components_3d /
filter_components_3d / components_record, visualization/sweep.py) against scipy.ndimage.label (tests/components_reference.py).  Labelling
has one canonical answer - components numbered in raster order of their first voxel - so labels, K, sizes and the record must EQUAL the
reference: there are no tolerances, and a second run must give the same bits."""
import numpy as np
import pytest
import torch

import components_reference as cr
import surface_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# fewer voxels than a workgroup, sizes that are no multiple of a wave, of the merge's 256-voxel workgroups or of the 2048-voxel chunks of
# the other kernels, single lines along each axis, more than one workgroup and chunk along each axis
SHAPES = [(5, 7, 3), (1, 1, 40), (1, 40, 1), (40, 1, 1), (33, 17, 65), (2, 300, 3), (300, 2, 3), (3, 2, 300), (64, 64, 64), (1024, 1, 3),
          (65, 64, 63)]
# the site-percolation thresholds of the cubic lattice with 26, 18 and 6 neighbours (about 0.10, 0.14, 0.31) are among them: there the
# components are large, tangled and cross every workgroup boundary
DENSITIES = (0.05, 0.1, 0.14, 0.2, 0.31, 0.5, 0.9)


def _run(mask, c):
    from nerf_for_angiography_amd.engine import components_record
    x = torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(DEV)
    labels, sizes, rec = components_record(x, c)
    assert labels.dtype == torch.int32 and labels.shape == x.shape and sizes.numel() == x.numel() and rec.shape == (8,)
    return labels.cpu().numpy(), sizes.cpu().numpy().view(np.uint32).astype(np.int64), rec.cpu().numpy()


def _check(mask, c, what=""):
    """Labels, sizes and record of the device against the reference; the same bits on a second run.  -> (reference labels, K)."""
    want, k = cr.label(mask, c)
    labels, sizes, rec = _run(mask, c)
    assert rec.tolist() == cr.record(want, k), (what, c, rec.tolist(), cr.record(want, k))
    assert np.array_equal(labels, want), (what, c, int((labels != want).sum()))
    assert np.array_equal(sizes[:k], cr.sizes(want)) and not sizes[k:].any(), (what, c)
    labels2, sizes2, rec2 = _run(mask, c)
    assert np.array_equal(labels2, labels) and np.array_equal(sizes2, sizes) and np.array_equal(rec2, rec), (what, c)
    return want, k


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_volumes_equal_scipy(shape):
    rng = np.random.default_rng(shape[0] * 7919 + shape[1] * 31 + shape[2])
    masks = [(f"p = {p}", rng.random(shape) < p) for p in DENSITIES]
    masks += [("all zero", np.zeros(shape, bool)), ("all one", np.ones(shape, bool))]
    for what, mask in masks:
        for c in (1, 2, 3):
            _check(mask, c, what)


def _serpentine(n=40):
    """A one-voxel-wide path through an n x n x 3 volume, as (mask, path): a snake over the plane k = 0 (every second row, joined at
    alternating ends), one voxel through k = 1, and the snake back over the plane k = 2."""
    plane = []
    for r, i in enumerate(range(0, n, 2)):
        row = [(i, j) for j in range(n)]
        row = row if r % 2 == 0 else row[::-1]
        plane += row
        if i + 2 < n:
            plane.append((i + 1, row[-1][1]))
    path = [(i, j, 0) for i, j in plane] + [(*plane[-1], 1)] + [(i, j, 2) for i, j in plane[::-1]]
    mask = np.zeros((n, n, 3), bool)
    for p in path:
        mask[p] = True
    assert mask.sum() == len(path) == 2 * (n // 2 * n + n // 2 - 1) + 1
    return mask, path


def test_long_chains():
    mask, path = _serpentine()
    broken = mask.copy()
    for p in path[96::97]:                             # every 97th voxel of the path removed
        broken[p] = False
    for m, what in ((mask, "serpentine"), (broken, "broken serpentine")):
        for view, name in ((m, ""), (m.transpose(2, 0, 1), " with the runs along axis 2"), (m.transpose(1, 2, 0), " with the runs along axis 0")):
            for c in (1, 2, 3):
                want, k = _check(view, c, what + name)
                if m is mask:
                    assert k == 1, (name, c, k)
                elif c == 1:                           # (with diagonal neighbours a gap at a turn of the path does not part it)
                    assert k == len(path) // 97 + 1, (name, k)


def test_pairs_across_a_workgroup_boundary_and_the_checkerboard():
    """The pairs lie on both sides of linear index 2048 of a 3 x 40 x 64 volume: the end of a 2048-voxel chunk and of a 256-voxel
    workgroup of the merge."""
    shape = (3, 40, 64)
    edge = cr.edge_pair(shape, at=(0, 31, 40))         # linear indices 2024 and 2089
    corner = cr.corner_pair(shape, at=(0, 5, 5))       # 325 and 2950
    for m in (edge, corner):
        idx = np.flatnonzero(m.ravel())
        assert len(idx) == 2 and idx[0] < 2048 <= idx[1]
    assert [_check(edge, c, "edge pair")[1] for c in (1, 2, 3)] == [2, 1, 1]
    assert [_check(corner, c, "corner pair")[1] for c in (1, 2, 3)] == [2, 2, 1]
    assert [_check(cr.edge_pair(), c)[1] for c in (1, 2, 3)] == [2, 1, 1]
    assert [_check(cr.corner_pair(), c)[1] for c in (1, 2, 3)] == [2, 2, 1]
    assert [_check(cr.checkerboard(), c, "checkerboard")[1] for c in (1, 2, 3)] == [168, 1, 1]


def _phantom_with_floaters():
    """tube_and_ball in the corner of a 40 x 36 x 44 volume with three floaters: a single voxel, a 2 x 2 x 2 cube and a copy of the ball."""
    shape = (24, 20, 28)
    body = sr.tube_and_ball(shape) >= 0.5
    idx = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), -1)
    ball = body & (np.sqrt(((idx - 0.8 * np.asarray(shape)) ** 2).sum(-1)) <= 4.8)
    m = np.zeros((40, 36, 44), bool)
    m[:24, :20, :28] = body
    m[2, 30, 40] = True                                # the single voxel: first in raster order
    m[30:32, 3:5, 5:7] = True                          # the cube
    ball_only = np.zeros_like(m)
    for i, j, k in np.argwhere(ball):
        m[i + 14, j + 16, k + 16] = ball_only[i + 14, j + 16, k + 16] = True
    ball_only[:24, :20, :28] |= ball
    return m, ball_only, int(ball.sum())


def test_sizes_record_and_the_tie():
    m, two_balls, n_ball = _phantom_with_floaters()
    for c in (1, 2, 3):
        want, k = _check(m, c, "phantom with floaters")
        assert k == 4 and sorted(cr.sizes(want).tolist())[:3] == [1, 8, n_ball]
        assert cr.largest(want)[0] == want[:24, :20, :28].max() and cr.largest(want)[1] > n_ball
        want, k = _check(two_balls, c, "two equal balls")
        assert k == 2 and cr.sizes(want).tolist() == [n_ball, n_ball] and cr.record(want, k)[2:4] == [n_ball, 1]      # the smaller label wins
        flipped = two_balls[::-1, ::-1, ::-1]          # the other ball comes first now
        want, k = _check(flipped, c, "two equal balls, reversed")
        assert cr.record(want, k)[2:4] == [n_ball, 1]


def test_filter_keeps_the_largest_and_drops_the_specks():
    from nerf_for_angiography_amd.engine import filter_components_3d
    m, two_balls, n_ball = _phantom_with_floaters()
    x = torch.from_numpy(m).to(DEV)
    for c in (1, 3):
        want, k = cr.label(m, c)
        sizes = cr.sizes(want)
        big, _, _ = cr.largest(want)
        got = filter_components_3d(x, c, largest_only=True)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want == big)
        got8 = filter_components_3d(x, c, min_size=8).cpu().numpy()
        assert np.array_equal(got8, (want != 0) & (sizes[np.maximum(want, 1) - 1] >= 8))
        assert not got8[2, 30, 40] and got8[30:32, 3:5, 5:7].all() and got8.sum() == m.sum() - 1
        got9 = filter_components_3d(x, c, min_size=9).cpu().numpy()
        assert np.array_equal(got9, (want != 0) & (sizes[np.maximum(want, 1) - 1] >= 9)) and not got9[30:32, 3:5, 5:7].any()
        assert np.array_equal(filter_components_3d(x, c).cpu().numpy(), m)                     # min_size = 1 keeps everything
        both = filter_components_3d(x, c, largest_only=True, min_size=int(sizes.max()) + 1)
        assert not both.any()
        tie = filter_components_3d(torch.from_numpy(two_balls).to(DEV), c, largest_only=True).cpu().numpy()
        assert np.array_equal(tie, cr.label(two_balls, c)[0] == 1)
    empty = torch.zeros(7, 9, 11, device=DEV)
    for kw in (dict(), dict(largest_only=True), dict(min_size=5)):
        out = filter_components_3d(empty, 2, **kw)
        assert out.shape == empty.shape and out.dtype == torch.bool and not out.any()


def test_input_handling():
    from nerf_for_angiography_amd.engine import label_components_3d
    from nerf_for_angiography_amd._lib import AfxError
    rng = np.random.default_rng(5)
    x = rng.random((9, 6, 11)) * (rng.random((9, 6, 11)) < 0.3)
    want, k = cr.label(x, 2)
    for t in (torch.from_numpy(x != 0), torch.from_numpy(x.astype(np.float32)), torch.from_numpy(x), torch.from_numpy(np.ceil(x * 100).astype(np.int64))):
        labels, got_k, sizes = label_components_3d(t.to(DEV), 2, return_sizes=True)
        assert labels.dtype == torch.int32 and sizes.dtype == torch.int64 and got_k == k
        assert np.array_equal(labels.cpu().numpy(), want) and np.array_equal(sizes.cpu().numpy(), cr.sizes(want))
    labels, got_k = label_components_3d(torch.from_numpy(x).to(DEV))                           # connectivity 1, no sizes
    assert got_k == cr.label(x, 1)[1] and np.array_equal(labels.cpu().numpy(), cr.label(x, 1)[0])
    view = torch.from_numpy(x).to(DEV).permute(2, 0, 1)                                        # not contiguous
    assert not view.is_contiguous()
    labels, got_k = label_components_3d(view, 3)
    want_t, k_t = cr.label(x.transpose(2, 0, 1), 3)
    assert got_k == k_t and np.array_equal(labels.cpu().numpy(), want_t)
    with pytest.raises(ValueError):
        label_components_3d(torch.ones(4, 4, device=DEV))
    with pytest.raises(AfxError):
        label_components_3d(torch.ones(1025, 1, 2, device=DEV))
    with pytest.raises(AfxError):
        label_components_3d(torch.ones(4, 4, 4, device=DEV), connectivity=4)


def test_label_and_filter_replay_from_a_graph():
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.engine import components_filter, components_record
    shape = (33, 17, 65)
    rng = np.random.default_rng(9)
    a = torch.from_numpy((rng.random(shape) < 0.2).astype(np.uint8)).to(DEV)
    b = torch.from_numpy((rng.random(shape) < 0.1).astype(np.uint8)).to(DEV)
    eager = {}
    for name, x in (("a", a), ("b", b)):
        labels, sizes, rec = components_record(x, 3)
        eager[name] = (labels, sizes, rec, components_filter(labels, sizes, rec, largest_only=True, min_size=2))
        assert np.array_equal(labels.cpu().numpy(), cr.label(x.cpu().numpy(), 3)[0])
    static_x = a.clone()
    ws = torch.empty(int(_lib.load().afx_label_components_3d_workspace_bytes(*shape)), dtype=torch.uint8, device=DEV)
    labels = torch.zeros(shape, dtype=torch.int32, device=DEV)
    sizes = torch.zeros(a.numel(), dtype=torch.int32, device=DEV)
    rec = torch.zeros(8, dtype=torch.int64, device=DEV)
    out = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            components_record(static_x, 3, labels=labels, sizes=sizes, record=rec, workspace=ws)
            components_filter(labels, sizes, rec, largest_only=True, min_size=2, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for name, x in (("b", b), ("a", a)):
        static_x.copy_(x)
        for t in (labels, sizes, rec, out):
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((labels, sizes, rec, out), eager[name]):
            assert torch.equal(got, want), name


def _host_topology(pred, gt, thr, c):
    a, b = pred >= np.float32(thr), gt >= np.float32(thr)
    la, ka = cr.label(a, c)
    big, n_big, _ = cr.largest(la)
    lcc = la == big
    return {"n_components": ka, "n_components_gt": cr.label(b, c)[1], "n_pred": int(a.sum()), "n_gt": int(b.sum()), "n_largest": n_big,
            "lcc_fraction": n_big / int(a.sum()), "dice_lcc": 2.0 * int((lcc & b).sum()) / (n_big + int(b.sum())), "connectivity": c,
            "threshold": thr}, lcc


def test_sweep_topology_scores_and_columns(golden):
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from nerf_for_angiography_amd.visualization.sweep import (TOPOLOGY_METRICS, evaluation_sweep, reconstruction_surface_metrics,
                                                              reconstruction_topology_metrics)
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    scores, pred, ref, lcc = reconstruction_topology_metrics(m, vol, 100.0, 33)
    assert pred.shape == ref.shape == lcc.shape == (33, 33, 33) and lcc.dtype == torch.bool
    thr = float(torch.mean(ref))
    want, want_lcc = _host_topology(pred.cpu().numpy(), ref.cpu().numpy(), thr, 3)
    print(f"topology: got {scores}\n want {want}")
    assert scores == want                              # all counts and both ratios exactly
    assert np.array_equal(lcc.cpu().numpy(), want_lcc)
    for c in (1, 2):
        got_c, _, _, lcc_c = reconstruction_topology_metrics(m, vol, 100.0, 33, threshold=thr * 0.5, connectivity=c)
        want_c, want_lcc_c = _host_topology(pred.cpu().numpy(), ref.cpu().numpy(), thr * 0.5, c)
        assert got_c == want_c and np.array_equal(lcc_c.cpu().numpy(), want_lcc_c)
    with pytest.raises(ValueError, match="pred or gt"):
        reconstruction_topology_metrics(m, vol, 100.0, 33, threshold=1e30)
    df, _ = evaluation_sweep(m, gt, angles, *geo, metrics=["DICE 3D LCC", "PSNR", "COMPONENTS 3D", "HD 3D", "LCC FRACTION 3D"], volume=vol,
                             volume_outside=100.0, volume_points=33)
    assert list(df.columns) == BASE + ["PSNR", "HD 3D"] + list(TOPOLOGY_METRICS)
    for col, key in zip(TOPOLOGY_METRICS, ("n_components", "lcc_fraction", "dice_lcc")):
        assert df[col].nunique() == 1 and df[col][0] == scores[key], col                       # one value per column, repeated on every row
    # the surface scores of the largest component alone
    voxel = 2.0 * 100.0 / 32
    only, pred2, ref2 = reconstruction_surface_metrics(m, vol, 100.0, 33, largest_component=True)
    assert torch.equal(pred2, pred) and torch.equal(ref2, ref)
    host = sr.surface_metrics(want_lcc.astype(np.float32), ref.cpu().numpy(), 0.5, thr)
    for key in ("n_pred", "n_gt", "n_overlap", "n_surface_pred", "n_surface_gt", "dice_vessel"):
        assert only[key] == host[key], key
    assert only["n_pred"] == scores["n_largest"] and only["dice_vessel"] == scores["dice_lcc"]
    assert only["hd"] == host["hd"] * voxel and only["hd_percentile"] == host["hd_percentile"] * voxel
    assert abs(only["assd"] - host["assd"] * voxel) <= sr.assd_bound(host["n_surface_pred"], host["n_surface_gt"]) * host["assd"] * voxel
    # the default is what it was
    plain, _, _ = reconstruction_surface_metrics(m, vol, 100.0, 33)
    before = sr.surface_metrics(pred.cpu().numpy(), ref.cpu().numpy(), thr, thr)
    assert plain == reconstruction_surface_metrics(m, vol, 100.0, 33, largest_component=False, connectivity=1)[0]
    assert plain["n_pred"] == scores["n_pred"] == before["n_pred"] and plain["hd"] == before["hd"] * voxel
    assert plain["dice_vessel"] == before["dice_vessel"] and plain["hd_percentile"] == before["hd_percentile"] * voxel
