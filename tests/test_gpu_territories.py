"""The territories on the GPU (include/afx.h: afx_feature_transform_3d, afx_label_overlap_3d): the device against the NumPy restatement
tests/territory_reference.py bit for bit - the feature transform on shapes that cross the 64-lane chunks, leave tiles of lines partly
empty and take the narrower tile, on empty, full, corner and random site sets and on explicit ties; the overlap counts at ragged sizes;
both eagerly, twice and replayed from a captured graph - then the sweep family, its columns and the driver's --save_branches."""
import csv
import itertools

import numpy as np
import pytest
import torch

import territory_reference as tr
from nerf_for_angiography_amd import engine as eng

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(1, 1, 1), (1, 1, 70), (1, 1, 129), (5, 1, 3), (7, 9, 11), (3, 40, 5), (2, 3, 33), (3, 5, 17), (520, 2, 3), (2, 520, 3)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _check_ft(sites, what):
    """feature_transform_3d of a bool array equals the brute-force restatement exactly; -> (d2, nearest) on the device."""
    want_d2, want_near = tr.feature_transform(sites)
    d2, near = eng.feature_transform_3d(_dev(sites))
    assert d2.dtype == torch.int64 and near.dtype == torch.int64 and tuple(d2.shape) == sites.shape == tuple(near.shape)
    if not torch.equal(d2.cpu(), torch.from_numpy(want_d2)):
        bad = np.argwhere(d2.cpu().numpy() != want_d2)
        raise AssertionError(f"d2, {what}: {len(bad)} voxels differ, first {bad[0].tolist()}: {d2.cpu().numpy()[tuple(bad[0])]} != {want_d2[tuple(bad[0])]}")
    if not torch.equal(near.cpu(), torch.from_numpy(want_near)):
        bad = np.argwhere(near.cpu().numpy() != want_near)
        raise AssertionError(f"nearest, {what}: {len(bad)} voxels differ, first {bad[0].tolist()}: {near.cpu().numpy()[tuple(bad[0])]} != "
                             f"{want_near[tuple(bad[0])]}")
    return d2, near


def _site_sets(shape):
    rng = np.random.RandomState(shape[0] * 7919 + shape[1] * 131 + shape[2])
    yield "none", np.zeros(shape, bool)
    yield "all", np.ones(shape, bool)
    for corner in sorted(set(itertools.product(*[(0, s - 1) for s in shape]))):
        s = np.zeros(shape, bool)
        s[corner] = True
        yield f"corner {corner}", s
    yield "5 %", rng.rand(*shape) < 0.05
    yield "50 %", rng.rand(*shape) < 0.5


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_feature_transform_equals_the_brute_force(shape):
    for name, sites in _site_sets(shape):
        d2, near = _check_ft(sites, name)
        # independent of the restatement: the EDT of the inverted mask, the named site is a site, at that distance, and a site names itself
        s = _dev(sites)
        edt2 = eng.distance_transform_edt_3d(~s, return_squared=True)[1]
        assert torch.equal(d2, edt2), name
        if sites.any():
            flat = near.reshape(-1)
            assert bool(s.reshape(-1)[flat].all()), name
            n0, n1, n2 = shape
            lin = torch.arange(s.numel(), device=DEV)
            dd = (lin // (n1 * n2) - flat // (n1 * n2)) ** 2 + (lin // n2 % n1 - flat // n2 % n1) ** 2 + (lin % n2 - flat % n2) ** 2
            assert torch.equal(dd, d2.reshape(-1)), name
            assert torch.equal(flat[s.reshape(-1)], lin[s.reshape(-1)]), name
        else:
            assert bool((d2 == 0xffffffff).all()) and bool((near == -1).all())


def _tie(shape, centre, sites):
    s = np.zeros(shape, bool)
    for p in sites:
        s[p] = True
    d2, near = _check_ft(s, f"tie {sites}")
    return int(d2[centre]), int(near[centre]), lambda p: int(np.ravel_multi_index(p, shape))


def test_explicit_ties_go_to_the_lowest_linear_index():
    shape, c = (7, 9, 11), (3, 4, 5)
    d2, near, lin = _tie(shape, c, [(1, 4, 5), (5, 4, 5)])                           # mirrored along axis 0
    assert (d2, near) == (4, lin((1, 4, 5))) == (4, 148)
    d2, near, lin = _tie(shape, c, [(3, 1, 5), (3, 7, 5)])                           # along axis 1
    assert (d2, near) == (9, lin((3, 1, 5))) == (9, 313)
    d2, near, lin = _tie(shape, c, [(3, 4, 2), (3, 4, 8)])                           # along axis 2
    assert (d2, near) == (9, lin((3, 4, 2))) == (9, 343)
    for axes in ((0, 1), (0, 2), (1, 2)):                                           # the four corners of a square around the voxel
        square = []
        for sa, sb in itertools.product((-2, 2), repeat=2):
            p = list(c)
            p[axes[0]] += sa
            p[axes[1]] += sb
            square.append(tuple(p))
        d2, near, lin = _tie(shape, c, square)
        assert (d2, near) == (8, min(lin(p) for p in square)) == (8, lin(square[0]))
    cube = [tuple(np.add(c, o)) for o in itertools.product((-2, 2), repeat=3)]      # the eight corners of a cube
    d2, near, lin = _tie(shape, c, cube)
    assert (d2, near) == (12, lin((1, 2, 3))) == (12, 124)
    # a site straight along the axis at distance d ties with an earlier find at (d - k, ...): where a greater-or-equal break stops too early
    d2, near, lin = _tie(shape, c, [(0, 4, 5), (3, 4, 2), (3, 4, 8), (3, 1, 5), (3, 7, 5)])
    assert (d2, near) == (9, lin((0, 4, 5))) == (9, 49)
    d2, near, lin = _tie((2, 520, 3), (1, 260, 1), [(1, 0, 1), (1, 519, 1), (1, 1, 1)])      # the narrower tile: 260 against 259
    assert (d2, near) == (259 ** 2, lin((1, 1, 1)))
    d2, near, lin = _tie((520, 2, 3), (260, 1, 1), [(0, 1, 1), (519, 1, 1), (1, 1, 1)])
    assert (d2, near) == (259 ** 2, lin((1, 1, 1))) == (67081, 10)


def _overlap_case(n, n_labels, seed, with_index=True, with_d2=True, with_b=True):
    rng = np.random.RandomState(seed)
    labels = rng.randint(-2, n_labels + 3, n).astype(np.int32)                      # negative and too large labels go to row 0
    index = rng.randint(-3, n, n).astype(np.int32) if with_index else None          # negative entries: row 0
    max_d2 = 9
    d2 = rng.choice([0, 1, 8, 9, 10, 400, tr.NONE], n).astype(np.int64) if with_d2 else None      # exactly at, one below, one above max_d2
    a = (rng.rand(n) < 0.6).astype(np.uint8)
    b = (rng.rand(n) < 0.4).astype(np.uint8) if with_b else None
    return labels, a, b, index, d2, max_d2 if with_d2 else None


def _check_overlap(labels, a, b, index, d2, max_d2, n_labels, what):
    want_counts, want_terr = tr.label_overlap(labels, a, b, index, d2, max_d2, n_labels)
    opt = lambda x: None if x is None else _dev(x)
    counts, terr = eng.label_overlap_3d(_dev(labels), _dev(a), opt(b), opt(index), opt(d2), max_d2, n_labels, return_territory=True)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (n_labels + 1, 4) and terr.dtype == torch.int32
    assert torch.equal(counts.cpu(), torch.from_numpy(want_counts)), (what, counts.cpu().tolist()[:8], want_counts.tolist()[:8])
    assert torch.equal(terr.cpu(), torch.from_numpy(want_terr)), what
    n = labels.size
    totals = [n, int((a != 0).sum()), 0 if b is None else int((b != 0).sum()), 0 if b is None else int(((a != 0) & (b != 0)).sum())]
    assert counts.sum(dim=0).cpu().tolist() == totals, what                          # every column sums to its total
    return counts


@pytest.mark.parametrize("n_labels", [1, 3, 300])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_overlap_counts_equal_the_restatement(n, n_labels):
    seed = n * 1000 + n_labels
    _check_overlap(*_overlap_case(n, n_labels, seed), n_labels, "index, d2, b")
    _check_overlap(*_overlap_case(n, n_labels, seed + 1, with_b=False), n_labels, "b = None")
    _check_overlap(*_overlap_case(n, n_labels, seed + 2, with_index=False, with_d2=False), n_labels, "labels alone")
    labels, a, b, _, _, _ = _overlap_case(n, n_labels, seed + 3)
    one = np.full(n, n_labels, np.int32)                                             # every voxel in one label
    counts = _check_overlap(one, a, b, None, None, None, n_labels, "one label")
    assert int(counts[n_labels, 0]) == n and int(counts[:n_labels].sum()) == 0


def test_overlap_cut_is_inclusive_and_counts_are_zeroed_by_the_call():
    labels = np.array([1, 1, 1, 2], np.int32)
    d2 = np.array([8, 9, 10, 9], np.int64)
    a = np.ones(4, np.uint8)
    counts, terr = eng.label_overlap_3d(_dev(labels), _dev(a), d2=_dev(d2), max_d2=9, n_labels=2, return_territory=True)
    assert terr.cpu().tolist() == [1, 1, 0, 2] and counts.cpu().tolist() == [[1, 1, 0, 0], [2, 2, 0, 0], [1, 1, 0, 0]]
    # the record variant into buffers full of garbage
    lab, au = _dev(labels), _dev(a)
    buf = torch.full((3, 4), -0x0123456789abcdef, dtype=torch.int64, device=DEV)
    terr = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    eng.label_overlap_record(lab, au, 2, counts=buf, territory=terr)
    assert buf.cpu().tolist() == [[0, 0, 0, 0], [3, 3, 0, 0], [1, 1, 0, 0]] and terr.cpu().tolist() == [1, 1, 1, 2]
    with pytest.raises(eng.AfxError, match="n_labels"):
        eng.label_overlap_record(lab, au, 4096)
    with pytest.raises(eng.AfxError, match="1..1024"):
        eng.feature_transform_record(torch.zeros((1, 1, 1025), dtype=torch.uint8, device=DEV))


def test_two_runs_and_a_graph_replay_are_equal():
    """Both _record entry points into caller buffers: a second run and a replay of the captured launches give the eager result."""
    rng = np.random.RandomState(11)
    shape = (9, 20, 70)
    sites_np = rng.rand(*shape) < 0.03
    site_labels = np.where(sites_np, rng.randint(1, 6, shape), 0).astype(np.int32)
    a_np, b_np = rng.rand(*shape) < 0.5, rng.rand(*shape) < 0.5
    sites, labels, a, b = _dev(sites_np, torch.uint8), _dev(site_labels), _dev(a_np, torch.uint8), _dev(b_np, torch.uint8)
    d2 = torch.empty(shape, dtype=torch.int32, device=DEV)
    near, terr = torch.empty_like(d2), torch.empty_like(d2)
    counts = torch.empty((6, 4), dtype=torch.int64, device=DEV)

    def run():
        eng.feature_transform_record(sites, d2, near)
        eng.label_overlap_record(labels, a, 5, b, near, d2, 30, counts, terr)

    def scrub():
        for t in (d2, near, terr, counts):
            t.fill_(-5)

    want_d2, want_near = tr.feature_transform(sites_np)
    want_counts, want_terr = tr.label_overlap(site_labels, a_np, b_np, want_near, want_d2, 30, 5)

    def check(what):
        assert torch.equal(d2.cpu().to(torch.int64) & 0xffffffff, torch.from_numpy(want_d2)), what
        assert torch.equal(near.cpu().to(torch.int64), torch.from_numpy(want_near)), what
        assert torch.equal(counts.cpu(), torch.from_numpy(want_counts)) and torch.equal(terr.cpu(), torch.from_numpy(want_terr)), what

    for what in ("first call", "second call"):
        scrub()
        run()
        check(what)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run()
    torch.cuda.current_stream().wait_stream(side)
    scrub()
    graph.replay()
    torch.cuda.synchronize()
    check("graph replay")


# ---- the sweep family on the three hand-built scenes ----
@pytest.fixture(scope="module")
def truth():
    from nerf_for_angiography_amd.visualization.sweep import grid_index_to_world
    a = grid_index_to_world(tr.OUTSIDE, tr.N)
    mask = tr.y_truth()
    return mask, tr.tree(mask, a), a


def _scene(truth, name):
    mask, tree, a = truth
    if name == "same":
        return mask
    if name == "dilated":
        return tr.dilated(mask)
    return tr.without_branch(mask, tree, int(name[-1]))


@pytest.mark.parametrize("name", ["same", "without 1", "without 2", "without 3", "dilated"])
def test_branch_metrics_equal_the_restatements_table(truth, name):
    from nerf_for_angiography_amd.visualization import sweep
    mask, tree, a = truth
    pred = _scene(truth, name)
    want, table, want_terr = tr.branch_table(pred, mask, tr.tree(pred, a), tree)
    an = sweep.GridAnalysis(_dev(pred, torch.float32), _dev(mask, torch.float32), tr.OUTSIDE, tr.N)
    scores, rows, terr = sweep.reconstruction_branch_metrics(None, None, tr.OUTSIDE, tr.N, threshold=0.5, grids=an)
    print(name, scores)
    for key, value in want.items():                                                 # integers, and fp64 from the same operations in the same order
        assert scores[key] == value or (value != value and scores[key] != scores[key]), (key, scores[key], value)
    for key, col in table.items():
        assert np.array_equal(np.asarray(rows[key], np.float64), np.asarray(col, np.float64), equal_nan=True), (key, rows[key], col)
    got_terr = eng.territory_overlap(terr, _dev(pred) | _dev(mask), return_territory=True)[1]
    assert torch.equal(got_terr.cpu(), torch.from_numpy(want_terr))
    assert scores["threshold"] == 0.5 and scores["voxel_size"] == 1.0 and scores["n_branches"] == 3
    if name == "same":
        assert scores["branch_recall"] == 1.0 and scores["worst_branch_dice"] == 1.0 and scores["branch_radius_err"] == 0.0
        assert scores["unassigned"] == 0.0 and (rows["offset"] == 0.0).all()
    elif name == "dilated":
        assert scores["branch_recall"] == 1.0 and (rows["radius_pred"][:3] > rows["radius_true"][:3]).all()
    else:
        k = int(name[-1]) - 1
        assert scores["branch_recall"] == 2.0 / 3.0 and scores["worst_branch_dice"] == 0.0 and rows["dice"][k] == 0.0 and not rows["found"][k]
    again = sweep.reconstruction_branch_metrics(None, None, tr.OUTSIDE, tr.N, threshold=0.5, grids=an, max_distance=1.0)[0]
    assert again["unassigned"] > 0.0                                                  # tubes of radius 2.2: voxels beyond one voxel belong to nobody


def test_sweep_tabulates_the_branch_columns(golden):
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from nerf_for_angiography_amd.visualization import sweep
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    n = 25
    with pytest.raises(ValueError, match="ground-truth volume"):
        sweep.evaluation_sweep(m, gt, angles, *geo, metrics=["PSNR"] + list(sweep.BRANCH_METRICS), volume_outside=100.0, volume_points=n)
    ref = sweep.reconstruction_branch_metrics(m, vol, 100.0, n)[0]
    print(ref)
    assert ref["n_branches"] >= 1 and 0.0 <= ref["branch_recall"] <= 1.0
    df, _ = sweep.evaluation_sweep(m, gt, angles, *geo, metrics=["BRANCH RADIUS ERR 3D", "PSNR", "BRANCH RECALL 3D", "BRANCHES 3D", "WORST BRANCH DICE 3D"],
                                   volume=vol, volume_outside=100.0, volume_points=n)
    assert list(df.columns) == BASE + ["PSNR", "BRANCHES 3D"] + list(sweep.BRANCH_METRICS)
    for col, key in zip(sweep.BRANCH_METRICS, ("branch_recall", "worst_branch_dice", "branch_radius_err")):
        v = df[col].to_numpy()
        assert len(v) == len(angles) and ((v == ref[key]).all() or (np.isnan(v).all() and ref[key] != ref[key])), col


def test_save_branches_writes_a_row_per_branch_and_junction(truth, tmp_path):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import BRANCH_CSV_COLUMNS, save_branches
    mask, tree, a = truth
    grid = _dev(mask, torch.float32)
    info = save_branches(None, tr.OUTSIDE, tr.N, 0.5, str(tmp_path / "branches.csv"), grid=grid)
    rec = tree["graph"]["record"]
    rows = list(csv.reader(open(info["path"])))
    assert tuple(rows[0]) == BRANCH_CSV_COLUMNS and len(rows) == 1 + rec["branches"] + rec["nodes"] == 1 + info["n_rows"]
    col = {name: i for i, name in enumerate(rows[0])}
    labels, nb, nk = tr.site_labels(tree["graph"])
    want = tr.label_overlap(labels, mask, None, tr.feature_transform(labels > 0)[1], None, None, nb + nk)[0]
    for l, r in enumerate(rows[1:], start=1):
        assert int(r[col["label"]]) == l and r[col["kind"]] == ("branch" if l <= nb else "junction")
        assert int(r[col["territory_voxels"]]) == want[l, 1] and float(r[col["territory_volume"]]) == float(want[l, 1])      # a grid step of 1
        assert int(r[col["centreline_voxels"]]) == int((labels == l).sum())
        assert float(r[col["r_min"]]) <= float(r[col["r_mean"]]) <= float(r[col["r_max"]])
        if l <= nb:
            b = tree["graph"]["branches"][l - 1]
            assert float(r[col["length"]]) == b["length"] and (int(r[col["node_start"]]), int(r[col["node_end"]])) == (b["node_start"], b["node_end"])
    assert info["n_voxels"] == int(mask.sum()) == info["n_assigned"]
    with pytest.raises(ValueError, match="--save_branches"):
        save_branches(None, tr.OUTSIDE, tr.N, 0.5, str(tmp_path / "branches.txt"), grid=grid)
