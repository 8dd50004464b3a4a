"""The view map on the GPU (afx_view_map, engine.view_map and optimal_views, sweep.reconstruction_view_metrics, the driver's
--save_view_map): every output equals the NumPy restatement tests/viewmap_reference.py exactly, with and without the cull, on a second
launch and on a replay from a captured graph (run with -m gpu on an MI355X)."""
import csv
import functools

import numpy as np
import pytest
import torch

import viewmap_reference as vr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_SEGMENTS = [1, 255, 256, 257, 600]                # the chunk of 256 segments and its two neighbours
DETECTORS = [(1, 1), (16, 16), (17, 33), (40, 23)]  # (W, H): one pixel, one whole tile, partial tiles in both axes
N_VIEWS = [1, 3, 70]
BRANCHES = ["1", "4", "N"]
CASES = sorted({(n, det, v, min(n, {"1": 1, "4": 4, "N": n}[b])) for n in N_SEGMENTS for det in DETECTORS for v in N_VIEWS for b in BRANCHES},
               key=lambda c: (c[0], c[1], c[2], c[3]))
RAW = ("count", "area", "shared", "tree", "proj", "length")


def _engine():
    from nerf_for_angiography_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _case(case):
    """(segments, seg_branch, records, W, H, the restatement's result), made once per case and left unchanged."""
    n, (width, height), n_views, nb = CASES[case]
    seg, br = vr.wavy_tree(n, nb, case)
    rec = _engine().hull_view_records(*vr.scene_views(n_views, width, height, case))
    return seg, br, rec, width, height, vr.view_map(seg, br, rec, width, height)


def _bits(x):
    """A result as integers: equal bits, not equal values (a NaN equals itself, -0 differs from +0)."""
    x = x.cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if x.dtype == torch.uint16:
        return x.view(torch.int16)
    return x.view(torch.int64) if x.dtype == torch.float64 else x


def _assert_same(got, want, what):
    for key in RAW:
        assert tuple(got[key].shape) == tuple(want[key].shape), (what, key)
        assert torch.equal(_bits(got[key]), _bits(want[key])), (what, key)


IDS = [f"N{n}-{d[0]}x{d[1]}-V{v}-B{b}" for n, d, v, b in CASES]


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_bytes_equal_the_restatement(case):
    """count, area, shared, tree, proj and length equal the restatement exactly, the culled launch and the brute one alike."""
    eng = _engine()
    seg, br, rec, width, height, want = _case(case)
    got = eng.view_map_record(seg, br, rec, width, height)
    assert got["count"].dtype == torch.uint16 and got["area"].dtype == torch.int32 and got["proj"].dtype == torch.float64
    _assert_same(got, want, "culled")
    _assert_same(eng.view_map_record(seg, br, rec, width, height, brute=True), want, "brute")


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_culling_on_and_off(case):
    """brute=True and the default give equal bytes; and so do the halves of the call taken alone."""
    eng = _engine()
    seg, br, rec, width, height, _ = _case(case)
    culled, brute = eng.view_map_record(seg, br, rec, width, height), eng.view_map_record(seg, br, rec, width, height, brute=True)
    _assert_same(culled, brute, "culled against brute")
    only_counts = eng.view_map_record(seg, br, rec, width, height, foreshortening=False)
    only_lengths = eng.view_map_record(seg, br, rec, width, height, counts=False)
    assert sorted(only_counts) == ["area", "count", "shared", "tree"] and sorted(only_lengths) == ["length", "proj"]
    for key, part in [(k, only_counts) for k in RAW[:4]] + [(k, only_lengths) for k in RAW[4:]]:
        assert torch.equal(_bits(part[key]), _bits(culled[key])), key


def test_the_cases_are_what_they_claim():
    """From the restatement's own numbers: a run of one branch straddles segment 256; the inside view sees some segments and not others;
    a branch covers no pixel somewhere; some view has shared pixels and another has none; the close view's capsules leave the detector
    over all four edges; one segment is degenerate and one has no radius; a tile's list skips a branch between two it keeps."""
    case = CASES.index((600, (40, 23), 3, 4))
    seg, br, rec, width, height, want = _case(case)
    assert br[255] == br[256] and len(set(br.tolist())) == 4
    assert np.array_equal(seg[1, 0:3], seg[1, 3:6]) and seg[2, 6] == 0.0 and seg[3, 6] > 0.0
    tree = want["tree"]
    assert 0 < tree[0, 2] < 600 and tree[1, 2] == 0                         # view 0: the source inside the tree
    assert (tree[:, 1] > 0).any() and (tree[:, 1] == 0).any() and (tree[:, 0] > 0).all()
    assert (want["area"] == 0).any() and (want["area"] > 0).any()
    assert ((want["shared"] > 0).any(axis=1) == (tree[:, 1] > 0)).all()
    u0, w0, d0 = vr.project(seg[:, 0:3], rec[1], width, height)
    assert (d0 > 0).all() and (u0 < 0).any() and (u0 > width - 1).any() and (w0 < 0).any() and (w0 > height - 1).any()
    # the face-on view 2: the four bands lie apart, so the tile of the top left corner is covered by branch 1 alone while the list goes on
    assert want["count"][2].max() == 1 and want["area"][2].min() > 0
    every = CASES.index((600, (40, 23), 3, 600))
    assert (_case(every)[5]["area"] == 0).any() and _case(every)[5]["tree"][0, 2] == 600      # every segment straddles the inside source


def test_repeatable_and_capturable():
    """A second launch and a replay from a captured graph give the same bytes; the replay follows the contents of the segment and view
    buffers, over outputs filled with sevens."""
    eng = _engine()
    width, height = 40, 23
    sets = []
    for case in (CASES.index((600, (40, 23), 70, 4)), CASES.index((600, (40, 23), 70, 600))):
        seg, br, rec, _, _, _ = _case(case)
        sets.append([torch.from_numpy(x).to(DEV) for x in (seg, br, rec)] + [int(br[-1])])
    # the captured call takes B as an argument: the second set is replayed as 4 branches of 150 segments
    sets[1][1], sets[1][3] = sets[0][1].clone(), 4
    eager = [eng.view_map_record(s, b, r, width, height, n_branches=nb) for s, b, r, nb in sets]
    again = eng.view_map_record(*sets[0][:3], width, height, n_branches=4)
    _assert_same(again, eager[0], "second launch")
    assert not torch.equal(_bits(eager[0]["count"]), _bits(eager[1]["count"]))
    static = [t.clone() for t in sets[0][:3]]
    out = {k: torch.zeros_like(_bits(v)).to(DEV).view(v.dtype) for k, v in eager[0].items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            eng.view_map_record(*static, width, height, n_branches=4, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 0):
        for dst, src in zip(static, sets[k][:3]):
            dst.copy_(src)
        for t in out.values():
            (t.view(torch.int16) if t.dtype == torch.uint16 else t).fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(out, eager[k], f"replay of set {k}")


def _raw_call(lib, **kw):
    import ctypes as C
    ptr = lambda t: None if t is None else (t if isinstance(t, C.c_void_p) else C.c_void_p(t.data_ptr()))
    rc = lib.afx_view_map(ptr(kw["segments"]), ptr(kw["seg_branch"]), kw["n"], kw["b"], ptr(kw["views"]), kw["v"], kw["w"], kw["h"], kw["flags"],
                          ptr(kw["count"]), ptr(kw["area"]), ptr(kw["shared"]), ptr(kw["tree"]), ptr(kw["proj"]), ptr(kw["length"]), None)
    return rc, (lib.afx_last_error() or b"").decode()


def test_entry_point_refuses_bad_arguments():
    """Null pointers, counts out of range, a non-positive detector and host pointers are refused before any launch, by name; a decreasing
    or non-positive seg_branch raises the flag in tree and nothing is written out of bounds."""
    from nerf_for_angiography_amd import _lib
    lib = _lib.load()
    seg, br = vr.wavy_tree(5, 2, 0)
    rec = _engine().hull_view_records(*vr.scene_views(1, 8, 8, 2))
    d = lambda x: torch.from_numpy(x).to(DEV)
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=DEV)
    good = dict(segments=d(seg), seg_branch=d(br), n=5, b=2, views=d(rec), v=1, w=8, h=8, flags=0, count=z((1, 8, 8), torch.int16),
                area=z((1, 2), torch.int32), shared=z((1, 2), torch.int32), tree=z((1, 4), torch.int32), proj=z((1, 2), torch.float64),
                length=z((2,), torch.float64))
    assert _raw_call(lib, **good)[0] == 0
    torch.cuda.synchronize()
    assert int(good["tree"][0, 3]) == 0
    host = torch.zeros(64, dtype=torch.float64)
    for change, word in ((dict(segments=None), "segments"), (dict(seg_branch=None), "seg_branch"), (dict(views=None), "views"),
                         (dict(count=None), "together"), (dict(tree=None), "together"), (dict(v=0), "n_views"), (dict(v=65536), "n_views"),
                         (dict(n=0), "n_segments"), (dict(b=0), "n_branches"), (dict(b=65536), "n_branches"), (dict(w=0), "width"),
                         (dict(h=-1), "height"), (dict(flags=2), "flags"), (dict(segments=host), "segments"), (dict(views=host), "views"),
                         (dict(proj=host), "proj"), (dict(area=host), "area"),
                         (dict(count=None, area=None, shared=None, tree=None, proj=None, length=None), "no output")):
        rc, msg = _raw_call(lib, **dict(good, **change))
        assert rc != 0 and msg.startswith("afx_view_map: ") and word in msg, (change, rc, msg)
    for bad in ([1, 1, 2, 1, 2], [0, 1, 1, 2, 2], [1, 1, 1, 1, 1], [1, 1, 2, 2, 3]):
        rc, msg = _raw_call(lib, **dict(good, seg_branch=torch.tensor(bad, dtype=torch.int32, device=DEV)))
        torch.cuda.synchronize()
        assert rc == 0 and int(good["tree"][0, 3]) != 0, bad
    eng = _engine()
    with pytest.raises(ValueError, match="seg_branch"):
        eng.view_map((seg, np.array([1, 1, 2, 1, 2], np.int32)), rec, 8, 8)
    with pytest.raises(ValueError, match="seg_branch"):
        eng.view_map((d(seg), torch.tensor([1, 1, 2, 1, 2], dtype=torch.int32, device=DEV)), d(rec), 8, 8)
    with pytest.raises(eng.AfxError, match="no CPU path"):
        eng.view_map((torch.from_numpy(seg), torch.from_numpy(br)), torch.from_numpy(rec), 8, 8)


# ---- engine.view_map from a centreline graph ----
def _y_phantom(n=24):
    """A Y of three capsules in an n^3 volume: a trunk along axis 0 that forks in the middle."""
    import skeleton_reference as sk
    c = (n - 1) / 2.0
    m = sk.capsule((n, n, n), (3, c, c), (c, c, c), 2.6)
    m |= sk.capsule((n, n, n), (c, c, c), (n - 4, 4, c - 2), 2.1)
    m |= sk.capsule((n, n, n), (c, c, c), (n - 4, n - 5, c + 3), 2.1)
    return m


def test_view_map_of_a_centreline_graph():
    """engine.view_map fed with a real centreline_graph equals the restatement fed with view_map_segments of the same points; chunked
    and unchunked views agree; the count comes back when asked for."""
    eng = _engine()
    a12 = (0.0, 1.5, 0.0, -17.0, 1.5, 0.0, 0.0, -17.0, 0.0, 0.0, 1.5, -17.0)
    mask = torch.from_numpy(_y_phantom()).to(DEV)
    d2 = eng.distance_transform_edt_3d(mask, return_squared=True)[1]
    skel = eng.skeletonize_3d(mask)
    graph = eng.centreline_graph(eng.prune_spurs(skel, d2), d2, a12)
    assert graph["n_branches"] >= 3
    angles = np.array([[t, p] for t in (-60.0, 0.0, 45.0) for p in (-30.0, 0.0, 90.0)])
    rec = eng.view_angles_records(angles, (0.0, 0.0, 120.0), 150.0)
    got = eng.view_map(graph, rec, 37, 29, index_to_world=a12, d2=d2, voxel_size=1.5, return_count=True)
    points, offsets = eng.centreline_world_points(graph, a12)
    vox = graph["path_voxels"].cpu().numpy()
    radius = np.sqrt((d2.reshape(-1).cpu().numpy().astype(np.int64) & 0xffffffff)[vox].astype(np.float64)) * 1.5
    seg, br = eng.view_map_segments(points, offsets, radius)
    assert got["n_segments"] == seg.shape[0] and br[-1] == graph["n_branches"]
    want = vr.view_map(seg, br, rec, 37, 29)
    derived = vr.derived(want)
    for key in ("area", "shared", "proj", "length", "count"):
        assert torch.equal(_bits(got[key]), _bits(want[key])), key
    for key, col in (("union", 0), ("multi", 1), ("n_invisible", 2)):
        assert np.array_equal(got[key], want["tree"][:, col]), key
    for key in ("foreshortening", "overlap", "tree_foreshortening", "tree_overlap"):
        assert torch.equal(_bits(got[key]), _bits(derived[key])), key
    assert (want["tree"][:, 1] > 0).any() and (want["tree"][:, 2] == 0).all()      # the branches meet at the junction: always a few shared pixels
    for chunk in (1, 4):
        part = eng.view_map(graph, rec, 37, 29, index_to_world=a12, d2=d2, voxel_size=1.5, chunk_views=chunk, return_count=True)
        for key in got:
            assert np.array_equal(_bits(part[key]).numpy(), _bits(got[key]).numpy()) if key != "n_segments" else part[key] == got[key], (chunk, key)
    fixed = eng.view_map(graph, rec, 37, 29, index_to_world=a12, radius=0.8)
    assert "count" not in fixed and np.array_equal(fixed["proj"], got["proj"]) and not np.array_equal(fixed["area"], got["area"])


def test_optimal_views_finds_the_view_built_to_be_best():
    """Two straight branches: one along x at z = 0, one along y at z = 4, crossing in projection only when seen along z.  For branch 1
    the view along y sees it at full length with nothing over it (view 1, the best); the view along z sees it at full length under
    branch 2; the view along x sees it end on."""
    eng = _engine()
    pts = np.array([[-5.0, 0, 0], [0.0, 0, 0], [5.0, 0, 0], [0, -5.0, 4], [0, 0.0, 4], [0, 5.0, 4]])
    seg, br = eng.view_map_segments(pts, [0, 3, 6], 0.5)
    rec = eng.view_angles_records([(0.0, 0.0), (90.0, 0.0), (0.0, 90.0)], (0.0, 0.0, 200.0), 600.0)
    vm = eng.view_map((seg, br), rec, 64, 64)
    idx, score = eng.optimal_views(vm, branch=1, k=3)
    assert idx.tolist() == [1, 0, 2] and score[0] < 1e-3 and vm["overlap"][1, 0] == 0.0 and vm["overlap"][0, 0] > 0.0
    assert vm["foreshortening"][2, 0] > 0.99
    want = vr.view_map(seg, br, rec, 64, 64)
    assert np.array_equal(vm["area"], want["area"]) and np.array_equal(vm["shared"], want["shared"])


# ---- the evaluation sweep and the driver ----
def test_sweep_view_metrics_and_columns(golden):
    """The truth as its own prediction scores 0, 0, 0; the three columns stand behind every other family, in the stated order, one
    value per column, equal to the function's."""
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from nerf_for_angiography_amd.visualization import sweep
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    n = 25
    truth = sweep.ground_truth_grid(vol, 100.0, n)
    scores, vm_p, vm_g = sweep.reconstruction_view_metrics(None, vol, 100.0, n, angles, *geo[:4], grids=(truth, truth))
    print(f"truth against itself: {scores}")
    assert (scores["foreshortening_err"], scores["overlap_err"], scores["view_regret"]) == (0.0, 0.0, 0.0)
    assert scores["best_view"] == scores["best_view_gt"] >= 0 and vm_g["foreshortening"].shape[0] == len(angles)
    assert np.isfinite(vm_g["tree_foreshortening"]).all() and (vm_g["union"] > 0).all()
    with pytest.raises(ValueError, match="ground-truth volume"):
        sweep.evaluation_sweep(m, gt, angles, *geo, metrics=["PSNR", "VIEW REGRET 3D"])
    df, _ = sweep.evaluation_sweep(m, gt, angles, *geo, metrics=["VIEW REGRET 3D", "PSNR", "OVERLAP ERR 3D", "BRANCHES 3D", "FORESHORTENING ERR 3D"],
                                   volume=vol, volume_outside=100.0, volume_points=n)
    assert list(df.columns) == BASE + ["PSNR", "BRANCHES 3D"] + list(sweep.VIEW_METRICS)
    ref = sweep.reconstruction_view_metrics(m, vol, 100.0, n, angles, *geo[:4])[0]
    print(f"model against the truth: {ref}")
    for col, key in zip(sweep.VIEW_METRICS, ("foreshortening_err", "overlap_err", "view_regret")):
        v = df[col].to_numpy()
        assert len(v) == len(angles) and ((v == ref[key]).all() or (np.isnan(v).all() and ref[key] != ref[key])), col
    assert not ref["view_regret"] < 0.0


def test_driver_saves_the_view_map(tmp_path):
    """--save_view_map on the synthetic phantom for a handful of iterations: one CSV row per sweep angle, finite whole-tree columns, the
    five best views in the info; the flag changes nothing else."""
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    driver = ["--synthetic", "--img_size", "16", "--num_layers", "4", "--num_hidden_units", "64", "--sample_size", "8", "--depth_samples", "32",
              "--n_iters", "4", "--display_every", "2", "--out_bias_init", "0.0", "--pos_enc", "fourier"]
    # (sigma ~ 0.5 everywhere, and the Fourier features give the untrained field structure: {sigma >= 0.5} has a centreline with branches)
    plain = main(driver + ["--log_dir", str(tmp_path / "a")])
    assert "view_map_info" not in plain
    out = main(driver + ["--log_dir", str(tmp_path / "b"), "--save_view_map", str(tmp_path / "views.csv"), "--mesh_threshold", "0.5",
                         "--view_map_step", "45"])
    assert torch.equal(out["model"].flat_params, plain["model"].flat_params)
    info = out["view_map_info"]
    rows = list(csv.reader(open(info["path"])))
    assert rows[0][:4] == ["theta", "phi", "tree_foreshortening", "tree_overlap"] and len(rows[0]) == 4 + 2 * info["n_branches"]
    assert info["n_views"] == 25 and len(rows) == 1 + 25 and info["n_branches"] >= 1 and info["n_segments"] >= 2
    body = np.array([[float(x) for x in r[:4]] for r in rows[1:]])
    assert np.isfinite(body).all() and sorted(set(body[:, 0])) == [-90.0, -45.0, 0.0, 45.0, 90.0]
    assert len(info["best"]) == 5 and info["best"][0][2] == np.min(body[:, 2] + body[:, 3])
