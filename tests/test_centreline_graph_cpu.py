"""The centreline graph without a GPU: the NumPy restatement of the definitions (tests/graph_reference.py) on shapes with a known answer,
its invariants on noise, the pruning rule's properties, the host-side profile of a branch, the sweep's handling of the graph metric
names, and the argument checks and workspace queries of afx_centreline_graph / afx_prune_spurs (include/afx.h), which return before
any HIP call."""
import ctypes as C
import math

import numpy as np
import pytest

import graph_reference as gr
import skeleton_reference as sk

AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
FAKE = C.c_void_p(0x10000)          # never dereferenced: every call below is refused before it reaches the device
BAD_SHAPES = ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1025, 4, 4), (4, 1025, 4), (4, 4, 1025), (1 << 20, 1, 1))


@pytest.fixture(scope="module")
def lib():
    from nerf_for_angiography_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def shapes():
    """{name: (mask, skeleton, squared EDT of the mask, graph of the skeleton)} of the references, computed once."""
    out = {}
    for name, m in (("bar", sk.bar()), ("torus", sk.torus()), ("cube", sk.cube()), ("shell", sk.shell()), ("tree", sk.capsule_tree(48))):
        s = sk.skeletonize(m)[0]
        d2 = gr.squared_edt(m)
        out[name] = (m, s, d2, gr.analyse(s, d2))
    return out


def test_known_graphs_of_the_skeleton_shapes(shapes):
    want = {"bar": (1, 3, 0, 3), "torus": (0, 1, 1, 0), "cube": (0, 1, 0, 2), "shell": (1, 0, 0, 0), "tree": (10, 25, 0, 16)}
    for name, (m, s, d2, g) in shapes.items():
        r = g["record"]
        assert (r["nodes"], r["branches"], r["cycles"], r["free_ends"]) == want[name], name
        assert r["free_ends"] == r["deg1"] + 2 * r["deg0"] and r["on"] == s.sum() == r["j_voxels"] + r["p_voxels"], name
        assert len(g["path_voxels"]) == r["p_voxels"] and sorted(g["path_voxels"]) == np.flatnonzero(g["branch_labels"]).tolist(), name
    torus = shapes["torus"][3]["branches"][0]
    assert torus["cycle"] and torus["att"] == 0 and torus["first"] == min(shapes["torus"][3]["path_voxels"])
    assert sum(torus["counts"]) == torus["n"]                                      # a cycle has as many steps as voxels
    diag = shapes["cube"][3]["branches"][0]
    assert diag["counts"][12] == diag["n"] - 1 and diag["length"] == float(diag["n"] - 1) * math.sqrt(3.0)


def test_pruning_the_bar_and_the_tree(shapes):
    m, s, d2, _ = shapes["bar"]
    p, rec = gr.prune(s, d2, 1.0)
    assert p.sum() == 14 == p[4, 5, :].sum() and rec["rounds"] == 2 and rec["converged"] == 1 and rec["voxels"] == 2      # on the bar's centre line
    r = gr.analyse(p, d2)["record"]
    assert (r["branches"], r["nodes"], r["free_ends"]) == (1, 0, 2)
    m, s, d2, _ = shapes["tree"]
    p, rec = gr.prune(s, d2, 1.0)
    r = gr.analyse(p, d2)["record"]
    assert (int(p.sum()), r["branches"], r["nodes"], r["free_ends"], rec["branches"], rec["rounds"]) == (56, 3, 1, 3, 15, 2)


def test_pruning_keeps_the_invariants_and_is_idempotent(shapes):
    extra = sk.smooth_noise((17, 18, 19), 3)
    cases = [(name, s, d2) for name, (m, s, d2, g) in shapes.items()] + [("smooth noise", sk.skeletonize(extra)[0], gr.squared_edt(extra))]
    for name, s, d2 in cases:
        for factor in (0.0, 1.0, 2.0):
            p, rec = gr.prune(s, d2, factor)
            assert not (p & ~s).any() and rec["remaining"] == p.sum() == s.sum() - rec["voxels"] and rec["converged"] == 1, (name, factor)
            assert sk.invariants(p) == sk.invariants(s), (name, factor)
            again, rec2 = gr.prune(p, d2, factor)
            assert np.array_equal(again, p) and rec2["rounds"] == 1 and rec2["voxels"] == 0, (name, factor)
            one = gr.prune(s, d2, factor, max_rounds=1)[0]
            assert not ((gr.degree(s) >= 3) & ~one).any(), (name, factor)          # a round never deletes a junction voxel of its graph
        assert np.array_equal(gr.prune(s, d2, 0.0)[0], s), name                    # a spur is at least one step long


@pytest.mark.parametrize("p", (0.05, 0.1, 0.3, 0.5))
def test_every_branch_is_a_path_or_a_cycle_on_noise(p):
    rng = np.random.default_rng(int(p * 100))
    for shape in ((5, 9, 17), (9, 17, 33), (17, 18, 19)):
        m = rng.random(shape) < p
        g = gr.analyse(m, gr.squared_edt(m))            # raises when a branch is neither (the restatement's own assertions)
        r = g["record"]
        assert r["free_ends"] == r["deg1"] + 2 * r["deg0"], (shape, p)
        assert sum(b["n"] for b in g["branches"]) == r["p_voxels"] == len(set(g["path_voxels"])), (shape, p)
        assert all(b["offset"] == sum(x["n"] for x in g["branches"][:i]) for i, b in enumerate(g["branches"]))
        # the total length is the formula on the summed counts, not a sum of the branches' lengths
        assert r["counts"] == [sum(b["counts"][c] for b in g["branches"]) for c in range(13)]
        assert r["length"] == gr.length_of(r["counts"], gr.unit_lengths())
        assert r["cycles"] == sum(b["cycle"] for b in g["branches"]) and r["nodes"] == g["node_labels"].max()


def test_step_classes_and_world_lengths():
    seen = set()
    for o in gr.OFFSETS:
        c = gr.step_class(o)
        assert c == gr.step_class(tuple(-x for x in o)) and 0 <= c <= 12
        seen.add(c)
    assert seen == set(range(13)) and gr.class_offset(0) == (0, 0, 1) and gr.class_offset(12) == (1, 1, 1)
    assert gr.unit_lengths()[0] == 1.0 and gr.unit_lengths()[1] == math.sqrt(2.0) and gr.unit_lengths()[2] == 1.0 and gr.unit_lengths()[12] == math.sqrt(3.0)
    from nerf_for_angiography_amd import engine
    a = (0.0, 0.5, 0.0, -3.0, 0.25, 0.0, 0.0, 1.0, 0.0, 0.0, 2.0, 7.0)            # axes exchanged, anisotropic
    assert engine.graph_step_lengths(a) == gr.world_lengths(a) and engine.graph_step_lengths(None) is None
    assert gr.world_lengths(a)[0] == 2.0 and gr.world_lengths(a)[8] == 0.25        # (0,0,1) and (1,0,0)


def test_branch_profile_on_a_hand_made_path():
    import torch
    from nerf_for_angiography_amd import engine
    shape = (4, 5, 12)
    s = np.zeros(shape, bool)
    path = [(1, 1, 1), (1, 1, 2), (1, 2, 3), (2, 3, 4), (2, 3, 5), (2, 3, 6)]
    for v in path:
        s[v] = True
    d2 = np.zeros(shape, np.int64)
    for v, x in zip(path, (16, 9, 4, 1, 9, 16)):
        d2[v] = x
    g = gr.analyse(s, d2)
    assert g["record"]["branches"] == 1 and g["branches"][0]["path"] == path
    graph = {"n_branches": 1, "path_offset": torch.tensor([0]), "branch_size": torch.tensor([6]), "shape": shape,
             "path_voxels": torch.tensor(g["path_voxels"])}
    prof = engine.centreline_branch_profile(graph, torch.from_numpy(d2), 1, 0.5)
    want_arc = np.cumsum([0.0, 0.5, 0.5 * math.sqrt(2.0), 0.5 * math.sqrt(3.0), 0.5, 0.5])
    assert prof["voxels"].tolist() == g["path_voxels"]
    assert np.allclose(prof["arc_length"].numpy(), want_arc, rtol=0, atol=1e-15)
    assert prof["radius"].tolist() == [2.0, 1.5, 1.0, 0.5, 1.5, 2.0]
    assert prof["r_min"] == 0.5 and prof["r_median"] == 1.5 and prof["stenosis"] == 1.0 - 0.5 / 1.5
    aniso = engine.centreline_branch_profile(graph, torch.from_numpy(d2), 1, (1.0, 2.0, 3.0))
    assert aniso["arc_length"][1].item() == 3.0 and aniso["arc_length"][2].item() == 3.0 + math.sqrt(4.0 + 9.0) and aniso["radius"][0].item() == 4.0
    with pytest.raises(ValueError, match="outside"):
        engine.centreline_branch_profile(graph, torch.from_numpy(d2), 2)


def test_unpacked_rows_equal_the_restatement(shapes):
    import torch
    from nerf_for_angiography_amd import engine
    g = shapes["tree"][3]
    rows = np.array([gr.row_slots(r) for r in g["branches"]], dtype=np.uint64).view(np.int64)
    got = engine._unpack_branch_rows(torch.from_numpy(rows))
    for key, field in (("branch_size", "n"), ("path_offset", "offset"), ("free_ends", "free"), ("attachments", "att"), ("node_start", "node_start"),
                       ("node_end", "node_end"), ("d2_min", "d2_min"), ("d2_max", "d2_max"), ("d2_argmin", "argmin"), ("d2_start", "d2_start"),
                       ("d2_end", "d2_end"), ("first_voxel", "first"), ("last_voxel", "last"), ("length", "length"), ("radius_sum", "r_sum")):
        assert got[key].tolist() == [r[field] for r in g["branches"]], key
    assert got["step_counts"].tolist() == [r["counts"] for r in g["branches"]]
    assert got["is_spur"].tolist() == [bool(r["spur"]) for r in g["branches"]] and not got["is_cycle"].any()


def test_graph_scores_arithmetic():
    from nerf_for_angiography_amd.visualization.sweep import graph_scores
    gp = {"n_branches": 5, "n_nodes": 2, "n_free_ends": 4, "total_length": 30.0, "d2_min_all": 4}
    gl = {"n_branches": 3, "n_nodes": 1, "n_free_ends": 3, "total_length": 40.0, "d2_min_all": None}
    s = graph_scores(gp, gl, {"branches": 7, "rounds": 2}, {"branches": 1, "rounds": 2}, 0.5)
    assert (s["n_branches"], s["n_nodes"], s["n_free_ends"], s["n_spurs_removed"], s["length"], s["min_radius"]) == (5, 2, 4, 7, 30.0, 1.0)
    assert (s["n_branches_gt"], s["n_spurs_removed_gt"], s["length_gt"]) == (3, 1, 40.0) and math.isnan(s["min_radius_gt"])
    assert s["length_ratio"] == 30.0 / 40.0


def test_metric_columns_with_the_graph_names():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.GRAPH_METRICS == ("BRANCHES 3D", "JUNCTIONS 3D", "LENGTH RATIO 3D")
    assert sweep._VOLUME_METRICS[-3:] == sweep.GRAPH_METRICS and sweep._VOLUME_METRICS[-6:-3] == sweep.MESH_DISTANCE_METRICS
    assert not set(sweep.GRAPH_METRICS) & set(sweep._EXTRA_METRICS)                # appended: earlier columns keep their place
    got = sweep._check_metrics(["LENGTH RATIO 3D", "HD MESH", "BRANCHES 3D", "CLDICE 3D", "PSNR", "JUNCTIONS 3D", "DOT 3D"], None, object())
    assert got == ["PSNR", "DOT 3D", "CLDICE 3D", "HD MESH", "BRANCHES 3D", "JUNCTIONS 3D", "LENGTH RATIO 3D"]
    assert sweep._check_metrics("BRANCHES 3D", None, object()) == ["BRANCHES 3D"]
    assert sweep._check_metrics(None, None, object()) == ["PSNR", "DOT 2D"]          # the defaults do not grow
    for name in sweep.GRAPH_METRICS:
        with pytest.raises(ValueError, match="volume"):
            sweep._check_metrics([name], None, None)
    with pytest.raises(ValueError, match="unknown"):
        sweep._check_metrics(["BRANCHES 3D", "BRANCHES 2D"], None, object())


class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"evaluation_sweep touched the model ({name}) before rejecting its arguments")


def test_evaluation_sweep_refuses_graph_metrics_before_gpu_work():
    from nerf_for_angiography_amd.visualization.sweep import evaluation_sweep
    args = dict(model=_NoModel(), targets=None, angles=np.zeros((4, 2)), img_width=8, img_height=8, focal_length=100.0,
                src_pt=np.array([0, 0, 1500.0]), near_thresh=1400.0, far_thresh=1600.0, depth_samples_per_ray=16)
    with pytest.raises(ValueError, match="volume"):
        evaluation_sweep(metrics=["PSNR", "BRANCHES 3D"], **args)
    with pytest.raises(AssertionError, match="touched the model"):       # a request it can serve goes on to the model
        evaluation_sweep(metrics=["LENGTH RATIO 3D"], volume=object(), **args)


def test_host_tensors_are_refused():
    import torch
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd._lib import AfxError
    with pytest.raises(AfxError):
        engine.centreline_graph(torch.ones(4, 5, 6))
    with pytest.raises(AfxError):
        engine.prune_spurs(torch.ones(4, 5, 6), torch.ones(4, 5, 6, dtype=torch.int32))
    with pytest.raises(AfxError):
        engine.centreline_graph_record(torch.ones(4, 5, 6, dtype=torch.uint8))
    with pytest.raises(AfxError):
        engine.prune_record(torch.ones(4, 5, 6, dtype=torch.uint8), torch.ones(4, 5, 6, dtype=torch.int32), 1.0, 2)


def test_the_library_exports_the_new_symbols(lib):
    from nerf_for_angiography_amd import _lib
    for name in ("afx_centreline_graph_workspace_bytes", "afx_centreline_graph", "afx_prune_spurs_workspace_bytes", "afx_prune_spurs"):
        assert hasattr(lib, name) and name in _lib.exported_symbols(), name


def _r256(x):
    return (x + 255) // 256 * 256


def test_workspace_queries_equal_the_documented_formulas(lib):
    for shape in ((1, 1, 1), (5, 7, 3), (33, 17, 65), (201, 201, 201), (1024, 1, 1)):
        n = shape[0] * shape[1] * shape[2]
        label = lib.afx_label_components_3d_workspace_bytes(*shape)
        graph = 2 * _r256(n) + _r256(4 * n) + _r256(max(label, 2 * _r256(4 * n))) + _r256(4 * ((n + 2047) // 2048)) + 3 * 256
        assert lib.afx_centreline_graph_workspace_bytes(*shape) == graph, shape
        assert lib.afx_prune_spurs_workspace_bytes(*shape) == graph + 3 * _r256(4 * n) + _r256(n) + 256, shape
    for bad in BAD_SHAPES:
        assert lib.afx_centreline_graph_workspace_bytes(*bad) == 0 and lib.afx_prune_spurs_workspace_bytes(*bad) == 0, bad


def test_centreline_graph_argument_validation(lib):
    def call(skel=FAKE, d2=None, shape=(4, 5, 6), L=None, nl=FAKE, bl=FAKE, pv=FAKE, rows=FAKE, max_b=4, rec=FAKE, ws=FAKE, nbytes=1 << 40,
             need=None):
        return lib.afx_centreline_graph(skel, d2, *shape, L, nl, bl, pv, rows, max_b, rec, ws, nbytes, need, None)
    for name in ("skel", "nl", "bl", "pv", "rec"):
        assert call(**{name: None}) == AFX_E_INVALID and b"null" in lib.afx_last_error(), name
    for bad in BAD_SHAPES:
        assert call(shape=bad) == AFX_E_INVALID, bad
    assert call(max_b=-1) == AFX_E_INVALID and call(max_b=1 << 31) == AFX_E_INVALID and call(rows=None) == AFX_E_INVALID
    for bad in (-1.0, float("nan"), float("inf")):
        L = (C.c_double * 13)(*([1.0] * 12 + [bad]))
        assert call(L=L) == AFX_E_INVALID and b"step_lengths" in lib.afx_last_error(), bad
    need = C.c_size_t(0)
    assert call(nbytes=8, need=C.byref(need)) == AFX_E_WORKSPACE and need.value == lib.afx_centreline_graph_workspace_bytes(4, 5, 6)
    assert call(ws=None) == AFX_E_WORKSPACE and b"workspace" in lib.afx_last_error()
    assert call(nbytes=need.value - 1) == AFX_E_WORKSPACE


def test_prune_spurs_argument_validation(lib):
    def call(skel=FAKE, d2=FAKE, shape=(4, 5, 6), factor=1.0, max_rounds=4, sync_every=0, out=FAKE, rec=FAKE, ws=FAKE, nbytes=1 << 40, need=None):
        return lib.afx_prune_spurs(skel, d2, *shape, factor, max_rounds, sync_every, out, rec, ws, nbytes, need, None)
    for name in ("skel", "d2", "out", "rec"):
        assert call(**{name: None}) == AFX_E_INVALID and b"null" in lib.afx_last_error(), name
    for bad in BAD_SHAPES:
        assert call(shape=bad) == AFX_E_INVALID, bad
    for bad in (-0.5, float("nan"), float("inf")):
        assert call(factor=bad) == AFX_E_INVALID and b"factor" in lib.afx_last_error(), bad
    for k in (0, -1):
        assert call(max_rounds=k) == AFX_E_INVALID and b"max_rounds" in lib.afx_last_error(), k
    assert call(sync_every=-1) == AFX_E_INVALID and b"sync_every" in lib.afx_last_error()
    need = C.c_size_t(0)
    assert call(nbytes=8, need=C.byref(need)) == AFX_E_WORKSPACE and need.value == lib.afx_prune_spurs_workspace_bytes(4, 5, 6)
    assert call(ws=None) == AFX_E_WORKSPACE and call(nbytes=need.value - 1) == AFX_E_WORKSPACE


def test_polylines_and_their_vtk_file(tmp_path):
    import torch
    from nerf_for_angiography_amd.visualization import mesh_io, sweep
    s = np.zeros((4, 5, 12), bool)
    path = [(1, 1, 1), (1, 1, 2), (1, 2, 3), (2, 3, 4)]
    for v in path:
        s[v] = True
    s[3, 4, 10] = True                                                             # a second branch: one voxel
    g = gr.analyse(s)
    graph = {"path_voxels": torch.tensor(g["path_voxels"]), "shape": s.shape, "branch_size": torch.tensor([b["n"] for b in g["branches"]])}
    a = sweep.grid_index_to_world(100.0, 25)                                       # the first two axes exchanged, step 200 / 24
    pts, off, rad = sweep.centreline_polylines(graph, torch.full(s.shape, 4), a, 0.5)
    step = 200.0 / 24
    assert off.tolist() == [0, 4, 5] and rad.tolist() == [1.0] * 5
    assert np.array_equal(pts, np.array([[j * step - 100.0, i * step - 100.0, k * step - 100.0] for i, j, k in path + [(3, 4, 10)]]))
    out = mesh_io.write_vtk_polylines(tmp_path / "c.vtk", pts, off, {"radius": rad})
    lines = open(out).read().split("\n")
    assert lines[0] == "# vtk DataFile Version 3.0" and lines[2:5] == ["ASCII", "DATASET POLYDATA", "POINTS 5 double"]
    assert [float(x) for x in lines[5].split()] == pts[0].tolist()
    assert lines[10:13] == ["LINES 2 7", "4 0 1 2 3", "1 4"] and lines[13:16] == ["POINT_DATA 5", "SCALARS radius double 1", "LOOKUP_TABLE default"]
    assert [float(x) for x in lines[16:21]] == rad.tolist() and not [f for f in tmp_path.iterdir() if ".tmp." in f.name]
    mesh_io.write_vtk_polylines(tmp_path / "empty.vtk", np.zeros((0, 3)), [0])
    assert "LINES 0 0" in open(tmp_path / "empty.vtk").read()
    for bad in ([0, 3], [1, 5], [0, 2, 2, 5]):
        with pytest.raises(ValueError, match="offsets"):
            mesh_io.write_vtk_polylines(tmp_path / "bad.vtk", pts, bad)
    with pytest.raises(ValueError, match="point_data"):
        mesh_io.write_vtk_polylines(tmp_path / "bad.vtk", pts, off, {"radius": rad[:3]})
    assert not (tmp_path / "bad.vtk").exists()


def test_driver_checks_the_centreline_flag():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser, check_args
    base = ["--synthetic", "--img_size", "16", "--n_iters", "4"]
    assert build_parser().parse_args(base).save_centreline is None
    check_args(build_parser().parse_args(base + ["--save_centreline", "tree.vtk"]))
    with pytest.raises(ValueError, match=".vtk"):
        check_args(build_parser().parse_args(base + ["--save_centreline", "tree.stl"]))
