"""The centreline graph and spur pruning on the GPU (afx_centreline_graph, afx_prune_spurs; engine.centreline_graph / prune_spurs,
visualization/sweep.py) against the NumPy restatement of tests/graph_reference.py.  Every output is a pure function of the input - canonical
labels, canonical path order, integer step counts, fp64 formed from them in a stated order - so labels, paths, rows and records must
EQUAL the reference: there are no tolerances, the fp64 slots are compared as bits, and a second run gives the same bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import graph_reference as gr
import skeleton_reference as sk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# linear sizes one below, at and one above a wave of 64 voxels, a workgroup of 256 entries and a chunk of 2048 voxels, the long extent
# along each axis in turn; a single voxel, no interior, single lines and planes
SHAPES = [(1, 1, 1), (2, 2, 2), (1, 1, 9), (1, 8, 9), (7, 1, 33), (5, 65, 9), (9, 17, 33), (17, 18, 19), (1, 1, 257), (257, 1, 1),
          (2, 1, 1024), (1024, 2, 1), (1, 3, 683), (16, 8, 16)]


def _dev_mask(mask):
    return torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(DEV)


def _dev_d2(d2):
    """The uint32 squared EDT held in an int32 tensor, as the record-level calls take it."""
    return None if d2 is None else torch.from_numpy(np.asarray(d2, np.int64).astype(np.uint32).view(np.int32).reshape(np.shape(d2))).to(DEV)


def _raw(mask, d2=None, lengths=None, max_branches=None):
    """afx_centreline_graph -> (node_labels, branch_labels, path_voxels [all N], rows uint64 [max_branches, 16], record uint64 [16])."""
    from nerf_for_angiography_amd.engine import centreline_graph_record
    cap = int(np.size(mask)) if max_branches is None else max_branches
    nl, bl, pv, rows, rec = centreline_graph_record(_dev_mask(mask), _dev_d2(d2), lengths, cap)
    assert nl.dtype == bl.dtype == pv.dtype == torch.int32 and rows.shape == (cap, 16) and rec.shape == (16,)
    return nl.cpu().numpy(), bl.cpu().numpy(), pv.cpu().numpy(), rows.cpu().numpy().view(np.uint64), rec.cpu().numpy().view(np.uint64)


def _check(mask, d2=None, lengths=None, what="", max_branches=None):
    want = gr.analyse(mask, d2, lengths)
    nl, bl, pv, rows, rec = _raw(mask, d2, lengths, max_branches)
    nb = want["record"]["branches"]
    assert rec.tolist() == gr.record_slots(want["record"], max_branches), (what, rec.tolist(), gr.record_slots(want["record"], max_branches))
    assert np.array_equal(nl, want["node_labels"]) and np.array_equal(bl, want["branch_labels"]), what
    assert pv[:len(want["path_voxels"])].tolist() == want["path_voxels"], what
    for b in range(nb if max_branches is None else min(nb, max_branches)):
        assert rows[b].tolist() == gr.row_slots(want["branches"][b]), (what, b, rows[b].tolist(), gr.row_slots(want["branches"][b]))
    return want, (nl, bl, pv, rows, rec)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_any_mask_equals_the_reference(shape):
    rng = np.random.default_rng(shape[0] * 7919 + shape[1] * 31 + shape[2])
    masks = [(f"p = {p}", rng.random(shape) < p) for p in (0.02, 0.05, 0.1, 0.3, 0.9)]
    smooth = sk.smooth_noise(shape, shape[1] + 3)
    masks += [("skeleton of smooth noise", sk.skeletonize(smooth)[0]), ("all one", np.ones(shape, bool)), ("all zero", np.zeros(shape, bool))]
    for what, mask in masks:
        _check(mask, gr.squared_edt(smooth if what.startswith("skeleton") else mask), what=what)


@functools.lru_cache(maxsize=None)
def _shape(name):
    """(mask, reference skeleton), computed once per session."""
    m = {"bar": sk.bar, "torus": sk.torus, "shell": sk.shell, "cube": sk.cube, "tree": lambda: sk.capsule_tree(48),
         "smooth": lambda: sk.smooth_noise((17, 18, 19), 3)}[name]()
    return m, sk.skeletonize(m)[0]


def test_structured_shapes_with_the_device_edt():
    from nerf_for_angiography_amd.engine import centreline_graph, distance_transform_edt_3d
    counts = {"bar": (1, 3, 0, 3), "torus": (0, 1, 1, 0), "cube": (0, 1, 0, 2), "shell": (1, 0, 0, 0), "tree": (10, 25, 0, 16)}
    for name, expect in counts.items():
        m, s = _shape(name)
        d2 = distance_transform_edt_3d(torch.from_numpy(m).to(DEV), return_squared=True)[1]
        assert np.array_equal(d2.cpu().numpy(), gr.squared_edt(m)), name
        want, _ = _check(s, d2.cpu().numpy(), what=name)
        g = centreline_graph(torch.from_numpy(s).to(DEV), d2)                        # the public form: unpacked rows, integers
        assert (g["n_nodes"], g["n_branches"], g["n_cycles"], g["n_free_ends"]) == expect, name
        assert g["path_voxels"].tolist() == want["path_voxels"] and g["total_length"] == want["record"]["length"], name
        assert g["length"].tolist() == [r["length"] for r in want["branches"]] and g["radius_sum"].tolist() == [r["r_sum"] for r in want["branches"]]
        assert g["step_counts"].tolist() == [r["counts"] for r in want["branches"]] and g["d2_min"].tolist() == [r["d2_min"] for r in want["branches"]]
        assert g["d2_min_all"] == (want["record"]["d2_min"] if expect[1] else None), name


def test_hand_made_cycle_and_single_voxel_branches():
    tri = np.zeros((4, 5, 6), bool)
    tri[1, 2, 2] = tri[1, 2, 3] = tri[2, 3, 3] = True                                 # three voxels, each a neighbour of the other two
    want, _ = _check(tri, what="3-voxel cycle")
    assert want["record"]["cycles"] == 1 and want["branches"][0]["n"] == 3 and sum(want["branches"][0]["counts"]) == 3
    line = np.zeros((5, 5, 16), bool)
    line[2, 2, 1:15] = True
    for k in (3, 7, 9):                                                            # side voxels make junction clusters along a line ...
        line[1, 2, k] = line[3, 2, k] = True
    want, _ = _check(line, np.full(line.shape, 9), what="junction clusters")
    singles = [r for r in want["branches"] if r["n"] == 1 and r["att"] == 2]
    assert singles, [(r["n"], r["att"]) for r in want["branches"]]                   # ... with single-voxel branches between two of them
    assert any(r["node_start"] != r["node_end"] for r in singles)
    lone = np.zeros((3, 3, 3), bool)
    lone[1, 1, 1] = True
    want, _ = _check(lone, what="one voxel")
    assert want["record"]["free_ends"] == 2 and want["branches"][0]["free"] == 2


def test_anisotropic_lengths_no_d2_overflow_and_repeat():
    from nerf_for_angiography_amd.engine import centreline_graph, graph_step_lengths
    m, s = _shape("tree")
    a = (0.0, 0.37, 0.0, -3.0, 0.91, 0.0, 0.0, 1.0, 0.0, 0.0, 1.7, 7.0)
    L = graph_step_lengths(a)
    assert L == gr.world_lengths(a)
    want, first = _check(s, gr.squared_edt(m), L, what="anisotropic")
    assert want["record"]["length"] != gr.analyse(s)["record"]["length"]
    _, again = _check(s, gr.squared_edt(m), L, what="anisotropic, again")
    nb, npath = want["record"]["branches"], want["record"]["p_voxels"]
    for x, y in zip(first, again):                                                 # the same bits on a second run (of what the call defines)
        assert np.array_equal(x[:npath] if x.ndim == 1 and x.size > 16 else x[:nb] if x.ndim == 2 else x, y[:npath] if y.ndim == 1 and y.size > 16
                              else y[:nb] if y.ndim == 2 else y)
    want0, (_, _, _, rows, rec) = _check(s, None, what="no d2")
    assert rec[12] == gr.NONE and all(r["d2_max"] == 0 and r["r_sum"] == 0.0 for r in want0["branches"])
    nb = want["record"]["branches"]
    for cap in (0, 1, nb - 1, nb):
        _, (_, _, _, rows, rec) = _check(s, gr.squared_edt(m), what=f"max_branches = {cap}", max_branches=cap)
        assert int(rec[11]) == int(cap < nb) and int(rec[4]) == nb
    noise = np.random.default_rng(11).random((24, 40, 40)) < 0.1                       # more branches than the public call's first table
    ref = gr.analyse(noise)
    assert ref["record"]["branches"] > 1024
    g = centreline_graph(torch.from_numpy(noise).to(DEV), index_to_world=a)
    assert g["n_branches"] == ref["record"]["branches"] == g["length"].numel() and g["path_voxels"].tolist() == ref["path_voxels"]
    assert g["total_length"] == gr.analyse(noise, None, L)["record"]["length"] and g["d2_min_all"] is None


def _prune_raw(mask, d2, factor, max_rounds, sync_every, in_place=False):
    from nerf_for_angiography_amd.engine import prune_record
    x = _dev_mask(mask)
    out, rec = prune_record(x, _dev_d2(d2), factor, max_rounds, sync_every, out=x if in_place else None)
    assert out.dtype == torch.uint8 and rec.shape == (8,) and (out.data_ptr() == x.data_ptr()) == in_place
    if not in_place:
        assert np.array_equal(x.cpu().numpy(), np.asarray(mask, np.uint8))            # the input is left alone
    return out.cpu().numpy(), rec.cpu().tolist()


def test_pruning_equals_the_reference():
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.engine import prune_spurs
    for name in ("tree", "bar", "smooth", "torus"):
        m, s = _shape(name)
        d2 = gr.squared_edt(m)
        for factor in (0.0, 1.0, 2.0):
            want, rec = gr.prune(s, d2, factor)
            full = gr.prune_record_slots(rec)
            need = rec["rounds"]
            for sync, rounds, in_place in ((0, need, False), (0, need + 3, True), (1, need + 3, False), (2, need + 3, True)):
                got, r = _prune_raw(s, d2, factor, rounds, sync, in_place)           # more rounds than needed change nothing
                assert r == full and np.array_equal(got, want.astype(np.uint8)), (name, factor, sync, rounds, r, full)
            p, prec = prune_spurs(torch.from_numpy(s).to(DEV), torch.from_numpy(d2).to(DEV), factor, return_record=True)
            assert p.dtype == torch.bool and np.array_equal(p.cpu().numpy(), want) and list(prec.values()) == full[:7], (name, factor)
            again, r = _prune_raw(want, d2, factor, 2, 0)
            assert np.array_equal(again, want.astype(np.uint8)) and r[:4] == [1, 0, 0, 1], (name, factor)      # idempotent
    m, s = _shape("tree")
    d2 = gr.squared_edt(m)
    part, prec = gr.prune(s, d2, 1.0, max_rounds=1)
    assert prec["converged"] == 0
    for sync in (0, 1):
        got, r = _prune_raw(s, d2, 1.0, 1, sync)
        assert r == gr.prune_record_slots(prec) and np.array_equal(got, part.astype(np.uint8)), sync
    assert b"max_rounds" in _lib.load().afx_last_error()                              # the synchronised form says that it stopped early
    want, rec = gr.prune(s, d2, 1.0)
    r = gr.analyse(want, d2)["record"]
    assert (int(want.sum()), r["branches"], r["nodes"], r["free_ends"], rec["branches"]) == (56, 3, 1, 3, 15)


def test_refusals_on_the_device():
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.engine import centreline_graph, centreline_graph_record, prune_record, prune_spurs
    from nerf_for_angiography_amd._lib import AfxError
    lib = _lib.load()
    x = torch.ones(4, 5, 6, dtype=torch.uint8, device=DEV)
    d = torch.ones(4, 5, 6, dtype=torch.int32, device=DEV)
    small = torch.empty(64, dtype=torch.uint8, device=DEV)
    with pytest.raises(AfxError, match="workspace"):
        centreline_graph_record(x, None, None, 4, workspace=small)
    with pytest.raises(AfxError, match="workspace"):
        prune_record(x, d, 1.0, 2, workspace=small)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(AfxError, match="factor"):
            prune_spurs(x, d, bad)
    with pytest.raises(AfxError, match="max_rounds"):
        prune_spurs(x, d, 1.0, max_rounds=0)
    with pytest.raises(AfxError, match="sync_every"):
        prune_record(x, d, 1.0, 2, sync_every=-1)
    with pytest.raises(AfxError, match="step_lengths"):
        centreline_graph_record(x, None, [1.0] * 12 + [float("nan")], 4)
    with pytest.raises(AfxError, match="1024"):
        centreline_graph(torch.ones(1025, 1, 2, device=DEV))
    with pytest.raises(ValueError):
        centreline_graph(torch.ones(4, 4, device=DEV))
    with pytest.raises(ValueError, match="d2"):
        prune_spurs(x, None)
    need = C.c_size_t(0)
    rc = lib.afx_centreline_graph(x.data_ptr(), None, 4, 5, 6, None, d.data_ptr(), d.data_ptr(), d.data_ptr(), None, 0, d.data_ptr(), small.data_ptr(),
                                  64, C.byref(need), None)
    assert rc == -2 and need.value == lib.afx_centreline_graph_workspace_bytes(4, 5, 6)


def test_graph_and_pruning_replay_from_a_captured_graph():
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.engine import centreline_graph_record, prune_record
    lib = _lib.load()
    inputs = {}
    for name in ("smooth", "tree"):
        m, s = _shape(name)
        pad = np.zeros((48, 48, 48), bool)
        pad[:s.shape[0], :s.shape[1], :s.shape[2]] = s
        dd = np.zeros((48, 48, 48), np.int64)
        dd[:s.shape[0], :s.shape[1], :s.shape[2]] = gr.squared_edt(m)
        inputs[name] = (_dev_mask(pad), _dev_d2(dd))
    shape, rounds, cap = (48, 48, 48), 4, 256
    eager = {}
    for name, (x, d) in inputs.items():
        pruned, prec = prune_record(x, d, 1.0, rounds, 0)
        eager[name] = (pruned, prec) + centreline_graph_record(pruned, d, None, cap)
        want, wrec = gr.prune(x.cpu().numpy(), d.cpu().numpy(), 1.0)
        assert wrec["rounds"] <= rounds and np.array_equal(pruned.cpu().numpy(), want.astype(np.uint8)), name
    static_x, static_d = inputs["smooth"][0].clone(), inputs["smooth"][1].clone()
    n = 48 ** 3
    bufs = dict(out=torch.zeros(shape, dtype=torch.uint8, device=DEV), prec=torch.zeros(8, dtype=torch.int64, device=DEV),
                pws=torch.empty(int(lib.afx_prune_spurs_workspace_bytes(*shape)), dtype=torch.uint8, device=DEV),
                nl=torch.zeros(shape, dtype=torch.int32, device=DEV), bl=torch.zeros(shape, dtype=torch.int32, device=DEV),
                pv=torch.zeros(n, dtype=torch.int32, device=DEV), rows=torch.zeros((cap, 16), dtype=torch.int64, device=DEV),
                rec=torch.zeros(16, dtype=torch.int64, device=DEV),
                gws=torch.empty(int(lib.afx_centreline_graph_workspace_bytes(*shape)), dtype=torch.uint8, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            prune_record(static_x, static_d, 1.0, rounds, 0, out=bufs["out"], record=bufs["prec"], workspace=bufs["pws"])
            centreline_graph_record(bufs["out"], static_d, None, cap, node_labels=bufs["nl"], branch_labels=bufs["bl"], path_voxels=bufs["pv"],
                                    branches=bufs["rows"], record=bufs["rec"], workspace=bufs["gws"])
    torch.cuda.current_stream().wait_stream(side)
    for name in ("tree", "smooth"):
        static_x.copy_(inputs[name][0])
        static_d.copy_(inputs[name][1])
        for t in bufs.values():
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        pruned, prec, nl, bl, pv, rows, rec = eager[name]
        nb, npath = int(rec[4]), int(rec[2])
        assert nb <= cap and torch.equal(bufs["out"], pruned) and torch.equal(bufs["prec"], prec) and torch.equal(bufs["rec"], rec), name
        assert torch.equal(bufs["nl"], nl) and torch.equal(bufs["bl"], bl) and torch.equal(bufs["pv"][:npath], pv[:npath]), name
        assert torch.equal(bufs["rows"][:nb], rows[:nb]), name


def _host_graph_scores(pred, gt, thr, voxel, a, largest, factor):
    vp, vl = pred >= np.float32(thr), gt >= np.float32(thr)
    body = vp
    if largest:
        lab, k = ndimage.label(vp, structure=sk.S26)
        body = lab == 1 + int(np.argmax(np.bincount(lab.ravel())[1:]))
    out, pruned = {}, []
    for sfx, mask in (("", body), ("_gt", vl)):
        s = sk.skeletonize(mask)[0]
        d2 = gr.squared_edt(mask)
        p, rec = gr.prune(s, d2, factor)
        r = gr.analyse(p, d2, gr.world_lengths(a))["record"]
        out.update({"n_branches" + sfx: r["branches"], "n_nodes" + sfx: r["nodes"], "n_free_ends" + sfx: r["free_ends"],
                    "n_spurs_removed" + sfx: rec["branches"], "prune_rounds" + sfx: rec["rounds"], "length" + sfx: r["length"],
                    "min_radius" + sfx: float(r["d2_min"]) ** 0.5 * voxel if r["branches"] else float("nan")})
        pruned.append(p)
    out["length_ratio"] = out["length"] / out["length_gt"]
    out.update(voxel_size=voxel, threshold=thr)
    return out, pruned


def test_sweep_graph_scores_and_columns(golden):
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from nerf_for_angiography_amd.visualization.sweep import (GRAPH_METRICS, MESH_DISTANCE_METRICS, evaluation_sweep, grid_index_to_world,
                                                              reconstruction_graph_metrics)
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    n = 25
    voxel = 2.0 * 100.0 / (n - 1)
    a = grid_index_to_world(100.0, n)
    scores, pp, pl, graph_p, graph_l = reconstruction_graph_metrics(m, vol, 100.0, n)
    from nerf_for_angiography_amd.visualization.sweep import _reconstruction_grids
    pred, ref = _reconstruction_grids(m, vol, 100.0, n)
    thr = float(torch.mean(ref))
    want, (want_pp, want_pl) = _host_graph_scores(pred.cpu().numpy(), ref.cpu().numpy(), thr, voxel, a, False, 1.0)
    print(f"graph: got {scores}\n want {want}")
    assert scores.keys() == want.keys()
    for key in want:                                                                # integers, and fp64 from the same operations in the same order
        assert scores[key] == want[key] or (want[key] != want[key] and scores[key] != scores[key]), (key, scores[key], want[key])
    assert np.array_equal(pp.cpu().numpy(), want_pp) and np.array_equal(pl.cpu().numpy(), want_pl)
    assert graph_p["n_branches"] == scores["n_branches"] and scores["length_gt"] > 0.0 and scores["n_branches_gt"] >= 1
    only = reconstruction_graph_metrics(m, vol, 100.0, n, threshold=thr * 0.5, largest_component=True, prune_factor=2.0)[0]
    want1 = _host_graph_scores(pred.cpu().numpy(), ref.cpu().numpy(), thr * 0.5, voxel, a, True, 2.0)[0]
    for key in want1:
        assert only[key] == want1[key] or (want1[key] != want1[key] and only[key] != only[key]), (key, only[key], want1[key])
    df, _ = evaluation_sweep(m, gt, angles, *geo, metrics=["LENGTH RATIO 3D", "PSNR", "BRANCHES 3D", "HD MESH", "JUNCTIONS 3D", "CLDICE 3D"],
                             volume=vol, volume_outside=100.0, volume_points=n)
    assert list(df.columns) == BASE + ["PSNR", "CLDICE 3D", "HD MESH"] + list(GRAPH_METRICS)
    assert list(df.columns).index(MESH_DISTANCE_METRICS[1]) < list(df.columns).index(GRAPH_METRICS[0])
    for col, key in zip(GRAPH_METRICS, ("n_branches", "n_nodes", "length_ratio")):
        assert df[col].nunique() == 1 and df[col][0] == scores[key], col               # one value per column, repeated on every row


def test_driver_saves_the_centreline(tmp_path):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    driver = ["--synthetic", "--img_size", "16", "--num_layers", "4", "--num_hidden_units", "64", "--sample_size", "8", "--depth_samples", "32",
              "--n_iters", "4", "--display_every", "2", "--out_bias_init", "0.0"]      # (sigma ~ 0.5 everywhere: the 0.5 level is a real surface)
    plain = main(driver + ["--log_dir", str(tmp_path / "a")])
    assert "centreline_info" not in plain
    out = main(driver + ["--log_dir", str(tmp_path / "b"), "--save_centreline", str(tmp_path / "tree.vtk"), "--mesh_threshold", "0.5"])
    info = out["centreline_info"]
    assert torch.equal(out["model"].flat_params, plain["model"].flat_params)               # the flag changes nothing else
    text = open(info["path"]).read()
    assert info["path"] == str(tmp_path / "tree.vtk") and f"LINES {info['n_branches']} " in text and "SCALARS radius double 1" in text
    assert info["n_branches"] + info["n_nodes"] >= 1 and info["length"] >= 0.0
