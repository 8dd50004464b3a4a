"""The territories on the CPU (include/afx.h: afx_feature_transform_3d, afx_label_overlap_3d): the library's symbols and their argument
refusals, the host-side pieces of the engine, the sweep and the driver, and the NumPy restatement tests/territory_reference.py against
SciPy and on three hand-built scenes.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import territory_reference as tr
from nerf_for_angiography_amd import _lib, engine

AFX_E_INVALID = -1
FAKE = C.c_void_p(0x1000)      # never dereferenced: every refusal below comes before the device is touched
NAMES = ("afx_feature_transform_3d", "afx_label_overlap_3d")
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "afx.h")).read()
C_TYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64}
SHAPES = [(1, 1, 1), (1, 1, 70), (1, 1, 129), (5, 1, 3), (7, 9, 11), (3, 40, 5), (2, 3, 33), (3, 5, 17), (520, 2, 3), (2, 520, 3)]


def test_library_exports_both_symbols_and_the_header_agrees_with_the_ctypes_table():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.exported_symbols() and getattr(lib, name) is not None
        proto = re.search(rf"\nint {name}\((.*?)\);", HEADER, re.S)
        assert proto is not None, name
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",")]
        res, args = _lib._SIGS[name]
        assert res is C.c_int and len(params) == len(args), (name, params)
        for p, t in zip(params, args):
            want = C.c_void_p if "*" in p else C_TYPES[p.split()[0]]
            assert t is want, (name, p, t)
            assert p.split()[-1].lstrip("*") != "workspace"                          # every scratch buffer is a named, fully defined output
    assert "#define AFX_LABEL_OVERLAP_MAX_LABELS 4095\n" in HEADER and engine.LABEL_OVERLAP_MAX_LABELS == 4095
    assert "#define AFX_EDT3D_NONE 0xffffffffu\n" in HEADER and engine.EDT3D_NONE == tr.NONE == 0xffffffff


def _ft(lib, **kw):
    a = dict(sites=FAKE, n0=4, n1=5, n2=6, d2=FAKE, nearest=FAKE)
    a.update(kw)
    return lib.afx_feature_transform_3d(a["sites"], a["n0"], a["n1"], a["n2"], a["d2"], a["nearest"], None), lib.afx_last_error().decode()


def _ov(lib, **kw):
    a = dict(labels=FAKE, index=FAKE, d2=FAKE, max_d2=9, a=FAKE, b=FAKE, n=100, n_labels=3, counts=FAKE, territory=FAKE)
    a.update(kw)
    rc = lib.afx_label_overlap_3d(a["labels"], a["index"], a["d2"], a["max_d2"], a["a"], a["b"], a["n"], a["n_labels"], a["counts"], a["territory"],
                                  None)
    return rc, lib.afx_last_error().decode()


REFUSALS = [
    (_ft, dict(sites=None), "sites"), (_ft, dict(d2=None), "d2"), (_ft, dict(nearest=None), "nearest"),
    (_ft, dict(n0=0), "1..1024"), (_ft, dict(n1=0), "1..1024"), (_ft, dict(n2=0), "1..1024"), (_ft, dict(n0=1025), "1..1024"),
    (_ft, dict(n1=1025), "1..1024"), (_ft, dict(n2=1025), "1..1024"), (_ft, dict(n2=-3), "1..1024"),
    (_ov, dict(labels=None), "labels"), (_ov, dict(a=None), "null a"), (_ov, dict(counts=None), "counts"), (_ov, dict(n=-1), "n must"),
    (_ov, dict(n=2 ** 40 + 1), "n must"), (_ov, dict(n_labels=-1), "n_labels"), (_ov, dict(n_labels=4096), "n_labels"),
]


@pytest.mark.parametrize("call, kw, word", REFUSALS, ids=[f"{c.__name__}-{'-'.join(k)}:{n}" for n, (c, k, w) in enumerate(REFUSALS)])
def test_entry_points_refuse_before_any_device_call(call, kw, word):
    rc, msg = call(_lib.load(), **kw)
    assert rc == AFX_E_INVALID and msg.startswith("afx_") and word in msg, msg


def test_engine_has_no_cpu_path_and_checks_its_arguments():
    vol = torch.zeros(3, 4, 5, dtype=torch.uint8)
    for call in (lambda: engine.feature_transform_3d(vol), lambda: engine.feature_transform_record(vol),
                 lambda: engine.label_overlap_3d(vol.int(), vol), lambda: engine.label_overlap_record(vol.int(), vol, 3)):
        with pytest.raises(engine.AfxError, match="no CPU path"):
            call()


def test_sweep_names_and_checks():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.BRANCH_METRICS == ("BRANCH RECALL 3D", "WORST BRANCH DICE 3D", "BRANCH RADIUS ERR 3D")
    for names, _, _ in sweep._VOLUME_FAMILIES:                  # a tuple of its own, in no family
        assert not set(sweep.BRANCH_METRICS) & set(names)
    with pytest.raises(ValueError, match="ground-truth volume"):
        sweep._check_metrics(["PSNR", "BRANCH RECALL 3D"], None, None)
    with pytest.raises(ValueError, match="ground-truth volume"):
        sweep.evaluation_sweep(None, None, sweep.sweep_angles(40, 20), 8, 8, 100.0, (0, 0, 1500.0), 1400.0, 1600.0, 8,
                               metrics=list(sweep.BRANCH_METRICS))
    got = sweep._check_metrics(["WORST BRANCH DICE 3D", "PSNR", "BRANCH RECALL 3D", "CLDICE 3D"], None, object())
    assert got == ["PSNR", "CLDICE 3D", "BRANCH RECALL 3D", "WORST BRANCH DICE 3D"]      # behind every column there was before
    old = ["PSNR", "SSIM", "DICE 3D", "HD95 3D", "BRANCHES 3D", "CPR SSIM 3D"]
    assert sweep._check_metrics(list(reversed(old)), None, object()) == old


def test_driver_checks_the_flag():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import BRANCH_CSV_COLUMNS, build_parser, check_args, save_branches
    parse = lambda *extra: build_parser().parse_args(["--synthetic", *extra])
    assert parse().save_branches is None and BRANCH_CSV_COLUMNS[:3] == ("label", "kind", "territory_voxels")
    check_args(parse("--save_branches", "branches.csv"))
    with pytest.raises(ValueError, match="--save_branches"):
        check_args(parse("--save_branches", "branches.txt"))
    with pytest.raises(ValueError, match="--mesh_threshold"):
        check_args(parse("--save_branches", "branches.csv", "--mesh_threshold", "0"))
    with pytest.raises(ValueError, match="--save_branches"):
        save_branches(None, 100.0, 9, 0.5, "branches.txt")


# ---- the restatement ----
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_restated_d2_is_scipys_squared_edt(shape):
    rng = np.random.RandomState(sum(shape))
    for density in (0.05, 0.5):
        sites = rng.rand(*shape) < density
        if not sites.any():
            sites.reshape(-1)[rng.randint(sites.size)] = True
        d2, nearest = tr.feature_transform(sites)
        dist, idx = ndimage.distance_transform_edt(~sites, return_indices=True)
        assert np.array_equal(d2, np.rint(dist ** 2).astype(np.int64))
        coords = np.stack(np.unravel_index(nearest, shape))                         # the named site is a site at that distance
        assert sites[tuple(coords)].all() and np.array_equal(((np.indices(shape) - coords) ** 2).sum(0), d2)
        assert np.array_equal(((np.indices(shape) - idx) ** 2).sum(0), d2)          # SciPy's sites lie as far, whichever tie they take
        assert np.array_equal(nearest[sites], np.flatnonzero(sites))
    none = tr.feature_transform(np.zeros(shape, bool))
    assert (none[0] == tr.NONE).all() and (none[1] == -1).all()


def test_restated_ties_go_to_the_lowest_index():
    s = np.zeros((5, 5, 5), bool)
    s[0, 2, 2] = s[4, 2, 2] = s[2, 0, 2] = s[2, 4, 2] = s[2, 2, 0] = s[2, 2, 4] = True
    d2, nearest = tr.feature_transform(s)
    assert d2[2, 2, 2] == 4 and nearest[2, 2, 2] == np.ravel_multi_index((0, 2, 2), s.shape)


def test_restated_overlap_rows():
    labels = np.array([0, 1, 2, 5, -1, 2, 1, 3], np.int32)
    a = np.array([1, 1, 0, 1, 1, 1, 0, 1], np.uint8)
    b = np.array([1, 0, 0, 1, 0, 1, 1, 1], np.uint8)
    counts, terr = tr.label_overlap(labels, a, b, n_labels=3)
    assert terr.tolist() == [0, 1, 2, 0, 0, 2, 1, 3]
    assert counts.tolist() == [[3, 3, 2, 2], [2, 1, 1, 0], [2, 1, 1, 1], [1, 1, 1, 1]]
    index = np.array([1, 1, -1, 2, 7, 8, 0, 5], np.int32)
    d2 = np.array([4, 5, 0, 3, 4, 0, 0, tr.NONE], np.int64)
    counts, terr = tr.label_overlap(labels, a, None, index, d2, 4, 3)
    assert terr.tolist() == [1, 0, 0, 2, 3, 0, 0, 0] and counts[:, 2:].sum() == 0 and counts[:, 0].sum() == 8


@pytest.fixture(scope="module")
def truth():
    mask = tr.y_truth()
    return mask, tr.tree(mask, tr_index_to_world())


def tr_index_to_world():
    from nerf_for_angiography_amd.visualization.sweep import grid_index_to_world
    return grid_index_to_world(tr.OUTSIDE, tr.N)


def test_scene_pred_equals_truth(truth):
    mask, tree = truth
    scores, table, terr = tr.branch_table(mask, mask, tree, tree)
    nb = scores["n_branches"]
    assert nb == 3 and scores["n_junctions"] == 1
    assert scores["branch_recall"] == 1.0 and scores["branch_recall_length"] == 1.0 and scores["worst_branch_dice"] == 1.0
    assert table["dice"] == [1.0] * 4 and table["coverage"] == [1.0] * 4 and table["offset"] == [0.0] * 4
    assert scores["branch_radius_err"] == 0.0 and scores["unassigned"] == 0.0 and table["radius_pred"] == table["radius_true"]
    assert sum(table["n_gt"]) == int(mask.sum()) and (terr[mask] > 0).all()


@pytest.mark.parametrize("branch", [1, 2, 3])
def test_scene_one_branch_removed(truth, branch):
    mask, tree = truth
    pred = tr.without_branch(mask, tree, branch)
    scores, table, _ = tr.branch_table(pred, mask, tr.tree(pred, tr_index_to_world()), tree)
    assert scores["branch_recall"] == 2.0 / 3.0 and scores["worst_branch_dice"] == 0.0 and scores["n_found"] == 2
    assert table["dice"][branch - 1] == 0.0 and table["coverage"][branch - 1] == 0.0 and not table["found"][branch - 1]
    assert all(table["dice"][l] == 1.0 and table["found"][l] for l in range(3) if l != branch - 1)
    assert scores["branch_recall_length"] == pytest.approx(1.0 - table["length"][branch - 1] / sum(table["length"]), abs=1e-15)


def test_scene_truth_dilated(truth):
    mask, tree = truth
    pred = tr.dilated(mask)
    scores, table, _ = tr.branch_table(pred, mask, tr.tree(pred, tr_index_to_world()), tree)
    assert scores["branch_recall"] == 1.0 and table["coverage"][:3] == [1.0] * 3 and table["sensitivity"][:3] == [1.0] * 3
    assert all(table["radius_pred"][l] > table["radius_true"][l] for l in range(3))
    assert scores["branch_radius_err"] > 0 and 0 < scores["worst_branch_dice"] < 1 and all(p < 1 for p in table["precision"][:3])


def test_branch_scores_on_the_host_equal_the_restatement(truth):
    """sweep.branch_scores, fed with the restatement's own counts, gives the restatement's table: the host arithmetic is pinned without a GPU."""
    from nerf_for_angiography_amd.visualization.sweep import branch_scores
    mask, tree = truth
    pred = tr.without_branch(tr.dilated(mask), tree, 2)
    tree_p = tr.tree(pred, tr_index_to_world())
    want, table, _ = tr.branch_table(pred, mask, tree_p, tree)
    labels, nb, nk = tr.site_labels(tree["graph"])
    d2, nearest = tr.feature_transform(labels > 0)
    counts = tr.label_overlap(labels, pred, mask, nearest, None, None, nb + nk)[0]
    cover = tr.label_overlap(labels, pred, None, None, None, None, nb + nk)[0]
    vox = np.flatnonzero(labels)
    d2_off, near_p = tr.feature_transform(tree_p["pruned"])
    got, rows = branch_scores(counts, cover, nb, [r["length"] for r in tree["graph"]["branches"]], labels.reshape(-1)[vox], d2_off.reshape(-1)[vox],
                              tree["d2"].reshape(-1)[vox], tree_p["d2"].reshape(-1)[near_p.reshape(-1)[vox]])
    for key, value in want.items():
        assert got[key] == value or (value != value and got[key] != got[key]), key
    for key, col in table.items():
        assert np.array_equal(np.asarray(rows[key], np.float64), np.asarray(col, np.float64), equal_nan=True), key
