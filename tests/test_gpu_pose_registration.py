"""The 2D-3D pose registration on the GPU (include/afx.h: afx_pose_chamfer, afx_pose_compose, afx_pose_select, afx_pose_lm_step): the
device against the NumPy restatement tests/pose_reference.py bit for bit - the cost kernel at ragged sizes and slice counts, the compose
and selection launches, and the whole registration eagerly, twice and replayed from a captured graph - then the Python layer, the sweep
family and the driver's --save_poses."""
import csv
import itertools

import numpy as np
import pytest
import torch

import pose_reference as pr
import viewmap_reference as vr
from nerf_for_angiography_amd import engine as eng

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(x, dtype=torch.float64):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV)


def _views(field):
    v, h, w = field.shape
    return dict(field=_dev(field), records=None, n_views=v, width=w, height=h)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.int64 if got.dtype == np.float64 else got.dtype) != want.view(np.int64 if want.dtype == np.float64 else want.dtype))
        raise AssertionError(f"{what}: {len(bad)} of {got.size} differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


def _field(n_views, width, height, seed):
    """A distance-like image per view with values on both sides of 0 and beyond the truncation (the kernel does not care what it holds)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    out = []
    for v in range(n_views):
        if width < 8:                                            # four pixels: values on either side of 0 and of the truncation
            out.append(1.5 + 3.0 * rng.standard_normal((height, width)))
            continue
        cx, cy = rng.uniform(0, width - 1), rng.uniform(0, height - 1)
        out.append(0.9 * np.abs((xx - cx) * np.cos(v + 0.3) + (yy - cy) * np.sin(v + 0.3)) - 1.5 + 0.25 * rng.standard_normal((height, width)))
    return np.stack(out)


def _edge_record(width, height):
    """R = I, the source at (0, 0, 64), f = 64: the point (W / 2 - 1, 0, 0) projects to u = W - 1 exactly, w = H / 2."""
    rec = np.zeros(16)
    rec[[0, 4, 8]], rec[9:12], rec[12] = 1.0, (0.0, 0.0, 64.0), 64.0
    return rec


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("width, height", [(2, 2), (17, 33), (64, 64)])
def test_chamfer_equals_the_restatement(width, height, n):
    """Sums and counts bit for bit, over S in {1, 3} (N = 257 with S = 3 leaves two slices empty), V in {1, 3} views with M in {1, 5}
    candidates each through rec_view, radii and weights null and given, cost-only and full; the views are the three special kinds of
    viewmap_reference.scene_views and an oblique one; one more record puts point 0 exactly on u = W - 1, and point 2 is NaN."""
    rng = np.random.RandomState(1000 * width + n)
    pts, rad, _ = pr.tree_points(n, min(3, n), 4)
    pts[0] = (width / 2 - 1.0, 0.0, 0.0)
    if n >= 3:
        pts[2] = np.nan
    wt = rng.uniform(0.25, 2.0, n)
    edge = _edge_record(width, height)
    on_edge = pr.residuals(np.zeros((height, width)), pts[:1], None, edge, 4.0)
    assert on_edge["u"][0] == width - 1.0 and on_edge["kind"][0] != 3      # on the last column, and not lost
    poses, focal = vr.scene_views(4, width, height, 0)
    all_rec = eng.hull_view_records(poses, focal)
    d_pts = _dev(pts)
    combos = itertools.product((1, 3), (1, 3), (1, 5), (False, True), (False, True))
    total = np.zeros(4, np.int64)
    for case, (s, v, m, given, cost_only) in enumerate(combos):
        pick = [(case + i) % 4 for i in range(v)]
        base = all_rec[pick]
        field = _field(v, width, height, 7 + case)
        xi = np.concatenate([np.zeros((1, 6)), np.concatenate([rng.uniform(-0.02, 0.02, (m - 1, 3)), rng.uniform(-1.0, 1.0, (m - 1, 3))], axis=1)])
        records = np.concatenate([pr.compose_outer(base, xi).reshape(-1, 16), edge[None]])
        rec_view = np.concatenate([np.repeat(np.arange(v), m), [0]]).astype(np.int32)
        r, w = (rad, wt) if given else (None, None)
        want_s, want_c = pr.chamfer(field, pts, r, w, records, rec_view, 4.0, s, pr.COST_ONLY if cost_only else 0)
        got_s, got_c = eng.pose_chamfer_record(_views(field), d_pts, _dev(r), _dev(w), _dev(records), _dev(rec_view, torch.int32), 4.0, s, cost_only)
        what = f"{width}x{height} N={n} S={s} V={v} M={m} given={given} cost_only={cost_only}"
        _same(got_c, want_c, "counts " + what)
        _same(got_s, want_s, "sums " + what)
        assert (want_c.sum(axis=(1, 2)) == n).all()
        total += want_c.sum(axis=(0, 1))
    print(f"{width}x{height} N={n}: active, satisfied, saturated, lost = {total.tolist()}")
    assert total[3] > 0 and (n == 1 or (total[:3] > 0).all())     # every kind of point was met (a single point: at least a lost one)


def test_chamfer_drops_a_record_with_a_bad_view():
    pts, rad, _ = pr.tree_points(300, 3, 4)
    poses, focal = vr.scene_views(4, 17, 33, 0)
    rec = eng.hull_view_records(poses, focal)
    field = _field(2, 17, 33, 3)
    rec_view = np.array([1, 2, -1, 0], np.int32)
    want_s, want_c = pr.chamfer(field, pts, rad, None, rec, rec_view, 4.0, 2)
    got_s, got_c = eng.pose_chamfer_record(_views(field), _dev(pts), _dev(rad), None, _dev(rec), _dev(rec_view, torch.int32), 4.0, 2)
    _same(got_c, want_c, "counts")
    _same(got_s, want_s, "sums")
    assert (want_c[1:3] == -1).all() and np.isinf(want_s[1:3, :, 0]).all() and (want_c[[0, 3]] >= 0).all()


def test_compose_and_select_equal_the_restatement():
    rng = np.random.RandomState(9)
    poses, focal = vr.scene_views(7, 64, 64, 1)
    rec = eng.hull_view_records(poses, focal)
    rec[2, [1, 10]] = -0.0
    xi = np.concatenate([rng.uniform(-0.3, 0.3, (7, 3)), rng.uniform(-5.0, 5.0, (7, 3))], axis=1)
    xi[2] = [0.0, -0.0, 0.0, 0.0, 0.0, -0.0]                     # the identity returns the record as it is, negative zeros included
    xi[3, :3] = 0.0                                              # a pure translation
    xi[4, 3:] = 0.0                                              # a pure rotation
    _same(eng.pose_compose(_dev(rec), _dev(xi)), np.stack([pr.compose(r, x) for r, x in zip(rec, xi)]), "compose, elementwise")
    _same(eng.pose_compose(_dev(rec), _dev(xi[:5]), outer=True), pr.compose_outer(rec, xi[:5]), "compose, outer")
    assert eng.pose_compose(_dev(rec), _dev(xi))[2].cpu().numpy().tobytes() == rec[2].tobytes()
    # selection: V = 3 views, M = 6 candidates, S = 3 slices; a tie resolved to the lowest index, a NaN never chosen, all equal -> 0
    sums = rng.uniform(1.0, 2.0, (3, 6, 3, 32))
    sums[0, 4], sums[0, 2] = sums[0, 1] * 0.25, sums[0, 1] * 0.25      # candidates 2 and 4 tie below the rest
    sums[1, 0, 1, 0] = np.nan
    sums[1, 3, :, 0] = 0.5
    sums[2] = sums[2, 0]
    cand = rng.uniform(-1, 1, (3, 6, 16))
    want, _ = pr.select(sums.reshape(18, 3, 32), 3, 6)
    assert want.tolist() == [2, 0, 0]      # (view 1: candidate 0 is NaN and nothing is < NaN: it stays - candidate 0 is the caller's identity)
    b = dict(sel=torch.full((3,), 9, dtype=torch.int32, device=DEV), out=torch.zeros(3, 16, dtype=torch.float64, device=DEV))
    from nerf_for_angiography_amd import _lib
    lib = _lib.load()
    d_sums, d_cand = _dev(sums), _dev(cand)
    _lib.check(lib.afx_pose_select(eng._ptr(d_sums), 3, 6, 3, eng._ptr(d_cand), eng._ptr(b["sel"]), eng._ptr(b["out"]), eng.Engine._stream(DEV)))
    _same(b["sel"], want, "selected")
    _same(b["out"], cand[np.arange(3), want], "selected records")


@pytest.fixture(scope="module")
def scene():
    """The scene of the CPU convergence test: wavy_tree(300, 3, 1), 5 oblique views of 64 x 64, poses perturbed at the smaller scale."""
    pts, rad, seg = pr.tree_points(300, 3, 1)
    poses, focal = pr.oblique_views(5, 64)
    rec = eng.hull_view_records(poses, focal)
    masks = pr.silhouettes(seg, rec, 64, 64)
    field = np.stack([pr.signed_field(m) for m in masks])
    pert = np.stack([pr.compose(r, x) for r, x in zip(rec, pr.perturbation(5, 11))])
    return dict(pts=pts, rad=rad, rec=rec, masks=masks, field=field, pert=pert, poses=poses, focal=focal)


@pytest.mark.parametrize("search", [False, True], ids=["lm", "search27"])
def test_registration_equals_the_restatement_twice_and_from_a_graph(scene, search):
    """5 views of 64 x 64, 300 points, 20 iterations, two slices (256 + 44 points); with `search` a 27-candidate grid first.  The final
    state (records, cost, g, H, lambda, the three counters, the trial), the start records and the selection equal the restatement's bit
    for bit; so does a second call into the same buffers and a replay of the captured launches."""
    offsets = eng.pose_search_offsets(1.0, 0.6, 3) if search else None
    want = pr.register(scene["field"], scene["pts"], scene["rad"], None, scene["pert"], 20, 8.0, offsets=offsets, n_slices=2)
    for v in range(5):
        err = pr.reprojection_error(scene["pts"], scene["rec"][v], want["records"][v], 64, 64)
        print(f"view {v}: candidate {want['selected'][v]}, {err:.4f} px, accepted {int(want['state'][v, pr.ST_ACCEPTED])}")
        assert err < 0.5
    views = _views(scene["field"])
    pts, rad, pert, off = _dev(scene["pts"]), _dev(scene["rad"]), _dev(scene["pert"]), _dev(offsets)
    buf = eng.register_poses_buffers(5, 27 if search else 0, 2, DEV)

    def check(what):
        _same(buf["state"], want["state"], "state, " + what)
        _same(buf["start"], want["start"], "start, " + what)
        _same(buf["selected"], want["selected"], "selected, " + what)
        _same(buf["trial_records"], want["records"], "trial_records, " + what)      # the last step is FINAL: the trial is the refined record

    def scrub():
        for t in buf.values():
            if t.dtype == torch.float64:
                t.fill_(float("nan"))
        buf["selected"].fill_(-3)

    run = lambda: eng.register_poses_record(views, pts, rad, None, pert, 20, 8.0, 63, off, 2, buffers=buf)
    scrub()
    run()
    check("first call")
    scrub()
    run()
    check("second call")
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


def test_python_layer_on_the_scene(scene):
    """pose_views builds the restatement's signed field; pose_chamfer and register_poses report what the restatement computes; the
    dof masks leave their part of the pose untouched."""
    masks = torch.from_numpy(scene["masks"]).to(DEV)
    views = eng.pose_views(scene["poses"], masks, scene["focal"])
    assert np.array_equal(views["field"].cpu().numpy(), scene["field"]) and np.array_equal(views["records"].cpu().numpy(), scene["rec"])
    unsigned = eng.pose_views(scene["poses"], masks, scene["focal"], signed=False)["field"].cpu().numpy()
    assert (unsigned >= 0).all() and np.array_equal(unsigned > 0, ~scene["masks"])
    views["records"] = _dev(scene["pert"])
    score = eng.pose_chamfer(scene["pts"], scene["rad"], views, trunc=8.0, n_slices=1)
    sums, counts = pr.chamfer(scene["field"], scene["pts"], scene["rad"], None, scene["pert"], np.arange(5), 8.0, 1, pr.COST_ONLY)
    assert np.array_equal(score["cost"], sums[:, 0, 0]) and np.array_equal(score["counts"], counts[:, 0])
    assert np.array_equal(score["mean_residual"], sums[:, 0, 1] / sums[:, 0, 2])
    reg = eng.register_poses(scene["pts"], scene["rad"], views, n_slices=2)
    want = pr.register(scene["field"], scene["pts"], scene["rad"], None, scene["pert"], 20, 8.0, n_slices=2)
    assert np.array_equal(reg["records"], want["records"]) and reg["poses"].shape == (5, 4, 4) and reg["n_slices"] == 2
    assert np.array_equal(reg["accepted"], want["state"][:, pr.ST_ACCEPTED].astype(np.int64)) and (reg["selected"] == 0).all()
    assert (reg["cost_after"] < reg["cost_before"]).all() and (reg["rms_residual_after"] < reg["rms_residual_before"]).all()
    assert (reg["singular"] == 0).all() and (reg["accepted"] + reg["rejected"] == 20).all()
    for v in range(5):
        assert abs(reg["shift_px"][v] - pr.reprojection_error(scene["pts"], scene["pert"][v], reg["records"][v], 64, 64)) < 1e-9
    print("mean residual before", reg["mean_residual_before"], "after", reg["mean_residual_after"], "shift", reg["shift_px"])
    inplane = eng.register_poses(scene["pts"], scene["rad"], views, dof="inplane", search=(1.0, 0.6, 3), iterations=5)
    assert (inplane["cost_after"] <= inplane["cost_before"]).all()
    moved = eng.register_poses(scene["pts"], scene["rad"], views, dof="translation", iterations=5)
    assert np.array_equal(moved["records"][:, :9], scene["pert"][:, :9]) and not np.array_equal(moved["records"][:, 9:12], scene["pert"][:, 9:12])
    with pytest.raises(ValueError, match="dof"):
        eng.register_poses(scene["pts"], scene["rad"], views, dof=64)


def test_sweep_pose_metrics_need_no_truth(golden):
    """The three columns on a tiny grid: the truth's own centreline scored against silhouettes rendered from the truth, with and without
    the ground-truth volume; the columns stand last, one value per column, equal to the function's."""
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    from nerf_for_angiography_amd.visualization import sweep
    g, vol, m, gt, angles, geo = _sweep_setup(golden)
    w, h, focal, src = geo[:4]
    n = 25
    truth = sweep.ground_truth_grid(vol, 100.0, n)
    imgs = gt.reshape(len(angles), h, w).to(DEV)
    level = 0.5 * (imgs.amin(dim=(1, 2), keepdim=True) + imgs.amax(dim=(1, 2), keepdim=True))
    masks = imgs < level
    poses = sweep._poses(angles, src, (0.0, 0.0, 0.0), "cpu").numpy()
    views = eng.pose_views(poses[:4], masks[:4], focal)
    thr = float(torch.mean(truth))
    scores, reg = sweep.reconstruction_pose_metrics(None, vol, 100.0, n, views, grids=(truth, truth))
    print(f"truth against its own views: {scores}")
    assert scores["n_points"] > 0 and scores["threshold"] == thr and reg["records"].shape == (4, 16)
    assert np.isfinite([scores["chamfer"], scores["chamfer_refined"], scores["pose_shift"]]).all() and scores["chamfer"] >= 0
    assert (reg["rms_residual_after"] <= reg["rms_residual_before"]).all()
    blind, _ = sweep.reconstruction_pose_metrics(None, None, 100.0, n, views, threshold=thr, grids=(truth, None))      # volume=None works
    assert blind == scores
    with pytest.raises(ValueError, match="pose_views"):
        sweep.evaluation_sweep(m, gt, angles, *geo, metrics=["PSNR", "CHAMFER 2D"])
    df, _ = sweep.evaluation_sweep(m, gt, angles, *geo, metrics=["POSE SHIFT 2D", "PSNR", "CHAMFER 2D", "CHAMFER 2D REFINED"], pose_views=views,
                                   pose_threshold=0.5, volume_outside=100.0, volume_points=n)
    assert list(df.columns) == BASE + ["PSNR"] + list(sweep.POSE_METRICS)
    ref = sweep.reconstruction_pose_metrics(m, None, 100.0, n, views, threshold=0.5)[0]
    print(f"model, no truth: {ref}")
    for col, key in zip(sweep.POSE_METRICS, ("chamfer", "chamfer_refined", "pose_shift")):
        v = df[col].to_numpy()
        assert len(v) == len(angles) and ((v == ref[key]).all() or (np.isnan(v).all() and ref[key] != ref[key])), col


def test_driver_saves_the_poses(tmp_path):
    """--save_poses on a short --synthetic --pose_noise run: one well-formed CSV row per training view, the given poses the perturbed
    ones, the root-mean-square chamfer (what the registration minimises) never above the given one; the flag changes nothing else."""
    from nerf_for_angiography_amd.nerf.run_nerf_acc import POSE_CSV_COLUMNS, main
    driver = ["--synthetic", "--binary", "True", "--img_size", "16", "--num_layers", "4", "--num_hidden_units", "64", "--sample_size", "8",
              "--depth_samples", "32", "--n_iters", "4", "--display_every", "2", "--out_bias_init", "0.0", "--pos_enc", "fourier", "--pose_noise",
              "0.3", "2.0"]
    plain = main(driver + ["--log_dir", str(tmp_path / "a")])
    assert "pose_info" not in plain
    out = main(driver + ["--log_dir", str(tmp_path / "b"), "--save_poses", str(tmp_path / "poses.csv"), "--mesh_threshold", "0.5", "--pose_search",
                         "0.5", "2.0", "3"])
    assert torch.equal(out["model"].flat_params, plain["model"].flat_params)
    info = out["pose_info"]
    rows = list(csv.reader(open(info["path"])))
    assert tuple(rows[0]) == POSE_CSV_COLUMNS and info["n_points"] > 0 and len(rows) == 1 + info["n_views"] and info["n_views"] >= 2
    col = {name: i for i, name in enumerate(rows[0])}
    body = np.array([[float(x) for x in r] for r in rows[1:]])
    assert np.isfinite(body).all() and len(set(body[:, 0])) == info["n_views"]
    assert (body[:, col["rms_after"]] <= body[:, col["rms_before"]]).all() and (body[:, col["chamfer_before"]] >= 0).all()
    assert (body[:, col["shift_px"]] >= 0).all() and (body[:, col["selected"]] < 27).all()
    for r in body:
        rot = r[col["refined_00"]:col["refined_00"] + 12].reshape(3, 4)[:, :3]
        assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-12
    print("poses", info)
