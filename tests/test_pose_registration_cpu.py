"""The 2D-3D pose registration on the CPU: the library's symbols and their argument refusals, the host-side pieces of the engine, the sweep,
the dataset and the driver, and properties of the NumPy restatement tests/pose_reference.py (include/afx.h: afx_pose_chamfer,
afx_pose_compose, afx_pose_select, afx_pose_lm_step).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import pose_reference as pr
from nerf_for_angiography_amd import _lib, engine

AFX_E_INVALID = -1
FAKE = C.c_void_p(0x1000)      # never dereferenced: every refusal below comes before the device is touched
NAMES = ("afx_pose_chamfer", "afx_pose_compose", "afx_pose_select", "afx_pose_lm_step")
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "afx.h")).read()


def test_library_exports_the_symbols():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.exported_symbols() and getattr(lib, name) is not None and f"int {name}(" in HEADER
    assert "#define AFX_POSE_SUM_DOUBLES 32" in HEADER and engine.POSE_SUM_DOUBLES == pr.SUM_DOUBLES == 32
    assert "#define AFX_POSE_STATE_DOUBLES 64" in HEADER and engine.POSE_STATE_DOUBLES == pr.STATE_DOUBLES == 64
    assert "#define AFX_POSE_COST_ONLY 1u" in HEADER and engine.POSE_COST_ONLY == pr.COST_ONLY == 1
    for name, value in (("INIT", pr.LM_INIT), ("UPDATE", pr.LM_UPDATE), ("FINAL", pr.LM_FINAL)):
        assert f"#define AFX_POSE_LM_{name} {value}" in HEADER
    assert (engine.POSE_LM_INIT, engine.POSE_LM_UPDATE, engine.POSE_LM_FINAL) == (pr.LM_INIT, pr.LM_UPDATE, pr.LM_FINAL)
    for name, value in (("RECORD", pr.ST_RECORD), ("COST", pr.ST_COST), ("G", pr.ST_G), ("H", pr.ST_H), ("LAMBDA", pr.ST_LAMBDA),
                        ("ACCEPTED", pr.ST_ACCEPTED), ("REJECTED", pr.ST_REJECTED), ("SINGULAR", pr.ST_SINGULAR), ("TRIAL", pr.ST_TRIAL)):
        assert f"#define AFX_POSE_ST_{name} {value}\n" in HEADER
    assert (engine.POSE_ST_COST, engine.POSE_ST_LAMBDA, engine.POSE_ST_ACCEPTED, engine.POSE_ST_REJECTED, engine.POSE_ST_SINGULAR,
            engine.POSE_ST_TRIAL) == (pr.ST_COST, pr.ST_LAMBDA, pr.ST_ACCEPTED, pr.ST_REJECTED, pr.ST_SINGULAR, pr.ST_TRIAL)


def test_no_prototype_carries_a_workspace():
    """Every scratch buffer of the four entry points is a named, fully defined output: none has a parameter called workspace."""
    for name in NAMES:
        proto = re.search(rf"\nint {name}\((.*?)\);", HEADER, re.S)
        assert proto is not None and "workspace" not in proto.group(1), name


def _chamfer(lib, **kw):
    a = dict(field=FAKE, v=3, w=8, h=8, points=FAKE, radius=FAKE, weight=FAKE, n=5, records=FAKE, rec_view=FAKE, k=3, trunc=8.0, s=1, flags=0,
             sums=FAKE, counts=FAKE)
    a.update(kw)
    rc = lib.afx_pose_chamfer(a["field"], a["v"], a["w"], a["h"], a["points"], a["radius"], a["weight"], a["n"], a["records"], a["rec_view"],
                              a["k"], a["trunc"], a["s"], a["flags"], a["sums"], a["counts"], None)
    return rc, lib.afx_last_error().decode()


def _compose(lib, **kw):
    a = dict(records=FAKE, r=3, xi=FAKE, m=0, out=FAKE)
    a.update(kw)
    return lib.afx_pose_compose(a["records"], a["r"], a["xi"], a["m"], a["out"], None), lib.afx_last_error().decode()


def _select(lib, **kw):
    a = dict(sums=FAKE, v=3, m=5, s=1, cand=FAKE, selected=FAKE, out=FAKE)
    a.update(kw)
    return lib.afx_pose_select(a["sums"], a["v"], a["m"], a["s"], a["cand"], a["selected"], a["out"], None), lib.afx_last_error().decode()


def _lm_step(lib, **kw):
    a = dict(state=FAKE, v=3, sums=FAKE, s=1, phase=0, dof=63, lam=1e-3, rec=FAKE, trial=FAKE)
    a.update(kw)
    rc = lib.afx_pose_lm_step(a["state"], a["v"], a["sums"], a["s"], a["phase"], a["dof"], a["lam"], a["rec"], a["trial"], None)
    return rc, lib.afx_last_error().decode()


nan, inf = float("nan"), float("inf")
REFUSALS = [
    (_chamfer, dict(field=None), "field"), (_chamfer, dict(points=None), "points"), (_chamfer, dict(records=None), "records"),
    (_chamfer, dict(rec_view=None), "rec_view"), (_chamfer, dict(sums=None), "sums"), (_chamfer, dict(counts=None), "counts"),
    (_chamfer, dict(n=0), "n_points"), (_chamfer, dict(n=-2), "n_points"), (_chamfer, dict(k=0), "n_records"), (_chamfer, dict(k=65536), "n_records"),
    (_chamfer, dict(v=0), "n_views"), (_chamfer, dict(s=0), "n_slices"), (_chamfer, dict(s=-1), "n_slices"), (_chamfer, dict(w=1), "width"),
    (_chamfer, dict(h=1), "height"), (_chamfer, dict(w=0), "width"), (_chamfer, dict(trunc=0.0), "trunc"), (_chamfer, dict(trunc=-1.0), "trunc"),
    (_chamfer, dict(trunc=nan), "trunc"), (_chamfer, dict(trunc=inf), "trunc"), (_chamfer, dict(flags=2), "flags"),
    (_compose, dict(records=None), "records"), (_compose, dict(xi=None), "xi"), (_compose, dict(out=None), "out"), (_compose, dict(r=0), "n_records"),
    (_compose, dict(m=-1), "n_xi"),
    (_select, dict(sums=None), "sums"), (_select, dict(selected=None), "selected"), (_select, dict(cand=None), "cand_records"),
    (_select, dict(v=0), "n_views"), (_select, dict(m=0), "n_candidates"), (_select, dict(s=0), "n_slices"),
    (_lm_step, dict(state=None), "state"), (_lm_step, dict(sums=None), "sums"), (_lm_step, dict(trial=None), "trial_records"),
    (_lm_step, dict(rec=None), "records_in"), (_lm_step, dict(v=0), "n_views"), (_lm_step, dict(s=0), "n_slices"), (_lm_step, dict(phase=3), "phase"),
    (_lm_step, dict(phase=-1), "phase"), (_lm_step, dict(dof=64), "dof_mask"), (_lm_step, dict(lam=0.0), "lambda0"), (_lm_step, dict(lam=nan), "lambda0"),
]


@pytest.mark.parametrize("call, kw, word", REFUSALS, ids=[f"{c.__name__}-{'-'.join(k)}:{w}:{n}" for n, (c, k, w) in enumerate(REFUSALS)])
def test_entry_points_refuse(call, kw, word):
    rc, msg = call(_lib.load(), **kw)
    assert rc == AFX_E_INVALID and msg.startswith("afx_pose" + call.__name__) and word in msg, msg


def test_engine_has_no_cpu_path_and_checks_its_arguments():
    views = dict(field=torch.zeros(1, 4, 4, dtype=torch.float64), records=torch.zeros(1, 16, dtype=torch.float64), n_views=1, width=4, height=4)
    pts = np.zeros((3, 3))
    for call in (lambda: engine.pose_chamfer(pts, None, views), lambda: engine.register_poses(pts, None, views),
                 lambda: engine.pose_compose(torch.zeros(1, 16, dtype=torch.float64), torch.zeros(1, 6, dtype=torch.float64)),
                 lambda: engine.pose_chamfer_record(views, pts, None, None, views["records"], torch.zeros(1, dtype=torch.int32), 8.0)):
        with pytest.raises(engine.AfxError, match="no CPU path"):
            call()
    assert engine.POSE_DOF == {"all": 63, "rotation": 7, "translation": 56, "inplane": 28}


def test_search_offsets():
    off = engine.pose_search_offsets(2.0, 1.5, 3)
    assert off.shape == (27, 6) and off.dtype == np.float64 and (off[0] == 0.0).all() and (off[:, [0, 1, 5]] == 0.0).all()
    assert len({tuple(r) for r in off}) == 27 and np.isclose(np.abs(off[:, 2]).max(), np.tan(np.deg2rad(1.0)))
    assert sorted(set(off[:, 3])) == [-1.5, 0.0, 1.5] and sorted(set(off[:, 4])) == [-1.5, 0.0, 1.5]
    assert engine.pose_search_offsets(0.0, 0.0, 1).tolist() == [[0.0] * 6]
    for bad in ((1.0, 1.0, 2), (1.0, 1.0, 0), (-1.0, 1.0, 3), (1.0, float("nan"), 3), (180.0, 1.0, 3)):
        with pytest.raises(ValueError, match="pose_search_offsets"):
            engine.pose_search_offsets(*bad)
    assert engine.pose_default_slices(300, 5) == 2 and engine.pose_default_slices(100, 5) == 1 and engine.pose_default_slices(10 ** 6, 1) == 64
    assert engine.pose_default_slices(2000, 18225) == 1


def test_sweep_names_and_checks():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.POSE_METRICS == ("CHAMFER 2D", "CHAMFER 2D REFINED", "POSE SHIFT 2D")
    for names, _, _ in sweep._VOLUME_FAMILIES:                  # a tuple of its own, in no family
        assert not set(sweep.POSE_METRICS) & set(names)
    with pytest.raises(ValueError, match="pose_views"):
        sweep._check_metrics(["PSNR", "CHAMFER 2D"], None, object())
    with pytest.raises(ValueError, match="pose_views"):
        sweep.evaluation_sweep(None, None, sweep.sweep_angles(40, 20), 8, 8, 100.0, (0, 0, 1500.0), 1400.0, 1600.0, 8, metrics=["POSE SHIFT 2D"])
    with pytest.raises(ValueError, match="pose_threshold"):
        sweep._check_metrics(["CHAMFER 2D"], None, None, pose_views={})
    got = sweep._check_metrics(["POSE SHIFT 2D", "PSNR", "CHAMFER 2D"], None, None, pose_views={}, pose_threshold=0.5)      # no truth needed
    assert got == ["PSNR", "CHAMFER 2D", "POSE SHIFT 2D"]
    with pytest.raises(ValueError, match="threshold"):
        sweep.reconstruction_pose_metrics(None, None, 100.0, 9, {})


def _args(*extra):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser
    return build_parser().parse_args(["--synthetic", *extra])


def test_driver_checks_the_pose_flags():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import check_args
    a = _args()
    assert a.save_poses is None and a.pose_dof == "all" and a.pose_trunc == 8.0 and a.pose_search is None and a.pose_noise is None
    check_args(_args("--binary", "True", "--save_poses", "poses.csv", "--pose_dof", "inplane", "--pose_search", "1", "2", "3", "--pose_noise", "0.5", "1"))
    with pytest.raises(ValueError, match="--save_poses: needs --binary True"):
        check_args(_args("--save_poses", "poses.csv"))
    with pytest.raises(ValueError, match="--save_poses"):
        check_args(_args("--binary", "True", "--save_poses", "poses.txt"))
    with pytest.raises(ValueError, match="--pose_trunc"):
        check_args(_args("--binary", "True", "--save_poses", "poses.csv", "--pose_trunc", "0"))
    with pytest.raises(ValueError, match="--pose_search"):
        check_args(_args("--binary", "True", "--save_poses", "poses.csv", "--pose_search", "1", "1", "2"))
    with pytest.raises(ValueError, match="--pose_search: needs --save_poses"):
        check_args(_args("--pose_search", "1", "1", "3"))
    with pytest.raises(ValueError, match="--mesh_threshold"):
        check_args(_args("--binary", "True", "--save_poses", "poses.csv", "--mesh_threshold", "0"))
    with pytest.raises(ValueError, match="--pose_noise"):
        check_args(_args("--pose_noise", "-1", "0"))
    plain = _args("--pose_noise", "1", "1")
    plain.synthetic = False
    with pytest.raises(ValueError, match="--pose_noise: needs --synthetic"):
        check_args(plain)


def test_pose_noise_none_is_todays_dataset_and_noise_moves_only_the_poses():
    from nerf_for_angiography_amd.phantomdata import dataset as ds
    angles = ds.angle_grid(60.0, 1, (90, 0))
    base_p, base_r = ds.make_synthetic_dataset(angles, img_size=8, depth_samples_per_ray=8, seed=3)
    none_p, none_r = ds.make_synthetic_dataset(angles, img_size=8, depth_samples_per_ray=8, seed=3, pose_noise=None)
    assert base_p.equals(none_p) and base_r.equals(none_r)
    assert base_p.to_csv(sep=";") == none_p.to_csv(sep=";") and base_r.to_csv(sep=";") == none_r.to_csv(sep=";")
    assert (base_p["tform_cam2world"] == base_p["unshifted_tform_cam2world"]).all()
    noisy_p, noisy_r = ds.make_synthetic_dataset(angles, img_size=8, depth_samples_per_ray=8, seed=3, pose_noise=(0.5, 2.0))
    again_p, _ = ds.make_synthetic_dataset(angles, img_size=8, depth_samples_per_ray=8, seed=3, pose_noise=(0.5, 2.0))
    assert noisy_p.equals(again_p)                               # seeded
    assert (noisy_p["unshifted_tform_cam2world"] == base_p["tform_cam2world"]).all()
    assert (noisy_p["image_data"] == base_p["image_data"]).all() and noisy_r["pixel_value"].equals(base_r["pixel_value"])
    for given, true in zip(noisy_p["tform_cam2world"], noisy_p["unshifted_tform_cam2world"]):
        given, true = np.asarray(given), np.asarray(true)
        assert not np.array_equal(given, true) and np.abs(given[:3, :3] @ given[:3, :3].T - np.eye(3)).max() < 1e-14
        assert 0 < np.linalg.norm(given[:3, 3] - true[:3, 3]) <= 2.0 * np.sqrt(3) + 1e-9
        assert np.rad2deg(np.arccos(np.clip((np.trace(given[:3, :3].T @ true[:3, :3]) - 1) / 2, -1, 1))) <= 0.5 * np.sqrt(3) + 1e-6
    assert not noisy_r["ray_origins_x"].equals(base_r["ray_origins_x"])
    zero_p, zero_r = ds.make_synthetic_dataset(angles, img_size=8, depth_samples_per_ray=8, seed=3, pose_noise=(0.0, 0.0))
    assert np.allclose(np.asarray(zero_p["tform_cam2world"].tolist()), np.asarray(base_p["tform_cam2world"].tolist()), atol=0, rtol=0)
    with pytest.raises(ValueError, match="pose_noise"):
        ds.make_synthetic_dataset(angles, img_size=8, depth_samples_per_ray=8, pose_noise=(-1.0, 0.0))


# ---- properties of the restatement ----
W = 64


@pytest.fixture(scope="module")
def scene():
    """viewmap_reference.wavy_tree(300, 3, 1) with its radii, 5 oblique views of 64 x 64 at distance 60, focal 2.4 W; the silhouettes
    are the tree's capsules rasterised at the true poses."""
    pts, rad, seg = pr.tree_points(300, 3, 1)
    poses, focal = pr.oblique_views(5, W)
    rec = engine.hull_view_records(poses, focal)
    field = np.stack([pr.signed_field(m) for m in pr.silhouettes(seg, rec, W, W)])
    return pts, rad, rec, field


def test_compose_keeps_the_rotation_orthonormal_and_zero_is_the_identity(scene):
    rec = scene[2]
    rng = np.random.RandomState(5)
    worst = 0.0
    for r in rec:
        for scale in (1e-3, 0.05, 0.8, 3.0):
            out = pr.compose(r, rng.uniform(-scale, scale, 6))
            rot = out[:9].reshape(3, 3)
            worst = max(worst, np.abs(rot @ rot.T - np.eye(3)).max())
            assert out[12] == r[12]
        assert pr.compose(r, np.zeros(6)).tobytes() == r.tobytes()
        neg = r.copy()
        neg[[1, 10]] = -0.0                                      # a negative zero survives: the record is returned, not multiplied by I
        assert pr.compose(neg, np.array([0.0, -0.0, 0.0, 0.0, 0.0, -0.0])).tobytes() == neg.tobytes()
    print(f"compose: |R R^T - I| <= {worst:.3g}")
    assert worst <= 1e-14


def test_compose_moves_camera_coordinates_as_stated(scene):
    """q' = C(a) q + t: the camera coordinates of a point under the composed record."""
    pts, _, rec, _ = scene
    xi = np.array([0.02, -0.01, 0.03, 0.4, -0.3, 0.7])
    a, t = xi[:3], xi[3:]
    ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    cay = ((1 - a @ a) * np.eye(3) + 2 * np.outer(a, a) + 2 * ax) / (1 + a @ a)
    out = pr.compose(rec[0], xi)
    q = (pts - rec[0, 9:12]) @ rec[0, :9].reshape(3, 3)
    q_new = (pts - out[9:12]) @ out[:9].reshape(3, 3)
    assert np.abs(q_new - (q @ cay.T + t)).max() <= 1e-12


def test_jacobian_rows_agree_with_central_differences(scene):
    """On interior active points (the bilinear cell the same at both ends of the difference), radius 0 (the row ignores the radius
    term's dependence on d): every entry within 1e-6 of the row's largest."""
    pts, _, rec, field = scene
    xi = pr.perturbation(5, 11)
    step, checked = 1e-6, 0
    for v in range(5):
        r0 = pr.compose(rec[v], xi[v])
        base = pr.residuals(field[v], pts, None, r0, 8.0)
        fu, fw = base["u"] - np.floor(base["u"]), base["w"] - np.floor(base["w"])
        interior = (base["kind"] == 0) & (fu > 0.01) & (fu < 0.99) & (fw > 0.01) & (fw < 0.99) & (base["r"] > 0.01) & (base["r"] < 7.99)
        num = np.zeros((pts.shape[0], 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = step
            hi, lo = pr.residuals(field[v], pts, None, pr.compose(r0, d), 8.0), pr.residuals(field[v], pts, None, pr.compose(r0, -d), 8.0)
            same = (hi["kind"] == 0) & (lo["kind"] == 0) & (np.floor(hi["u"]) == np.floor(lo["u"])) & (np.floor(hi["w"]) == np.floor(lo["w"]))
            interior &= same
            num[:, k] = (hi["r"] - lo["r"]) / (2 * step)
        jac = base["J"][interior]
        scale = np.abs(jac).max(axis=1, keepdims=True)
        assert (np.abs(num[interior] - jac) <= 1e-6 * scale).all(), np.abs((num[interior] - jac) / scale).max()
        checked += int(interior.sum())
    assert checked >= 100


def test_masked_dofs_stay_exactly_zero(scene):
    pts, rad, rec, field = scene
    pert = np.stack([pr.compose(r, x) for r, x in zip(rec, pr.perturbation(5, 11))])
    sums, _ = pr.chamfer(field, pts, rad, None, pert, np.arange(5), 8.0)
    for mask in (0, 7, 56, 28, 1, 32, 63):
        for v in range(5):
            delta, singular = pr.solve(sums[v, 0, 3:9], sums[v, 0, 9:30], 1e-3, mask)
            assert not singular
            for k in range(6):
                assert ((mask >> k) & 1) or delta[k].tobytes() == np.float64(0.0).tobytes()
                assert not ((mask >> k) & 1) or delta[k] != 0.0
    out = pr.register(field, pts, rad, None, pert, 5, 8.0, dof_mask=56)      # translation only: the rotation is the perturbed one, bit for bit
    assert out["records"][:, :9].tobytes() == pert[:, :9].tobytes() and (out["records"][:, 9:12] != pert[:, 9:12]).any()


def test_slices_only_regroup_the_sums(scene):
    pts, rad, rec, field = scene
    one, c1 = pr.chamfer(field, pts, rad, None, rec, np.arange(5), 8.0, 1)
    two, c2 = pr.chamfer(field, pts, rad, None, rec, np.arange(5), 8.0, 2)
    assert (c1[:, 0] == c2.sum(axis=1)).all() and c1.sum() == 5 * 300 and (two[:, 1] != 0).any()
    assert np.allclose(one[:, 0], two.sum(axis=1), rtol=1e-12, atol=1e-12)
    bad, cb = pr.chamfer(field, pts, rad, None, rec[:2], np.array([0, 5]), 8.0, 2)
    assert (cb[1] == -1).all() and np.isinf(bad[1, :, 0]).all() and (bad[1, :, 1:] == 0).all() and (cb[0] >= 0).all()


def test_restatement_converges(scene):
    """Poses perturbed by up to +-0.5 degrees and +-0.5 world units per axis (0.4 to 2.6 px mean reprojection error) come back below the
    half-pixel rounding of a rasterised silhouette after 20 iterations; measured 0.058 to 0.107 px (twice the perturbation: the same)."""
    pts, rad, rec, field = scene
    pert = np.stack([pr.compose(r, x) for r, x in zip(rec, pr.perturbation(5, 11))])
    out = pr.register(field, pts, rad, None, pert, 20, 8.0)
    for v in range(5):
        before, after = pr.reprojection_error(pts, rec[v], pert[v], W, W), pr.reprojection_error(pts, rec[v], out["records"][v], W, W)
        st = out["state"][v]
        print(f"view {v}: {before:.3f} px -> {after:.4f} px, accepted {int(st[pr.ST_ACCEPTED])}, rejected {int(st[pr.ST_REJECTED])}")
        assert after < 0.5
        assert st[pr.ST_ACCEPTED] + st[pr.ST_REJECTED] == 20 and st[pr.ST_SINGULAR] == 0 and st[pr.ST_ACCEPTED] >= 1


def test_search_recovers_what_lm_cannot():
    """One branch, tau = 3, the pose shifted by 8 world units (20 px) along the detector: every point is saturated or lost, H = 0, and LM
    alone leaves the record bit-unchanged with every solve singular.  A 27-candidate grid that holds the exact opposite shift restores
    the unperturbed record and cost; candidate 0 is the identity, so a search never raises the cost."""
    pts, rad, seg = pr.tree_points(60, 1, 2)
    true = np.zeros((1, 16))
    true[0, [0, 4, 8]], true[0, 9:12], true[0, 12] = 1.0, (0.0, 0.0, 60.0), 2.4 * W      # face on: compose with +-8 along y is exact
    field = np.stack([pr.signed_field(m) for m in pr.silhouettes(seg, true, W, W)])
    pert = np.stack([pr.compose(true[0], [0, 0, 0, 0, 8.0, 0])])
    assert pr.compose(pert[0], [0, 0, 0, 0, -8.0, 0]).tobytes() == true[0].tobytes()
    sums0, _ = pr.chamfer(field, pts, rad, None, true, [0], 3.0)
    sums1, counts1 = pr.chamfer(field, pts, rad, None, pert, [0], 3.0)
    assert counts1[0, 0, 0] == 0 and counts1[0, 0, 1] == 0 and counts1[0, 0, 2:].sum() == 60      # all saturated or lost
    assert sums1[0, 0, 0] == 60 * 9.0 and sums0[0, 0, 0] < sums1[0, 0, 0]
    alone = pr.register(field, pts, rad, None, pert, 20, 3.0)
    assert alone["records"].tobytes() == pert.tobytes() and alone["state"][0, pr.ST_SINGULAR] == 20 and alone["state"][0, pr.ST_ACCEPTED] == 0
    offsets = engine.pose_search_offsets(0.0, 8.0, 3)
    found = pr.register(field, pts, rad, None, pert, 20, 3.0, offsets=offsets)
    assert found["start"].tobytes() == true.tobytes() and (offsets[found["selected"][0]] == [0, 0, 0, 0, -8.0, 0]).all()
    assert found["state"][0, pr.ST_COST] <= sums0[0, 0, 0]
    cand = pr.compose_outer(pert, offsets)
    csum, _ = pr.chamfer(field, pts, rad, None, cand.reshape(-1, 16), np.zeros(27, np.int32), 3.0, 1, pr.COST_ONLY)
    sel, cost = pr.select(csum, 1, 27)
    assert cost[0, sel[0]] == sums0[0, 0, 0] and cost[0, 0] == sums1[0, 0, 0] and cost[0, sel[0]] <= cost[0, 0]
    assert (csum[:, :, 3:] == 0).all()                            # cost-only leaves g and H at 0
    tie = np.zeros((4, 1, 32))
    tie[:, 0, 0] = [5.0, 2.0, 2.0, nan]
    assert pr.select(tie, 1, 4)[0].tolist() == [1]                # a tie goes to the lowest index, a NaN is never lower
