"""The visual hull's definition on the CPU (tests/hull_reference.py restates include/afx.h's afx_visual_hull): the inverse projection
against the project's forward ray model, the two guarantees G1 and G2 checked exactly on the capsule phantom, tightness, the edge cases of
the definition, and the host-side checks of the engine, the sweep and the driver.  No GPU."""
import argparse

import numpy as np
import pytest
import torch

import hull_reference as hr
from nerf_for_angiography_amd import engine
from nerf_for_angiography_amd._geometry import camera_rays
from nerf_for_angiography_amd.phantomdata.dataset import angle_grid
from nerf_for_angiography_amd.phantomdata.helpers import capsule_mu, capsule_tree
from nerf_for_angiography_amd.phantomdata.proj_helpers import source_matrix

SRC = np.array([0.0, 0.0, 1500.0])
EXCHANGE = ((0.0, 1.3, 0.0, -3.0), (0.7, 0.0, 0.0, 2.0), (0.0, 0.0, 0.9, 0.5))      # two axes exchanged, three spacings, det < 0
HALF, RES = 100.0, 64


def _poses(angles):
    return np.stack([source_matrix(SRC, th, ph) for th, ph in angles])


def test_project_inverts_the_forward_ray_model():
    """camera_rays(pose, px, py) origin + t direction, projected back, is (px, py) to 1e-9, and the depth along the view axis is t (the
    ray directions have camera z = -1) - at oblique poses, non-square detectors and non-integer pixels."""
    rng = np.random.RandomState(0)
    for (theta, phi), (w, h) in zip(((37.0, -61.0), (90.0, 0.0), (143.5, 22.25), (-20.0, 75.0)), ((64, 64), (9, 13), (13, 9), (100, 80))):
        pose = source_matrix(SRC, theta, phi)
        f = 13.0 * w
        px = torch.from_numpy(rng.uniform(-3.0, w + 2.0, 500))
        py = torch.from_numpy(rng.uniform(-3.0, h + 2.0, 500))
        t = rng.uniform(1400.0, 1600.0, 500)
        o, d = camera_rays(torch.from_numpy(pose), px, py, w, h, f)
        x = (o + d * torch.from_numpy(t)[:, None]).numpy()
        u, v, depth = hr.project(x, pose, f, w, h)
        assert np.abs(u - px.numpy()).max() < 1e-9 and np.abs(v - py.numpy()).max() < 1e-9
        assert np.abs(depth - t).max() < 1e-9


@pytest.fixture(scope="module")
def phantom():
    """200 000 points inside the capsule tree (capsule_mu > 0), the 64^3 lattice of cell centres over the +-100 box and the cell of every
    point; made once, left unchanged."""
    caps = capsule_tree(levels=5, seed=0)
    rng = np.random.RandomState(0)
    chunks, have = [], 0
    while have < 200000:
        i = rng.randint(len(caps), size=400000)
        a, b, r = caps[i, :3].astype(np.float64), caps[i, 3:6].astype(np.float64), caps[i, 6:7].astype(np.float64)
        p = a + rng.uniform(size=(len(i), 1)) * (b - a) + rng.uniform(-1, 1, size=(len(i), 3)) * r
        p = p[capsule_mu(torch.from_numpy(p), caps).numpy() > 0]
        chunks.append(p)
        have += len(p)
    pts = np.concatenate(chunks)[:200000]
    a12, rho = hr.box_lattice(HALF, RES)
    cell = np.floor((pts + HALF) / (2.0 * HALF / RES)).astype(np.int64)
    assert cell.min() >= 0 and cell.max() < RES
    return dict(points=pts, lattice=hr.lattice_points((RES,) * 3, a12), rho=rho, cell=(cell[:, 0] * RES + cell[:, 1]) * RES + cell[:, 2])


# every pose of angle_grid, the held-out one included: more views reject more, so this is the stricter reading for G1
VIEW_SETS = {"4+1 views 64^2": (1, 64), "9+1 views 64^2": (2, 64), "25+1 views 100^2": (4, 100)}


@pytest.mark.parametrize("name", list(VIEW_SETS))
def test_guarantees_hold_exactly_on_the_capsule_phantom(phantom, name):
    """Masks = the rounded projections of 200 000 points of the vessel; margin 1 (a point projects within sqrt(0.5) of the pixel centre it
    marks).  G1: no cell that holds one of the points is rejected by any view.  G2: a cell that holds a point which lands on the detector
    of k views is seen by at least k views."""
    number_angles, size = VIEW_SETS[name]
    poses = _poses(angle_grid(180, number_angles))
    f = 13.0 * size
    masks, inside = hr.masks_from_points(phantom["points"], poses, f, size, size)
    seen, rejects = hr.hull_counts(phantom["lattice"], phantom["rho"], poses, f, size, size, 1.0, hr.distance_stack(masks))
    cell = phantom["cell"]
    g1 = int((rejects[cell] != 0).sum())
    need = np.zeros(RES ** 3, np.int64)
    np.maximum.at(need, cell, inside.sum(axis=0))
    g2 = int((seen < need).sum())
    print(f"{name}: G1 violations {g1}, G2 violations {g2}, hull share {float(((rejects == 0) & (seen >= 1)).mean()):.4f}")
    assert g1 == 0
    assert g2 == 0
    assert need.max() == len(poses)      # (some cell is asked to be seen by every view: the check is not vacuous)


def test_hull_is_tight(phantom):
    """9 training views (angle_grid(180, 2) without the held-out pose: fewer views carve less) at 64^2, margin 1: the hull with
    min_seen = 1 is below half the grid (measured 12.7 %: profiles/r21_visual_hull.md)."""
    poses = _poses(angle_grid(180, 2)[:-1])
    masks, _ = hr.masks_from_points(phantom["points"], poses, 13.0 * 64, 64, 64)
    seen, rejects = hr.hull_counts(phantom["lattice"], phantom["rho"], poses, 13.0 * 64, 64, 64, 1.0, hr.distance_stack(masks))
    share = float(((rejects == 0) & (seen >= 1)).mean())
    print(f"hull share {share:.4f}, of which seen by all views {float(((rejects == 0) & (seen >= len(poses))).mean()):.4f}")
    assert 0.0 < share < 0.5


def test_zero_radius_zero_margin_one_pixel_mask():
    """rho = 0 and m = 0: a point is its own projection, and with one (interior) mask pixel exactly the lattice points in front of the
    source whose rounded projection is that pixel survive."""
    w, h, f = 16, 12, 13.0 * 16
    pose = source_matrix(SRC, 64.0, -31.0)
    a12, _ = hr.box_lattice(40.0, 24)
    x = hr.lattice_points((24,) * 3, a12)
    u, v, d = hr.project(x, pose, f, w, h)
    mask = np.zeros((1, h, w), bool)
    mask[0, 5, 9] = True
    seen, rejects = hr.hull_counts(x, 0.0, pose[None], f, w, h, 0.0, hr.distance_stack(mask))
    want = (d > 0) & (np.floor(u + 0.5) == 9) & (np.floor(v + 0.5) == 5)
    assert 3 < want.sum() < x.shape[0] // 4
    assert np.array_equal((seen >= 1) & (rejects == 0), want)
    on_detector = (d > 0) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
    assert np.array_equal(seen == 1, on_detector)      # rho = m = 0: seen is "projects among the pixel centres"


def test_point_too_close_to_the_source_is_unseen():
    """d - rho <= 0: the view neither sees nor rejects the point, whatever the mask says - also for 0 < d <= rho."""
    pose = source_matrix(np.array([0.0, 0.0, 5.0]), 90.0, 0.0)      # the source inside the lattice; a layer of points at d = 1.25 < rho
    a12, rho = hr.box_lattice(20.0, 16)
    x = hr.lattice_points((16,) * 3, a12)
    d = -hr.camera_coordinates(x, pose)[:, 2]
    for mask in (np.ones((1, 8, 8), bool), np.eye(8, dtype=bool)[None]):
        seen, rejects = hr.hull_counts(x, rho, pose[None], 30.0, 8, 8, 1.0, hr.distance_stack(mask))
        near = d - rho <= 0
        assert ((d > 0) & near).sum() > 0 and (~near).sum() > 0
        assert (seen[near] == 0).all() and (rejects[near] == 0).all()
        assert (seen[~near] == 1).any()


def test_empty_mask_is_refused():
    masks = np.zeros((3, 6, 7), bool)
    masks[0, 2, 3] = masks[2, 0, 0] = True
    with pytest.raises(ValueError, match="empty"):
        hr.distance_stack(masks)
    poses = _poses(angle_grid(180, 1)[:3])
    with pytest.raises(ValueError, match="view 1 is empty"):      # before anything asks for a GPU
        engine.visual_hull_views(poses, torch.from_numpy(masks), 91.0)
    with pytest.raises(ValueError, match="3 poses but 2 masks"):
        engine.visual_hull_views(poses, torch.ones(2, 6, 7, dtype=torch.bool), 91.0)


def test_view_records_and_lattices():
    poses = _poses(angle_grid(180, 1))
    rec = engine.hull_view_records(poses, [10.0, 20.0, 30.0, 40.0, 50.0])
    assert rec.shape == (5, engine.HULL_VIEW_DOUBLES) and rec.dtype == np.float64
    for v in range(5):
        assert np.array_equal(rec[v, :9].reshape(3, 3), poses[v, :3, :3]) and np.array_equal(rec[v, 9:12], poses[v, :3, 3])
    assert np.array_equal(rec[:, 12], [10.0, 20.0, 30.0, 40.0, 50.0]) and not rec[:, 13:].any()
    assert np.array_equal(engine.hull_view_records(poses[:, :3], 7.0)[:, :12], rec[:, :12])      # [V, 3, 4] poses
    sheared = poses.copy()
    sheared[1, 0, 1] += 0.01
    with pytest.raises(ValueError, match="orthonormal"):
        engine.hull_view_records(sheared, 7.0)
    with pytest.raises(ValueError, match="focal"):
        engine.hull_view_records(poses, [1.0, 2.0])
    # an occupancy grid's cell centres and half-diagonal, formed in fp64 from the float32 box
    a12, rho = engine.grid_cell_lattice([-100.0, -100, -100, 100, 100, 100], [64, 64, 64])
    want_a, want_rho = hr.box_lattice(HALF, RES)
    assert np.array_equal(a12, want_a) and rho == want_rho
    a12, rho = engine.grid_cell_lattice([-1.0, 0.0, 2.0, 3.0, 6.0, 5.0], [4, 3, 6])
    assert np.allclose(a12.reshape(3, 4), [[1, 0, 0, -0.5], [0, 2, 0, 1.0], [0, 0, 0.5, 2.25]]) and np.isclose(rho, 0.5 * np.sqrt(1 + 4 + 0.25))
    # the default radius: half the cell's longest diagonal, also under an axis exchange
    assert np.isclose(engine.hull_default_radius(EXCHANGE), 0.5 * np.sqrt(1.3 ** 2 + 0.7 ** 2 + 0.9 ** 2))
    assert np.isclose(engine.hull_default_radius(None), 0.5 * np.sqrt(3.0))
    skew = ((1.0, 1.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0))
    assert np.isclose(engine.hull_default_radius(skew), 0.5 * np.sqrt(4 + 1 + 1))


def test_sweep_names_and_scores():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.HULL_METRICS == ("OUTSIDE HULL 3D", "DICE 3D HULL", "HULL RATIO 3D")
    assert not set(sweep.HULL_METRICS) & set(sweep.METRICS + sweep._ALL_VOLUME_METRICS)
    with pytest.raises(ValueError, match="hull_views"):
        sweep._check_metrics(["PSNR", "OUTSIDE HULL 3D"], None, object())
    with pytest.raises(ValueError, match="ground-truth volume"):
        sweep._check_metrics(["DICE 3D HULL"], None, None, hull_views={})
    got = sweep._check_metrics(["HULL RATIO 3D", "PSNR", "OUTSIDE HULL 3D"], None, object(), hull_views={})
    assert got == ["PSNR", "OUTSIDE HULL 3D", "HULL RATIO 3D"]
    s = sweep.hull_scores(n_pred=40, n_pred_outside=10, n_hull=300, n_gt=100, n_both=90)
    assert s == dict(outside_hull=0.25, dice_hull=0.45, hull_ratio=3.0)
    s = sweep.hull_scores(0, 0, 0, 0, 0)
    assert all(np.isnan(v) for v in s.values())


def _args(*extra):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser
    return build_parser().parse_args(["--synthetic", *extra])


def test_driver_refuses_the_hull_where_it_would_be_wrong():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import check_args
    check_args(_args("--binary", "True", "--march", "grid", "--grid_init", "hull"))
    check_args(_args("--binary", "True", "--march", "grid_ops", "--grid_init", "hull", "--hull_margin", "2", "--save_hull", "votes.npy"))
    with pytest.raises(ValueError, match="--binary True"):
        check_args(_args("--binary", "False", "--march", "grid", "--grid_init", "hull"))
    with pytest.raises(ValueError, match="--binary True"):
        check_args(_args("--march", "grid", "--grid_init", "hull"))      # (the reference's default is data with background)
    with pytest.raises(ValueError, match="--march grid"):
        check_args(_args("--binary", "True", "--march", "dense", "--grid_init", "hull"))
    with pytest.raises(ValueError, match="--hull_margin"):
        check_args(_args("--binary", "True", "--march", "grid", "--grid_init", "hull", "--hull_margin", "-1"))
    with pytest.raises(ValueError, match="--save_hull"):
        check_args(_args("--binary", "True", "--march", "grid", "--save_hull", "votes.npy"))


def test_fingerprint_names_the_hull_only_when_set():
    """Without --grid_init the fingerprint is what a namespace that has never heard of the flag gives (state files written before keep
    theirs); with it the option and its three parameters are named."""
    from nerf_for_angiography_amd.nerf.checkpoint import config_fingerprint
    table = tuple(torch.arange(12.0).reshape(4, 3) + k for k in range(2)) + (torch.arange(4.0), torch.ones(4))
    model = dict(num_filters=64, device="cpu")
    plain = _args("--binary", "True", "--march", "grid")
    before = argparse.Namespace(**{k: v for k, v in vars(plain).items()
                                   if k not in ("grid_init", "hull_margin", "hull_max_rejects", "hull_threshold", "save_hull")})
    fp = config_fingerprint(plain, model, table)
    assert fp == config_fingerprint(before, model, table)
    assert not {"grid_init", "hull_margin", "hull_max_rejects", "hull_threshold"} & set(fp)
    carved = config_fingerprint(_args("--binary", "True", "--march", "grid", "--grid_init", "hull", "--hull_margin", "1.5"), model, table)
    assert carved["grid_init"] == "hull" and carved["hull_margin"] == 1.5 and carved["hull_max_rejects"] == 0 and carved["hull_threshold"] == 1.0
    assert {k: v for k, v in carved.items() if k not in ("grid_init", "hull_margin", "hull_max_rejects", "hull_threshold")} == fp
