"""Host-side half of the voxel-volume lookup tests: the restatement of tests/volume_reference.py is tied to scipy's RegularGridInterpolator
(and, on the exact problem, to the closed form), every mutation knob is shown to change what the GPU tests compare, and the preconditions
tests/test_gpu_volume_lookup.py assumes of the shared problems are asserted here, on the references alone.  The ray-table arithmetic of
engine.project_volume / Engine.march_render and VoxelVolume's refusals need no device either."""
import numpy as np
import pytest
import torch
from scipy.interpolate import RegularGridInterpolator

import volume_reference as vr
from nerf_for_angiography_amd import engine
from nerf_for_angiography_amd.phantomdata.helpers import VoxelVolume

CASES = vr.lattice_cases()
CASE_IDS = [f"{v.name}-n{lat.n}" for v, lat in CASES]


def _scipy(v, points, fill=None):
    interp = RegularGridInterpolator(v.axes, v.vol.astype(np.float64), method="linear", bounds_error=False,
                                     fill_value=v.fill if fill is None else fill)
    return interp(np.asarray(points).reshape(-1, 3)).reshape(np.asarray(points).shape[:-1])


def _changed(a, b):
    return int((~(a == b)).sum())      # (a NaN, the mark of a stray read, counts as a change)


def test_problem_a_is_exact():
    """Restatement == scipy == closed form, bit for bit, and every value is an fp32 number: the GPU test may ask for equality."""
    v, lat = vr.problem_a(), vr.A_LATTICE
    assert v.vol.shape == (5, 7, 11) and v.origin == (-3.0, -1.5, -0.75) and v.spacing == (0.5, 1.0, 0.25) and v.fill == -4096.0
    assert np.array_equal(vr.lattice_axis(*lat), -4.0 + 0.25 * np.arange(33))
    pts = vr.lattice_points(*lat)
    got = vr.vol_sample(v.vol, v.origin, v.spacing, v.fill, pts)
    assert np.array_equal(got, vr.a_closed_form(pts))
    assert np.array_equal(got, _scipy(v, pts))
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got)
    t = vr.lattice_axis(*lat)
    i, j, k = 12, 6, 20      # (t[j], t[i], t[k]) = (-2.5, -1.0, 1.0): u = 1, v = 0.5, w = 7
    assert (t[j], t[i], t[k]) == (-2.5, -1.0, 1.0)
    assert vr.volume_grid(v.vol, v.origin, v.spacing, v.fill, *lat)[i, j, k] == np.float32(1 + 3 + 8 + 896 + 3.5)


@pytest.mark.parametrize("v,lat", CASES[1:], ids=CASE_IDS[1:])
def test_restatement_matches_scipy(v, lat):
    """The general problems: the same fill pattern and values within 1e-13 of the volume's maximum (volume_reference.B_SPECS says why
    that holds on the long axes)."""
    assert all(np.array_equal(a, np.round(a[0] + (a[1] - a[0]) * np.arange(len(a)), 3)) for a in v.axes)      # three decimals
    assert len({tuple(v.vol.shape), v.origin, v.spacing}) == 3 and len(set(v.spacing)) == 3 and len(set(v.origin)) == 3
    assert v.vol.dtype == np.float32 and 0.2 <= v.vol.min() and v.vol.max() <= 2.0
    pts = vr.lattice_points(*lat)
    got, want = vr.vol_sample(v.vol, v.origin, v.spacing, v.fill, pts), _scipy(v, pts)
    assert np.array_equal(got == v.fill, want == v.fill)
    err = float(np.abs(got - want).max() / v.vol.max())
    print(f"{v.name} n={lat.n}: restatement vs scipy {err:.2e} of the maximum")
    assert err <= 1e-13


def test_a_box_without_the_world_origin():
    away = [s for s in vr.B_SHAPES if not all(lo <= 0 <= hi for lo, hi in zip(*vr.box_of(vr.problem_b(s))))]
    assert away, "no general problem's box leaves out the world origin"
    assert set(vr.RAY_SHAPES) <= set(vr.B_SHAPES) and set(vr.B_SHAPES) == {(2, 2, 2), (2, 3, 5), (6, 9, 4), (64, 3, 2), (3, 2, 130)}
    assert all(sorted(lat.n for lat in vr.lattices(s)) == [2, 33, 50] for s in vr.B_SHAPES)


def test_lattice_axis_is_linspace_in_fp32_and_far_from_a_rounding_tie():
    """t = float32(np.linspace(lo, hi, n)).  The kernel may fuse m * step + lo, which moves the fp64 value by an ulp at most: no lattice
    coordinate lies that close to the middle between two fp32 numbers, so the fp32 point is the same either way."""
    for v, lat in CASES:
        t64 = np.linspace(lat.lo, lat.hi, lat.n)
        t = vr.lattice_axis(*lat)
        assert np.array_equal(t, t64.astype(np.float32).astype(np.float64)) and t[-1] == np.float32(lat.hi)
        half = 0.5 * np.spacing(np.abs(t).astype(np.float32)).astype(np.float64)
        to_tie = np.abs(np.abs(t64 - t) - half)
        assert (to_tie > 8 * np.spacing(np.abs(t64)))[t64 != t].all(), (v.name, lat)


@pytest.mark.parametrize("v,lat", CASES, ids=CASE_IDS)
def test_lattices_exercise_fill_and_interior(v, lat):
    pts = vr.lattice_points(*lat)
    inside = vr.vol_sample(v.vol, v.origin, v.spacing, v.fill, pts) != v.fill
    assert 0.03 <= inside.mean() <= 0.97, inside.mean()
    if v.name != "A":      # the exact problem's lattice sits ON the faces, which is its point; no other sample point comes near one
        assert vr.face_margin(pts, v) > 1e-9


def test_every_mutation_changes_the_lattice_values():
    """The evidence that the GPU tests can fail: each mutant of the lookup differs from it at 100 points or more of problem A's lattice
    and of one general lattice at least.  The two upper-face mutants differ only ON an upper face, where no general problem may have a
    point (see above), so for them the second half is every upper-face probe of both probe volumes instead."""
    base = {id(c): vr.vol_sample(c[0].vol, c[0].origin, c[0].spacing, c[0].fill, vr.lattice_points(*c[1])) for c in CASES}
    print()
    for name, knobs in vr.MUTATIONS.items():
        counts = []
        for c in CASES:
            v, lat = c
            counts.append(_changed(vr.vol_sample(v.vol, v.origin, v.spacing, v.fill, vr.lattice_points(*lat), **knobs), base[id(c)]))
        print(f"{name:22s} A: {counts[0]:5d}   general: " + " ".join(f"{CASE_IDS[i]}:{n}" for i, n in enumerate(counts) if i and n))
        assert counts[0] >= 100, (name, counts[0])
        if name not in vr.FACE_MUTATIONS:
            assert max(counts[1:]) >= 100, (name, counts)
            continue
        assert max(counts[1:]) == 0
        for which in vr.PROBE_SHAPES:
            v, pr = vr.probe_volume(which), vr.probes(which)
            pts = np.array([p.point for p in pr])
            same = vr.vol_sample(v.vol, v.origin, v.spacing, v.fill, pts, **knobs) == vr.vol_sample(v.vol, v.origin, v.spacing, v.fill, pts)
            hi = vr.box_of(v)[1]
            on_upper = np.array([p.inside and any(c == h for c, h in zip(p.point, hi)) for p in pr])
            assert on_upper.sum() >= 7 + 9 + 3      # every corner but one, nine edges, three faces
            assert not same[on_upper].any(), (name, which)
    ij = [int((vr.volume_grid(v.vol, v.origin, v.spacing, v.fill, *lat) != vr.volume_grid(v.vol, v.origin, v.spacing, v.fill, *lat, indexing="ij")).sum())
          for v, lat in CASES]
    print(f"{'meshgrid ij':22s} A: {ij[0]:5d}   general: " + " ".join(f"{CASE_IDS[i]}:{n}" for i, n in enumerate(ij) if i and n))
    assert ij[0] >= 100 and max(ij[1:]) >= 100


@pytest.mark.parametrize("which", list(vr.PROBE_SHAPES))
def test_probes(which):
    """The probes are what they are named: distinct exact points, inside or outside as said, on dyadic axes whose upper face is the
    last point itself; scipy agrees on the pattern, and on the values to 1e-13; inside, exp(-mu) stays far from the outside's 1."""
    v, pr = vr.probe_volume(which), vr.probes(which)
    lo, hi = vr.box_of(v)
    assert all(a[-1] == h and a[0] == l for a, l, h in zip(v.axes, lo, hi)) and v.fill == 0.0
    assert 0.5 <= v.vol.min() and v.vol.max() <= 2.0 and len(set(v.vol.shape)) == 3
    pts = np.array([p.point for p in pr])
    assert len({p.point for p in pr}) == len(pr) == 8 + 12 + 6 * 3 + 5
    names = [p.name.split()[0] for p in pr]
    assert names.count("corner") == 8 and names.count("edge") == 12 and sum("outward" in p.name for p in pr) == 6
    on_face = np.array([[(c == lo[a]) or (c == hi[a]) for a, c in enumerate(p.point)] for p in pr])
    for p, f in zip(pr, on_face):
        if "one step" not in p.name and names[pr.index(p)] in ("corner", "edge", "face"):
            assert f.sum() == {"corner": 3, "edge": 2, "face": 1}[p.name.split()[0]], p
    mu = vr.vol_sample(v.vol, v.origin, v.spacing, v.fill, pts)
    assert [bool(m != 0) for m in mu] == [p.inside for p in pr]
    assert (mu[[p.inside for p in pr]] >= 0.5).all()      # exp(-mu) <= 0.61 inside
    want = _scipy(v, pts)
    assert np.array_equal(want == 0, mu == 0) and np.abs(want - mu).max() <= 1e-13 * v.vol.max()
    poses = vr.probe_poses(which)
    o, d = vr.pose_rays(poses, 1, 1, 1.0, np.arange(len(pr)))
    assert np.array_equal(vr.sample_points(o, d, np.zeros(1, np.float32))[:, 0], pts)      # o + d 0 is the probe, bit for bit


@pytest.mark.parametrize("shape", vr.RAY_SHAPES)
def test_ray_bundles(shape):
    """437 rays a pose; both ends of every ray outside the box; each of the six faces entered and left at least once; rays that miss the
    box altogether; no sample within 1e-9 of a face plane, for the fp64 rays of pose mode and for their fp32 roundings of arrays mode."""
    v, b = vr.problem_b(shape), vr.ray_bundle(shape)
    assert (b.w, b.h, len(b.z), b.poses.shape) == (23, 19, 61, (2, 3, 4)) and b.z.dtype == np.float32 and b.w * b.h == 437
    lo, hi = vr.box_of(v)
    for as_fp32 in (False, True):
        o, d = vr.bundle_rays(shape, as_fp32)
        hit, face_in, face_out = vr.faces_crossed(o, d, lo, hi)
        assert set(face_in[hit]) == set(range(6)) and set(face_out[hit]) == set(range(6))
        assert 50 <= (~hit).sum() and 50 <= hit[:437].sum() and 50 <= hit[437:].sum()
        pts = vr.sample_points(o, d, b.z)
        assert vr.face_margin(pts, v) > 1e-9
        inside = vr.vol_sample(v.vol, v.origin, v.spacing, 0.0, pts) != 0
        assert not inside[:, 0].any() and not inside[:, -1].any() and inside.sum(1).max() >= 10
        assert (inside.sum(1) == 0).sum() >= 50
        for type_ct in (True, False):
            img = vr.project(v.vol, v.origin, v.spacing, 0.0, o, d, b.z, type_ct)
            assert img.std() > 0.01 and img.min() > 1e-30      # structure, and nothing near the end of fp32's range
    rot = b.poses[:, :, :3]
    assert np.abs(rot.transpose(0, 2, 1) @ rot - np.eye(3)).max() < 1e-14


def test_pose_rays_match_camera_rays():
    """pose_rays against the library's own host ray generation (the reference's get_rays_np convention)."""
    from nerf_for_angiography_amd._geometry import camera_rays
    b = vr.ray_bundle((6, 9, 4))
    o, d = vr.pose_rays(b.poses, b.w, b.h, b.focal, np.arange(2 * 437))
    for p in range(2):
        pose = torch.from_numpy(np.concatenate([b.poses[p], [[0.0, 0.0, 0.0, 1.0]]]))
        ii, jj = torch.meshgrid(torch.arange(b.w, dtype=torch.float64), torch.arange(b.h, dtype=torch.float64), indexing="xy")
        ro, rd = camera_rays(pose, ii, jj, b.w, b.h, b.focal)
        assert np.abs(rd.reshape(-1, 3).numpy() - d[p * 437:(p + 1) * 437]).max() < 1e-14
        assert np.array_equal(ro.reshape(-1, 3).numpy(), o[p * 437:(p + 1) * 437])


def test_project_far_plane_rule():
    """'ct': the last sample carries dist = 1e10, so a non-zero fill behind the box takes every pixel to exactly 0 and fill = 0 none."""
    shape = (6, 9, 4)
    v, b = vr.problem_b(shape), vr.ray_bundle(shape)
    o, d = vr.bundle_rays(shape, False)
    assert (vr.project(v.vol, v.origin, v.spacing, 0.25, o, d, b.z, True) == 0).all()
    assert (vr.project(v.vol, v.origin, v.spacing, 0.0, o, d, b.z, True) > 0).all()
    assert (vr.project(v.vol, v.origin, v.spacing, 0.25, o, d, b.z, False) > 0).all()


# ---- the ray table ----------------------------------------------------------------------------------------------------------------
def test_ray_window_accepts_what_lies_in_the_table():
    rw = engine.ray_window
    assert rw("f", 2, 23, 19) == 874 and rw("f", 2, 23, 19, 400) == 474 and rw("f", 2, 23, 19, 400, 74) == 74
    assert rw("f", 2, 23, 19, 874, 0) == 0 and rw("f", 2, 23, 19, 874) == 0 and rw("f", 2, 23, 19, 0, 874) == 874
    assert rw("f", 2, 23, 19, 5, 0) == 0 and rw("f", 0, 23, 19) == 0
    ids = torch.tensor([873, 0, 0, 436, 437], dtype=torch.int64)
    assert rw("f", 2, 23, 19, ray_ids=ids) == 5 and rw("f", 2, 23, 19, n_rays=2, ray_ids=ids) == 2
    assert rw("f", 2, 23, 19, ray_ids=ids.to(torch.int32)) == 5 and rw("f", 2, 23, 19, ray_ids=ids[:0]) == 0
    assert rw("f", 1, 23, 19, n_rays=2, ray_ids=torch.tensor([3, 4, 9999])) == 2      # only the ids that are read count


@pytest.mark.parametrize("kw,word,shows_table", [
    (dict(ray_id0=-1), "ray_id0", True), (dict(ray_id0=-1, n_rays=1), "ray_id0", True), (dict(ray_id0=875), "ray_id0", True),
    (dict(n_rays=-1), "n_rays", True), (dict(n_rays=875), "n_rays", True), (dict(ray_id0=400, n_rays=475), "n_rays", True),
    (dict(ray_id0=874, n_rays=1), "n_rays", True), (dict(ray_id0=2 ** 40, n_rays=1), "ray_id0", True),
    (dict(ray_ids=torch.tensor([0, 874])), "ray_ids", True), (dict(ray_ids=torch.tensor([5, -1, 7])), "ray_ids", True),
    (dict(ray_ids=torch.tensor([2 ** 32 + 5])), "ray_ids", True), (dict(ray_ids=torch.tensor([1, 2]), n_rays=3), "n_rays", False),
    (dict(ray_ids=torch.tensor([1, 2]), n_rays=-1), "n_rays", False), (dict(ray_ids=torch.tensor([1.0, 2.0])), "ray_ids", False),
])
def test_ray_window_refuses_what_lies_outside(kw, word, shows_table):
    with pytest.raises(ValueError, match=word) as e:
        engine.ray_window("who", 2, 23, 19, **kw)
    msg = str(e.value)
    assert msg.startswith("who: ")
    if shows_table:      # the message shows the table and its range, as march_render's does
        assert "2 x 19 x 23 table" in msg and ("0 .. 874" in msg or "0 .. 873" in msg)


# ---- VoxelVolume --------------------------------------------------------------------------------------------------------------------
def test_voxel_volume_metadata_and_refusals():
    v = vr.problem_b((6, 9, 4))
    vol = VoxelVolume(*v.axes, v.vol, fill_value=v.fill, device="cpu")
    assert tuple(vol.origin) == v.origin == tuple(a[0] for a in v.axes)
    assert tuple(vol.spacing) == v.spacing == tuple(a[1] - a[0] for a in v.axes)
    assert tuple(vol.values.shape) == (6, 9, 4) and vol.values.is_contiguous() and np.array_equal(vol.values.numpy(), v.vol)
    assert VoxelVolume(*v.axes, v.vol, device="cpu").fill_value == float(v.vol.min())
    x, y, z = v.axes
    for perm in ((1, 0, 2), (2, 1, 0), (0, 2, 1), (1, 2, 0)):
        with pytest.raises(ValueError, match="values"):
            VoxelVolume(x, y, z, v.vol.transpose(perm), device="cpu")
    with pytest.raises(ValueError, match="points_y.*at least 2"):
        VoxelVolume(x, y[:1], z, v.vol[:, :1], device="cpu")
    with pytest.raises(ValueError, match="points_z.*ascending"):
        VoxelVolume(x, y, z[::-1], v.vol, device="cpu")
    with pytest.raises(ValueError, match="points_x.*ascending"):
        VoxelVolume(np.array([0.0, 1.0, 1.0, 2.0, 3.0, 4.0]), y, z, v.vol, device="cpu")
    with pytest.raises(ValueError, match="points_x.*regular"):
        VoxelVolume(np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.5]), y, z, v.vol, device="cpu")
