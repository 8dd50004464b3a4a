"""Curved-planar reformation without a GPU: the argument checks of afx_reformat_planes (include/afx.h), which return before any HIP call;
the host geometry of engine.py (main path, smoothing, resampling, rotation-minimising frames, sample tables) against closed forms and
hand-made graphs; the NumPy restatement of the kernel (tests/reformat_reference.py) on exact cases and on the stenosis phantom; the
sweep's metric names and the driver's flag."""
import ctypes as C
import math

import numpy as np
import pytest

import lumen_reference as lr
import reformat_reference as rr

AFX_E_INVALID = -1
FAKE = C.c_void_p(0x10000)          # never dereferenced: every call below is refused, or returns, before it reaches the device
GOOD_W = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]


@pytest.fixture(scope="module")
def lib():
    from nerf_for_angiography_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- the library
def test_the_library_exports_and_declares_the_symbol(lib):
    import os
    import re
    from conftest import ROOT
    from nerf_for_angiography_amd import _lib
    assert hasattr(lib, "afx_reformat_planes") and "afx_reformat_planes" in _lib.exported_symbols()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "afx.h")).read(), flags=re.S)
    proto = re.findall(r"\bafx_reformat_planes\s*\(([^;{}]*?)\)\s*;", header)
    assert len(proto) == 1 and not re.search(r"\bworkspace\b", proto[0])       # no workspace: nothing for the workspace contract to pin
    assert len(proto[0].split(",")) == len(_lib._SIGS["afx_reformat_planes"][1]) == 15


def test_reformat_planes_argument_validation(lib):
    def call(vol=FAKE, shape=(4, 5, 6), W=GOOD_W, planes=FAKE, P=3, table=FAKE, Q=5, H=0, mode=0, fill=0.0, out=FAKE):
        w = None if W is None else (C.c_double * 12)(*W)
        return lib.afx_reformat_planes(vol, 0, *shape, w, planes, P, table, Q, H, mode, fill, out, None)

    def refused(word, **kw):
        assert call(**kw) == AFX_E_INVALID and word in lib.afx_last_error(), (kw, lib.afx_last_error())

    refused(b"vol", vol=None)
    refused(b"world_to_index", W=None)
    for name, word in (("planes", b"planes"), ("table", b"table"), ("out", b"out")):
        refused(word, **{name: None})
        assert b"null" in lib.afx_last_error()
    for bad in ((1, 5, 6), (4, 1, 6), (4, 5, 1), (0, 5, 6), (-3, 5, 6)):
        refused(b"n0, n1, n2", shape=bad)
    for bad in ((1 << 11, 1 << 10, 1 << 10), (46341, 46341, 2), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1)):
        refused(b"2^31", shape=bad)
    for bad in (-1, 1 << 31):
        refused(b"n_planes", P=bad)
    for bad in (-1, (1 << 20) + 1, 1 << 31):
        refused(b"n_table", Q=bad)
    for bad in (-1, 128, 1 << 20):
        refused(b"half_slab", H=bad)
    for bad in (-1, 2, 7):
        refused(b"mode", mode=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(b"fill", fill=bad)
        refused(b"world_to_index", W=GOOD_W[:7] + [bad] + GOOD_W[8:])
    # nothing to launch: AFX_OK without a HIP call, whatever the device pointers are
    assert call(P=0) == 0 and call(Q=0) == 0 and call(P=0, Q=0, planes=None, table=None, out=None) == 0
    assert call(P=0, H=127, mode=1, shape=(2, 2, 2), Q=1 << 20) == 0
    refused(b"mode", P=0, mode=3)                                           # the checks come before the early return
    refused(b"half_slab", Q=0, H=200)


def test_host_tensors_are_refused():
    import torch
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd._lib import AfxError
    vol, planes, table = torch.ones(4, 5, 6), torch.zeros(3, 9, dtype=torch.float64), torch.zeros(5, 4, dtype=torch.float64)
    with pytest.raises(AfxError):
        engine.reformat_planes_record(vol, planes, table, engine.lumen_world_to_index(None))
    pts = np.array([[1.0, 1, 1], [2, 2, 2], [3, 3, 3]])
    for call in (lambda: engine.straighten_volume(vol, pts), lambda: engine.cpr_images(vol, pts), lambda: engine.centreline_cpr({}, vol, None)):
        with pytest.raises(AfxError):
            call()


# ---------------------------------------------------------------- frames
def _frenet_twist_error(n):
    """max |theta(s) - theta(0) + tau s| of the frame's angle about the tangent against the helix's Frenet frame."""
    from nerf_for_angiography_amd import engine
    pts, s, tau = rr.helix(n)
    t, u, v, flags = engine.rotation_minimising_frames(pts, 3)
    phi = s / math.sqrt(5.0 ** 2 + 1.5 ** 2)
    normal = np.stack([-np.cos(phi), -np.sin(phi), 0.0 * phi], axis=1)
    tangent = np.stack([-5.0 * np.sin(phi), 5.0 * np.cos(phi), 1.5 + 0.0 * phi], axis=1) / math.sqrt(5.0 ** 2 + 1.5 ** 2)
    binormal = np.cross(tangent, normal)
    theta = np.unwrap(np.arctan2((u * binormal).sum(axis=1), (u * normal).sum(axis=1)))
    return float(np.abs((theta - theta[0]) + tau * s).max()), (t, u, v, flags)


def test_a_plane_curve_keeps_the_frame_in_its_plane_exactly():
    from nerf_for_angiography_amd import engine
    phi = np.linspace(0.2, 1.3, 57)                                         # both in-plane tangent components stay away from 0
    pts = np.stack([9.0 * np.cos(phi) + 0.3 * phi, 7.0 * np.sin(phi), np.full_like(phi, 2.5)], axis=1)
    t, u, v, flags = engine.rotation_minimising_frames(pts, 3)
    assert not flags.any()
    assert (t[:, 2] == 0).all() and (u[:, 2] == 0).all() and (v[:, 0] == 0).all() and (v[:, 1] == 0).all()      # the reflections leave them alone
    assert np.abs(np.abs(v[:, 2]) - 1.0).max() <= 1e-15


def test_frames_are_orthonormal_on_a_long_helix():
    err, (t, u, v, flags) = _frenet_twist_error(3200)
    assert not flags.any()
    assert np.abs((u * t).sum(axis=1)).max() <= 1e-14 and np.abs((v * t).sum(axis=1)).max() <= 1e-14
    assert np.abs(np.sqrt((u * u).sum(axis=1)) - 1.0).max() <= 1e-14


@pytest.mark.parametrize("n,bar", ((200, 2.56e-3), (800, 1.94e-4), (3200, 1.26e-5)))
def test_the_twist_follows_the_closed_form(n, bar):
    """A rotation-minimising frame turns against the Frenet frame of a helix (radius 5, pitch 1.5 per radian, two turns) by -tau s.  With
    half_window = 3 tangents the largest deviation (radians) measured with the operation order of the docstring is 1.2802e-3 at 200
    points, 9.7191e-5 at 800 and 6.3345e-6 at 3200 (it falls with the square of the spacing: the chord tangents' and the double
    reflection's own error); each bar is twice the measured figure."""
    err, _ = _frenet_twist_error(n)
    print(f"helix, {n} points: twist error {err:.4e} rad (bar {bar:.2e})")
    assert err <= bar


def test_the_largest_turn_between_neighbouring_frames():
    """The voxelised helix (radius 20, pitch 6 per radian, three turns, rounded, duplicates removed: 376 voxels) after 8 smoothing passes,
    resampled at unit arc length: the rotation-minimising frame turns by at most 3.2 degrees between neighbours (the bending of the line:
    2.6 on average), the per-point rule of the lumen profile by 97 on the same points (101 on the raw voxels)."""
    from nerf_for_angiography_amd import engine
    raw = rr.voxel_helix()
    pts = engine.polyline_resample(engine.polyline_smooth(raw, 8), 1.0)
    t, u, v, flags = engine.rotation_minimising_frames(pts, 3)
    ours = np.degrees(rr.turn_angles(t, u))
    theirs = np.degrees(rr.turn_angles(*rr.per_point_frames(pts, 3)))
    print(f"{len(raw)} voxels -> {len(pts)} points: rotation-minimising {ours.max():.2f} deg (mean {ours.mean():.2f}), per point {theirs.max():.2f} deg")
    assert 350 <= len(raw) <= 420 and not flags.any()
    assert ours.max() <= 10.0
    assert theirs.max() > 45.0


def test_frames_of_degenerate_polylines():
    from nerf_for_angiography_amd import engine
    t, u, v, flags = engine.rotation_minimising_frames(np.zeros((0, 3)))
    assert t.shape == (0, 3) and flags.shape == (0,)
    t, u, v, flags = engine.rotation_minimising_frames([[1.0, 2, 3]])
    assert flags.tolist() == [engine.FRAME_KEPT] and not t.any() and not u.any()
    # a doubled point keeps the frame before it and is flagged; the frame goes on behind it
    pts = np.array([[0.0, 0, 0], [1, 0.2, 0], [2, 0.5, 0.1], [2, 0.5, 0.1], [3, 0.9, 0.3], [4, 1.0, 0.6]])
    t, u, v, flags = engine.rotation_minimising_frames(pts, 1)
    assert flags.tolist() == [0, 0, 0, engine.FRAME_KEPT, 0, 0]
    assert np.array_equal(u[3], u[2]) and np.array_equal(t[3], t[2]) and np.array_equal(v[3], v[2])
    assert np.abs((u * t).sum(axis=1)).max() <= 1e-15 and np.abs(np.sqrt((u * u).sum(axis=1)) - 1).max() <= 1e-15
    # an axis-aligned line: step 2's first smallest component decides u_0, and nothing turns
    t, u, v, flags = engine.rotation_minimising_frames(np.array([[0.0, 0, z] for z in range(6)]), 3)
    assert (t == [0, 0, 1]).all() and (u == u[0]).all() and abs(u[0, 1]) == 1.0 and not flags.any()
    with pytest.raises(ValueError, match="half_window"):
        engine.rotation_minimising_frames(pts, 0)


# ---------------------------------------------------------------- smoothing and resampling
def test_polyline_smooth():
    from nerf_for_angiography_amd import engine
    line = np.array([[1.0, 2.0, 3.0]]) + np.arange(20)[:, None] * np.array([[1.0, -2.0, 0.5]])
    assert np.array_equal(engine.polyline_smooth(line, 8, 0.5), line)      # straight and equally spaced: unchanged to the bit
    rng = np.random.default_rng(3)
    pts = line + rng.normal(0.0, 0.3, line.shape)
    out = engine.polyline_smooth(pts, 8)
    assert np.array_equal(out[0], pts[0]) and np.array_equal(out[-1], pts[-1]) and out.shape == pts.shape
    rough = lambda x: np.abs(x[:-2] - 2.0 * x[1:-1] + x[2:]).sum()
    assert rough(out) < 0.2 * rough(pts)
    one = engine.polyline_smooth(pts, 1, 0.25)                              # one Jacobi pass: every point from the old neighbours
    assert np.array_equal(one[1:-1], pts[1:-1] + 0.25 * ((pts[:-2] + pts[2:]) / 2.0 - pts[1:-1]))
    assert np.array_equal(engine.polyline_smooth(pts, 0), pts) and np.array_equal(engine.polyline_smooth(pts[:2], 8), pts[:2])


def test_polyline_resample():
    from nerf_for_angiography_amd import engine
    pts = np.array([[0.0, 0, 0], [3, 4, 0], [3, 4, 12], [3, 4, 12], [3, 10, 12]])       # lengths 5, 12, 0, 6
    out = engine.polyline_resample(pts, 2.0)
    assert len(out) == 12 and np.array_equal(out[0], pts[0])                # 0, 2, .., 22; the last partial step (23) is dropped
    assert np.allclose(out[1], [1.2, 1.6, 0.0], rtol=0, atol=1e-15) and np.allclose(out[3], [3, 4, 1.0], rtol=0, atol=1e-15)
    assert np.allclose(out[-1], [3, 9.0, 12], rtol=0, atol=1e-14)
    helix = rr.helix(400)[0]
    out = engine.polyline_resample(helix, 0.37)
    step = np.sqrt(((out[1:] - out[:-1]) ** 2).sum(axis=1))
    assert np.array_equal(out[0], helix[0]) and step.max() <= 0.37 * (1 + 1e-12) and step.min() >= 0.37 * (1 - 1e-3)      # chords of a fine polyline
    whole = engine.polyline_resample(np.array([[0.0, 0, 0], [0, 0, 3.0]]), 1.0)
    assert np.array_equal(whole[:, 2], [0.0, 1.0, 2.0, 3.0])                # an end that falls on a step is kept
    with pytest.raises(ValueError, match="spacing"):
        engine.polyline_resample(pts, 0.0)


# ---------------------------------------------------------------- the main path
SHAPE = (4, 16, 16)
LIN = lambda ijk: (ijk[0] * SHAPE[1] + ijk[1]) * SHAPE[2] + ijk[2]


def _graph(branches):
    """A hand-made `centreline_graph` result: branches = [(voxels [(i, j, k), ..] in path order, node_start, node_end, length, cycle)]."""
    vox = [LIN(v) for b in branches for v in b[0]]
    size = [len(b[0]) for b in branches]
    return {"shape": SHAPE, "path_voxels": np.array(vox, np.int64), "branch_size": np.array(size), "path_offset": np.concatenate([[0], np.cumsum(size)[:-1]]),
            "is_cycle": np.array([b[4] for b in branches]), "node_start": np.array([b[1] for b in branches]), "node_end": np.array([b[2] for b in branches]),
            "length": np.array([b[3] for b in branches], np.float64)}


def _d2(values):
    d2 = np.zeros(SHAPE, np.int64)
    for ijk, v in values.items():
        d2[ijk] = v
    return d2


def test_main_path_of_a_y_tree_with_a_reversed_branch():
    from nerf_for_angiography_amd import engine
    trunk = [(0, 8, k) for k in range(5)]                                   # free at (0, 8, 0); the junction voxel is (0, 8, 5)
    long_arm = [(0, 12, 9), (0, 11, 8), (0, 10, 7), (0, 9, 6)]              # stored from its free end: entered from its end side
    short_arm = [(0, 7, 6), (0, 6, 7)]
    g = _graph([(trunk, 0, 1, 5.0, False), (short_arm, 1, 0, 2.8, False), (long_arm, 0, 1, 5.6, False)])
    a = [[0.0, 2.0, 0.0, -1.0], [2.0, 0.0, 0.0, 3.0], [0.0, 0.0, 0.5, 0.0]]          # the first two axes exchanged, anisotropic
    d2 = _d2({trunk[0]: 9, long_arm[0]: 4, short_arm[-1]: 1})
    path = engine.centreline_main_path(g, a, d2=d2)
    assert path["branches"] == [1, 3] and path["reversed"] == [False, True]
    want = trunk + long_arm[::-1]
    assert path["voxels"].tolist() == [LIN(v) for v in want] and (path["start"], path["end"]) == (LIN(trunk[0]), LIN(long_arm[0]))
    assert path["length"] == 5.0 + 5.6
    ijk = np.array(want, np.float64)
    assert np.array_equal(path["points"], np.stack([2.0 * ijk[:, 1] - 1.0, 2.0 * ijk[:, 0] + 3.0, 0.5 * ijk[:, 2]], axis=1))
    # the junction cluster is bridged by the straight step between the two extremes next to it
    assert np.array_equal(path["points"][5] - path["points"][4], [2.0 * (9 - 8) - 0.0, 0.0, 0.5 * (6 - 4)])
    # the ostium is where d2 is largest; a given start and end are taken as they are
    other = engine.centreline_main_path(g, a, d2=_d2({trunk[0]: 1, long_arm[0]: 9, short_arm[-1]: 1}))
    assert other["branches"] == [3, 1] and other["reversed"] == [False, True] and other["voxels"].tolist() == path["voxels"].tolist()[::-1]
    chosen = engine.centreline_main_path(g, a, start=LIN(short_arm[-1]), end=LIN(trunk[0]))
    assert chosen["branches"] == [2, 1] and chosen["reversed"] == [True, True] and chosen["length"] == 2.8 + 5.0
    with pytest.raises(ValueError, match="free end"):
        engine.centreline_main_path(g, a, start=LIN(trunk[2]))


def test_main_path_ignores_cycles_and_crosses_a_single_voxel_branch():
    from nerf_for_angiography_amd import engine
    inlet = [(1, 2, k) for k in range(3)]                                   # free .. node 1
    link = [(1, 2, 4)]                                                      # one voxel between node 1 and node 2
    outlet = [(1, 2, 6), (1, 2, 7), (1, 2, 8)]                              # node 2 .. free
    ring = [(2, 5, 5), (2, 5, 6), (2, 6, 6), (2, 6, 5)]                     # a cycle: no free end, no edge
    g = _graph([(inlet, 0, 1, 3.0, False), (link, 1, 2, 2.0, False), (outlet, 2, 0, 3.0, False), (ring, 0, 0, 4.0, True)])
    path = engine.centreline_main_path(g, None)
    assert path["branches"] == [1, 2, 3] and path["reversed"] == [False, False, False] and path["length"] == 8.0
    assert path["voxels"].tolist() == [LIN(v) for v in inlet + link + outlet]
    back = engine.centreline_main_path(g, None, start=LIN(outlet[-1]))
    assert back["branches"] == [3, 2, 1] and back["reversed"] == [True, True, True]
    with pytest.raises(ValueError, match="no free end"):
        engine.centreline_main_path(_graph([(ring, 0, 0, 4.0, True)]), None)


def test_main_path_tie_rules_and_unconnected_ends():
    from nerf_for_angiography_amd import engine
    inlet = [(0, 1, 1), (0, 1, 2)]
    way_a, way_b = [(0, 2, 4), (0, 3, 5)], [(0, 0, 4), (0, 0, 5)]           # two ways from node 1 to node 2, equally long
    out_a, out_b = [(0, 1, 8), (0, 1, 9)], [(0, 3, 8), (0, 4, 9)]            # two distal ends, equally far
    g = _graph([(inlet, 0, 1, 2.0, False), (way_b, 1, 2, 3.0, False), (way_a, 1, 2, 3.0, False), (out_b, 2, 0, 2.5, False), (out_a, 2, 0, 2.5, False)])
    path = engine.centreline_main_path(g, None, start=LIN(inlet[0]))
    assert path["branches"] == [1, 2, 5]                                    # the smaller branch label; the end with the smaller voxel index
    assert path["end"] == LIN(out_a[-1]) < LIN(out_b[-1])
    # without d2 every free end ties: the smallest voxel index is the start
    assert engine.centreline_main_path(g, None)["start"] == LIN(inlet[0])
    tie = engine.centreline_main_path(g, None, d2=_d2({inlet[0]: 4, out_a[-1]: 4, out_b[-1]: 4}))
    assert tie["start"] == LIN(inlet[0])
    island = [(3, 9, 9), (3, 9, 10), (3, 9, 11)]
    two = _graph([(inlet, 0, 1, 2.0, False), (way_a, 1, 0, 3.0, False), (island, 0, 0, 2.0, False)])
    assert engine.centreline_main_path(two, None, start=LIN(island[0]))["voxels"].tolist() == [LIN(v) for v in island]
    with pytest.raises(ValueError, match="not connected"):
        engine.centreline_main_path(two, None, start=LIN(inlet[0]), end=LIN(island[-1]))


# ---------------------------------------------------------------- tables
def test_grid_tables_tiled_and_in_rows():
    from nerf_for_angiography_amd import engine
    k, step = 8, 0.25
    rows, perm_r = engine.reformat_table_grid(k, step, tiled=False)
    tiled, perm_t = engine.reformat_table_grid(k, step, tiled=True)
    side = 2 * k + 1
    assert rows.shape == tiled.shape == (side * side, 4) and perm_r.tolist() == list(range(side * side))
    assert sorted(perm_t.tolist()) == perm_r.tolist() and np.array_equal(tiled, rows[perm_t])      # the same rows up to the stated permutation
    i, j = np.divmod(np.arange(side * side), side)
    assert np.array_equal(rows[:, 0], (i - k) * step) and np.array_equal(rows[:, 1], (j - k) * step) and not rows[:, 2:].any()
    assert rows[side * k + k].tolist() == [0.0, 0.0, 0.0, 0.0]
    first = perm_t[:64]                                                     # the first 64 rows: one 8 x 8 patch
    assert set(zip((first // side).tolist(), (first % side).tolist())) == {(a, b) for a in range(8) for b in range(8)}
    back = np.empty_like(tiled)
    back[perm_t] = tiled
    assert np.array_equal(back, rows)
    assert engine.reformat_table_grid(0, 1.0)[0].tolist() == [[0.0, 0.0, 0.0, 0.0]]


def test_cpr_table_lies_on_the_grid_tables_middle_row_and_column():
    from nerf_for_angiography_amd import engine
    k, step = 5, 0.5
    side = 2 * k + 1
    grid = engine.reformat_table_grid(k, step)[0].reshape(side, side, 4)
    cpr = engine.reformat_table_cpr(k, step, (0.0, 90.0, 30.0)).reshape(3, side, 4)
    tiny = 1e-15 * k * step                                                 # cos(pi / 2) in fp64 is 6e-17, not 0
    assert np.array_equal(cpr[0, :, :2], grid[:, k, :2])                    # 0 degrees: along u, the middle column j = k
    assert np.abs(cpr[1, :, :2] - grid[k, :, :2]).max() <= tiny             # 90 degrees: along v, the middle row i = k
    assert np.abs(cpr[0, :, 2:] - [0.0, step]).max() <= tiny and np.abs(cpr[1, :, 2:] - [-step, 0.0]).max() <= tiny
    r = (np.arange(side) - k) * step
    assert np.abs(cpr[2, :, 0] - r * math.cos(math.pi / 6)).max() <= tiny and np.abs(cpr[2, :, 1] - r * math.sin(math.pi / 6)).max() <= tiny
    wide = engine.reformat_table_cpr(k, step, (30.0,), slab_step=2.0)
    assert np.abs(wide[:, 2] + 2.0 * math.sin(math.pi / 6)).max() <= tiny and np.array_equal(wide[:, :2], cpr[2, :, :2])
    assert np.abs(wide[:, 3] - 2.0 * math.cos(math.pi / 6)).max() <= tiny


# ---------------------------------------------------------------- the restatement
def test_the_restatement_on_exact_cases():
    from nerf_for_angiography_amd import engine
    rng = np.random.default_rng(5)
    vol = rng.integers(0, 200, (6, 7, 8)).astype(np.float32)
    w = engine.lumen_world_to_index(None)
    table, _ = engine.reformat_table_grid(1, 1.0)
    planes = np.array([[2.0 + p, 3.0, 4.0, 0, 1.0, 0, 0, 0, 1.0] for p in range(3)])      # u = axis 1, v = axis 2
    out = rr.reformat_planes(vol, w, planes, table).reshape(3, 3, 3)
    assert np.array_equal(out, vol[2:5, 2:5, 3:6].astype(np.float64))
    # slab: the maximum and the mean over m, in the definition's order
    slab = np.array([[0.0, 0.0, 0.0, 1.0], [0.5, 0.0, 0.25, 0.5]])
    singles = [rr.reformat_planes(vol, w, planes, np.stack([slab[:, 0] + m * slab[:, 2], slab[:, 1] + m * slab[:, 3], 0 * slab[:, 0], 0 * slab[:, 0]], 1))
               for m in (-2.0, -1.0, 0.0, 1.0, 2.0)]
    assert np.array_equal(rr.reformat_planes(vol, w, planes, slab, 2, rr.MAX), np.max(singles, axis=0))
    assert np.array_equal(rr.reformat_planes(vol, w, planes, slab, 2, rr.MEAN), ((((singles[0] + singles[1]) + singles[2]) + singles[3]) + singles[4]) / 5.0)
    assert np.array_equal(rr.reformat_planes(vol, w, planes, slab, 0, rr.MAX), singles[2])
    # outside: fill; a NaN, an infinite and a huge row are outside; the last lattice plane is inside
    bad = np.array([[np.nan] * 9, [np.inf, 0, 0, 1, 0, 0, 0, 1, 0], [1e300] * 3 + [0, 1.0, 0, 0, 0, 1.0], [5.0, 6.0, 7.0, 0, 1.0, 0, 0, 0, 1.0]])
    out, inside = rr.reformat_planes(vol, w, bad, table, 0, rr.MEAN, -1.0, return_inside=True)
    assert (out[:3] == -1.0).all() and not inside[:3].any()
    assert inside[3].reshape(3, 3)[:2, :2].all() and out[3].reshape(3, 3)[1, 1] == vol[5, 6, 7] and out[3].reshape(3, 3)[2, 2] == -1.0
    assert rr.reformat_planes(vol, w, planes[:0], table).shape == (0, 9) and rr.reformat_planes(vol, w, planes, table[:0]).shape == (3, 0)


# the bars of the phantom comparisons: 1.5 x the worst value of the restatement (0.5026 voxels; 0.02935), which the device equals bit
# for bit (tests/test_gpu_reformat.py runs the same comparison on the device's images)
WIDTH_BAR, WAIST_BAR = 0.7538, 0.0440
PHANTOM_ANGLES = (0.0, 45.0, 90.0, 135.0)


def phantom_errors(images, step, s, diameter_stenosis):
    """(the worst |width - true diameter| over all rows and angles, the worst |waist - diameter stenosis| over the angles, the smallest
    width) of the longitudinal images [A, P, K] of the stenosis phantom."""
    widths = rr.image_widths(images, step)
    true = 2.0 * lr.stenosis_radius(s)
    return float(np.abs(widths - true[None, :]).max()), max(abs(rr.waist(w) - diameter_stenosis) for w in widths), float(widths.min())


def phantom_diameter_stenosis(vol, pts):
    from nerf_for_angiography_amd import engine
    cs, coef = engine.lumen_ray_table(64)
    p = len(pts)
    prof, flags, _ = lr.lumen_profile(vol, engine.lumen_world_to_index(None), pts, np.zeros(p, np.int32), np.full(p, p - 1, np.int32), 3, 64, cs, coef,
                                      0.5, 0.5, 64)
    return float(engine.lumen_branch_summary({"area": prof[:, 0], "flags": flags, "branch": np.ones(p, np.int64)})["diameter_stenosis"][0])


def test_the_longitudinal_images_of_the_stenosis_phantom_show_its_waist():
    """Through the restatement: per row and angle the run of samples >= 0.5 misses the tube's true diameter 2 rho(s) by at most 0.5026
    voxels (one sample of 0.5, the centreline being rounded to voxels), and the waist 1 - min / lower median of each image misses the
    diameter stenosis of the lumen summary (0.4960) by at most 0.02935."""
    vol, pts, s = lr.oblique_tube(48, lr.stenosis_radius, 16)
    images, flags = rr.cpr_images_host(vol, pts, None, PHANTOM_ANGLES, 16, 0.5)
    width_err, waist_err, narrowest = phantom_errors(images, 0.5, s, phantom_diameter_stenosis(vol, pts))
    print(f"width error {width_err:.4f} voxels (bar {WIDTH_BAR}), waist error {waist_err:.5f} (bar {WAIST_BAR}), narrowest row {narrowest}")
    assert images.shape == (4, 33, 33) and narrowest > 0.0                  # every row is measured
    assert width_err <= WIDTH_BAR and waist_err <= WAIST_BAR


# ---------------------------------------------------------------- sweep and driver
def test_metric_columns_with_the_cpr_names():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.CPR_METRICS == ("CPR PSNR 3D", "CPR SSIM 3D", "CPR CORR 3D")
    others = sweep.METRICS + sweep._ALL_VOLUME_METRICS + sweep.HULL_METRICS + sweep.SIRT_METRICS + sweep.SIRT_TV_METRICS + sweep.VIEW_METRICS
    assert not set(sweep.CPR_METRICS) & set(others)
    for names, _, _ in sweep._VOLUME_FAMILIES:                              # a tuple of its own, in no family
        assert not set(sweep.CPR_METRICS) & set(names)
    got = sweep._check_metrics(["CPR CORR 3D", "VIEW REGRET 3D", "PSNR", "CPR PSNR 3D", "STENOSIS ERR 3D"], None, object())
    assert got == ["PSNR", "STENOSIS ERR 3D", "VIEW REGRET 3D", "CPR PSNR 3D", "CPR CORR 3D"]      # behind the view columns
    assert sweep._check_metrics(None, None, object()) == ["PSNR", "DOT 2D"]                        # the defaults do not grow
    for name in sweep.CPR_METRICS:
        with pytest.raises(ValueError, match="ground-truth volume"):
            sweep._check_metrics([name], None, None)


def test_cpr_scores_arithmetic():
    from nerf_for_angiography_amd.visualization.sweep import cpr_scores
    g = np.array([[[0.0, 2.0], [4.0, 1.0]]])
    same, p, q = cpr_scores(g, g)
    assert same["cpr_psnr"] == math.inf and same["cpr_corr"] == 1.0 and np.array_equal(p, g / 4.0) and np.array_equal(q, g / 4.0)
    pred = np.array([[[-1.0, 2.0], [8.0, 3.0]]])                            # normalised and clamped: 0, 0.5, 1, 0.75
    got, p, q = cpr_scores(pred, g)
    assert np.array_equal(p, [[[0.0, 0.5], [1.0, 0.75]]])
    assert got["cpr_psnr"] == -10.0 * np.log10(0.25 / 4.0) and got["cpr_corr"] == rr.pearson(p, q)
    empty, _, _ = cpr_scores(pred, np.zeros_like(g))
    assert math.isnan(empty["cpr_psnr"]) and math.isnan(empty["cpr_corr"])
    flat, _, _ = cpr_scores(np.ones_like(g), g)
    assert math.isnan(flat["cpr_corr"]) and flat["cpr_psnr"] > 0


def test_driver_checks_the_cpr_flag():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser, check_args
    base = ["--synthetic", "--img_size", "16", "--n_iters", "4"]
    args = build_parser().parse_args(base)
    assert args.save_cpr is None and args.cpr_angles == [0.0, 45.0, 90.0, 135.0] and args.cpr_half_width == 16
    check_args(build_parser().parse_args(base + ["--save_cpr", "cpr.npy", "--cpr_angles", "0", "60", "--cpr_half_width", "8"]))
    with pytest.raises(ValueError, match=".npy"):
        check_args(build_parser().parse_args(base + ["--save_cpr", "x.csv"]))
    with pytest.raises(ValueError, match="cpr_half_width"):
        check_args(build_parser().parse_args(base + ["--save_cpr", "x.npy", "--cpr_half_width", "-1"]))
