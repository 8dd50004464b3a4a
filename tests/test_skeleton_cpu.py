"""3-D thinning without a GPU: the sequential yardstick of the GPU tests (tests/skeleton_reference.py) on shapes with a known answer,
the simple-point predicate the kernels call (afx_simple_point_26, a host export of the same function) against the yardstick's
scipy.ndimage.label form, the clDice arithmetic and the sweep's handling of the centreline metric names, and the argument checks and
workspace query of afx_skeletonize_3d (include/afx.h), which return before any HIP call."""
import ctypes as C
import itertools

import numpy as np
import pytest

import skeleton_reference as sk

AFX_E_INVALID, AFX_E_WORKSPACE = -1, -2
FAKE = C.c_void_p(0x10000)          # never dereferenced: every call below is refused before it reaches the device


@pytest.fixture(scope="module")
def lib():
    from nerf_for_angiography_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def thinned():
    """{name: (mask, skeleton, record)} of the reference, computed once."""
    rng = np.random.default_rng(3)
    shapes = {"bar": sk.bar(), "torus": sk.torus(), "shell": sk.shell(), "cube": sk.cube(), "tree": sk.capsule_tree(48),
              "noise 50 %": rng.random((9, 17, 33)) < 0.5, "noise 90 %": rng.random((7, 9, 33)) < 0.9,
              "smooth noise": sk.smooth_noise((17, 18, 19), 3)}
    return {name: (m, *sk.skeletonize(m)) for name, m in shapes.items()}


def test_invariants_subset_and_idempotence_on_every_shape(thinned):
    for name, (m, s, rec) in thinned.items():
        assert not (s & ~m).any(), name                                            # a subset of the input
        assert sk.invariants(s) == sk.invariants(m), (name, sk.invariants(m), sk.invariants(s))
        assert rec["converged"] == 1 and rec["deleted_last"] == 0 and rec["remaining"] == s.sum() == m.sum() - rec["deleted"], name
        again, rec2 = sk.skeletonize(s)
        assert np.array_equal(again, s) and rec2["passes"] == 1 and rec2["deleted"] == 0, name
        assert sk.undeleted_candidates(s) == 0, name


def test_the_bar_gives_its_centre_line(thinned):
    m, s, rec = thinned["bar"]
    assert m.sum() == 450 and s.sum() == 16 and rec["passes"] == 3
    line = np.zeros_like(m)
    line[4, 5, 4:18] = True                                                        # the axis of the bar [2:7, 3:8, 2:20]
    assert not (line & ~s).any()
    assert np.argwhere(s & ~line).tolist() == [[3, 5, 3], [5, 5, 3]]               # the two-voxel fork at one end
    assert sk.end_points(s).sum() == 3


def test_the_torus_gives_one_closed_loop(thinned):
    m, s, rec = thinned["torus"]
    assert sk.invariants(m) == (1, 0, 0) and rec["passes"] == 4
    assert sk.components26(s) == 1 and (sk.n_neighbours(s)[s] == 2).all()


def test_the_shell_keeps_its_cavity_and_the_cube_its_diagonal(thinned):
    m, s, rec = thinned["shell"]
    assert sk.invariants(m) == sk.invariants(s) == (1, 1, 2) and rec["passes"] == 3
    assert not s[9, 9, 9] and sk.end_points(s).sum() == 0                          # still a closed surface around the centre
    m, s, rec = thinned["cube"]
    assert m.sum() == 4096 and rec["passes"] == 9
    assert np.argwhere(s).tolist() == [[d, d, d] for d in range(1, 16)]            # the order of the subfields picks this diagonal


def test_the_tree_thins_to_curves(thinned):
    m, s, rec = thinned["tree"]
    assert sk.invariants(m) == (1, 0, 1) and rec["passes"] == 5
    assert sk.n_neighbours(s)[s].max() <= 4 and sk.end_points(s).sum() >= 4        # curve voxels; the 4 true ends and some short spurs
    assert s.sum() < 0.05 * m.sum()


def test_max_passes_stops_early(thinned):
    m, s, rec = thinned["cube"]
    for k in (1, 4, 8):
        part, r = sk.skeletonize(m, max_passes=k)
        assert r["passes"] == k and r["converged"] == 0 and not (s & ~part).any()
    assert np.array_equal(sk.skeletonize(m, max_passes=8)[0], s)                   # the 9th pass only finds nothing left to delete
    assert sk.skeletonize(m, max_passes=9)[1] == rec


def _words_with(k_bits):
    """Every 27-bit word (centre clear) with exactly k of the 26 neighbour bits set."""
    pos = [b for b in range(27) if b != 13]
    return [sum(1 << b for b in c) for c in itertools.combinations(pos, k_bits)]


def _same(lib, words):
    bad = [w for w in words if lib.afx_simple_point_26(w) != int(sk.is_simple(sk.cube_of(w)))]
    assert not bad, (len(bad), [hex(w) for w in bad[:5]])


def test_simple_point_on_sparse_and_full_words(lib):
    all26 = (1 << 27) - 1 - (1 << 13)
    few = [w for k in range(4) for w in _words_with(k)]
    assert len(few) == 1 + 26 + 325 + 2600
    _same(lib, few)
    _same(lib, [all26 ^ w for w in few])                                           # at least 23 neighbour bits set
    assert lib.afx_simple_point_26(0) == 0 and lib.afx_simple_point_26(all26) == 0  # isolated; interior


def test_simple_point_on_single_neighbours_and_the_ignored_bits(lib):
    singles = _words_with(1)
    offs = {w: sum(abs(d - 1) for d in np.unravel_index(w.bit_length() - 1, (3, 3, 3))) for w in singles}
    assert sorted(offs.values()).count(1) == 6 and sorted(offs.values()).count(2) == 12 and sorted(offs.values()).count(3) == 8
    for w in singles:                                                              # a curve end point is simple (the end-point rule keeps it)
        assert lib.afx_simple_point_26(w) == 1 == int(sk.is_simple(sk.cube_of(w))), hex(w)
    rng = np.random.default_rng(7)
    for w in rng.integers(0, 1 << 27, 200).tolist():                               # the centre bit and the bits from 27 up change nothing
        want = lib.afx_simple_point_26(w)
        assert lib.afx_simple_point_26(w ^ (1 << 13)) == want and lib.afx_simple_point_26(w | 0xf8000000) == want


@pytest.mark.parametrize("p", [0.2, 0.5, 0.8])
def test_simple_point_on_random_words(lib, p):
    rng = np.random.default_rng(int(p * 10))
    words = ((rng.random((7000, 27)) < p).astype(np.int64) << np.arange(27)).sum(1).tolist()
    _same(lib, words)
    got = sum(lib.afx_simple_point_26(w) for w in words)
    assert 0 < got < len(words)                                                    # both answers occur


def test_cldice_arithmetic_on_hand_made_masks():
    import torch
    from nerf_for_angiography_amd.visualization.sweep import cldice_scores
    a = sk.capsule((12, 14, 30), (6, 7, 4), (6, 7, 25), 2.6)
    sa = sk.skeletonize(a)[0]
    t = torch.from_numpy
    same = cldice_scores(t(a), t(a), t(sa), t(sa))
    assert same["cldice"] == same["tprec"] == same["tsens"] == 1.0 and same["n_skeleton"] == same["n_skeleton_gt"] == sa.sum()
    far = np.zeros_like(a)                                                         # a line that shares no voxel with the capsule
    far[0, 0, 2:20] = True
    assert not (a & far).any()
    sfar = sk.skeletonize(far)[0]
    apart = cldice_scores(t(a), t(far), t(sa), t(sfar))
    assert apart["cldice"] == apart["tprec"] == apart["tsens"] == 0.0
    for shift, axis in ((1, 0), (1, 2), (2, 1)):
        r = np.roll(a, shift, axis=axis)
        sr_ = sk.skeletonize(r)[0]
        want = sk.cldice(a, r, sa, sr_)
        got = cldice_scores(t(a), t(r), t(sa), t(sr_))
        assert (got["cldice"], got["tprec"], got["tsens"]) == want[:3], (shift, axis)
        assert got["tprec"] == int((sa & r).sum()) / int(sa.sum()) and 0.0 < got["cldice"] <= 1.0
    with pytest.raises(ValueError, match="empty"):
        cldice_scores(t(a), t(a), t(np.zeros_like(a)), t(sa))


def test_metric_columns_with_the_centreline_names():
    from nerf_for_angiography_amd.visualization import sweep
    assert sweep.CENTRELINE_METRICS == ("CLDICE 3D", "TPREC 3D", "TSENS 3D")
    got = sweep._check_metrics(["TSENS 3D", "DICE 3D LCC", "CLDICE 3D", "HD 3D", "PSNR", "TPREC 3D", "DOT 3D"], None, object())
    assert got == ["PSNR", "DOT 3D", "HD 3D", "DICE 3D LCC", "CLDICE 3D", "TPREC 3D", "TSENS 3D"]
    assert sweep._check_metrics("CLDICE 3D", None, object()) == ["CLDICE 3D"]
    assert sweep._check_metrics(None, None, object()) == ["PSNR", "DOT 2D"]          # the defaults do not grow
    for name in sweep.CENTRELINE_METRICS:
        with pytest.raises(ValueError, match="volume"):
            sweep._check_metrics([name], None, None)
    with pytest.raises(ValueError, match="unknown"):
        sweep._check_metrics(["CLDICE 3D", "CLDICE 2D"], None, object())


class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"evaluation_sweep touched the model ({name}) before rejecting its arguments")


def test_evaluation_sweep_refuses_centreline_metrics_before_gpu_work():
    from nerf_for_angiography_amd.visualization.sweep import evaluation_sweep
    args = dict(model=_NoModel(), targets=None, angles=np.zeros((4, 2)), img_width=8, img_height=8, focal_length=100.0,
                src_pt=np.array([0, 0, 1500.0]), near_thresh=1400.0, far_thresh=1600.0, depth_samples_per_ray=16)
    with pytest.raises(ValueError, match="volume"):
        evaluation_sweep(metrics=["PSNR", "CLDICE 3D"], **args)
    with pytest.raises(AssertionError, match="touched the model"):       # a request it can serve goes on to the model
        evaluation_sweep(metrics=["TSENS 3D"], volume=object(), **args)


def test_host_tensors_are_refused():
    import torch
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd._lib import AfxError
    with pytest.raises(AfxError):
        engine.skeletonize_3d(torch.ones(4, 5, 6))
    with pytest.raises(AfxError):
        engine.skeletonize_3d(np.ones((4, 5, 6), np.uint8))
    with pytest.raises(AfxError):
        engine.skeleton_record(torch.ones(4, 5, 6, dtype=torch.uint8), 3)


BAD_SHAPES = ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1025, 4, 4), (4, 1025, 4), (4, 4, 1025), (1 << 20, 1, 1))


def test_workspace_query_equals_the_documented_formula(lib):
    for shape in ((1, 1, 1), (5, 7, 3), (33, 17, 65), (201, 201, 201), (1024, 1, 1)):
        cap = ((shape[0] + 1) // 2) * ((shape[1] + 1) // 2) * ((shape[2] + 1) // 2)
        want = (8 * cap * 4 + 255) // 256 * 256 + 256
        assert lib.afx_skeletonize_3d_workspace_bytes(*shape) == want, shape
    for bad in BAD_SHAPES:
        assert lib.afx_skeletonize_3d_workspace_bytes(*bad) == 0, bad


def test_skeletonize_argument_validation(lib):
    def call(fg=FAKE, shape=(4, 5, 6), max_passes=8, sync_every=0, skel=FAKE, rec=FAKE, ws=FAKE, nbytes=1 << 40):
        return lib.afx_skeletonize_3d(fg, *shape, max_passes, sync_every, skel, rec, ws, nbytes, None)
    assert call(fg=None) == AFX_E_INVALID and call(skel=None) == AFX_E_INVALID and call(rec=None) == AFX_E_INVALID
    for bad in BAD_SHAPES:
        assert call(shape=bad) == AFX_E_INVALID, bad
    for k in (0, -1):
        assert call(max_passes=k) == AFX_E_INVALID and b"max_passes" in lib.afx_last_error(), k
    assert call(sync_every=-1) == AFX_E_INVALID and b"sync_every" in lib.afx_last_error()
    assert call(nbytes=8) == AFX_E_WORKSPACE and call(ws=None) == AFX_E_WORKSPACE and b"workspace" in lib.afx_last_error()
    assert call(nbytes=lib.afx_skeletonize_3d_workspace_bytes(4, 5, 6) - 1) == AFX_E_WORKSPACE
