"""The grid ray march without a GPU: the preconditions of tests/test_gpu_march.py and the host-side bound.

 - the exact problems (a, b) really are exact: the kernels' arithmetic with every operation rounded to fp32 (march_reference.march32)
   gives the float64 reference bit for bit, so any deviation on the device is the kernel's; they hold the ties, origins, near / far
   settings, grids and occupancies they are meant to hold;
 - the general problems (c): oracle.march_grid obeys the margin rule against the float64 reference, the undecided share stays under
   its cap, and the margin is no smaller than the bar the fp32 emulation's distance gives;
 - afx_march_max_steps bounds march_range's count for every t_min tried and is attained at t_min = max(0, near)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import march_reference as mr
from oracle import angio_oracle as orc


@functools.lru_cache(maxsize=None)
def _exact():
    return [(p, mr.march64(p, beyond=1)) for p in mr.exact_problems()]


def _assert_exact(p, m):
    ri, ts, te, pos, off = m.packed()
    ri32, ts32, te32, mid32, off32, _, dec32 = mr.march32(p)
    assert np.array_equal(ri, ri32) and np.array_equal(off, off32), p.name
    for name, a, b in (("t_starts", ts, ts32), ("t_ends", te, te32), ("mid-points", pos, mid32), ("decision points", pos, dec32)):
        assert b.dtype == np.float32 and np.array_equal(a, b.astype(np.float64)), (p.name, name)
    assert off[-1] == ri.size and (np.diff(ri) >= 0).all()


def test_reference_on_hand_computed_rays():
    """The reference itself, on rays whose march is known in closed form."""
    def one(o, d, near, far, dt, scene=mr.SCENE_A, **grid):
        p = mr.Problem("hand", np.array([o], np.float32), np.array([d], np.float32), scene, near, far, dt, **grid)
        return mr.march64(p).packed()
    ri, ts, te, pos, off = one((1, 10, 100), (0, 0, -1), None, None, 2.0)
    assert ri.size == 64 and ts[0] == 36.0 and te[-1] == 164.0 and (pos[:, 2] == 63.0 - 2.0 * np.arange(64)).all() and off.tolist() == [0, 64]
    assert one((1, 10, 100), (0, 0, -1), None, 57.0, 2.0)[0].size == 10          # mid-points 37 .. 55; 57 == t_max is out
    assert one((1, 10, 100), (0, 0, -1), None, 57.5, 2.0)[0].size == 11
    assert one((1, 10, 100), (0, 0, -1), 37.0, None, 2.0)[0].size == 63          # mid-points 38 .. 162; 164 == t_max is out
    assert one((1, 10, 100), (0, 0, 1), None, None, 2.0)[0].size == 0            # the box is behind the ray
    assert one((1, 10, 3), (0, 0, -1), None, None, 2.0)[0].size == 33            # from inside: t_min = 0, t_max = 67, mid-points 1 .. 65
    assert one((1, 10, -64), (1, 0, 0), None, None, 2.0)[0].size == 31           # lower face, zero component: grazes (t_max = 63, mid-points 1 .. 61)
    assert one((1, 10, 64), (1, 0, 0), None, None, 2.0)[0].size == 0             # upper face: misses
    assert one((1, 10, -64), (-0.0, 1, 0), None, None, 2.0)[0].size == 43        # -0.0 is a zero component (y: 10 .. 96)
    assert one((-104, 8, 3), (1, -1, 0), None, None, 2.0)[0].size == 0           # touches an edge at one t
    # one occupied cell of (16, 12, 20) on SCENE_A: cells are 8 x 32/3 x 6.4; cell (8, 3, 10) = [0, 8) x [0, 10.67) x [0, 6.4)
    occ = np.zeros((16, 12, 20), bool)
    occ[8, 3, 10] = True
    assert mr.pack_bits(occ).view(np.uint32)[((8 * 12 + 3) * 20 + 10) >> 5] == 1 << (((8 * 12 + 3) * 20 + 10) & 31)
    ri, ts, te, pos, _ = one((1, 1, 101), (0, 0, -1), 38.0, None, 2.0, grid_box=mr.SCENE_A, grid_res=(16, 12, 20), occ=occ)
    assert pos[:, 2].tolist() == [6.0, 4.0, 2.0, 0.0]                            # z = 0 belongs to the upper cell, z = 6.4 .. 0
    ri, ts, te, pos, _ = one((1, 10, 101), (0, 0, -1), 38.0, 150.0, 2.0, grid_box=mr.GRID_INNER, grid_res=(1, 1, 1), occ=np.ones((1, 1, 1), bool))
    assert pos[0, 2] == 30.0 and pos[-1, 2] == -32.0 and ri.size == 32          # u = 1 (z = 32) is outside, u = 0 (z = -32) inside


def test_exact_problems_are_exact_in_fp32():
    for p, m in _exact():
        _assert_exact(p, m)


def test_exact_problems_cover_what_they_claim():
    probs = _exact()
    p0 = probs[0][0]
    o, d = p0.origins.astype(np.float64), p0.dirs.astype(np.float64)
    lo, hi = np.array(mr.SCENE_A[:3]), np.array(mr.SCENE_A[3:])
    assert ((o * 2) == np.rint(o * 2)).all()                                              # integers and halves
    for dv in mr.DIRS_A:
        assert (p0.dirs == np.array(dv, np.float32)).all(1).any(), dv
    assert (np.signbit(p0.dirs) & (p0.dirs == 0)).any()                                   # a -0.0 component
    for q in range(3):                                                                   # outside each of the six faces, heading in
        assert ((o[:, q] < lo[q]) & (d[:, q] > 0)).any() and ((o[:, q] > hi[q]) & (d[:, q] < 0)).any()
    inside = ((o > lo) & (o < hi)).all(1)
    on_face = ((o == lo) | (o == hi)).any(1) & ((o >= lo) & (o <= hi)).all(1)
    along = (((o == lo) | (o == hi)) & (d == 0)).any(1)
    assert inside.any() and on_face.any() and (on_face & along).any() and (along & ((o == lo) & (d == 0)).any(1)).any() \
        and (along & ((o == hi) & (d == 0)).any(1)).any()
    assert ((((o == lo) | (o == hi)) & (d == 0)).sum(1) == 2).any()                       # along an edge
    m0 = mr.march64(p0)
    assert np.isnan(m0.t_min).any() and (m0.t_min == m0.t_max).any()                      # misses, and touching at one t (edge / corner)
    # settings
    assert {(p.near, p.far) for p, _ in probs} >= set(mr.NEAR_FAR_A) and {p.dt for p, _ in probs} == {0.5, 2.0}
    assert any(p.near is not None and p.far is not None and p.near > p.far for p, _ in probs)
    assert {p.grid_res for p, _ in probs} >= {None, (1, 1, 1), (3, 5, 7), (16, 12, 20)}
    assert {p.grid_box for p, _ in probs} >= {None, mr.SCENE_A, mr.GRID_INNER, mr.GRID_PARTIAL}
    assert {t for p, _ in probs for t in p.tags} >= {"all", "none", "checker", "fill30"}
    assert (3 * 5 * 7) % 32 != 0 and mr.pack_bits(np.ones((3, 5, 7), bool)).view(np.uint32)[-1] == (1 << (105 % 32)) - 1
    # ties, by construction
    tie_tmax = sum(int((m.m_tmax == 0).sum()) for _, m in probs)
    tie_far = sum(int(((m.m_tmax == 0) & (m.t_max[m.ray] == (p.far if p.far is not None else np.nan))).sum()) for p, m in probs)
    grid = [(p, m) for p, m in probs if p.occ is not None]
    interior = [sum(int((m.in_range & (m.face_axes[:, q] == 0) & (m.u[:, q] > 0) & (m.u[:, q] < 1) & (m.outside_by == 0)).sum())
                    for p, m in grid if p.grid_res == (16, 12, 20)) for q in range(3)]
    others_in = lambda m, q: np.all([(m.u[:, a] >= 0) & (m.u[:, a] < 1) for a in range(3) if a != q], axis=0)
    lower = sum(int((m.in_range & (m.u[:, q] == 0) & others_in(m, q)).sum()) for _, m in grid for q in range(3))
    upper = sum(int((m.in_range & (m.u[:, q] == 1) & others_in(m, q)).sum()) for _, m in grid for q in range(3))
    upper_inner = sum(int((m.in_range & (m.u[:, q] == 1) & others_in(m, q)).sum()) for p, m in grid if p.grid_box == mr.GRID_INNER for q in range(3))
    print(f"ties: t_max {tie_tmax} (far {tie_far}), interior cell faces per axis {interior}, lower grid face {lower}, upper grid face {upper}")
    assert tie_tmax > 0 and tie_far > 0 and tie_tmax > tie_far and min(interior) > 0 and lower > 0 and upper > 0 and upper_inner > 0
    assert sum(int(m.keep.sum()) for _, m in probs) > 50000 and sum(m.keep.sum() == 0 for _, m in probs) >= 4


@pytest.mark.parametrize("kept", mr.KEPT_B)
def test_chunk_problems_are_exact_and_have_the_wanted_counts(kept):
    for n_rays in mr.RAY_COUNTS_B:
        p = mr.chunk_problem(n_rays, kept)
        m = mr.march64(p, beyond=1)
        _assert_exact(p, m)
        in_range = np.bincount(m.ray[m.in_range], minlength=n_rays)
        counts, clamped = np.array(mr.chunk_counts(n_rays)), np.array(mr.chunk_clamped(n_rays))
        assert np.array_equal(in_range, counts), (n_rays, kept)
        assert np.array_equal(mr.count32(*mr.range32(p), p.dt), counts)
        shift = np.where(clamped, 8, 0)                                                     # a clamped ray's step k sits where step k + 8 would
        assert (m.t_min == np.where(clamped, mr.NEAR_B, mr.FAR_B - mr.DT_B * counts)).all() and (m.t_min >= mr.NEAR_B).all()
        assert (m.k[m.in_range] + shift[m.ray[m.in_range]] == 511 - np.floor(m.u[m.in_range, 2] * 512)).all()
        occupied = set(mr.chunk_kept_steps(n_rays, kept))
        want = np.array([sum(1 for k in range(c) if k + s in occupied) for c, s in zip(counts, shift)])
        assert np.array_equal(np.bincount(m.ray[m.keep], minlength=n_rays), want), (n_rays, kept)
        free = ~clamped & (counts > 0)
        closed = {"all": counts, "none": 0 * counts, "alternate": (counts + 1) // 2, "first": np.minimum(counts, 1)}.get(kept)
        if closed is not None:
            assert np.array_equal(want[free], closed[free])
        else:                                                                               # "last": the very last step of every ray is kept
            assert all(m.k[m.keep & (m.ray == r)].max() == counts[r] - 1 for r in np.flatnonzero(free))
    assert set(mr.chunk_counts(1025)) == set(mr.STEP_COUNTS_B) and len(set(mr.chunk_counts(3))) == 3 and mr.chunk_counts(1) == [257]
    assert 40 < sum(mr.chunk_clamped(1025)) < 80 and not any(mr.chunk_clamped(1))


def test_general_problems_oracle_obeys_the_margin_rule():
    """oracle.march_grid (fp32, the kernels' expressions) against the float64 reference, by margin; the undecided share; bar <= m."""
    probs = mr.general_problems()
    o, d = probs[0].origins.astype(np.float64), probs[0].dirs.astype(np.float64)
    assert probs[0].n_rays == 448 and len({tuple(r) for r in np.sign(d[:384]).tolist()} & {(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)}) == 8
    assert np.allclose(np.linalg.norm(o[:384] - [0, 10, 0], axis=1), 1500, atol=1e-3) and np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-6)
    lo, hi = np.array(mr.SCENE_C[:3]), np.array(mr.SCENE_C[3:])
    assert ((o[384:416] > lo) & (o[384:416] < hi)).all()
    marches = [mr.march64(p, beyond=3) for p in probs]
    assert all(np.isnan(m.t_min[416:]).all() and not np.isnan(m.t_min[:416]).any() for m in marches)
    dist = [mr.fp32_distance(p, m) for p, m in zip(probs, marches)]
    bar = mr.general_bar()
    print(f"fp32 emulation against fp64: largest distance in t {max(a for a, _ in dist):.3e}, in position {max(b for _, b in dist):.3e}; "
          f"bar = 4 x = {bar:.3e}; m = {mr.MARGIN_C:.1e}")
    assert bar == 4 * max(max(a, b) for a, b in dist) and 0 < bar <= mr.MARGIN_C
    for p, m in zip(probs, marches):
        binary = None if p.occ is None else torch.from_numpy(p.occ)
        ri, ts, te = orc.march_grid(torch.from_numpy(p.origins), torch.from_numpy(p.dirs), torch.tensor(p.scene), p.near, p.far, p.dt, binary,
                                    None if p.occ is None else torch.tensor(p.grid_box))
        mid = p.origins[ri.numpy()] + p.dirs[ri.numpy()] * (ts + te).numpy()[:, None] / np.float32(2.0)
        st = mr.check_margin_rule(p, m, mr.MARGIN_C, bar, ri.numpy(), ts.numpy(), te.numpy(), mid)
        print(f"{p.name}: {st['candidates']} candidates, {st['undecided']} undecided ({100 * st['share']:.3f} %), "
              f"oracle within {st['max_dt']:.3e} (t) / {st['max_dpos']:.3e} (position)")
        assert st["share"] <= mr.UNDECIDED_CAP_C and st["candidates"] > 3000
        assert p.occ is None or st["undecided"] > 0


# --- the bound -------------------------------------------------------------------------------------------------------------

def _bound(near, far, dt):
    from nerf_for_angiography_amd import _lib
    lib = _lib.load()
    m = _lib.MarchArgs()
    m.n_rays, m.has_aabb, m.step = 1, 0, float(dt)
    m.has_near, m.near_plane, m.has_far, m.far_plane = 1, float(near), 1, float(far)
    return int(lib.afx_march_max_steps(C.byref(m)))


def test_step_bound_covers_every_t_min():
    """march_range's count, emulated in fp32 (ceil, then the two mid-point corrections, separate rounded operations), never exceeds
    afx_march_max_steps, for every fp32 t_min of the windows: 0 .. 8 ulps above near, within 8 ulps of near + j dt / 2 (j = 0 .. 6),
    10 000 random ones in [near, far]; and equals it at t_min = max(0, near).  (DESIGN: why the bound holds for every t_min.)"""
    triples = mr.bound_triples()
    assert len(triples) == 6 + 398
    ratios = [(f - n) / d for n, f, d in triples[6:]]
    assert all(abs(r - (i + 3.5)) < 1e-3 for i, r in enumerate(ratios))
    cases, worst = 0, 0
    for near, far, dt in triples:
        bound = _bound(near, far, dt)
        t_min = mr.tmin_windows(near, far, dt, 10000)
        assert t_min.dtype == np.float32 and t_min.size > 10000 and t_min.min() == np.float32(max(near, 0.0))
        n = mr.count32(t_min, np.full(t_min.shape, far, np.float32), dt)
        cases += t_min.size
        worst = max(worst, int((n - bound).max()))
        assert (n <= bound).all(), (near, far, dt, bound, int(n.max()), float(t_min[n.argmax()]))
        at_near = mr.count32(np.array([max(near, 0.0)], np.float32), np.array([far], np.float32), dt)
        assert int(at_near[0]) == bound, (near, far, dt, bound, int(at_near[0]))
    print(f"no t_min above the bound over {cases} cases of {len(triples)} triples (largest count - bound: {worst})")
    assert worst == 0


def test_count_emulation_agrees_with_the_oracle_march():
    """The fp32 count emulation against oracle.march_grid's step counts on the named triples (no box: every ray spans [near, far])."""
    for near, far, dt in mr.bound_triples()[:6]:
        t_min = mr.tmin_windows(near, far, dt, 40)[::7]
        want = mr.count32(t_min, np.full(t_min.shape, far, np.float32), dt)
        for tm, w in zip(t_min.tolist(), want.tolist()):
            ri, _, _ = orc.march_grid(torch.zeros(1, 3), torch.tensor([[0.0, 0.0, 1.0]]), None, tm, far, dt)
            assert ri.numel() == w
