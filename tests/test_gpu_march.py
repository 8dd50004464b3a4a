"""The grid ray march on the device (engine.march: k_march_count, afx_ray_offsets, k_march_write) against the NumPy float64 restatement of
tests/march_reference.py, whose problems' preconditions tests/test_march_cpu.py asserts.

 a. exact problems (dyadic numbers, no fp32 operation rounds): rays from every side, from inside, on faces, along edges, through corners,
    ties on t_max, on cell faces and on both grid faces, grids with a partial last word and beside the scene box - bit for bit;
 b. chunk and block edges: 0 .. 257 steps per ray, every / no / every second / the first / the last step kept, 1 .. 1025 rays - bit for bit;
 c. general rays from every side: against oracle.march_grid (indices equal, floats within an ulp of the operands' magnitude) and against
    the float64 reference by margin (DESIGN: "The march against an independent reference");
 d. the per-ray count against its fp32 emulation and against afx_march_max_steps, at chosen fp32 t_min;
 e. refusals before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import march_reference as mr
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

EXACT = mr.exact_problems()
GENERAL = mr.general_problems()


def _march(p, want_points=True):
    from nerf_for_angiography_amd import engine
    bits = None if p.occ is None else torch.from_numpy(mr.pack_bits(p.occ)).to(DEV)
    return engine.march(torch.from_numpy(p.origins).to(DEV), torch.from_numpy(p.dirs).to(DEV), None if p.scene is None else list(p.scene),
                        p.near, p.far, p.dt, grid_bits=bits, grid_aabb=None if p.occ is None else list(p.grid_box),
                        grid_res=None if p.occ is None else p.grid_res, want_points=want_points)


def _assert_bit_for_bit(p):
    ri_w, ts_w, te_w, pos_w, off_w = mr.march64(p).packed()
    ri, ts, te, mid, off = _march(p)
    n = int(off_w[-1])
    assert ri.dtype == torch.int32 and off.dtype == torch.int64 and ts.dtype == te.dtype == mid.dtype == torch.float32
    assert torch.equal(off.cpu(), torch.from_numpy(off_w)), (p.name, "offsets")
    assert int(off[-1]) == n == ri.numel() == ts.numel() == te.numel() and tuple(mid.shape) == (n, 3)
    assert torch.equal(ri.cpu(), torch.from_numpy(ri_w)), (p.name, "ray_indices")
    assert bool((ri[1:] >= ri[:-1]).all())
    for name, got, want in (("t_starts", ts, ts_w), ("t_ends", te, te_w), ("mid-points", mid, pos_w)):
        w32 = want.astype(np.float32)
        assert np.array_equal(w32.astype(np.float64), want)                       # the reference value is an fp32 number
        assert torch.equal(got.cpu(), torch.from_numpy(w32)), (p.name, name, int((got.cpu() != torch.from_numpy(w32)).sum()))
    ri2, ts2, te2, none, off2 = _march(p, want_points=False)
    assert none is None and torch.equal(ri2, ri) and torch.equal(ts2, ts) and torch.equal(te2, te) and torch.equal(off2, off)
    return n


# --- a ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", EXACT, ids=[p.name for p in EXACT])
def test_exact_problems_bit_for_bit(p):
    _assert_bit_for_bit(p)


# --- b ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kept", mr.KEPT_B)
@pytest.mark.parametrize("n_rays", mr.RAY_COUNTS_B)
def test_chunk_and_block_edges_bit_for_bit(n_rays, kept):
    p = mr.chunk_problem(n_rays, kept)
    n = _assert_bit_for_bit(p)
    assert (n == 0) == (kept == "none")


# --- c ---------------------------------------------------------------------------------------------------------------------

def _same(a, b, what, scale=None):      # test_grid_kernels_vs_oracle's rule: one unit in the last place of the operands' magnitude
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape, what
    diff = (a.double() - b.double()).abs()
    tol = 1.2e-7 * (float(b.abs().max()) if scale is None else scale)
    assert bool((diff <= tol).all()), (what, int((diff > tol).sum()), float(diff.max()))


@pytest.mark.parametrize("p", GENERAL, ids=[p.name for p in GENERAL])
def test_general_rays_against_the_oracle(p):
    from oracle import angio_oracle as orc
    o, d = torch.from_numpy(p.origins), torch.from_numpy(p.dirs)
    ri_c, ts_c, te_c = orc.march_grid(o, d, torch.tensor(p.scene), p.near, p.far, p.dt, None if p.occ is None else torch.from_numpy(p.occ),
                                      None if p.occ is None else torch.tensor(p.grid_box))
    ri, ts, te, mid, off = _march(p)
    assert ri_c.numel() > 500
    assert torch.equal(ri.cpu().long(), ri_c), p.name
    _same(ts, ts_c, "t_starts"); _same(te, te_c, "t_ends")
    assert torch.equal(off.cpu(), torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(ri_c, minlength=p.n_rays).cumsum(0)]))
    _same(mid, o[ri_c] + d[ri_c] * (ts_c + te_c)[:, None] / 2.0, "mid-points", 1700.0)


@pytest.mark.parametrize("p", GENERAL, ids=[p.name for p in GENERAL])
def test_general_rays_against_the_reference_by_margin(p):
    """Decided-in steps present, decided-out steps absent, floats within the bar; at most 1 % of the candidates undecided."""
    bar, m = mr.general_bar(), mr.MARGIN_C
    assert 0 < bar <= m
    ri, ts, te, mid, off = _march(p)
    st = mr.check_margin_rule(p, mr.march64(p, beyond=3), m, bar, ri.cpu().numpy(), ts.cpu().numpy(), te.cpu().numpy(), mid.cpu().numpy())
    print(f"{p.name}: bar {bar:.3e}, m {m:.1e}; {st['candidates']} candidates, {st['undecided']} undecided ({100 * st['share']:.3f} %); device "
          f"within {st['max_dt']:.3e} (t) / {st['max_dpos']:.3e} (position) of fp64")
    assert st["share"] <= mr.UNDECIDED_CAP_C
    counts = np.diff(off.cpu().numpy())
    assert (counts[416:] == 0).all() and counts[:384].max() > 0


# --- d ---------------------------------------------------------------------------------------------------------------------

BOUND_TRIPLES = mr.bound_triples()[:6] + [t for t, n in zip(mr.bound_triples()[6:], range(3, 401)) if n in (3, 4, 31, 43, 63, 64, 65, 86, 124, 127, 128, 129, 248, 255, 256, 400)]
# (N = 43, 86, 124, 248: with t_min + k dt fused into one fma, a ray at t_min = near kept one step more than the bound)


@pytest.mark.parametrize("near,far,dt", BOUND_TRIPLES, ids=[f"near{n:g}-far{f:g}-dt{d:g}" for n, f, d in BOUND_TRIPLES])
def test_step_count_and_bound_on_the_device(near, far, dt):
    """No grid: the per-ray counts are march_range's.  The ray starts at z = t_min on the axis and looks along -z at a box whose upper z
    face is z = 0 and which is far oversized otherwise: it enters at t = (0 - z) * (1 / -1) = z exactly, and t_min = max(z, near)."""
    from nerf_for_angiography_amd import _lib, engine
    t_min = mr.tmin_windows(near, far, dt, 3000)
    entry = np.concatenate([t_min, np.array([0.0, near / 2, near], np.float32)])      # the last three enter the box before `near`: clamped
    t_min = np.maximum(entry, np.float32(near))
    assert 3000 < t_min.size <= 4000
    o = np.zeros((t_min.size, 3), np.float32)
    o[:, 2] = entry
    d = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (t_min.size, 1))
    box = [-1e6, -1e6, -1e6, 1e6, 1e6, 0.0]
    ri, ts, te, _, off = engine.march(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV), box, near, far, dt, want_points=False)
    counts = np.diff(off.cpu().numpy())
    want = mr.count32(t_min, np.full(t_min.shape, far, np.float32), dt)
    assert np.array_equal(counts, want), (int((counts != want).sum()), t_min[counts != want][:5], counts[counts != want][:5], want[counts != want][:5])
    first = off.cpu().numpy()[:-1][counts > 0]
    assert np.array_equal(ts.cpu().numpy()[first], t_min[counts > 0])              # t_min is the chosen number
    m = _lib.MarchArgs()
    m.n_rays, m.has_aabb, m.step = 1, 0, float(dt)
    m.has_near, m.near_plane, m.has_far, m.far_plane = 1, float(near), 1, float(far)
    bound = int(_lib.load().afx_march_max_steps(C.byref(m)))
    print(f"near {near:g} far {far:g} dt {dt:g}: {t_min.size} rays, counts {counts.min()} .. {counts.max()}, bound {bound}")
    assert counts.max() <= bound and counts[0] == bound                            # the first ray starts at max(0, near)


# --- e ---------------------------------------------------------------------------------------------------------------------

def test_refusals_before_any_launch():
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd._lib import AfxError
    o = torch.zeros(8, 3, device=DEV)
    o[:, 2] = 100.0
    d = torch.tensor([[0.0, 0.0, -1.0]], device=DEV).repeat(8, 1)
    box, res = list(mr.SCENE_A), (3, 5, 7)
    bits = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    ri, *_ = engine.march(o, d, box, None, None, 2.0, grid_bits=bits, grid_aabb=box, grid_res=res)      # 105 cells, 4 words: accepted
    assert ri.numel() == 8 * 64
    refused = (ValueError, AfxError)
    with pytest.raises(refused, match=r"grid_bits must be .*at least 4 elements .*got torch\.int32 \(3,\)"):
        engine.march(o, d, box, None, None, 2.0, grid_bits=bits[:3], grid_aabb=box, grid_res=res)
    with pytest.raises(refused, match=r"grid_bits must be .*at least 120 elements .*got torch\.int32 \(4,\)"):
        engine.march(o, d, box, None, None, 2.0, grid_bits=bits, grid_aabb=box, grid_res=(16, 12, 20))
    with pytest.raises(refused, match=r"grid_bits must be a contiguous torch\.int32 .*got torch\.int64"):
        engine.march(o, d, box, None, None, 2.0, grid_bits=bits.to(torch.int64), grid_aabb=box, grid_res=res)
    with pytest.raises(refused, match=r"grid_bits must be a contiguous torch\.int32 .*got torch\.uint8"):
        engine.march(o, d, box, None, None, 2.0, grid_bits=bits.to(torch.uint8), grid_aabb=box, grid_res=res)
    with pytest.raises(refused, match=r"grid_bits must be .* on cuda:0, got .* on cpu"):
        engine.march(o, d, box, None, None, 2.0, grid_bits=bits.cpu(), grid_aabb=box, grid_res=res)
    with pytest.raises(refused, match="grid_aabb and grid_res"):
        engine.march(o, d, box, None, None, 2.0, grid_bits=bits, grid_res=res)
    with pytest.raises(refused, match="grid_aabb and grid_res"):
        engine.march(o, d, box, None, None, 2.0, grid_bits=bits, grid_aabb=box)
    with pytest.raises(refused, match=r"\[R, 3\]"):
        engine.march(o, d[:7], box, None, None, 2.0)
    with pytest.raises(refused, match=r"\[R, 3\]"):
        engine.march(o.reshape(-1), d.reshape(-1), box, None, None, 2.0)
    with pytest.raises(refused, match=r"\[R, 3\]"):
        engine.march(o.reshape(6, 4), d.reshape(6, 4), box, None, None, 2.0)
    with pytest.raises(refused, match=r"\[R, 3\]"):
        engine.march(o, d.reshape(2, 4, 3), box, None, None, 2.0)
    for step in (0.0, -2.0, float("nan")):
        with pytest.raises(refused, match="must be > 0"):
            engine.march(o, d, box, None, None, step)
    with pytest.raises(refused, match="neither"):
        engine.march(o, d, None, 10.0, None, 2.0)
    ri, *_ = engine.march(o, d, None, 10.0, 30.0, 2.0)                                                  # a far plane alone is enough
    assert ri.numel() == 8 * 10
