"""The packed-sample kernels at ragged lengths and chunk boundaries: afx_march_visibility (vis_chunk, the 64-lane transmittance scan
k_march_render_composite and k_single_eval_composite share), afx_march_compact, afx_ray_offsets, afx_pack_groups, afx_composite_packed with
its backward, afx_fine_depths / afx_fine_depths_from_tau - each against the plain restatement of tests/packed_reference.py.

The problems come from the seeded CPU builders of tests/packed_reference.py; tests/test_packed_edges_cpu.py asserts their preconditions
(exact problems: fp32 and fp64 give the same mask; raw path: no decision within 1e-3 of a threshold; fine depths: no draw with
cdf[above] - cdf[below] in [1e-6, 1e-4]) and these tests assume them.  Where a result is not exact the bar is taken from the fp32 CPU
restatement's own distance to the fp64 one, and every test prints the measured error next to it."""
import ctypes as C

import pytest
import torch

import packed_reference as pr
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- a. visibility on exact problems: vis_chunk, the T carry between chunks, k_march_compact and the offsets behind it -------------------
@pytest.mark.parametrize("eps,thre", pr.EXACT_PAIRS)
def test_visibility_exact(eps, thre):
    from nerf_for_angiography_amd import engine
    for v in range(pr.N_VARIANTS):
        alphas, ts, te, off = pr.exact_visibility_problem(eps, v)
        keep, _ = pr.render_visibility(alphas, off, eps, thre)
        ri_c, ts_c, te_c, off_c = pr.compact(keep, off, ts, te)
        ri, ts2, te2, off2 = engine.march_visibility(alphas.to(DEV), ts.to(DEV), te.to(DEV), off.to(DEV), eps, thre, is_alpha=True,
                                                     return_offsets=True)
        assert ri.dtype == torch.int32 and off2.dtype == torch.int64
        assert torch.equal(off2.cpu(), off_c), (v, off2.tolist(), off_c.tolist())
        assert torch.equal(ri.cpu(), ri_c) and torch.equal(ts2.cpu(), ts_c) and torch.equal(te2.cpu(), te_c), v
        if eps == 2.0:      # T = 1 < eps in front of the first sample: nothing is kept
            assert ri.numel() == 0 and ts2.numel() == 0 and te2.numel() == 0 and not bool(off2.any())
        else:
            assert ri.numel() > 0


# ---- b. visibility through the raw path: alpha formed in the kernel, the kept set that of the fp64 reference exactly -----------------------
@pytest.mark.parametrize("seed", pr.RAW_SEEDS)
def test_visibility_raw_path(seed):
    from nerf_for_angiography_amd import engine
    raw, ts, te, off, alpha64 = pr.raw_visibility_problem(seed)
    for eps, thre in pr.RAW_PAIRS:
        keep, _ = pr.render_visibility(alpha64, off, eps, thre)
        ri_c, ts_c, te_c, off_c = pr.compact(keep, off, ts, te)
        ri, ts2, te2, off2 = engine.march_visibility(raw.to(DEV), ts.to(DEV), te.to(DEV), off.to(DEV), eps, thre, return_offsets=True)
        print(f"raw path seed {seed} eps {eps:g}: kept {ri.numel()} of {raw.numel()} (reference {int(keep.sum())})")
        assert torch.equal(off2.cpu(), off_c)
        assert torch.equal(ri.cpu(), ri_c) and torch.equal(ts2.cpu(), ts_c) and torch.equal(te2.cpu(), te_c)
        # [n,1] inputs, as the marching wrappers hand them on, are the same call
        ri3, ts3, te3 = engine.march_visibility(raw.to(DEV)[:, None], ts.to(DEV)[:, None], te.to(DEV)[:, None], off.to(DEV), eps, thre)
        assert torch.equal(ri3, ri) and torch.equal(ts3, ts2) and torch.equal(te3, te2)


# ---- c. afx_ray_offsets: the single-block two-level scan ----------------------------------------------------------------------------------------
def _counts(pattern, n_rays):
    g = torch.Generator().manual_seed(n_rays)
    if pattern == "zero":
        return torch.zeros(n_rays, dtype=torch.int32)
    c = torch.tensor([0, 1, 31, 32, 33, 64, 300], dtype=torch.int32)[torch.randint(0, 7, (n_rays,), generator=g)]
    if pattern == "huge":      # five rays of 2^30 (fewer where there are fewer rays): the totals pass 2^32; no sample is allocated
        c[torch.linspace(0, n_rays - 1, min(5, n_rays)).long()] = 1 << 30
    return c


@pytest.mark.parametrize("pattern", ["zero", "mixed", "huge"])
def test_ray_offsets(pattern):
    from nerf_for_angiography_amd import _lib, engine
    lib, dev = _lib.load(), torch.device(DEV)
    for n_rays in (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 5625):
        counts = _counts(pattern, n_rays)
        off_c, goff_c, tot, gtot = pr.offsets_of(counts)
        if pattern == "huge" and n_rays >= 5:
            assert tot > 1 << 32
        cd = counts.to(dev)
        for with_groups in (True, False):
            off = torch.full((n_rays + 1,), -7, dtype=torch.int64, device=dev)
            goff = torch.full((n_rays + 1,), -7, dtype=torch.int64, device=dev) if with_groups else None
            totals = torch.full((2,), -7, dtype=torch.int64, device=dev) if with_groups else None
            _lib.check(lib.afx_ray_offsets(_ptr(cd), n_rays, _ptr(off), _ptr(goff), _ptr(totals), engine.Engine._stream(dev)), "afx_ray_offsets")
            assert torch.equal(off.cpu(), off_c), (pattern, n_rays)
            if with_groups:
                assert torch.equal(goff.cpu(), goff_c), (pattern, n_rays)
                assert totals.tolist() == [tot, gtot], (pattern, n_rays)


# ---- d. afx_pack_groups -------------------------------------------------------------------------------------------------------------------------
def test_pack_groups():
    from nerf_for_angiography_amd import _lib, engine
    dev = torch.device(DEV)
    _, _, ts, te = pr.ragged_problem(pr.LENGTHS, 5)
    off = pr.offsets_from_lengths(pr.LENGTHS)
    ts_c, te_c, gray_c = pr.pack_groups(off, ts, te)
    n_groups = gray_c.numel()
    assert torch.equal(gray_c.bincount(minlength=len(pr.LENGTHS)), torch.tensor([(n + 31) // 32 for n in pr.LENGTHS]))
    # the buffers pack_groups is about to get from the caching allocator, full of NaN
    stale = [torch.full((32 * n_groups,), float("nan"), device=dev), torch.full((32 * n_groups,), float("nan"), device=dev),
             torch.full((n_groups,), -1, dtype=torch.int32, device=dev)]
    del stale
    pg = engine.pack_groups(off.to(dev), ts.to(dev), te.to(dev))
    assert pg.n_groups == n_groups and pg.n_rays == len(pr.LENGTHS)
    assert torch.equal(pg.group_offsets.cpu(), pr.offsets_of(pr.LENGTHS)[1])
    assert torch.equal(pg.ts_pad.cpu(), ts_c) and torch.equal(pg.te_pad.cpu(), te_c) and torch.equal(pg.group_ray.cpu(), gray_c)
    # ... and the entry point itself on NaN-filled buffers: every slot is written, the padding with exactly 0, every group exactly once
    ts_pad = torch.full((32 * n_groups,), float("nan"), device=dev)
    te_pad = torch.full((32 * n_groups,), float("nan"), device=dev)
    gray = torch.full((n_groups,), -1, dtype=torch.int32, device=dev)
    tsd, ted, offd = ts.to(dev), te.to(dev), off.to(dev)
    _lib.check(_lib.load().afx_pack_groups(_ptr(offd), _ptr(pg.group_offsets), len(pr.LENGTHS), _ptr(tsd), _ptr(ted), _ptr(ts_pad), _ptr(te_pad),
                                           _ptr(gray), engine.Engine._stream(dev)), "afx_pack_groups")
    assert torch.equal(ts_pad.cpu(), ts_c) and torch.equal(te_pad.cpu(), te_c) and torch.equal(gray.cpu(), gray_c)
    pad = torch.ones(32 * n_groups, dtype=torch.bool)
    for r, n in enumerate(pr.LENGTHS):
        g0 = int(pg.group_offsets[r])
        pad[32 * g0:32 * g0 + n] = False
    assert int(pad.sum()) == 32 * n_groups - sum(pr.LENGTHS) and bool((ts_pad.cpu()[pad] == 0).all()) and bool((te_pad.cpu()[pad] == 0).all())


# ---- e. afx_composite_packed and its backward -------------------------------------------------------------------------------------------------------
def _weighted(x, w, ri, ts, te, n_rays):      # the expression `bars` differentiates: sum_r w_r rgb_r
    return pr.composite_packed(x, ri, ts, te, n_rays) * w


@pytest.mark.parametrize("seed", [0, 3, 4])
def test_composite_packed(seed):
    from nerf_for_angiography_amd import engine
    n_rays = len(pr.LENGTHS)
    pred, ri, ts, te = pr.ragged_problem(pr.LENGTHS, seed)
    d_rgb = torch.linspace(-1.0, 2.0, n_rays)
    rgb64, _, bar_v, _ = pr.bars(_weighted, pred, torch.ones(n_rays), ri, ts, te, n_rays)
    _, g64, _, bar_g = pr.bars(_weighted, pred, d_rgb, ri, ts, te, n_rays)
    pd, rid, tsd, ted = pred.to(DEV), ri.to(DEV), ts.to(DEV), te.to(DEV)
    rgb = engine.composite_packed(pd, rid, tsd, ted, n_rays)
    d_pred = engine.composite_packed_backward(pd, rid, tsd, ted, n_rays, rgb, d_rgb.to(DEV))
    err_v, err_g = pr.rel_l2(rgb, rgb64), pr.rel_l2(d_pred, g64)
    print(f"composite_packed seed {seed}: value {err_v:.2e} (bar {bar_v:.2e}), gradient {err_g:.2e} (bar {bar_g:.2e})")
    empty = torch.tensor([n == 0 for n in pr.LENGTHS])
    assert bool((rgb.cpu()[empty] == 1.0).all())      # a ray without samples: exactly 1
    assert err_v < bar_v and err_g < bar_g
    # [n,1] and non-contiguous t_starts / t_ends are the same call
    both = torch.stack([tsd, ted], 1)
    assert torch.equal(engine.composite_packed(pd[:, None], rid, both[:, 0], both[:, 1:], n_rays), rgb)
    assert torch.equal(engine.composite_packed_backward(pd[:, None], rid, both[:, 0], both[:, 1:], n_rays, rgb, d_rgb.to(DEV))[:, 0], d_pred)


def test_composite_packed_exact_facts():
    from nerf_for_angiography_amd import engine
    n_rays = len(pr.LENGTHS)
    pred, ri, ts, te = pr.ragged_problem(pr.LENGTHS, 0)
    d_rgb = torch.linspace(-1.0, 2.0, n_rays)
    d_rgb[9] = 0.0                                       # (the ray of 65 samples)
    flat = torch.arange(pred.numel()) % 7 == 3
    te2 = torch.where(flat, ts, te)                      # samples with te == ts
    pd, rid, tsd, ted = pred.to(DEV), ri.to(DEV), ts.to(DEV), te2.to(DEV)
    rgb = engine.composite_packed(pd, rid, tsd, ted, n_rays)
    d_pred = engine.composite_packed_backward(pd, rid, tsd, ted, n_rays, rgb, d_rgb.to(DEV)).cpu()
    assert bool((d_pred[flat] == 0).all()) and bool((d_pred[ri.long() == 9] == 0).all()) and bool((d_pred[~flat & (ri.long() != 9)] != 0).all())
    # ... and such a sample contributes exactly 1: the pixels are those of the list without them, bit for bit
    rgb_without = engine.composite_packed(pd[~flat.to(DEV)], rid[~flat.to(DEV)], tsd[~flat.to(DEV)], ted[~flat.to(DEV)], n_rays)
    assert torch.equal(rgb, rgb_without)
    # saturated inputs: sigmoid(40) = 1 and sigmoid(-100) = 0 in fp32; finite pixels, no gradient
    for value in (40.0, -100.0):
        sat = torch.full_like(pred, value).to(DEV)
        rgb_s = engine.composite_packed(sat, rid, tsd, te.to(DEV), n_rays)
        assert bool(torch.isfinite(rgb_s).all())
        if value < 0:
            assert bool((rgb_s == 1.0).all())
        assert bool((engine.composite_packed_backward(sat, rid, tsd, te.to(DEV), n_rays, rgb_s, d_rgb.to(DEV)) == 0).all())
    # no samples at all
    none = torch.zeros(0, device=DEV)
    rgb0 = engine.composite_packed(none, torch.zeros(0, dtype=torch.int32, device=DEV), none, none, 5)
    assert rgb0.tolist() == [1.0] * 5
    assert engine.composite_packed_backward(none, torch.zeros(0, dtype=torch.int32, device=DEV), none, none, 5, rgb0, torch.ones(5, device=DEV)).numel() == 0
    # what the wrappers do not convert, they refuse - on the device too
    from nerf_for_angiography_amd._lib import AfxError
    with pytest.raises(ValueError, match=r"ray_indices must be a contiguous torch\.int32 tensor.*got torch\.int64"):
        engine.composite_packed(pd, rid.long(), tsd, ted, n_rays)
    with pytest.raises(ValueError, match=r"ray_indices must be a contiguous torch\.int32 tensor.*contiguous = False"):
        engine.composite_packed(pd, torch.stack([rid, rid], 1)[:, 0], tsd, ted, n_rays)
    with pytest.raises(ValueError, match=r"t_ends must be a torch\.float32 tensor.* on cuda:0, got .* on cpu"):
        engine.composite_packed(pd, rid, tsd, te2, n_rays)
    with pytest.raises(ValueError, match=r"offsets must be a contiguous torch\.int64 tensor.*got torch\.int32"):
        engine.march_visibility(pd, tsd, ted, pr.offsets_from_lengths(pr.LENGTHS).int().to(DEV), 1e-2, 1e-3)


# ---- f. afx_fine_depths / afx_fine_depths_from_tau ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_ray_z", [False, True], ids=["shared_z", "per_ray_z"])
@pytest.mark.parametrize("kind", pr.FINE_KINDS)
@pytest.mark.parametrize("s,nf", pr.FINE_SIZES)
def test_fine_depths(s, nf, kind, per_ray_z):
    """Sorted, S + NF long, every coarse depth present exactly (as a multiset); the NF other values against the fp64 reference.  The bar,
    per case (packed_reference.fine_expectation): 10 x the largest deviation of the fp32 CPU restatement from the fp64 one, at least one
    ulp of the largest depth.  In the peaked cases the draws on a knot and at 1 - 2^-24 lie on the steps the flat bins make of the
    inverse cdf, where the fp32 and the fp64 cdf order draw and knot differently: those (at most two per ray) are held to the nearer of
    the two restatements and left out of the bar, and the `den < 1e-5` rule is pinned by the draws half-way between two knots in front of
    the peak, which both precisions put into the same flat bin (tests/test_packed_edges_cpu.py: without the rule, or with its constant
    below the flat bins' 1e-7, the restatement misses this bar)."""
    from nerf_for_angiography_amd import engine
    p = pr.fine_problem(s, nf, kind, per_ray_z)
    z, w, u, from_tau = p.z, p.w, p.u, p.from_tau
    smp64, smp32, bar = pr.fine_expectation(p)
    fn = engine.fine_depths_from_tau if from_tau else engine.fine_depths
    out = fn(z.to(DEV), w.to(DEV), u.to(DEV)).cpu()
    assert out.shape == (pr.FINE_RAYS, s + nf) and bool(torch.isfinite(out).all())
    assert bool((out[:, 1:] >= out[:, :-1]).all())
    zz = z if per_ray_z else z.repeat(pr.FINE_RAYS, 1)
    present, rest = pr.split_merged(out, zz)
    assert present and rest.shape == (pr.FINE_RAYS, nf)
    err = pr.fine_error(rest, smp64, smp32, p.loose)
    err32 = float((rest - torch.sort(smp32, 1)[0]).abs().max())
    print(f"fine depths S {s} NF {nf} {kind} {'per-ray z' if per_ray_z else 'shared z'}: {err:.2e} (bar {bar:.2e}); vs the fp32 restatement {err32:.2e}")
    assert err <= bar


def test_fine_depths_refusals():
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd._lib import AfxError
    for fn, name in ((engine.fine_depths, "afx_fine_depths"), (engine.fine_depths_from_tau, "afx_fine_depths_from_tau")):
        for s, nf, msg in ((2, 4, "n_coarse must be in 3..512"), (513, 4, "n_coarse must be in 3..512"), (8, 0, "n_fine must be in 1..512"),
                           (8, 513, "n_fine must be in 1..512")):
            z = torch.linspace(1.0, 2.0, s, device=DEV)
            with pytest.raises(AfxError, match=f"{name}: {msg}"):
                fn(z, torch.ones(3, s, device=DEV), torch.rand(3, nf, device=DEV))
