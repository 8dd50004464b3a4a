"""Host-side half of the packed-sample edge tests: the problems tests/test_gpu_packed_edges.py runs are built here from the seeded CPU
generators of tests/packed_reference.py and their preconditions are asserted on the references alone (the GPU tests import the same
builders and assume them); the references are tied to oracle/angio_oracle.py; the engine wrappers' refusals are pinned on host tensors."""
import pytest
import torch

import packed_reference as pr
from nerf_for_angiography_amd import engine
from nerf_for_angiography_amd._lib import AfxError
from oracle import angio_oracle as orc


def _ray_index(offsets):
    off = offsets.tolist()
    return torch.arange(len(off) - 1).repeat_interleave(torch.tensor([b - a for a, b in zip(off, off[1:])]))


def stop_positions(t_front, offsets, eps):
    """Per ray: the in-ray position of the first sample with T < eps in front of it (the first one the early stop drops), or None."""
    off, out = offsets.tolist(), []
    for a, b in zip(off, off[1:]):
        hit = (t_front[a:b] < eps).nonzero()
        out.append(int(hit[0]) if hit.numel() else None)
    return out


def visibility_margins(alpha64, offsets, eps, thre):
    """The raw-path preconditions on the fp64 reference -> (min |alpha - thre| / thre, min |T / eps - 1|) over EVERY sample."""
    _, t_front = pr.render_visibility(alpha64, offsets, eps, thre)
    return float(((alpha64 - thre).abs() / thre).min()), float((t_front / eps - 1.0).abs().min())


def den_outside_band(den64, lo=1e-6, hi=1e-4):
    return bool(((den64 < lo) | (den64 > hi)).all())


def test_exact_visibility_problems():
    seen, never, touched = set(), set(), 0
    for eps, thre in pr.EXACT_PAIRS:
        for v in range(pr.N_VARIANTS):
            alphas, ts, te, off = pr.exact_visibility_problem(eps, v)
            assert alphas.dtype == torch.float32 and bool(((alphas == 0) | (alphas == 0.5) | (alphas == 0.75)).all())
            assert eps == 0 or torch.frexp(torch.tensor(eps))[0] == 0.5      # a power of two
            k32, t32 = pr.render_visibility(alphas, off, eps, thre)
            k64, t64 = pr.render_visibility(alphas.double(), off, eps, thre)
            assert torch.equal(k32, k64)
            assert eps == 0 or torch.equal(t32.double(), t64)      # (without a stop T underflows in fp32; the masks do not depend on it)
            if eps in (0.0, 2.0):
                assert bool(k64.any()) == (eps == 0.0)      # eps = 2 keeps nothing, eps = 0 never stops
                continue
            for n, p in zip(pr.LENGTHS, stop_positions(t64, off, eps)):
                seen.add(p) if p is not None else never.add(n)
            # T == eps in front of a sample that is kept: the rule is `<`
            touched += int(((t64 == eps) & k64).sum())
    assert set(pr.STOP_TARGETS) <= seen, sorted(set(pr.STOP_TARGETS) - seen)
    assert never == set(pr.LENGTHS)
    assert touched > 0


def test_raw_visibility_problems():
    for seed in pr.RAW_SEEDS:
        raw, ts, te, off, alpha64 = pr.raw_visibility_problem(seed)
        late = []
        for eps, thre in pr.RAW_PAIRS:
            m_alpha, m_t = visibility_margins(alpha64, off, eps, thre)
            assert m_alpha >= 1e-3 and m_t >= 1e-3, (seed, eps, m_alpha, m_t)
            keep, t_front = pr.render_visibility(alpha64, off, eps, thre)
            thin_dropped = (alpha64 < thre) & ~(t_front < eps)
            assert bool(thin_dropped.any()) and bool((t_front < eps).any())      # both outcomes
            stops = [p for p in stop_positions(t_front, off, eps) if p is not None]
            assert 0 < len(stops) < sum(n > 0 for n in pr.LENGTHS)               # rays that stop early and rays that do not
            late += [p for p in stops if p >= 64]
        assert late                                                              # a stop behind the ray's first 64-sample chunk


def test_fine_depth_problems():
    for s, nf in pr.FINE_SIZES:
        for kind in pr.FINE_KINDS:
            for per_ray_z in (False, True):
                p = pr.fine_problem(s, nf, kind, per_ray_z)
                z, w, u, from_tau = p.z, p.w, p.u, p.from_tau
                assert w.shape == (pr.FINE_RAYS, s) and u.shape == (pr.FINE_RAYS, nf)
                assert bool((u == 0).any()) and bool((u == pr.U_TOP).any()) and float(u.max()) < 1.0
                if per_ray_z:
                    assert bool((z[:, 1:] >= z[:, :-1]).all()) and bool((z[:, 1:] == z[:, :-1]).any())
                bins32, cdf32 = pr.fine_cdf(z, w, from_tau)
                knots = cdf32[:, None, 1:] if s > 3 else cdf32[:, None, :]      # (S = 3: the cdf is {0, 1}, and u < 1)
                assert bool((u[:, :, None] == knots).any())                     # a draw on a knot of the fp32 cdf
                merged, den64, _ = pr.fine_depths(z.double(), w.double(), u.double(), from_tau)
                assert den_outside_band(den64), (s, nf, kind, per_ray_z)
                assert bool(torch.isfinite(merged).all())
                assert bool(p.loose.any()) == (kind == "peak") and not bool((p.loose & p.mid).any())
                _, _, bar = pr.fine_expectation(p)
                assert bar < 0.1, (s, nf, kind, per_ray_z, bar)      # every bar far below the depth range of 200 (0.39 is a bin at S = 512)
                if kind == "peak":
                    assert float(w.max(1)[0].min()) >= 100.0 and bool(((w == 0).sum(1) == s - 1).all())
                    assert int(p.loose.sum(1).max()) <= 2
                    if s > 3:
                        assert bool(((den64 > 0) & (den64 < 1e-6)).any())      # draws in the flat bins: below the band
                    if nf >= 7:
                        # the draws between two knots in front of the peak: at least a third of the rays have them (S = 4: the rays whose peak is the second bin); fp32 and fp64 put each into the same flat
                        # bin, well inside it; the rule is what keeps them on the bin's lower edge, half a bin (>= 10 bars) from where
                        # they land without it
                        assert int(p.mid.any(1).sum()) > pr.FINE_RAYS // 3
                        cdf64 = pr.fine_cdf(z.double(), w.double(), from_tau)[1]
                        i32 = torch.searchsorted(cdf32.contiguous(), u.contiguous(), right=True)[p.mid]
                        i64 = torch.searchsorted(cdf64.contiguous(), u.double().contiguous(), right=True)[p.mid]
                        assert torch.equal(i32, i64)
                        rows = p.mid.nonzero()[:, 0]
                        lo, hi, um = cdf64[rows, i64 - 1], cdf64[rows, i64], u.double()[p.mid]
                        assert bool(((um - lo) > 0.25 * (hi - lo)).all()) and bool(((hi - um) > 0.25 * (hi - lo)).all())
                        assert bool((den64[p.mid] < 1e-6).all())
                        half = 0.5 * (bins32[rows, i32] - bins32[rows, i32 - 1])
                        assert int((half.double() > 10.0 * bar).sum()) > pr.FINE_RAYS // 3


def test_references_against_the_oracle():
    for eps, thre in pr.EXACT_PAIRS[:2]:
        alphas, ts, te, off = pr.exact_visibility_problem(eps, 3)
        assert torch.equal(pr.render_visibility(alphas.double(), off, eps, thre)[0], orc.render_visibility(alphas.double(), _ray_index(off), eps, thre))
    raw, ts, te, off, alpha64 = pr.raw_visibility_problem(0)
    for eps, thre in pr.RAW_PAIRS:
        keep = pr.render_visibility(alpha64, off, eps, thre)[0]
        assert torch.equal(keep, orc.render_visibility(alpha64, _ray_index(off), eps, thre))
        ri2, ts2, te2, off2 = pr.compact(keep, off, ts, te)
        assert torch.equal(ri2.long(), _ray_index(off)[keep]) and torch.equal(off2, pr.offsets_from_lengths(torch.bincount(ri2.long(), minlength=len(pr.LENGTHS))))
    n_rays = len(pr.LENGTHS)
    for seed in (0, 3, 4):
        pred, ri, ts, te = pr.ragged_problem(pr.LENGTHS, seed)
        mine = pr.composite_packed(pred.double(), ri, ts, te, n_rays)
        theirs = orc.acc_render_volume_density(pred.double()[:, None], ri, ts.double()[:, None], te.double()[:, None], n_rays)      # (returns fp32)
        alpha = torch.exp(-torch.sigmoid(pred.double()) * (te.double() - ts.double()))
        prod = torch.ones(n_rays, dtype=torch.float64).index_reduce(0, ri.long(), alpha, "prod")
        assert float((mine - prod).abs().max()) <= 1e-12 and torch.equal(prod.float(), theirs)
    for s, nf in pr.FINE_SIZES:
        for kind in pr.FINE_KINDS:
            for per_ray_z in (False, True):
                z, w, u, from_tau = pr.fine_problem(s, nf, kind, per_ray_z)[:4]
                w64 = w.double()
                if from_tau:
                    a = torch.exp(-w64)
                    w64 = (1 - a + 1e-10) * orc.cumprod_exclusive(a)
                want = orc.fine_depths(z.double(), w64, u.double(), pr.FINE_RAYS)
                got = pr.fine_depths(z.double(), w.double(), u.double(), from_tau)[0]
                # (1e-12 of the depths, which are ~ 1500: the two differ in the order the cdf is summed in)
                assert float(((got - want) / want).abs().max()) <= 1e-12, (s, nf, kind, per_ray_z, float((got - want).abs().max()))
    # offsets_of and pack_groups against the torch expressions engine.pack_groups starts from
    counts = torch.tensor([0, 1, 31, 32, 33, 64, 300, 0])
    off, goff, tot, gtot = pr.offsets_of(counts)
    assert torch.equal(off[1:], counts.cumsum(0)) and torch.equal(goff[1:], ((counts + 31) // 32).cumsum(0)) and (tot, gtot) == (461, 17)
    ts = torch.arange(1.0, 462.0)
    ts_pad, te_pad, group_ray = pr.pack_groups(off, ts, ts + 0.5)
    assert ts_pad.numel() == 32 * gtot and int((ts_pad == 0).sum()) == 32 * gtot - tot and torch.equal(ts_pad[ts_pad > 0], ts)
    assert torch.equal(te_pad[te_pad > 0], ts + 0.5) and group_ray.tolist() == [1, 2, 3, 4, 4] + [5] * 2 + [6] * 10
    assert float(ts_pad[32 * int(goff[6])]) == float(ts[int(off[6])])      # every ray starts on a group


def test_one_line_mutations_of_the_references_are_caught():
    """What the GPU tests compare the kernels with moves under a one-line change of the rule: `<` -> `<=` in the stop rule, an
    off-by-one in the scan - each on the problems of the GPU tests (sample_pdf's constants: the next test)."""
    moved = 0
    for v in range(pr.N_VARIANTS):
        alphas, _, _, off = pr.exact_visibility_problem(2.0 ** -3, v)
        keep, t_front = pr.render_visibility(alphas, off, 2.0 ** -3, 0.25)
        keep_le = keep & ~(t_front <= 2.0 ** -3)      # the rule with <=: T never grows, so this is the whole difference
        moved += int((keep != keep_le).sum())
    assert moved > 0
    counts = torch.tensor([0, 1, 31, 32, 33, 64, 300])
    off, goff, _, _ = pr.offsets_of(counts)
    assert not torch.equal(off[:-1], counts.cumsum(0)) and not torch.equal(goff[1:], (counts // 32).cumsum(0))      # inclusive scan; floor

def _as_test_f_sees(p, **mutation):
    """The error test f of tests/test_gpu_packed_edges.py would measure, and its bar, for a kernel that computes the fp32 restatement with
    one constant of sample_pdf changed."""
    smp64, smp32, bar = pr.fine_expectation(p)
    mutated = pr.fine_depths(p.z, p.w, p.u, p.from_tau, **mutation)[2]
    return pr.fine_error(torch.sort(mutated, 1)[0], smp64, smp32, p.loose), bar


def test_mutations_of_sample_pdf_fail_the_fine_depth_check():
    """sample_pdf without the `den < 1e-5` rule, with its constant moved below the flat bins (1e-8) or above the smooth ones (1e-3), and
    without the + 1e-5: each moves the fp32 restatement beyond the bar of the cases built for it, so `err <= bar` of test f fails; the
    restatement as it stands passes every case.  (Constants between the flat bins' 1e-7 and the smooth bins' 6e-4 decide every draw of
    these problems the same way - that is the band the problems keep clear of.)"""
    for s, nf in pr.FINE_SIZES:
        for kind in pr.FINE_KINDS:
            for per_ray_z in (False, True):
                err, bar = _as_test_f_sees(pr.fine_problem(s, nf, kind, per_ray_z))
                assert err <= 0.1 * bar, (s, nf, kind, per_ray_z, err, bar)
    for s, nf in pr.FINE_SIZES[1:]:
        for per_ray_z in (False, True):
            p = pr.fine_problem(s, nf, "peak", per_ray_z)
            for mutation in (dict(den_rule=None), dict(den_rule=1e-8), dict(plus=0.0)):
                err, bar = _as_test_f_sees(p, **mutation)
                assert not err <= bar, (s, nf, per_ray_z, mutation, err, bar)
            err, bar = _as_test_f_sees(pr.fine_problem(s, nf, "zero", per_ray_z), plus=0.0)      # 0 / 0
            assert err != err
    for per_ray_z in (False, True):
        err, bar = _as_test_f_sees(pr.fine_problem(512, 512, "smooth", per_ray_z), den_rule=1e-3)
        assert not err <= bar, (per_ray_z, err, bar)


def test_wrappers_refuse_what_they_cannot_pass_by_pointer():
    """engine.composite_packed / composite_packed_backward / march_visibility: dtype and size violations are named before the device is
    looked at; conforming host tensors are refused for living on the host.  Nothing is converted on this path."""
    pred, ri = torch.zeros(6), torch.tensor([0, 0, 1, 1, 1, 2], dtype=torch.int32)
    ts, te = torch.arange(6.0), torch.arange(6.0) + 0.5
    rgb, d_rgb, off = torch.ones(3), torch.ones(3), torch.tensor([0, 2, 5, 6])
    for fn, args in ((engine.composite_packed, ()), (engine.composite_packed_backward, (rgb, d_rgb))):
        with pytest.raises(AfxError, match="pred must be a tensor on a GPU; there is no CPU path"):
            fn(pred, ri, ts, te, 3, *args)
        with pytest.raises(ValueError, match=r"ray_indices must be a contiguous torch\.int32 tensor of 6 elements .*got torch\.int64"):
            fn(pred, ri.long(), ts, te, 3, *args)
        with pytest.raises(ValueError, match=r"pred must be a torch\.float32 tensor.*got torch\.float64"):
            fn(pred.double(), ri, ts, te, 3, *args)
        with pytest.raises(ValueError, match=r"t_starts must be a torch\.float32 tensor.*got torch\.float64"):
            fn(pred, ri, ts.double(), te, 3, *args)
        with pytest.raises(ValueError, match=r"t_ends must be a torch\.float32 tensor.*got torch\.float16"):
            fn(pred, ri, ts, te.half(), 3, *args)
        with pytest.raises(ValueError, match=r"t_starts must be a torch\.float32 tensor of 6 elements .*got torch\.float32 \(5,\)"):
            fn(pred, ri, ts[:5], te, 3, *args)
        with pytest.raises(ValueError, match=r"ray_indices must be a contiguous torch\.int32 tensor of 6 elements .*got torch\.int32 \(5,\)"):
            fn(pred, ri[:5], ts, te, 3, *args)
        with pytest.raises(ValueError, match=r"t_ends must be a torch\.float32 tensor.*got list"):
            fn(pred, ri, ts, te.tolist(), 3, *args)
    with pytest.raises(ValueError, match=r"d_rgb must be a torch\.float32 tensor.*got torch\.float64"):
        engine.composite_packed_backward(pred, ri, ts, te, 3, rgb, d_rgb.double())
    with pytest.raises(ValueError, match=r"\brgb must be a torch\.float32 tensor of 3 elements .*got torch\.float32 \(2,\)"):
        engine.composite_packed_backward(pred, ri, ts, te, 3, rgb[:2], d_rgb)
    with pytest.raises(AfxError, match="raw must be a tensor on a GPU; there is no CPU path"):
        engine.march_visibility(pred, ts, te, off, 1e-2, 1e-3)
    with pytest.raises(ValueError, match=r"offsets must be a contiguous torch\.int64 tensor.*got torch\.int32"):
        engine.march_visibility(pred, ts, te, off.int(), 1e-2, 1e-3)
    with pytest.raises(ValueError, match=r"raw must be a torch\.float32 tensor.*got torch\.float64"):
        engine.march_visibility(pred.double(), ts, te, off, 1e-2, 1e-3)
    with pytest.raises(ValueError, match=r"\bte must be a torch\.float32 tensor of 6 elements .*got torch\.float32 \(5,\)"):
        engine.march_visibility(pred, ts, te[:5], off, 1e-2, 1e-3)
    # acc_render_volume_density converts its inputs first, as before: a host call gets its own refusal, not a dtype complaint
    from nerf_for_angiography_amd.nerf.nerf_helpers_acc import acc_render_volume_density
    with pytest.raises(AfxError, match="acc_render_volume_density: tensors must live on the GPU"):
        acc_render_volume_density(pred.double()[:, None], ri.long(), ts[:, None], te[:, None], 3, 0)
