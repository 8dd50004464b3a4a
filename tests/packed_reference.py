"""Plain restatements of the packed-sample kernels (afx_march_visibility, afx_march_compact, afx_ray_offsets, afx_pack_groups,
afx_composite_packed, afx_fine_depths / afx_fine_depths_from_tau) and the seeded problems tests/test_packed_edges_cpu.py and
tests/test_gpu_packed_edges.py share.  NumPy / torch on the CPU, Python loops where the order of operations matters; every function works
in the dtype it is given, so the same lines serve as the fp64 yardstick and as the fp32 restatement the tolerance rules are taken from.
tests/test_packed_edges_cpu.py ties them to oracle/angio_oracle.py and asserts the problems' preconditions on the references alone."""
import collections
import functools

import numpy as np
import torch

from ray_entropy_reference import RAGGED, bars, ragged_problem, rel_l2  # noqa: F401  (re-exported to the two test files)

# ragged lengths: 0, 1, < 32, the 32-sample group and the 64-lane chunk with their neighbours, two and more chunks; an empty ray in front
# and one behind, so the ray count (18) is no multiple of the 4 rays of a block
L = RAGGED + [127, 128, 129, 0]
LENGTHS = [0] + L + [0]


# ---- the operations ---------------------------------------------------------------------------------------------------------------
def offsets_from_lengths(lengths):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.as_tensor(lengths, dtype=torch.int64).cumsum(0)])


def render_visibility(alphas, offsets, eps, thre):
    """nerfacc's render_visibility, sequentially per ray in alphas' dtype: stop once T < eps; skip WITHOUT attenuating T when
    alpha < thre; otherwise keep the sample and T *= 1 - alpha.  -> (keep bool [n], T in front of every sample [n])."""
    a = alphas.detach().cpu().numpy()
    dt = a.dtype.type
    eps, thre, one = dt(eps), dt(thre), dt(1)
    keep, t_front = np.zeros(a.shape[0], dtype=bool), np.ones(a.shape[0], dtype=a.dtype)
    off = [int(x) for x in offsets]
    for r in range(len(off) - 1):
        T = one
        for i in range(off[r], off[r + 1]):
            t_front[i] = T
            if T < eps:
                continue
            if a[i] < thre:
                continue
            keep[i] = True
            T = dt(T * (one - a[i]))
    return torch.from_numpy(keep), torch.from_numpy(t_front)


def offsets_of(counts):
    """counts[R] -> (offsets int64 [R+1], group_offsets int64 [R+1], total, group total): exclusive scans of counts and of ceil(counts / 32)."""
    c = torch.as_tensor(counts).to(torch.int64)
    off, goff = torch.zeros(c.numel() + 1, dtype=torch.int64), torch.zeros(c.numel() + 1, dtype=torch.int64)
    s = g = 0
    for r, v in enumerate(c.tolist()):
        s += v
        g += (v + 31) // 32
        off[r + 1], goff[r + 1] = s, g
    return off, goff, s, g


def pack_groups(offsets, ts, te):
    """The group-aligned copy of include/afx.h: ray r's samples start at padded index 32 group_offsets[r]; the rest of its last 32-sample
    group is padding with ts = te = 0; group_ray[g] = the ray of group g.  -> (ts_pad, te_pad, group_ray int32)."""
    off = [int(x) for x in offsets]
    ts_pad, te_pad, group_ray = [], [], []
    for r in range(len(off) - 1):
        cnt = off[r + 1] - off[r]
        groups = (cnt + 31) // 32
        pad = torch.zeros(groups * 32 - cnt, dtype=ts.dtype)
        ts_pad += [ts[off[r]:off[r + 1]], pad]
        te_pad += [te[off[r]:off[r + 1]], pad]
        group_ray += [r] * groups
    return torch.cat(ts_pad), torch.cat(te_pad), torch.tensor(group_ray, dtype=torch.int32)


def compact(keep, offsets, ts, te):
    """The kept samples in order -> (ray_indices int32, t_starts, t_ends, offsets int64 of the kept list)."""
    off = [int(x) for x in offsets]
    lengths = torch.tensor([off[r + 1] - off[r] for r in range(len(off) - 1)])
    ri = torch.arange(len(off) - 1, dtype=torch.int32).repeat_interleave(lengths)
    counts = [int(keep[off[r]:off[r + 1]].sum()) for r in range(len(off) - 1)]
    return ri[keep], ts[keep], te[keep], offsets_of(counts)[0]


def composite_packed(pred, ri, ts, te, n_rays):
    """prod over the ray's samples, in order, of exp(-sigmoid(pred) (te - ts)), in pred's dtype; 1 for a ray without samples.  Differentiable."""
    f = torch.exp(-torch.sigmoid(pred) * (te.to(pred.dtype) - ts.to(pred.dtype)))
    off = torch.searchsorted(ri.long(), torch.arange(n_rays + 1)).tolist()
    return torch.stack([f[off[r]:off[r + 1]].prod() for r in range(n_rays)]) if n_rays else f.new_zeros(0)


def fine_cdf(z, w_or_tau, from_tau, plus=1e-5):
    """-> (bins [R,S-1] = mid-points of the depths, cdf [R,S-1] of sample_pdf over weights[..., 1:-1]), summed in order, in w's dtype.
    (`plus`: sample_pdf's + 1e-5; another value is a mutation for tests/test_packed_edges_cpu.py.)"""
    w = w_or_tau
    dt = w.dtype
    r, s = w.shape
    zz = (z.repeat(r, 1) if z.dim() == 1 else z).to(dt)
    if from_tau:      # render_volume_density's weights: (1 - a + 1e-10) cumprod_exclusive(a), a = exp(-tau)
        a = torch.exp(-w)
        T, cols = torch.ones(r, dtype=dt), []
        for i in range(s):
            cols.append((1 - a[:, i] + 1e-10) * T)
            T = T * a[:, i]
        w = torch.stack(cols, 1)
    wi = w[:, 1:-1] + plus
    wsum = torch.zeros(r, dtype=dt)
    for i in range(s - 2):
        wsum = wsum + wi[:, i]
    run, cdf = torch.zeros(r, dtype=dt), [torch.zeros(r, dtype=dt)]
    for i in range(s - 2):
        run = run + wi[:, i] / wsum
        cdf.append(run)
    return 0.5 * (zz[:, 1:] + zz[:, :-1]), torch.stack(cdf, 1)


def fine_depths(z, w_or_tau, u, from_tau=False, plus=1e-5, den_rule=1e-5):
    """The oracle's sample_pdf plus merge (nerf_helpers.py:178-222) in w's dtype -> (merged depths [R,S+NF] ascending, den [R,NF] =
    cdf[above] - cdf[below] of every draw before the `den < 1e-5 -> 1` rule, the NF drawn depths [R,NF] in u's order).
    (`plus`, `den_rule`: the two constants of sample_pdf; other values, or den_rule=None for no rule, are mutations for the CPU tests.)"""
    dt = w_or_tau.dtype
    bins, cdf = fine_cdf(z, w_or_tau, from_tau, plus)
    u = u.to(dt).contiguous()
    idx = torch.searchsorted(cdf.contiguous(), u, right=True)
    lo, hi = (idx - 1).clamp(min=0), idx.clamp(max=cdf.shape[1] - 1)
    c_lo, c_hi = torch.gather(cdf, 1, lo), torch.gather(cdf, 1, hi)
    b_lo, b_hi = torch.gather(bins, 1, lo), torch.gather(bins, 1, hi)
    den = c_hi - c_lo
    smp = b_lo + (u - c_lo) / (den if den_rule is None else torch.where(den < den_rule, torch.ones_like(den), den)) * (b_hi - b_lo)
    zz = (z.repeat(u.shape[0], 1) if z.dim() == 1 else z).to(dt)
    return torch.sort(torch.cat([zz, smp], 1), 1)[0], den, smp


def split_merged(out, z):
    """A merged row set out[R,S+NF] (ascending) and the coarse depths z[R,S] (ascending) -> (whether every coarse depth is present exactly,
    as a multiset; the other NF values [R,NF], ascending)."""
    out, z = out.detach().cpu().numpy(), z.detach().cpu().numpy()
    ok, rest = True, []
    for o, zr in zip(out, z):
        first = np.searchsorted(o, zr, side="left")
        rank = np.arange(zr.size) - np.searchsorted(zr, zr, side="left")      # position inside a run of equal depths
        pos = first + rank
        ok = ok and bool((pos < o.size).all()) and bool((o[np.minimum(pos, o.size - 1)] == zr).all())
        rest.append(np.delete(o, np.minimum(pos, o.size - 1)))
    return ok, torch.from_numpy(np.stack(rest))


# ---- the problems (seeded CPU generators; tests/test_packed_edges_cpu.py asserts their preconditions) ---------------------------------
# (early_stop_eps, alpha_thre) of the exact visibility problems.  The first four are the set the kernels are pinned at; with alphas in
# {0, 0.5, 0.75} a ray cannot stop behind its first sample at eps <= 2^-2, so the stop at in-ray position 1 needs the pair (2^-1, 0.25).
EXACT_PAIRS = [(2.0 ** -3, 0.25), (2.0 ** -10, 0.0), (0.0, 0.6), (2.0, 0.25), (2.0 ** -1, 0.25)]
STOP_TARGETS = [1, 62, 63, 64, 65, 127, 128, 129]      # in-ray position of the first sample the early stop drops
N_VARIANTS = len(STOP_TARGETS) + 1                      # ray j of variant v aims at STOP_TARGETS[(v + j) % 9], the ninth choice being "never"


def _halvings(eps):
    return {2.0 ** -3: 3, 2.0 ** -10: 10, 2.0 ** -1: 1}.get(eps, 3)      # (eps = 0 and eps = 2 re-use the eps = 2^-3 design)


@functools.lru_cache(maxsize=None)
def exact_visibility_problem(eps, variant):
    """Alphas in {0, 0.5, 0.75} over LENGTHS (every kept factor a power of two) -> (alphas fp32, t_starts, t_ends, offsets).  With
    k = -log2(eps): a ray that aims at stop position p carries exactly k halvings (0.5 = one, 0.75 = two) somewhere in its samples
    0 .. p-2, so T == eps exactly there and the march goes on (the rule is T < eps), and a thick sample at p-1; if p - 1 positions cannot
    hold k halvings, k-1 of them and 0.75 at p-1.  Behind p the alphas are random.  A ray that aims at "never", or is too short for its
    target, carries k halvings (as many as fit) at random positions and zeros elsewhere, and ends at T >= eps."""
    g = torch.Generator().manual_seed(1000 * _halvings(eps) + variant)
    k = _halvings(eps)
    rows = []
    for j, n in enumerate(LENGTHS):
        a = torch.zeros(n)
        choice = (variant + j) % N_VARIANTS
        p = STOP_TARGETS[choice] if choice < len(STOP_TARGETS) else None
        if p is not None and p < n and 2 * (p - 1) >= k - 1:
            before, last = (k, 0.5) if 2 * (p - 1) >= k else (k - 1, 0.75)      # halvings in front of sample p-1, and its own alpha
            pairs = int(torch.randint(max(0, before - (p - 1)), before // 2 + 1, (1,), generator=g))      # how many of them as 0.75
            thick = [0.75] * pairs + [0.5] * (before - 2 * pairs)
            pos = torch.randperm(p - 1, generator=g)[:len(thick)]
            a[pos] = torch.tensor(thick) if thick else a[pos]
            a[p - 1] = last
            a[p:] = torch.tensor([0.0, 0.5, 0.75])[torch.randint(0, 3, (n - p,), generator=g)]
        else:
            m = min(k, n)
            a[torch.randperm(n, generator=g)[:m]] = 0.5
        rows.append(a)
    alphas = torch.cat(rows)
    _, _, ts, te = ragged_problem(LENGTHS, 77)
    return alphas, ts, te, offsets_from_lengths(LENGTHS)


RAW_PAIRS = [(1e-2, 1e-3), (1e-4, 1e-3)]
RAW_SEEDS = [0, 1, 3]


@functools.lru_cache(maxsize=None)
def raw_visibility_problem(seed):
    """Raw MLP outputs over LENGTHS: thin samples (raw = -20: alpha ~ 1e-9, far below alpha_thre = 1e-3) and thick ones (raw in [-1, 3],
    dt ~ 0.5: alpha in 0.1 .. 0.4, far above it), the thick share drawn per ray from 0.1 .. 0.9 so that the early stop falls in the first,
    second or a later 64-sample chunk or not at all.  -> (raw fp32, t_starts, t_ends, offsets, alpha fp64 of the fp32 inputs)."""
    g = torch.Generator().manual_seed(seed)
    n = sum(LENGTHS)
    ri = torch.arange(len(LENGTHS)).repeat_interleave(torch.tensor(LENGTHS))
    share = 0.1 + 0.8 * torch.rand(len(LENGTHS), generator=g)
    thick = torch.rand(n, generator=g) < share[ri]
    raw = torch.where(thick, 4.0 * torch.rand(n, generator=g) - 1.0, torch.full((n,), -20.0))
    dt = 0.5 * (0.8 + 0.4 * torch.rand(n, generator=g))
    te = torch.cumsum(dt + 0.05 * torch.rand(n, generator=g), 0).float()
    ts = (te - dt).float()
    alpha64 = 1.0 - torch.exp(-torch.sigmoid(raw.double()) * (te.double() - ts.double()))
    return raw, ts, te, offsets_from_lengths(LENGTHS), alpha64


FINE_SIZES = [(3, 1), (4, 7), (33, 64), (512, 512)]
# (no peaked tau: render_volume_density's weights are at most 1, so the bins beside a peak have a pdf of ~ 1e-5 - on the `den < 1e-5`
# rule itself, where fp32 and fp64 part; the weights form carries the peak)
FINE_KINDS = ["smooth", "zero", "peak", "tau_smooth", "tau_zero", "tau_saturated"]
FINE_RAYS = 37
FineProblem = collections.namedtuple("FineProblem", "z w u from_tau loose mid")
U_TOP = 1.0 - 2.0 ** -24      # the largest fp32 below 1


@functools.lru_cache(maxsize=None)
def fine_problem(s, nf, kind, per_ray_z):
    """-> FineProblem(z [S] or [R,S], w or tau [R,S] fp32, u [R,NF] fp32, from_tau, loose [R,NF], mid [R,NF]).  Weights / optical depths: smooth random (pdf of every bin above
    1e-4), all zero (a uniform pdf), one peak (>= 100, weights only) beside exact zeros (the other bins' pdf ~ 1e-7: sample_pdf's
    `den < 1e-5` rule), and for tau a saturated front sample (tau = 50: every later weight is ~ 1e-22).  u: uniform draws in no order, with
    0, 1 - 2^-24 and a knot of the fp32 cdf written over three of them (NF < 3: one of the three per ray).  Per-ray z: ascending random
    depths, with two equal neighbours in every third ray and three (a zero-width bin) in every third other one.
    The peaked cases (NF >= 7) also draw `mid`: u half-way between two neighbouring knots of the fp32 cdf in the flat region in front of
    the peak (the widest one or two such bins of the ray).  There the cdf is ~ j 1e-7 with a relative error of ~ 1e-7, so fp32 and fp64
    pick the same bin; with the `den < 1e-5` rule the draw lands on the bin's lower edge, without it half a bin further.
    `loose` marks the knot and 1 - 2^-24 draws of the peaked cases: they lie ON the steps the flat bins make of the inverse cdf, where
    the fp32 and the fp64 cdf order draw and knot differently and the two restatements differ by whole bins (see fine_expectation)."""
    from_tau = kind.startswith("tau_")
    g = torch.Generator().manual_seed(10007 * s + 31 * nf + FINE_KINDS.index(kind) + 7 * int(per_ray_z))
    r = FINE_RAYS
    if per_ray_z:
        z = torch.sort(1400.0 + 200.0 * torch.rand(r, s, generator=g), 1)[0]
        for i in range(r):
            k = int(torch.randint(0, s - 1, (1,), generator=g))
            if i % 3 == 1:
                z[i, k + 1] = z[i, k]
            elif i % 3 == 2 and s >= 4:
                k = min(k, s - 3)
                z[i, k + 1] = z[i, k + 2] = z[i, k]
    else:
        z = torch.linspace(1400.0, 1600.0, s)
    base = kind[4:] if from_tau else kind
    if base == "smooth":
        w = 0.5 + torch.rand(r, s, generator=g)
        w = w / s if from_tau else w
    elif base == "zero":
        w = torch.zeros(r, s)
    elif base == "peak":
        w = torch.zeros(r, s)
        at = torch.randint(1, s - 1, (r,), generator=g)
        at[0], at[1] = 1, s - 2      # the first and the last bin
        w[torch.arange(r), at] = 100.0 + 50.0 * torch.rand(r, generator=g)
    else:      # saturated
        w = (0.5 + torch.rand(r, s, generator=g)) / s
        w[:, 0] = 50.0
    u = torch.rand(r, nf, generator=g)
    _, cdf32 = fine_cdf(z, w, from_tau)
    knot = cdf32[torch.arange(r), torch.randint(1, max(s - 2, 2), (r,), generator=g).clamp(max=s - 2)]
    special = torch.stack([torch.zeros(r), torch.full((r,), U_TOP), knot.clamp(max=U_TOP)], 1)
    loose, mid = torch.zeros(r, nf, dtype=torch.bool), torch.zeros(r, nf, dtype=torch.bool)
    if nf >= 3:
        for c, col in enumerate((nf // 2, 0, nf - 1)):
            u[:, col] = special[:, c]
            loose[:, col] = base == "peak" and c > 0
    else:
        u[:, 0] = special[torch.arange(r), torch.arange(r) % 3]
        loose[:, 0] = (torch.arange(r) % 3 > 0) & (base == "peak")
    if base == "peak" and nf >= 7:
        bins32 = fine_cdf(z, w, from_tau)[0]
        for i in range(r):
            flat = int(at[i]) - 1      # the bins 0 .. flat-1 lie in front of the peak
            if flat >= 1:
                widest = torch.argsort(bins32[i, 1:flat + 1] - bins32[i, :flat], descending=True)
                for c, col in enumerate((1, nf - 2)):
                    j = int(widest[min(c, flat - 1)])
                    u[i, col] = 0.5 * (cdf32[i, j] + cdf32[i, j + 1])
                    mid[i, col] = True
    return FineProblem(z, w, u, from_tau, loose, mid)


def fine_expectation(p):
    """What test f holds the NF drawn depths to -> (smp64 [R,NF], smp32 [R,NF], bar).  The bar: 10 x the largest deviation of the fp32
    restatement from the fp64 one, at least one ulp of the largest depth - over every draw, except the `loose` ones of the peaked cases,
    which fine_error compares with the nearer of the two restatements instead (so they cannot widen the bar to more than the depth range)."""
    smp64 = fine_depths(p.z.double(), p.w.double(), p.u.double(), p.from_tau)[2]
    smp32 = fine_depths(p.z, p.w, p.u, p.from_tau)[2]
    ulp = float(torch.finfo(torch.float32).eps) * 2.0 ** (int(torch.frexp(p.z.max())[1]) - 1)
    dev = (smp32.double() - smp64).abs()[~p.loose]
    return smp64, smp32, max(10.0 * float(dev.max()), ulp)


def fine_error(rest, smp64, smp32, loose):
    """rest [R,NF] (ascending: the drawn depths a merged row holds) against the restatements -> the largest absolute deviation from the
    sorted fp64 draws, where every `loose` draw of a ray is taken from the fp32 or the fp64 restatement, whichever set fits the row best."""
    import itertools
    if not bool(torch.isfinite(rest).all()):
        return float("nan")
    worst = 0.0
    for r in range(rest.shape[0]):
        cols = loose[r].nonzero().reshape(-1).tolist()
        best = None
        for pick in itertools.product((0, 1), repeat=len(cols)):
            cand = smp64[r].clone()
            for c, from32 in zip(cols, pick):
                if from32:
                    cand[c] = smp32[r, c].double()
            err = float((rest[r].double() - torch.sort(cand)[0]).abs().max())
            best = err if best is None else min(best, err)
        worst = max(worst, best)
    return worst
