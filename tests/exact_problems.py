"""Exactly representable CPPN problems for the points-mode backward (afx_mlp_infer / afx_mlp_backward): not a test module.

`make(layers, width, n_pts, seed)` builds a ReLU CPPN with no input encoding, points and a cotangent `d_out` whose every forward value,
pre-activation gradient and weight-gradient sum is exact in every precision of the fused kernels.  A correct kernel must then return
the float64 answer bit for bit; an operand permutation, a mis-tiled slab, a dropped tile or a wrong power-of-two un-scaling moves whole
units.  Construction:
  - points are small integers; the first layer picks one coordinate per row with a weight from {+-1, +-1/2, +-2};
  - a hidden row has one nonzero weight (a quarter of the rows two) from {+-1, +-1/2, +-2}; the columns come from two permutations, so
    no column of a weight matrix has more than two nonzeros and the input-gradient chain grows slowly;
  - biases are small dyadic values, drawn per row until no pre-activation of that row is exactly 0, its values stay on the grid below
    and its ReLU is on for some points and off for others;
  - d_out = +-2^k.  One point has k = 0, two k = -1, four k = -2 ... (as many binades as the point count and `spread` allow), so the
    f16 path's chunk scale and the relative size of the terms vary while the sum of |g| stays near (binades + 1).  The f16 path forms
    H (g Ls) in f16, Ls = 2^-e from the largest |g|: 10 binades of g on the 2^-3 grid of H keep that product a normal f16 value.
Pre-activations of exactly 0 are excluded, so nothing here depends on the ReLU derivative at 0.

`check(p)` asserts the guarantees the exactness argument needs (tests/test_exact_problems_cpu.py runs it for every shape the GPU test
uses); `make` only returns problems that pass it.
"""
import numpy as np

GRID = 2.0 ** -3          # every forward value is a multiple of GRID ...
VMAX = 2.0 ** 4           # ... below VMAX in magnitude: at most 7 significant bits (bf16 keeps 8)
F16_MIN_NORMAL = 2.0 ** -14
WEIGHTS = np.array([1.0, -1.0, 0.5, -0.5, 2.0, -2.0])


def param_names(layers):
    """State-dict names of the fused CPPN's Linears, in layer order (first layer, hidden layers, output)."""
    names = [f"early_pts_layers.{2 * i}" for i in range(layers + 1)] + ["output_linear.0"]
    return names


def _forward(ws, bs, x):
    """float64 forward: pre-activations Z_1..Z_{N+1}, activations H_0 (= x) .. H_{N+1}, raw."""
    hs, zs = [x], []
    for w, b in zip(ws[:-1], bs[:-1]):
        z = hs[-1] @ w.T + b
        zs.append(z)
        hs.append(np.maximum(z, 0.0))
    raw = hs[-1] @ ws[-1].T + bs[-1]
    return zs, hs, raw[:, 0]


def _backward(ws, zs, hs, d_out):
    """float64 backward of sum(raw * d_out): per-Linear weight / bias gradients, the dZ of every ReLU layer and J = dZ / g."""
    dz = d_out[:, None]                     # dL/draw
    grads_w, grads_b, dzs = [None] * len(ws), [None] * len(ws), [None] * (len(ws) - 1)
    for li in range(len(ws) - 1, -1, -1):
        grads_w[li] = dz.T @ hs[li]
        grads_b[li] = dz.sum(0)
        if li == 0:
            break
        dz = (dz @ ws[li]) * (zs[li - 1] > 0)
        dzs[li - 1] = dz
    return grads_w, grads_b, dzs


def _reference(ws, bs, x, d_out):
    zs, hs, raw = _forward(ws, bs, x)
    gw, gb, dzs = _backward(ws, zs, hs, d_out)
    return zs, hs, raw, gw, gb, dzs


def _on_grid(v, q=GRID, vmax=VMAX):
    s = v / q
    return bool(np.abs(v).max(initial=0.0) < vmax and np.array_equal(s, np.round(s)))


def _roundtrips(v):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
    return all(bool(torch.equal(t.to(dt).double(), t)) for dt in (torch.float32, torch.bfloat16, torch.float16))


def _f16_normal(v):
    """Exactly an f16 value and either 0 or at least f16's smallest normal (so no denormal handling of any unit is involved)."""
    a = np.abs(v)
    return _roundtrips(v) and bool(np.all((a == 0) | (a >= F16_MIN_NORMAL)))


def _lowbit(v):
    """Largest power of two dividing every nonzero entry (the common quantum of a set of dyadic values)."""
    a = np.abs(v[v != 0])
    if a.size == 0:
        return np.inf
    m, e = np.frexp(a)
    # a = m 2^e with m in [0.5, 1); the lowest set bit of m sits at 2^-(bits of m)
    bits = np.zeros_like(e)
    mm = m.copy()
    for _ in range(60):
        frac = mm != np.floor(mm)
        if not frac.any():
            break
        mm = np.where(frac, mm * 2, mm)
        bits = bits + frac
    return float(np.min(np.ldexp(1.0, (e - bits).astype(np.int64))))


def _exact_sum(terms_abs_sum, quantum):
    return terms_abs_sum < 2.0 ** 24 * quantum


def _contraction_exact(a, b):
    """sum_n a[n, o] b[n, i] for every (o, i) is exact in fp32 in any order: all terms are multiples of one quantum and the sum of
    their magnitudes stays below 2^24 quanta."""
    q = _lowbit(a) * _lowbit(b)
    if not np.isfinite(q):
        return True
    return bool(np.all(np.abs(a).T @ np.abs(b) < 2.0 ** 24 * q))


def _ls_scale(d_out):
    """f16 path: Ls = 2^-e, e the frexp exponent of max |g| (wgrad_scale_exp): g Ls lies in [., 1)."""
    gm = float(np.max(np.abs(d_out)))
    return 1.0 if gm == 0 else float(np.ldexp(1.0, -int(np.frexp(gm)[1])))


def check(p):
    """Assert every guarantee the bit-exact comparison relies on (AssertionError names the first that fails)."""
    ws, bs, x, d_out = p["ws"], p["bs"], p["pts"], p["d_out"]
    zs, hs, raw, gw, gb, dzs = _reference(ws, bs, x, d_out)
    n_layers = len(ws) - 1                                              # ReLU layers (first + hidden)
    assert _roundtrips(x) and _roundtrips(d_out)
    for w, b in zip(ws, bs):
        assert _roundtrips(w) and _roundtrips(b), "parameters are not exact in bf16 / f16"
    off = 0
    for l, z in enumerate(zs):
        assert not np.any(z == 0.0), f"pre-activation exactly 0 in layer {l}"
        assert _on_grid(z) and _f16_normal(z), f"forward values of layer {l} leave the grid"
        off += int((z < 0).sum())
    assert off >= sum(z.size for z in zs) / 3, "fewer than a third of the ReLUs are off"
    # raw = w_out . H_N + b_out: an exact fp32 sum in any order
    assert _contraction_exact(np.concatenate([hs[-1] * ws[-1][0][None, :], np.full((x.shape[0], 1), bs[-1][0])], 1).T,
                              np.ones((hs[-1].shape[1] + 1, 1))), "raw is not an exact fp32 sum"
    g = d_out
    ls = _ls_scale(g)
    assert _f16_normal(g * ls), "g Ls (f16 path) is not a normal f16 value"
    for l, dz in enumerate(dzs):
        J = dz / g[:, None]
        assert _roundtrips(dz), f"dZ of layer {l} is not exact in bf16 / f16"
        assert _f16_normal(J), f"J = dZ / g of layer {l} is not a normal f16 value"
        # f16 path: B = H_{l-1} (g Ls) is formed in f16 before the contraction with J
        assert _f16_normal(hs[l] * (g * ls)[:, None]), f"H (g Ls) feeding layer {l} is not a normal f16 value"
    # every weight and bias gradient is an exact fp32 sum in any order (and so is the f16 path's scaled form: a power of two apart)
    all_dz = dzs + [d_out[:, None]]
    for li in range(len(ws)):
        dz = all_dz[li]
        assert _contraction_exact(dz, hs[li]), f"weight gradient of Linear {li} is not an exact fp32 sum"
        assert _contraction_exact(dz, np.ones((x.shape[0], 1))), f"bias gradient of Linear {li} is not an exact fp32 sum"
        assert np.any(gw[li] != 0), f"weight gradient of Linear {li} is zero"
    return True


def _dout(rng, n_pts, spread):
    k = np.floor(np.log2(np.arange(1, n_pts + 1))).astype(np.int64)
    k = np.minimum(k, spread)
    rng.shuffle(k)
    return np.ldexp(1.0, -k) * rng.choice([-1.0, 1.0], n_pts)


def _row(rng, h, cols, weights, frac_lo=0.15, frac_hi=0.75, tries=64):
    """Weights of one row on `cols` and a bias such that the row's pre-activations avoid 0, stay on the grid and are mixed."""
    for _ in range(tries):
        w = rng.choice(weights, len(cols))
        base = h[:, cols] @ w
        if not _on_grid(base, GRID, VMAX):
            continue
        srt = np.unique(base)
        cand = np.arange(-4.0 / GRID, 4.0 / GRID + 1) * GRID
        cand = cand[(np.abs(srt[0] + cand) < VMAX) & (np.abs(srt[-1] + cand) < VMAX)]
        cand = cand[~np.isin(-cand, srt)]
        if cand.size == 0:
            continue
        on = 1.0 - np.searchsorted(np.sort(base), -cand, side="right") / base.size
        ok = cand[(on >= frac_lo) & (on <= frac_hi)]
        if ok.size:
            return w, float(rng.choice(ok))
    return None


def _try(layers, width, n_pts, rng, spread):
    x = rng.integers(-4, 5, (n_pts, 3)).astype(np.float64)
    ws, bs = [], []
    h = x
    for li in range(layers + 1):
        k_in = h.shape[1]
        w = np.zeros((width, k_in))
        b = np.zeros(width)
        if li == 0:
            pa, pb = rng.integers(0, 3, width), None
        else:
            pa, pb = rng.permutation(k_in), rng.permutation(k_in)
        for o in range(width):
            cols = [int(pa[o])]
            if pb is not None and rng.random() < 0.25 and int(pb[o]) != cols[0]:
                cols.append(int(pb[o]))
            r = _row(rng, h, cols, WEIGHTS if li == 0 else WEIGHTS[:4] if len(cols) == 2 else WEIGHTS)
            if r is None:
                r = _row(rng, h, cols[:1], WEIGHTS[:4], 0.0, 1.0)
                cols = cols[:1]
            if r is None:
                return None
            w[o, cols], b[o] = r
        ws.append(w)
        bs.append(b)
        h = np.maximum(h @ w.T + b, 0.0)
    w_out = rng.choice([1.0, -1.0, 0.5, -0.5], (1, width))
    ws.append(w_out)
    bs.append(np.array([0.375]))
    p = dict(ws=ws, bs=bs, pts=x, d_out=_dout(rng, n_pts, spread))
    try:
        check(p)
    except AssertionError:
        return None
    return p


def make(layers, width, n_pts, seed, spread=10):
    """An exact problem: dict with `params` (state-dict name -> float32 array), `pts` [P, 3], `d_out` [P] (float32) and the float64
    reference `raw` [P] and `grads` (state-dict name -> array).  Seeds are rejection-sampled: the returned problem passed check()."""
    for attempt in range(400):
        rng = np.random.default_rng([seed, layers, width, n_pts, attempt])
        sp = spread if attempt < 100 else max(4, spread // 2)
        p = _try(layers, width, n_pts, rng, sp)
        if p is None:
            continue
        zs, hs, raw, gw, gb, _ = _reference(p["ws"], p["bs"], p["pts"], p["d_out"])
        names = param_names(layers)
        p["params"] = {}
        p["grads"] = {}
        for nm, w, b, dw, db in zip(names, p["ws"], p["bs"], gw, gb):
            p["params"][nm + ".weight"] = w.astype(np.float32)
            p["params"][nm + ".bias"] = b.astype(np.float32)
            p["grads"][nm + ".weight"] = dw
            p["grads"][nm + ".bias"] = db
        p["raw"] = raw
        p["attempt"] = attempt
        p["pts"] = p["pts"].astype(np.float32)
        p["d_out64"] = p["d_out"]
        p["d_out"] = p["d_out"].astype(np.float32)
        return p
    raise RuntimeError(f"no exact problem found for {layers}x{width}, {n_pts} points, seed {seed}")
