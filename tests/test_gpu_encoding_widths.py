"""The input encodings at every band count afx_create admits (run with -m gpu on an MI355X): L = 1 ... 10, i.e. K0 = 3 + 6 L = 9 ... 63
first-layer columns, where every other GPU test uses L = 5 (K0 = 33).  K0 steers the column map of enc_value / enc_dcoef, the first-layer
slab and the encoded-input stash of the three kernel families, the k0pad -> k0 repack of the first-layer weight gradient, the fourier
coefficients' contraction and the input-gradient kernel; the edges are L = 1 (three of the four 16-column k-steps are padding), L = 2
(the padding starts at the last column of the first k-step) and L = 10 (one padding column; k0pad == width at width 64).

Reference: the CPU oracle (oracle.angio_oracle) on float32 parameters, as in test_gpu_parity; float64 for the input gradients, as in
test_gpu_input_grads.  Bars: TOL / PIX_C1 of test_gpu_parity and BAR of test_gpu_input_grads, unchanged.  Every comparison against the
float32 oracle also evaluates the oracle in float64 on the same input and prints their distance (the reference's own error) with the
error; the bars are constants and no case takes a derived one.  Measured on the host: at most 7.9e-7 on raw outputs (TOL f32 mlp 1e-5)
and 5.3e-7 on pixels (1e-5); on the gradients f32 is compared on, 6.9e-5 (fourier, L = 1, 2x128, early_pts_layers.0.weight) and 4.9e-5
(barf, L = 10, 2x256, the same key) against TOL f32 grad 1e-4, every other at most 4.5e-5 - a ReLU that switches between float32 and
float64, as in BAR's comment; the f32 kernels sit at 1.3e-6 and 2.8e-5 from the float32 oracle there.

Conditioning.  The bars were measured at L = 5 on a unit scene, where the top BARF argument is 16 pi |x|.  For BARF with L > 5 the
points are scaled by 2^(5-L), so that the top band sees the arguments it sees at L = 5; the fourier arguments do not grow with L, and
its scene stays (its coefficients are scaled as in the existing tests).  In rays mode the ORIGINS AND DIRECTIONS are scaled and near /
far stay: the points o + t d scale, the step lengths do not.  (Scaling near and far instead shrinks the optical depth with the scene -
at L = 10 to at most 2 / 32, every pixel above 0.94 - and no output-layer scale brings sigmoid's values above 1.)  The output layer is
scaled per geometry (`_state`) to the thin regime the pixel bars belong to (test_barf_backward_vs_oracle's "x4, bias -4", densities of
a few per cent; the densest ray no denser than the L = 5 controls'): the oracle's pixels then lie in (0.72, 0.995) and differ by 0.07
... 0.25 between rays, where that test's all lie within 0.001 of 0.96; they are asserted to stay inside (0.05, 0.995) and to span more
than 0.05.  A denser regime weighs a 16-bit raw error more in the pixel: at raw mean -2 (pixels inside (0.05, 0.95)) four times, and the
L = 5 control itself then misses PIX_C1 (2.6e-4 at f16).

BARF weights are the literal formula's (CPPN.barf_coefficients): band k is closed (weight exactly 0) for alpha < k + 1, on its ramp for
k + 1 <= alpha < k + 2 - the ramp starts at (1 - cos(2 * 3.1415)) / 2, which is 0.0 in float32 - and open from alpha = k + 2.  So at
alpha = L the last band is still exactly closed, at alpha = L - 0.5 band L - 2 is mid-ramp, and all L bands are open from alpha = L + 1:
the forward tests run all three.  Which columns must be exactly zero is read off the weights themselves.

Every comparison prints the error it saw and its bar ("[encw] ...")."""
import functools

import pytest
import torch

from conftest import rel_l2
from oracle import angio_oracle as orc
from test_gpu_input_grads import BAR, _check, _points, _pts_grad, _rays
from test_gpu_parity import DEV, PIX_C1, TOL, _grads_by_name, make_model
from workspace_contract import guards_intact, same_bits, typed_arena

pytestmark = pytest.mark.gpu

PRECS = ["f32", "bf16x3", "bf16", "f16", "f16s8"]
assert set(BAR) == set(PRECS)
ENCS = ["barf", "fourier"]
NEAR, FAR, S_RAYS, N_RAYS = 0.5, 2.5, 40, 300      # the ray problem of test_barf_backward_vs_oracle
N_PTS = 3001


RAW_MEAN = -3.5      # mean of the raw outputs on the ray problem's samples (their standard deviation is 1): see _state
MIN_PIXEL = 0.75     # ... unless the densest ray's pixel falls below this, the L = 5 controls' (barf 0.77, fourier 0.75)


def _scale(L, enc):
    """BARF: 2^(5-L) for L > 5.  The fourier arguments 2 pi x c do not grow with L (the coefficients' scale is the conditioning there)."""
    return 2.0 ** min(0, 5 - L) if enc == "barf" else 1.0


def _pix_bar(prec):
    """300 rays x 40 samples through a 64-wide model is the C1-sized problem of test_gpu_parity (few terms per sum to average the 16-bit
    operand rounding over): its pixel bars; f32 has one bar."""
    return PIX_C1.get(prec, TOL[prec]["pix"])


def _bar(existing, spread, what):
    """The existing bar, as it stands.  `spread`, the float32 oracle's own distance from float64 on the same input, is printed next to
    every error: it is what the issue's derived bar (max(existing, twice the distance), at most 10x) would start from, should a case ever
    miss for the reference's sake.  None does, so none is derived."""
    return existing


def _report(what, err, bar, spread=None):
    print(f"[encw] {what}: {err:.3e} (bar {bar:.1e}" + (f", oracle f32 vs f64 {spread:.1e})" if spread is not None else ")"))


def _cfg(layers, width, enc, L):
    return dict(num_early_layers=layers, num_filters=width, pos_enc=enc, pos_enc_basis=L)


@functools.lru_cache(maxsize=None)
def _state(layers, width, enc, L, coef_scale=0.1):
    """Parameters of one geometry, the same at every precision (made on the host): nn.Linear's initialisation, fourier coefficients
    scaled to sigma 0.5 (0.1: arguments of a few radians on a unit scene; 0.02 for large coordinates), and the output layer scaled and
    shifted so that the raw outputs on the ray problem's samples (every BARF band open) have mean RAW_MEAN and standard deviation 1:
    the thin regime of test_barf_backward_vs_oracle's "x4, bias -4" (whose pixels all lie within 0.001 of 0.96 here, whatever L is)
    with the same variation along the rays at every band count and width.  Where that leaves the densest ray denser than the L = 5
    controls' (pixel MIN_PIXEL), the bias is lowered until it is not: a 16-bit raw error weighs in a pixel as the density does."""
    from nerf_for_angiography_amd.model.CPPN import CPPN
    torch.manual_seed(7000 + 100 * L + layers + width + (1 if enc == "fourier" else 0))
    md = dict(num_early_layers=layers, num_late_layers=0, num_filters=width, num_input_channels=3, num_output_channels=1,
              num_input_channels_views=0, use_bias=True, pos_enc=enc, pos_enc_basis=L, act_func="relu", fourier_sigma=5, num_img=1,
              device=torch.device("cpu"))
    m = CPPN(md)
    with torch.no_grad():
        if enc == "fourier":
            m.fourier_coefficients.mul_(coef_scale)
        state = {k: v.detach().clone() for k, v in m.state_dict().items() if k != "barf_weights"}
        o, d, _ = _ray_problem(L, enc)
        ri, ts, te = orc.march_uniform(NEAR, FAR, S_RAYS, N_RAYS)
        p = dict(state, barf_weights=torch.ones(3 * L))
        raw = orc.cppn_forward(orc.points_acc(o, d, ri, ts, te), _cfg(layers, width, enc, L), p).double()
        mean, std = float(raw.mean()), float(raw.std())
        assert std > 0
        state["output_linear.0.weight"] = (state["output_linear.0.weight"].double() / std).float()
        z = ((raw - mean) / std).reshape(N_RAYS, S_RAYS)

        def min_pixel(b):
            return float(torch.exp(-torch.sigmoid(z + b).sum(1) * ((FAR - NEAR) / S_RAYS)).min())

        shift = RAW_MEAN
        if min_pixel(shift) < MIN_PIXEL:
            lo, hi = shift - 10.0, shift      # min_pixel falls as the bias rises
            for _ in range(40):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if min_pixel(mid) >= MIN_PIXEL else (lo, mid)
            shift = lo
        state["output_linear.0.bias"] = ((state["output_linear.0.bias"].double() - mean) / std + shift).float()
    return state


def _barf_w(L, alpha):
    from nerf_for_angiography_amd.model.CPPN import CPPN
    k = torch.repeat_interleave(torch.arange(0.0, L), 3)
    return CPPN.barf_coefficients(None, alpha, k).detach()


def _params(layers, width, enc, L, alpha=None, dtype=torch.float32, coef_scale=0.1):
    p = {k: v.to(dtype) for k, v in _state(layers, width, enc, L, coef_scale).items()}
    if enc == "barf":
        p["barf_weights"] = _barf_w(L, alpha).to(dtype)
    return p


def _model(layers, width, enc, L, prec, alpha=None, coef_scale=0.1):
    m = make_model(layers, width, enc, precision=prec, basis=L)
    missing, unexpected = m.load_state_dict(_state(layers, width, enc, L, coef_scale), strict=False)
    assert not unexpected and set(missing) <= {"barf_weights"}
    if enc == "barf":
        m.update_barf_alpha(alpha, "pts")
        assert torch.equal(m.barf_weights.detach().cpu(), _barf_w(L, alpha))
    if enc == "fourier" and prec == "f32":
        m.fourier_coefficients.requires_grad_(False)      # (their own gradient needs a 16-bit precision)
    assert m.fused and m.engine.k0 == 3 + 6 * L
    return m


def _ray_problem(L, enc, n_rays=N_RAYS, seed=11):
    g = torch.Generator().manual_seed(seed)
    s = _scale(L, enc)
    o = (torch.tensor([[0.0, 0.0, 1.5]]).repeat(n_rays, 1) + torch.randn(n_rays, 3, generator=g) * 0.01) * s
    d = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g) * 0.2 + torch.tensor([0, 0, -1.0]), dim=-1) * s
    return o.float().contiguous(), d.float().contiguous(), torch.rand(n_rays, generator=g).float()


def _pts_problem(L, enc, n=N_PTS, seed=12):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, 3, generator=g) * 2 - 1) * _scale(L, enc)).float().contiguous()


def _spread_ok(pix):
    lo, hi = float(pix.min()), float(pix.max())
    assert 0.05 < lo and hi < 0.995 and hi - lo > 0.05, (lo, hi)


@functools.lru_cache(maxsize=None)
def _oracle_forward(layers, width, enc, L, alpha):
    """-> raw [P] and pixels [R] of the float32 oracle, and its distance from the float64 oracle on the same inputs."""
    cfg, pts, (o, d, _) = _cfg(layers, width, enc, L), _pts_problem(L, enc), _ray_problem(L, enc)
    out = {}
    for dt in (torch.float32, torch.float64):
        p = _params(layers, width, enc, L, alpha, dt)
        with torch.no_grad():
            raw = orc.cppn_forward(pts.to(dt), cfg, p).reshape(-1)
            pix = orc.render_rays(o.to(dt), d.to(dt), cfg, p, near=NEAR, far=FAR, n_samples=S_RAYS, convention="acc")
        out[dt] = (raw.numpy(), pix.numpy())
    _spread_ok(out[torch.float64][1])
    raw, pix = out[torch.float32]
    return raw, pix, rel_l2(raw, out[torch.float64][0]), rel_l2(pix, out[torch.float64][1])


@functools.lru_cache(maxsize=None)
def _oracle_backward(layers, width, enc, L, alpha):
    """-> pixels and gradients by name of the float32 oracle (MSE against the problem's targets), and per name the distance of the
    float32 gradient from the float64 one."""
    cfg, (o, d, tgt) = _cfg(layers, width, enc, L), _ray_problem(L, enc)
    res = {}
    for dt in (torch.float32, torch.float64):
        p = _params(layers, width, enc, L, alpha, dt)
        # (the oracle's 'acc' compositing returns float32 pixels whatever it computed in: the targets stay float32)
        pix, _, grads = orc.loss_and_grads(o.to(dt), d.to(dt), tgt, cfg, p, near=NEAR, far=FAR, n_samples=S_RAYS, convention="acc")
        res[dt] = (pix.numpy(), {k: v.numpy() for k, v in grads.items()})
    _spread_ok(res[torch.float64][0])
    pix, grads = res[torch.float32]
    spread = {k: rel_l2(v, res[torch.float64][1][k]) for k, v in grads.items()}
    spread["pix"] = rel_l2(pix, res[torch.float64][0])
    return pix, grads, spread


def _alpha_bwd(L):
    return L + 0.5      # bands 0 ... L-2 open, the last one mid-ramp (weight 0.4999)


# ------------------------------------------------------------------------------------------------- (a) forward, every band count
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("L", range(1, 11))
def test_forward_at_every_band_count(L, enc, prec):
    """4x64 through model(x) and render_rays under no_grad.  BARF at alpha = L + 1 (every band open), L (the last band still exactly
    closed: its 6 columns are zeros) and L - 0.5 (band L - 2 mid-ramp)."""
    from nerf_for_angiography_amd.render import render_rays
    pts, (o, d, _) = _pts_problem(L, enc), _ray_problem(L, enc)
    for alpha in ((L + 1.0, float(L), L - 0.5) if enc == "barf" else (None,)):
        raw_c, pix_c, s_raw, s_pix = _oracle_forward(4, 64, enc, L, alpha)
        m = _model(4, 64, enc, L, prec, alpha)
        with torch.no_grad():
            raw = m(pts.to(DEV)).reshape(-1).cpu().numpy()
            pix = render_rays(m, o.to(DEV), d.to(DEV), S_RAYS, NEAR, FAR, mode="acc").rgb_map.cpu().numpy()
        what = f"forward L={L} {enc} alpha={alpha} {prec}"
        bar_raw, bar_pix = _bar(TOL[prec]["mlp"], s_raw, what), _bar(_pix_bar(prec), s_pix, what)
        e_raw, e_pix = rel_l2(raw, raw_c), rel_l2(pix, pix_c)
        _report(what + " raw", e_raw, bar_raw, s_raw)
        _report(what + " pixels", e_pix, bar_pix, s_pix)
        assert e_raw < bar_raw, (what, e_raw)
        assert e_pix < bar_pix, (what, e_pix)


@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("L", [1, 2, 10])
def test_large_coordinates_at_the_edges(L, enc):
    """test_encoding_large_coordinates (the kernels' own argument reduction at arguments of 1e5 rad) at the edge band counts, against
    the float32 oracle at the same bar: |x| up to 2 000 x 2^(5-L) for L > 5, which puts the top BARF argument where that test has it.
    (The float32 oracle rounds the arguments as the kernels do; float64 does not, so its distance says nothing here.)"""
    cs = 0.02
    m = _model(2, 64, enc, L, "f32", L + 1.0, coef_scale=cs)
    pts = (torch.rand(8192, 3, generator=torch.Generator().manual_seed(21)) * 2 - 1) * (2000.0 * _scale(L, enc))
    with torch.no_grad():
        want = orc.cppn_forward(pts, _cfg(2, 64, enc, L), _params(2, 64, enc, L, L + 1.0, coef_scale=cs)).reshape(-1).numpy()
        got = m(pts.to(DEV)).reshape(-1).cpu().numpy()
    _report(f"large coordinates L={L} {enc}", rel_l2(got, want), 5e-5)
    assert rel_l2(got, want) < 5e-5


# ------------------------------------------------------------------------------------------------- (b) backward, the edges at every width
def _check_grads(what, got, want, spread, bar_of, keys=None):
    assert set(want) <= set(got) | {"fourier_coefficients"}, (what, set(want) - set(got))
    for k, v in want.items():
        if k not in got or (keys is not None and k not in keys):
            continue
        bar = _bar(bar_of(k), spread[k], (what, k))
        err = rel_l2(got[k], v)
        _report(f"{what} {k}", err, bar, spread[k])
        assert err < bar, (what, k, err)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("width", [64, 128, 256])
@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("L", [1, 2, 5, 10])
def test_backward_at_the_edges(L, enc, width, prec):
    """Every parameter gradient by name against the oracle's autograd, 2 hidden layers: render_rays + autograd at every precision, the
    fused train step at the 16-bit ones (bf16x3: its forward is the plain-bf16 backward kernel's, so the Linear parameters take bf16's
    bar as in test_fused_train_step_matches_autograd_path).  Fourier at a 16-bit precision: the coefficients' gradient at twice the
    precision's own bar in rays mode (autograd and train step) and at twice that again in points mode, both as in
    test_fourier_coefficients_train.  Points mode uses POSITIVE cotangents: with that test's random-sign ones the sum cancels, by an
    amount that depends on the geometry - sqrt(sum of the squared terms) over |their sum|, in float64 on the host, is 0.8 ... 1.0 for
    the L = 5 controls but 2.0 (L = 1, 2x64) and 2.8 (L = 2, 2x256), and just those cases carried the plain-bf16 backward's rounding
    past the bar (bf16x3: 0.145 and 0.161, and 0.136 at L = 1, 2x128, against 0.12).  With cotangents in (0.5, 1.5) the ratio is 0.1
    ... 0.4 for every case, below the controls', so the existing bar applies as it stands."""
    from nerf_for_angiography_amd.engine import RenderSpec
    from nerf_for_angiography_amd.render import render_rays, train_step_mse
    alpha = _alpha_bwd(L) if enc == "barf" else None
    pix_c, grads_c, spread = _oracle_backward(2, width, enc, L, alpha)
    m = _model(2, width, enc, L, prec, alpha)
    o, d, tgt = (t.to(DEV) for t in _ray_problem(L, enc))
    what = f"backward L={L} {enc} 2x{width} {prec}"
    coef = "fourier_coefficients"

    out = render_rays(m, o, d, S_RAYS, NEAR, FAR, mode="acc")
    torch.nn.functional.mse_loss(out.rgb_map, tgt).backward()
    bar = _bar(_pix_bar(prec) if width == 64 else TOL[prec]["pix"], spread["pix"], what)
    e_pix = rel_l2(out.rgb_map.detach().cpu().numpy(), pix_c)
    _report(what + " pixels", e_pix, bar, spread["pix"])
    assert e_pix < bar, (what, e_pix)
    got = _grads_by_name(m)
    assert (coef in got) == (enc == "fourier" and prec != "f32")
    _check_grads(what + " autograd", got, grads_c, spread, lambda k: (2 if k == coef else 1) * TOL[prec]["grad"])
    if prec == "f32":
        return

    m.zero_grad(set_to_none=True)
    spec = RenderSpec(n_rays=N_RAYS, n_samples=S_RAYS, origins=o, dirs=d, mode="acc", t_near=NEAR, t_far=FAR)
    train_step_mse(m, spec, tgt)
    btol = prec if prec in ("f16", "f16s8") else "bf16"
    _check_grads(what + " train step", _grads_by_name(m), grads_c, spread,
                 lambda k: 2 * TOL[prec]["grad"] if k == coef else TOL[btol]["grad"])
    if enc != "fourier":
        return

    # points mode: d(sum c_p raw_p) / d coef
    m.zero_grad(set_to_none=True)
    pts = _pts_problem(L, enc, 1000, seed=13)
    c = torch.rand(1000, 1, generator=torch.Generator().manual_seed(14)) + 0.5
    (m(pts.to(DEV)) * c.to(DEV)).sum().backward()
    want = {}
    for dt in (torch.float32, torch.float64):
        p = _params(2, width, enc, L, None, dt)
        p[coef] = p[coef].clone().requires_grad_(True)
        (orc.cppn_forward(pts.to(dt), _cfg(2, width, enc, L), p) * c.to(dt)).sum().backward()
        want[dt] = p[coef].grad.numpy()
    s = rel_l2(want[torch.float32], want[torch.float64])
    bar = _bar(4 * TOL[prec]["grad"], s, what)
    err = rel_l2(m.fourier_coefficients.grad.cpu().numpy(), want[torch.float32])
    _report(what + " points-mode coefficients", err, bar, s)
    assert err < bar, (what, err)


# ------------------------------------------------------------------------------------------------- (c) exact zeros
def _w0_grad(m, L, mode, seed, zero_coord=None):
    """early_pts_layers.0.weight.grad [64, 3 + 6 L] and the first-layer bias gradient after one backward pass; zero_coord: that
    coordinate of every sample is exactly 0 (rays: of every origin and direction)."""
    from nerf_for_angiography_amd.render import render_rays
    m.zero_grad(set_to_none=True)
    enc = m.use_pos_enc
    if mode == "rays":
        o, d, tgt = (t.to(DEV) for t in _ray_problem(L, enc, seed=seed))
        if zero_coord is not None:
            o[:, zero_coord] = 0.0
            d[:, zero_coord] = 0.0
        torch.nn.functional.mse_loss(render_rays(m, o, d, S_RAYS, NEAR, FAR, mode="acc").rgb_map, tgt).backward()
    else:
        pts = _pts_problem(L, enc, seed=seed).to(DEV)
        if zero_coord is not None:
            pts[:, zero_coord] = 0.0
        w = torch.randn(N_PTS, 1, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
        (m(pts) * w).sum().backward()
    lin = m.early_pts_layers[0]
    return lin.weight.grad.detach().cpu(), lin.bias.grad.detach().cpu()


# (L, alpha): the closed bands' columns are exact zeros.  (10, 2.0), (1, 0.0) and (2, 1.0) leave bands 1 ... 9, band 0, and both bands
# closed (a ramp starts at exactly 0.0); (10, 2.5), (2, 1.5) put the last open band mid-ramp next to the first closed one, and
# (10, 11.0), (1, 2.0) open every band: no column may be zero then.
ZERO_CASES = [(10, 2.0), (10, 2.5), (10, 11.0), (1, 0.0), (1, 2.0), (2, 1.0), (2, 1.5)]


@pytest.mark.parametrize("mode,prec", [("rays", p) for p in PRECS] + [("points", p) for p in ("f32", "f16", "f16s8")])
@pytest.mark.parametrize("L,alpha", ZERO_CASES)
def test_closed_barf_bands_give_exactly_zero_gradient_columns(L, alpha, mode, prec):
    """Column 3 + 3 k + c of W0 is w_k sin(2^k pi x_c), column 3 + 3 L + 3 k + c its cosine.  A band with weight exactly 0 feeds zeros,
    so its 2 x 3 columns of the first-layer weight gradient are exactly 0.0 at every precision; the raw columns and every open band's
    columns are not.  No tolerance: an off-by-one in the sin / cos boundary, the coordinate index or the k0pad -> k0 repack moves a
    non-zero into a column that must be zero (or a zero into one that must not be)."""
    w = _barf_w(L, alpha)
    m = _model(2, 64, "barf", L, prec, alpha)
    g, _ = _w0_grad(m, L, mode, seed=31)
    assert g.shape == (64, 3 + 6 * L)
    live = torch.cat([torch.ones(3, dtype=torch.bool), w != 0, w != 0])
    assert all(float(x) == 0.0 or float(x) > 0.49 for x in w)      # closed, or at least mid-ramp: nothing that a 16-bit format flushes
    col_max = g.abs().max(dim=0).values
    print(f"[encw] zeros L={L} alpha={alpha} {mode} {prec}: live columns {int(live.sum())} of {live.numel()}, smallest live |max| "
          f"{float(col_max[live].min()):.3e}, largest dead |max| {float(col_max[~live].max()) if (~live).any() else 0.0:.3e}")
    assert torch.isfinite(g).all()
    assert bool((col_max[~live] == 0.0).all()), [int(i) for i in torch.nonzero(~live & (col_max != 0)).reshape(-1)]
    assert bool((col_max[live] > 0.0).all()), [int(i) for i in torch.nonzero(live & (col_max == 0)).reshape(-1)]


@pytest.mark.parametrize("mode,prec", [("rays", p) for p in PRECS] + [("points", p) for p in ("f32", "f16", "f16s8")])
@pytest.mark.parametrize("L,idx", [(1, 1), (2, 5), (10, 0), (10, 29)])
def test_a_zero_fourier_coefficient_gives_a_zero_sine_column(L, idx, mode, prec):
    """coefficient idx = 0.0: sin(0) = 0 exactly, so column 3 + idx of the W0 gradient is exactly zero and no other column is;
    cos(0) = 1 exactly, so column 3 + 3 L + idx is the first-layer bias gradient (within the gradient bar: the 16-bit kernels contract
    the two in different kernels)."""
    m = _model(2, 64, "fourier", L, prec)
    with torch.no_grad():
        m.fourier_coefficients[idx] = 0.0
    g, gb = _w0_grad(m, L, mode, seed=33)
    col_max = g.abs().max(dim=0).values
    zero = [int(i) for i in torch.nonzero(col_max == 0).reshape(-1)]
    assert zero == [3 + idx], zero
    err = rel_l2(g[:, 3 + 3 * L + idx].numpy(), gb.numpy())
    _report(f"fourier zero coefficient L={L} idx={idx} {mode} {prec}: cos column vs bias gradient", err, TOL[prec]["grad"])
    assert err < TOL[prec]["grad"]


@pytest.mark.parametrize("mode,prec", [("rays", p) for p in PRECS] + [("points", p) for p in ("f32", "f16", "f16s8")])
@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("L,coord", [(1, 0), (1, 2), (2, 1), (10, 0), (10, 1), (10, 2)])
def test_a_zero_coordinate_gives_zero_raw_and_sine_columns(L, coord, enc, mode, prec):
    """The band weights are the same for the three coordinates, so the closed-band test cannot see WHICH coordinate feeds a column.
    With coordinate c of every sample exactly 0 (every band open), the raw column c and the sine columns 3 + 3 k + c of every band k
    receive zeros - sin(0) = 0 exactly in enc_sincos - and no other column does (the cosine columns receive w_k).  No tolerance: a
    wrong coordinate index moves the zero columns."""
    m = _model(2, 64, enc, L, prec, L + 1.0)
    g, _ = _w0_grad(m, L, mode, seed=35, zero_coord=coord)
    col_max = g.abs().max(dim=0).values
    assert torch.isfinite(g).all()
    zero = [int(i) for i in torch.nonzero(col_max == 0).reshape(-1)]
    assert zero == [coord] + [3 + 3 * k + coord for k in range(L)], zero


# ------------------------------------------------------------------------------------------------- (d) input gradients at the edges
def _min_ws(m, q_args):
    from nerf_for_angiography_amd import _lib
    e = m.engine
    e.max_workspace_bytes = int(e.lib.afx_query(e.h, _lib.Q_BWD_INPUTS_WORKSPACE_MIN, *q_args, _lib.PREC[m.precision]))
    e._ws = None


def _full_ws(m):
    m.engine.max_workspace_bytes = 24 << 30
    m.engine._ws = None


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("width", [64, 256])
@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("L", [1, 2, 10])
def test_point_gradients_at_the_edges(L, enc, width, prec):
    """dL/dx through model(x) against the float64 oracle on the same (rescaled) points, at BAR; bit-identical between the FULL workspace
    and AFX_Q_BWD_INPUTS_WORKSPACE_MIN (one tile per chunk), and with and without the parameter gradients (grad_flat) requested."""
    alpha = _alpha_bwd(L) if enc == "barf" else None
    m = _model(4, width, enc, L, prec, alpha)
    pts = _pts_problem(L, enc, seed=15)
    _, w = _points(N_PTS, 16)
    got = _pts_grad(m, pts, w)
    assert got.shape == (N_PTS, 3)
    x = pts.double().requires_grad_(True)
    (orc.cppn_forward(x, _cfg(4, width, enc, L), _params(4, width, enc, L, alpha, torch.float64)).squeeze(-1) * w.double()).sum().backward()
    _check(f"points L={L} {enc} 4x{width} {prec}", got, x.grad, prec)
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    assert "early_pts_layers.0.weight" in grads
    _min_ws(m, (0, N_PTS))
    m.zero_grad(set_to_none=True)
    assert torch.equal(_pts_grad(m, pts, w), got)
    _full_ws(m)
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = None
    assert torch.equal(_pts_grad(m, pts, w), got)
    assert all(p.grad is None for p in m.parameters())


def _ray_grads_acc(m, o, d, wpix, S, params_grad=True):
    """_ray_grads of test_gpu_input_grads ('acc', near 1, far 3), except that at f32 the fourier coefficients stay frozen (their gradient
    needs a 16-bit precision; _ray_grads switches requires_grad of every parameter)."""
    from nerf_for_angiography_amd.render import render_rays
    for k, p in m.named_parameters():
        p.requires_grad_(params_grad and not (k == "fourier_coefficients" and m.precision == "f32"))
        p.grad = None
    og, dg = o.to(DEV).clone().requires_grad_(True), d.to(DEV).clone().requires_grad_(True)
    out = render_rays(m, og, dg, S, 1.0, 3.0, mode="acc")
    (out.rgb_map * wpix.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return og.grad, dg.grad


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("L", [1, 2, 10])
def test_ray_gradients_at_the_edges(L, enc, prec):
    """dL/d(origins, directions) through render_rays ('acc', 37 rays x 33 samples, near 1 / far 3 as in test_gpu_input_grads) at 4x64."""
    R, S = 37, 33
    alpha = _alpha_bwd(L) if enc == "barf" else None
    m = _model(4, 64, enc, L, prec, alpha)
    o, d, wpix = _rays(R, 17)
    o, d = (o * _scale(L, enc)).contiguous(), (d * _scale(L, enc)).contiguous()
    go, gd = _ray_grads_acc(m, o, d, wpix, S)
    od, dd = o.double().requires_grad_(True), d.double().requires_grad_(True)
    pix = orc.render_rays(od, dd, _cfg(4, 64, enc, L), _params(4, 64, enc, L, alpha, torch.float64), near=1.0, far=3.0, n_samples=S,
                          convention="acc")
    (pix * wpix.double()).sum().backward()
    _check(f"rays L={L} {enc} {prec} origins", go, od.grad, prec)
    _check(f"rays L={L} {enc} {prec} dirs", gd, dd.grad, prec)
    _min_ws(m, (R, S))
    go2, gd2 = _ray_grads_acc(m, o, d, wpix, S)
    _full_ws(m)
    go3, gd3 = _ray_grads_acc(m, o, d, wpix, S, params_grad=False)
    assert all(p.grad is None for p in m.parameters())
    assert torch.equal(go, go2) and torch.equal(gd, gd2)
    assert torch.equal(go, go3) and torch.equal(gd, gd3)


# ------------------------------------------------------------------------------------------------- (e) workspace and output discipline
@pytest.mark.parametrize("prec", ["f32", "f16", "f16s8"])
@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("L", [1, 10])
def test_results_do_not_depend_on_stale_workspace_at_the_edges(L, enc, prec):
    """test_results_do_not_depend_on_stale_workspace at K0 = 9 and 63: the same step with the workspace pre-filled with zeros, 0xFF
    bytes and random bytes gives bit-identical pixels and gradients - render + autograd, the fused train step, points mode; the workspace
    is twice AFX_Q_BWD_WORKSPACE_MIN, which splits the 300 x 40 rays into chunks."""
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.engine import RenderSpec
    from nerf_for_angiography_amd.render import render_rays, train_step_mse
    dev = torch.device(DEV)
    alpha = _alpha_bwd(L) if enc == "barf" else None
    o, d, tgt = (t.to(dev) for t in _ray_problem(L, enc))
    pts = _pts_problem(L, enc).to(dev)
    wp = torch.randn(N_PTS, 1, generator=torch.Generator().manual_seed(18)).to(dev)

    def run(fill, mode):
        m = _model(3, 64, enc, L, prec, alpha)
        e = m.engine
        ws_bytes = 2 * int(e.lib.afx_query(e.h, _lib.Q_BWD_WORKSPACE_MIN, N_RAYS, S_RAYS, _lib.PREC[prec]))
        e.max_workspace_bytes = ws_bytes
        ws = e._workspace(ws_bytes, dev)
        if fill == "zero":
            ws.zero_()
        elif fill == "ff":
            ws.fill_(255)
        else:
            ws.random_(0, 256)
        if mode == "points":
            pix = m(pts)
            (pix * wp).sum().backward()
            pix = pix.detach()
        elif mode == "fused":
            _, pix = train_step_mse(m, RenderSpec(n_rays=N_RAYS, n_samples=S_RAYS, origins=o, dirs=d, mode="acc", t_near=NEAR, t_far=FAR), tgt)
        else:
            out = render_rays(m, o, d, S_RAYS, NEAR, FAR, mode="acc")
            torch.nn.functional.mse_loss(out.rgb_map, tgt).backward()
            pix = out.rgb_map.detach()
        assert e._ws is ws      # the painted buffer is the one the step used
        return pix.cpu(), torch.cat([p.grad.reshape(-1) for p in m.parameters() if p.grad is not None]).cpu()

    for mode in ("autograd", "fused", "points"):
        if mode == "fused" and prec == "f32":
            continue
        ref = run("zero", mode)
        assert float(ref[1].abs().max()) > 0 and bool(torch.isfinite(ref[1]).all())
        for fill in ("ff", "rand"):
            got = run(fill, mode)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (mode, fill)


@pytest.mark.parametrize("prec", ["f32", "f16", "f16s8"])
@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("L", [1, 2, 10])
def test_c_abi_writes_param_count_floats_and_no_more(L, enc, prec):
    """afx_render_backward and afx_mlp_backward with grad_flat carved out of a larger allocation, guard bands painted on both sides:
    the guards are intact, the interior is the gradient a plain buffer receives, and a second run gives the same bits."""
    from nerf_for_angiography_amd.engine import RenderSpec
    alpha = _alpha_bwd(L) if enc == "barf" else None
    m = _model(2, 64, enc, L, prec, alpha)
    e, prep = m.engine, m._prepared()
    n = e.param_count
    assert n == 64 * (3 + 6 * L) + 64 + 2 * (64 * 64 + 64) + 65
    o, d, tgt = (t.to(DEV) for t in _ray_problem(L, enc))
    spec = RenderSpec(n_rays=N_RAYS, n_samples=S_RAYS, origins=o, dirs=d, mode="acc", t_near=NEAR, t_far=FAR)
    pixel, _, _ = e.render_forward(prep, spec, prec)
    d_pixel = (2.0 / N_RAYS) * (pixel - tgt)
    pts = _pts_problem(L, enc).to(DEV)
    d_out = torch.randn(N_PTS, generator=torch.Generator().manual_seed(19)).to(DEV)

    def rays(grad):
        e.render_backward(prep, spec, pixel, d_pixel, grad, prec)

    def points(grad):
        e.mlp_backward(prep, pts, d_out, grad, prec)

    for call in (rays, points):
        plain = torch.zeros(n, dtype=torch.float32, device=DEV)
        call(plain)
        torch.cuda.synchronize()
        assert float(plain.abs().max()) > 0
        runs = []
        for fill in (0xFF, "random"):
            whole, grad = typed_arena((n,), torch.float32, fill, DEV, seed=L)
            grad.zero_()
            before = whole.clone()
            call(grad)
            torch.cuda.synchronize()
            assert guards_intact(whole, 4 * n, before), (call.__name__, fill)
            assert same_bits(grad, plain), (call.__name__, fill)
            runs.append(grad.clone())
        assert same_bits(runs[0], runs[1])


def test_graph_replay_of_the_train_step_at_63_columns():
    """afx_train_step_mse at L = 10, f16s8, captured and replayed as in test_hip_graph_capture_of_the_render_and_train_step: the replay is
    the eager result bit for bit."""
    from nerf_for_angiography_amd.engine import RenderSpec
    L, prec = 10, "f16s8"
    m = _model(4, 64, "barf", L, prec, _alpha_bwd(L))
    o, d, tgt = (t.to(DEV) for t in _ray_problem(L, "barf"))
    spec = RenderSpec(n_rays=N_RAYS, n_samples=S_RAYS, origins=o, dirs=d, mode="acc", t_near=NEAR, t_far=FAR)
    eng, prepared = m.engine, m._prepared()
    grad_eager = torch.zeros(eng.param_count, device=DEV)
    pix_eager = eng.train_step_mse(prepared, spec, tgt, 1.0 / N_RAYS, grad_eager, prec)      # also sizes the workspace
    torch.cuda.synchronize()
    assert float(grad_eager.abs().max()) > 0
    grad_g = torch.zeros(eng.param_count, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            grad_g.zero_()
            pix_g = eng.train_step_mse(prepared, spec, tgt, 1.0 / N_RAYS, grad_g, prec)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pix_g, pix_eager)
    assert torch.equal(grad_g, grad_eager)


# ------------------------------------------------------------------------------------------------- (f) the exact-fp32 kernels' LDS
@pytest.mark.parametrize("L", [8, 9, 10])
def test_f32_lds_limit_of_encoded_8x256_models(L):
    """launch_chain's LDS sum at f32, 8 hidden layers of width 256: the forward pass needs 142 336 B at L = 10 and runs; the backward pass
    needs 171 264 B at L = 9 and 179 456 B at L = 10 (> 163 840 B: refused with a clear error), and fits for L <= 8, which trains."""
    from nerf_for_angiography_amd._lib import AfxError
    from nerf_for_angiography_amd.render import render_rays
    alpha = _alpha_bwd(L)
    pix_c, grads_c, spread = _oracle_backward(8, 256, "barf", L, alpha)
    m = _model(8, 256, "barf", L, "f32", alpha)
    o, d, tgt = (t.to(DEV) for t in _ray_problem(L, "barf"))
    what = f"f32 8x256 barf L={L}"
    with torch.no_grad():
        pix = render_rays(m, o, d, S_RAYS, NEAR, FAR, mode="acc").rgb_map
    bar = _bar(TOL["f32"]["pix"], spread["pix"], what)
    _report(what + " pixels (no_grad)", rel_l2(pix.cpu().numpy(), pix_c), bar, spread["pix"])
    assert rel_l2(pix.cpu().numpy(), pix_c) < bar
    out = render_rays(m, o, d, S_RAYS, NEAR, FAR, mode="acc")
    loss = torch.nn.functional.mse_loss(out.rgb_map, tgt)
    if L >= 9:
        with pytest.raises(AfxError, match="LDS"):
            loss.backward()
        return
    loss.backward()
    _check_grads(what, _grads_by_name(m), grads_c, spread, lambda k: TOL["f32"]["grad"])
