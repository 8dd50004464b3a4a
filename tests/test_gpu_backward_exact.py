"""Exact and invariance tests for the 16-bit and 8-bit-stash backward (run with -m gpu on an MI355X).

A. Points mode (afx_mlp_infer / afx_mlp_backward through CPPN's autograd Function) on problems whose every intermediate is exact in every
   precision (tests/exact_problems.py): raw and every gradient must equal the float64 reference bit for bit, at all five precisions.
B. Rays mode: transformations that cannot change the answer.  The 8-bit stash rounds dZ' stochastically with random bits hashed from the
   sample's position, layer and feature tile, and normalises g per 32-sample group (one ray's), so every group's bytes are fixed by its ray:
   permuting rays, splitting a batch, scaling the loss by a power of two and chunking change only the order of fp32 sums.
   Every test prints the largest error it saw ("[exact] ...")."""
import functools

import numpy as np
import pytest
import torch

import exact_problems
from conftest import rel_l2
from test_gpu_parity import DEV, make_model
from test_gpu_round3 import _ref_iteration_problem

pytestmark = pytest.mark.gpu

PRECS = ["f32", "bf16x3", "bf16", "f16", "f16s8"]


def _report(what, err):
    print(f"[exact] {what}: {err:.3e}")


# ------------------------------------------------------------------------------------------------ A. exact points-mode problems
SHAPES = [(1, 64, 1), (4, 64, 255), (8, 64, 33), (12, 64, 257), (1, 128, 31), (4, 128, 4097), (8, 128, 255), (1, 256, 257),
          (4, 256, 33), (8, 256, 1025)]
CHUNKED = (4, 64, 12001)


@functools.lru_cache(maxsize=None)
def _problem(layers, width, n_pts):
    return exact_problems.make(layers, width, n_pts, seed=1)


def _exact_run(layers, width, n_pts, prec, ws_cap=None):
    p = _problem(layers, width, n_pts)
    m = make_model(layers, width, precision=prec)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p["params"].items()}, strict=False)
    if ws_cap is not None:
        m.engine.max_workspace_bytes = ws_cap(m)
        m.engine._ws = None
    raw = m(torch.from_numpy(p["pts"]).to(DEV))
    (raw.squeeze(-1) * torch.from_numpy(p["d_out"]).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(raw.detach().squeeze(-1).cpu().numpy(), p["raw"].astype(np.float32)), "raw"
    got = {k: q.grad.detach().cpu().numpy() for k, q in m.named_parameters() if q.grad is not None}
    assert set(p["grads"]) <= set(got)
    for k, want in p["grads"].items():
        bad = int((got[k] != want.astype(np.float32)).sum())
        assert bad == 0, (k, bad)
    return m


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layers,width,n_pts", SHAPES)
def test_points_mode_is_exact_on_dyadic_problems(layers, width, n_pts, prec):
    """Widths 64 / 128 / 256, 1 ... 12 hidden layers, 1 ... 4 097 points (ragged last tiles): raw and every gradient bit for bit.  (f16s8 takes
    the 16-bit stash in points mode: this pins k_wgrad_bf16 and the points-mode chain at every precision.)"""
    _exact_run(layers, width, n_pts, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_points_mode_is_exact_over_several_chunks(prec):
    """~70 000 points with the workspace capped (as test_backward_chunking_is_invisible does) so that the backward runs in >= 3 chunks."""
    from nerf_for_angiography_amd import _lib
    layers, width, n_pts = CHUNKED

    def cap(m):
        q = lambda n: int(m.engine.lib.afx_query(m.engine.h, _lib.Q_BWD_WORKSPACE_FULL, 0, n, _lib.PREC[prec]))
        return q(1) + (q(n_pts) - q(1)) // 4          # room for ~1/4 of the tiles per chunk
    _exact_run(layers, width, n_pts, prec, ws_cap=cap)


# ------------------------------------------------------------------------------------------------ B. rays-mode invariances
R = 1001                 # odd: the last tile is ragged
BAR = 2e-6               # fp32 re-association: the largest error seen on an MI355X was 6e-7 (permutation, acc, 300 samples, f16)
NEAR, FAR = 1400.0, 1600.0


def _model(layers, width, prec, enc="none", bias=-5.0):
    torch.manual_seed(0)
    m = make_model(layers, width, enc, precision=prec)
    if enc == "barf":
        m.update_barf_alpha(2.5, "pts")
    with torch.no_grad():
        m.output_linear[0].weight.mul_(4.0)
        m.output_linear[0].bias.fill_(bias)
    return m


def _rays(n=R, seed=11):
    o, d, tgt = _ref_iteration_problem(n, seed=seed)
    return o.to(DEV), d.to(DEV), tgt.to(DEV)


def _grads(m):
    out = torch.cat([q.grad.reshape(-1) for q in m._fn_params()]).detach().double().cpu()
    m.zero_grad(set_to_none=True)
    return out


def _perm(n, seed=5):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _autograd(m, o, d, s, w, mode="acc", z=None):
    from nerf_for_angiography_amd.render import render_rays
    out = render_rays(m, o, d, s, NEAR, FAR, mode=mode, z=z)
    (out.rgb_map * w).sum().backward()
    return out.rgb_map.detach()


PERM_CASES = [("acc32", "f16s8"), ("acc32", "f16"), ("acc64", "f16s8"), ("acc64", "f16"), ("acc64", "bf16"), ("acc50", "f16s8"), ("acc300", "f16s8"), ("acc300", "f16"),
              ("dense_shared_z", "f16s8"), ("dense_per_ray_z", "f16s8"), ("dense_per_ray_z", "f16"), ("pose", "f16s8"),
              ("fused64", "f16s8"), ("fused64", "f16"), ("fused64", "bf16"), ("split300", "f16s8"), ("hierarchical", "f16s8"),
              ("barf_autograd", "f16s8"), ("barf_fused", "f16s8")]


PERM_PARAMS = [c + (4, 128) for c in PERM_CASES] + [c + (8, 256) for c in PERM_CASES if c[0] in ("acc32", "acc64", "fused64", "split300", "barf_fused")]


@pytest.mark.parametrize("case,prec,layers,width", PERM_PARAMS)
def test_ray_permutation_invariance(case, prec, layers, width):
    """Rays in their order and under a permutation (targets, depth rows, uniforms and ray ids permuted with them): pixels bit-identical once
    un-permuted, every gradient within fp32 re-association.  Permuting moves each 32-sample group to another stage partner, tile and chunk
    position - the change that exposed a block-scale mix-up in k_wgrad_s8 once."""
    from nerf_for_angiography_amd.render import render_projection, train_step_mse, hierarchical_train_step_mse
    from nerf_for_angiography_amd.engine import RenderSpec
    from nerf_for_angiography_amd.phantomdata.helpers import get_ray_values
    enc = "barf" if case.startswith("barf") else "none"
    m = _model(layers, width, prec, enc, bias=-25.0 if case.startswith("dense") or case == "hierarchical" else -5.0)
    o, d, tgt = _rays()
    z1 = torch.linspace(NEAR, FAR, 75, device=DEV)
    z2 = (z1[None, :] + torch.rand(R, 75, device=DEV, generator=torch.Generator(DEV).manual_seed(2)) * 2.0).sort(dim=-1).values.contiguous()
    u = torch.rand(R, 64, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    w = 40
    _, _, m44, _, _ = get_ray_values(33.0, 5.0, 0.0, np.array([0, 0, 1500.0]), w, w, 13.0 * w, DEV)
    poses = torch.from_numpy(m44[None]).to(DEV)
    ids0 = torch.randperm(w * w, generator=torch.Generator().manual_seed(4))[:R].to(DEV, torch.int32)

    def run(p):
        oo, dd, tt = o[p].contiguous(), d[p].contiguous(), tgt[p].contiguous()
        ww = 2.0 * (torch.rand(R, device=DEV, generator=torch.Generator(DEV).manual_seed(6)) - 0.5)[p].contiguous()
        if case.startswith("acc") or case == "barf_autograd":
            s = 64 if case in ("acc64", "barf_autograd") else int(case[3:])
            pix = _autograd(m, oo, dd, s, ww)
        elif case == "dense_shared_z":
            pix = _autograd(m, oo, dd, 0, ww, mode="dense", z=z1)
        elif case == "dense_per_ray_z":
            pix = _autograd(m, oo, dd, 0, ww, mode="dense", z=z2[p].contiguous())
        elif case == "pose":
            out = render_projection(m, poses, w, w, 13.0 * w, 64, NEAR, FAR, ray_ids=ids0[p].contiguous())
            (out.rgb_map * ww).sum().backward()
            pix = out.rgb_map.detach()
        elif case in ("fused64", "split300", "barf_fused"):
            s = 300 if case == "split300" else 64
            _, pix = train_step_mse(m, RenderSpec(n_rays=R, n_samples=s, origins=oo, dirs=dd, mode="acc", t_near=NEAR, t_far=FAR), tt)
        else:
            zc = torch.linspace(NEAR, FAR, 128, device=DEV)
            _, pix, _ = hierarchical_train_step_mse(m, oo, dd, zc, 64, tt, u=u[p].contiguous())
        torch.cuda.synchronize()
        return pix, _grads(m)

    ident = torch.arange(R, device=DEV)
    pix0, g0 = run(ident)
    pi = _perm(R)
    pix1, g1 = run(pi)
    assert float(g0.abs().max()) > 0
    assert torch.equal(pix1, pix0[pi]), int((pix1 != pix0[pi]).sum())
    err = rel_l2(g1.numpy(), g0.numpy())
    _report(f"permutation {case} {prec} {layers}x{width}", err)
    assert err <= BAR


@pytest.mark.parametrize("fn", ["packed", "march", "capturable", "single_eval"])
def test_grid_steps_ray_permutation_invariance(fn):
    """The grid family at f16s8 (packed step, one-call march step, capturable step, single-evaluation step): counters identical, pixels
    bit-identical once un-permuted, gradients within fp32 re-association."""
    from nerf_for_angiography_amd.render import train_step_packed_mse, march_train_step_mse
    from nerf_for_angiography_amd.nerf.occupancy import ray_marching
    from test_gpu_grid_graph import AABB, NEAR as GN, FAR as GF, SPR, EPS, THRE, _grid
    grid = _grid("sphere")
    o, d, tgt = _rays(1501, seed=17)
    m = _model(4, 128, "f16s8", bias=-3.0)

    def run(p):
        oo, dd, tt = o[p].contiguous(), d[p].contiguous(), tgt[p].contiguous()
        if fn == "packed":
            ri, _, _, packed = ray_marching(oo, dd, scene_aabb=torch.tensor(AABB), grid=grid, near_plane=GN, far_plane=GF,
                                            render_step_size=(GF - GN) / SPR, return_packed=True)
            _, pix = train_step_packed_mse(m, oo, dd, packed, tt)
            counts = (int(ri.numel()), int(packed.n_groups))
        elif fn == "march":
            _, pix, _ = march_train_step_mse(m, grid, AABB, oo, dd, SPR, GN, GF, EPS, THRE, tt)
            counts = m.engine.last_march_counts
        else:
            grad = torch.zeros(m.engine.param_count, device=DEV)
            call = m.engine.march_train_step_mse_capturable if fn == "capturable" else m.engine.march_train_step_mse_single_eval
            pix, c, _ = call(m._prepared(), oo, dd, tt, 1.0 / oo.shape[0], grad, "f16s8", AABB, GN, GF, (GF - GN) / SPR, EPS, THRE,
                             grid_bits=grid.bits, grid_aabb=grid._aabb_host, grid_res=grid._res_host)
            counts = tuple(c.tolist())
            torch.cuda.synchronize()
            return pix.clone(), grad.double().cpu(), counts
        torch.cuda.synchronize()
        return pix, _grads(m), counts

    pix0, g0, c0 = run(torch.arange(1501, device=DEV))
    pi = _perm(1501)
    pix1, g1, c1 = run(pi)
    assert c0 == c1 and c0[0] > 1000
    assert torch.equal(pix1, pix0[pi])
    err = rel_l2(g1.numpy(), g0.numpy())
    _report(f"permutation grid {fn}", err)
    assert err <= BAR


@pytest.mark.parametrize("prec", ["f16s8", "f16"])
@pytest.mark.parametrize("layers,width", [(4, 128), (8, 256)])
def test_exponent_spread_additivity(prec, layers, width):
    """d_pixel magnitudes 2^k over 30 binades, interleaved in ray order (adjacent groups of a stage carry different block scales); rays split
    into interleaved halves A and B with A 2^8 above B: grad(A u B) = grad(A) + grad(B), also under permutation.  A block-scale mix-up
    between the groups of a stage gets B's share wrong by factors of 2^8."""
    m = _model(layers, width, prec)
    o, d, _ = _rays()
    k = -(torch.arange(R, device=DEV) * 7 % 30).float()
    sgn = torch.where(torch.arange(R, device=DEV) % 3 == 0, -1.0, 1.0)
    a = (torch.arange(R, device=DEV) % 2 == 0)
    c = sgn * torch.exp2(k + 8.0 * a)

    def grad(w, p=None):      # 32 samples per ray: a 64-sample stage holds two rays, i.e. two different block scales
        if p is None:
            _autograd(m, o, d, 32, w)
        else:
            _autograd(m, o[p].contiguous(), d[p].contiguous(), 32, w[p].contiguous())
        return _grads(m)

    g_ab, g_a, g_b = grad(c), grad(c * a), grad(c * ~a)
    err = rel_l2(g_ab.numpy(), (g_a + g_b).numpy())
    pi = _perm(R)
    g_ab_p = grad(c, pi)
    err_p = rel_l2(g_ab_p.numpy(), (g_a + g_b).numpy())
    _report(f"additivity {prec} {layers}x{width}", err)
    _report(f"additivity under permutation {prec} {layers}x{width}", err_p)
    assert float(g_b.abs().max()) > 0
    assert err <= BAR and err_p <= BAR


@pytest.mark.parametrize("prec,s", [("f16s8", 64), ("f16", 64), ("f16s8", 300), ("bf16", 64)])
def test_power_of_two_homogeneity(prec, s):
    """The fused step with inv_n = 2^-k / n, k in {-40, -12, 12, 40}: pixels unchanged, gradients exactly 2^-k times those of k = 0 at f16s8 /
    f16 (their scales are normalised powers of two); bf16 (unnormalised bf16 dZ) the same - nothing rounds differently either."""
    from nerf_for_angiography_amd.engine import RenderSpec
    m = _model(4, 128, prec)
    o, d, tgt = _rays()
    spec = RenderSpec(n_rays=R, n_samples=s, origins=o, dirs=d, mode="acc", t_near=NEAR, t_far=FAR)
    res = {}
    for k in (0, -40, -12, 12, 40):
        grad = torch.zeros(m.engine.param_count, device=DEV)
        pix = m.engine.train_step_mse(m._prepared(), spec, tgt, float(np.ldexp(1.0 / R, -k)), grad, prec)
        torch.cuda.synchronize()
        res[k] = (pix.clone(), grad.double().cpu())
    worst = 0.0
    for k in (-40, -12, 12, 40):
        assert torch.equal(res[k][0], res[0][0]), k
        scaled = torch.ldexp(res[k][1], torch.tensor(float(k), dtype=torch.float64))
        worst = max(worst, rel_l2(scaled.numpy(), res[0][1].numpy()))
        assert torch.equal(scaled, res[0][1]), (k, int((scaled != res[0][1]).sum()))
    _report(f"homogeneity {prec} S={s}", worst)


@pytest.mark.parametrize("prec,s", [("f16s8", 64), ("f16s8", 300), ("f16", 64)])
def test_zero_and_subnormal_gradients(prec, s):
    """Rays whose d_pixel is exactly 0 (target = the pixel of the same step) or subnormal (1e-40, through autograd) contribute nothing
    measurable: the gradient is finite and equals the batch without them; with every ray at zero the gradient is exactly 0."""
    from nerf_for_angiography_amd.engine import RenderSpec
    from nerf_for_angiography_amd.render import train_step_mse
    m = _model(4, 128, prec)
    o, d, tgt = _rays()
    spec = lambda oo, dd: RenderSpec(n_rays=oo.shape[0], n_samples=s, origins=oo, dirs=dd, mode="acc", t_near=NEAR, t_far=FAR)
    _, pix = train_step_mse(m, spec(o, d), tgt)
    _grads(m)
    zero = (torch.arange(R, device=DEV) % 4 == 1)
    tz = torch.where(zero, pix, tgt)
    train_step_mse(m, spec(o, d), tz, n_global=R)
    g_mixed = _grads(m)
    keep = ~zero
    train_step_mse(m, spec(o[keep].contiguous(), d[keep].contiguous()), tgt[keep].contiguous(), n_global=R)
    g_keep = _grads(m)
    assert bool(torch.isfinite(g_mixed).all())
    err = rel_l2(g_mixed.numpy(), g_keep.numpy())
    train_step_mse(m, spec(o, d), pix)
    g_all = _grads(m)
    assert float(g_all.abs().max()) == 0.0
    # subnormal d_pixel through autograd
    w = torch.where(zero, torch.full_like(tgt, 1e-40), torch.where(torch.arange(R, device=DEV) % 4 == 2, 0.0, 1.0))
    _autograd(m, o, d, s, w)
    g_sub = _grads(m)
    sel = torch.arange(R, device=DEV) % 4 >= 3
    sel = sel | (torch.arange(R, device=DEV) % 4 == 0)
    _autograd(m, o[sel].contiguous(), d[sel].contiguous(), s, torch.ones(int(sel.sum()), device=DEV))
    g_sel = _grads(m)
    assert bool(torch.isfinite(g_sub).all())
    err_sub = rel_l2(g_sub.numpy(), g_sel.numpy())
    _report(f"zero rays {prec} S={s}", err)
    _report(f"subnormal rays {prec} S={s}", err_sub)
    assert err <= BAR and err_sub <= BAR


@pytest.mark.parametrize("prec,s", [("f16", 64), ("f16s8", 64), ("bf16", 64), ("f16s8", 300), ("f16", 300), ("bf16", 300)])
def test_backward_chunking_is_invisible_16bit(prec, s):
    """test_backward_chunking_is_invisible at the 16-bit precisions, the fused step (64 samples) and 300 samples per ray (f16s8: the split
    step; f16 / bf16: render + backward): a workspace that forces several chunks gives the one-chunk gradients."""
    from nerf_for_angiography_amd.engine import RenderSpec
    from nerf_for_angiography_amd.render import train_step_mse
    from nerf_for_angiography_amd import _lib
    m = _model(4, 128, prec)
    o, d, tgt = _rays(700, seed=5)
    spec = RenderSpec(n_rays=700, n_samples=s, origins=o, dirs=d, mode="acc", t_near=NEAR, t_far=FAR)

    def grads(ws_bytes):
        m.engine.max_workspace_bytes = ws_bytes
        m.engine._ws = None
        _, pix = train_step_mse(m, spec, tgt)
        torch.cuda.synchronize()
        return pix, _grads(m)

    pix_full, full = grads(8 << 30)
    q = lambda a0: int(m.engine.lib.afx_query(m.engine.h, _lib.Q_BWD_WORKSPACE_FULL, a0, s, _lib.PREC[prec]))
    small = q(1) + (q(700) - q(1)) // 4 + (2 << 20)      # a few chunks of whole rays (+ the step's per-ray head)
    pix_part, part = grads(small)
    assert torch.equal(pix_part, pix_full)
    err = rel_l2(part.numpy(), full.numpy())
    _report(f"chunking {prec} S={s}", err)
    assert err <= BAR
