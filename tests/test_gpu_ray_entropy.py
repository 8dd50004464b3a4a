"""The ray-entropy regulariser on the GPU (afx_ray_entropy_packed / _dense and their backward kernels, acc_ray_entropy, ray_entropy,
--entropy_weight) against the reference fixture g12 and the fp64 torch restatement of tests/ray_entropy_reference.py.

Tolerances (tests/ray_entropy_reference.py `bars`): the same torch expression on the CPU in fp32 and in fp64 on the test's inputs; the
bar for the kernel is 10 x that fp32-vs-fp64 relative L2, separately for value and gradient, floor 1e-6.  Every comparison first asserts,
on the fp64 side, that no ray lies within 1e-3 of the mask threshold.  Each test prints its measured errors next to the bars."""
import numpy as np
import pytest
import torch

import ray_entropy_reference as rer
from test_gpu_parity import DEV, make_model

pytestmark = pytest.mark.gpu


def _fixture(golden):
    g = golden("g12_ray_entropy")
    return g, torch.from_numpy(g["raw"]), torch.from_numpy(g["rgb_map"])


def _sample_mask(rgb64, ri=None, n_samples=None):
    m = (1.0 - rgb64) > 0.4
    return m[ri.long()] if ri is not None else m[:, None].expand(-1, n_samples).reshape(-1)


def test_dense_against_the_reference_fixture(golden):
    from nerf_for_angiography_amd.nerf.nerf_helpers import ray_entropy
    g, raw, rgb = _fixture(golden)
    assert rer.mask_margin(rgb) >= 1e-3
    sm = _sample_mask(rgb, n_samples=raw.shape[1])
    _, _, bar_e, bar_g = rer.bars(rer.entropy_dense, raw, rgb, sample_mask=sm.reshape(raw.shape))
    x = raw.to(DEV).requires_grad_(True)
    ent = ray_entropy(x, rgb.float().to(DEV))
    ent.sum().backward()
    err_e = rer.rel_l2(ent, torch.from_numpy(g["entropy"]))
    err_g = rer.rel_l2(x.grad.cpu().reshape(-1)[sm], torch.from_numpy(g["d_raw"]).reshape(-1)[sm])
    print(f"dense vs g12: value {err_e:.2e} (bar {bar_e:.2e}), gradient {err_g:.2e} (bar {bar_g:.2e})")
    off = torch.from_numpy(~((1.0 - g["rgb_map"]) > 0.4))
    assert bool((ent.cpu()[off] == 0).all()) and bool((x.grad.cpu()[off] == 0).all())      # masked rays: exactly 0, no gradient
    assert err_e < bar_e and err_g < bar_g
    # [R,S,1], the shape the model's output has, is the same call
    x3 = raw.to(DEV)[..., None].requires_grad_(True)
    ent3 = ray_entropy(x3, rgb.float().to(DEV))
    ent3.sum().backward()
    assert torch.equal(ent3, ent) and torch.equal(x3.grad[..., 0], x.grad)


def test_dense_forward_against_the_composite_kernel(golden):
    from nerf_for_angiography_amd.nerf.nerf_helpers import ray_entropy, render_volume_density
    g, raw, rgb64 = _fixture(golden)
    _, _, bar_e, _ = rer.bars(rer.entropy_dense, raw, rgb64)
    rgb, _, _, ent_old, _ = render_volume_density(raw.to(DEV)[..., None], torch.from_numpy(g["dirs"]).to(DEV), torch.from_numpy(g["z"]).to(DEV))
    ent_new = ray_entropy(raw.to(DEV), rgb)
    err = rer.rel_l2(ent_new, ent_old)
    print(f"dense vs k_composite_dense: value {err:.2e} (bar {bar_e:.2e}); rgb_map vs g12 {rer.rel_l2(rgb, rgb64):.2e}")
    assert torch.equal(ent_new != 0, ent_old != 0)      # identical masks
    assert torch.equal((ent_new != 0).cpu(), (1.0 - rgb64) > 0.4)
    assert err < bar_e


@pytest.mark.parametrize("seed", [0, 3, 4])
def test_packed_ragged(seed):
    from nerf_for_angiography_amd.nerf.nerf_helpers_acc import acc_ray_entropy, acc_render_volume_density
    n_rays = len(rer.RAGGED)
    pred, ri, ts, te = rer.ragged_problem(rer.RAGGED, seed)
    t64 = rer.transmittance(pred.double(), ri, ts, te, n_rays)
    assert rer.mask_margin(t64) >= 1e-3
    on = (1.0 - t64) > 0.4
    assert 0 < int(on.sum()) < n_rays - 2      # both mask states among the rays that have samples
    x = pred.to(DEV).requires_grad_(True)
    with torch.no_grad():
        rgb, _ = acc_render_volume_density(x, ri.to(DEV), ts.to(DEV), te.to(DEV), n_rays, 0)
    assert torch.equal(((1.0 - rgb) > 0.4).cpu(), on)
    sm = _sample_mask(t64, ri=ri)
    e64, g64, bar_e, bar_g = rer.bars(rer.entropy_packed, pred, rgb.cpu(), ri, n_rays, sample_mask=sm)
    ent = acc_ray_entropy(x, ri.to(DEV), rgb, n_rays)
    ent.sum().backward()
    err_e, err_g = rer.rel_l2(ent, e64), rer.rel_l2(x.grad.cpu()[sm], g64[sm])
    print(f"packed ragged seed {seed}: value {err_e:.2e} (bar {bar_e:.2e}), gradient {err_g:.2e} (bar {bar_g:.2e})")
    empty = torch.tensor([n == 0 for n in rer.RAGGED])
    assert bool((ent.cpu()[empty] == 0).all())      # zero-length rays: exactly 0
    assert bool((ent.cpu()[~on] == 0).all()) and bool((x.grad.cpu()[~sm] == 0).all())
    assert err_e < bar_e and err_g < bar_g
    # a weighted upstream gradient (d_entropy differs per ray), against the restatement's autograd
    w = torch.linspace(-1.0, 2.0, n_rays)
    x2 = pred.double().requires_grad_(True)
    (g64w,) = torch.autograd.grad((rer.entropy_packed(x2, rgb.cpu().double(), ri, n_rays) * w.double()).sum(), x2)
    x.grad = None
    (acc_ray_entropy(x, ri.to(DEV), rgb, n_rays) * w.to(DEV)).sum().backward()
    assert rer.rel_l2(x.grad.cpu()[sm], g64w[sm]) < bar_g


def test_combined_loss_through_the_module():
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd.nerf.nerf_helpers_acc import acc_ray_entropy, acc_render_volume_density
    problem = rer.module_problem(3)
    lengths, pts, ri, ts, te, target, params = problem
    n_rays = target.numel()
    g64, t64 = rer.module_grads_cpu(problem, 0.1, torch.float64)
    g32, _ = rer.module_grads_cpu(problem, 0.1, torch.float32)
    assert rer.mask_margin(t64) >= 1e-3
    bar = max(10.0 * rer.rel_l2(g32, g64), 1e-6)
    model = make_model(2, 64, precision="f32")
    model.load_state_dict(params, strict=False)
    names = sorted(params)
    named = dict(model.named_parameters())
    pts_d, ri_d, ts_d, te_d, tgt_d = pts.to(DEV), ri.to(DEV), ts.to(DEV), te.to(DEV), target.to(DEV)

    def grads(loss_fn):
        model.zero_grad()
        pred = model(pts_d)
        pred.retain_grad()
        loss_fn(pred).backward()
        return torch.cat([named[k].grad.reshape(-1) for k in names]).clone(), pred.grad.reshape(-1).clone(), pred.detach().reshape(-1)

    def module_loss(weight):
        def fn(pred):
            rgb, _ = acc_render_volume_density(pred, ri_d, ts_d, te_d, n_rays, 0)
            loss = torch.nn.functional.mse_loss(rgb, tgt_d)
            return loss if weight is None else loss + weight * acc_ray_entropy(pred, ri_d, rgb, n_rays).mean()
        return fn

    g_mod, dp_mod, pred = grads(module_loss(0.1))
    g_ops, dp_ops, _ = grads(lambda p: rer.combined_loss(p.reshape(-1), ri_d, ts_d, te_d, tgt_d, 0.1))
    rgb = engine.composite_packed(pred, ri_d, ts_d, te_d, n_rays)
    assert torch.equal(((1.0 - rgb) > 0.4).cpu(), (1.0 - t64) > 0.4)
    err, err_cpu = rer.rel_l2(g_mod, g_ops), rer.rel_l2(g_mod, g64)
    print(f"combined loss: parameter gradients module vs torch operators {err:.2e}, vs CPU fp64 {err_cpu:.2e} (bar {bar:.2e}); "
          f"d_pred {rer.rel_l2(dp_mod, dp_ops):.2e}")
    assert err < bar
    # the accumulate path: the entropy gradient added by the kernel onto the compositing gradient is the sum autograd formed
    d_rgb = (2.0 / n_rays) * (rgb - tgt_d)
    buf = engine.composite_packed_backward(pred, ri_d, ts_d, te_d, n_rays, rgb, d_rgb)
    _, sums = engine.ray_entropy_packed(pred, ri_d, rgb, n_rays)
    out = engine.ray_entropy_packed_backward(pred, ri_d, rgb, sums, torch.full((n_rays,), 0.1 / n_rays, device=DEV), out=buf)
    assert out is buf
    err_acc = rer.rel_l2(buf, dp_mod)
    print(f"accumulate path vs autograd's sum: {err_acc:.2e}")
    assert err_acc < 1e-6      # the same two fp32 terms, added once by the kernel and once by autograd (their seeds may differ in the last bit)
    # weight 0: bit-identical to the MSE-only backward
    g_zero, _, _ = grads(module_loss(0.0))
    g_mse, _, _ = grads(module_loss(None))
    assert torch.equal(g_zero, g_mse)
    assert not torch.equal(g_mod, g_mse)


def test_determinism_and_graph_capture():
    from nerf_for_angiography_amd import engine
    n_rays = len(rer.RAGGED)
    pred, ri, ts, te = rer.ragged_problem(rer.RAGGED, 0)
    pred, ri = pred.to(DEV), ri.to(DEV)
    rgb = engine.composite_packed(pred, ri, ts.to(DEV), te.to(DEV), n_rays)
    d_ent = torch.linspace(0.5, 1.5, n_rays, device=DEV)

    def run():
        ent, sums = engine.ray_entropy_packed(pred, ri, rgb, n_rays)
        return ent, sums, engine.ray_entropy_packed_backward(pred, ri, rgb, sums, d_ent)

    a, b = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    raw = pred[:640].reshape(20, 32).contiguous()
    rgb_d = torch.linspace(0.1, 0.9, 20, device=DEV)

    def run_dense():
        ent, sums = engine.ray_entropy_dense(raw, rgb_d)
        return ent, sums, engine.ray_entropy_dense_backward(raw, rgb_d, sums, d_ent.repeat(2)[:20].contiguous())

    c, d = run_dense(), run_dense()
    assert all(torch.equal(x, y) for x, y in zip(c, d))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = run() + run_dense()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(captured, a + c))


DRIVER = ["--synthetic", "--img_size", "16", "--num_layers", "4", "--num_hidden_units", "64", "--sample_size", "8", "--depth_samples", "32",
          "--march", "grid_ops", "--n_iters", "20", "--display_every", "10", "--out_bias_init", "0.0"]      # (sigma ~ 0.5: the rays absorb, the mask is on)
WALL_CLOCK = ("sec", "it_per_s")


def test_driver(tmp_path):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    plain = main(DRIVER + ["--log_dir", str(tmp_path / "a")])
    zero = main(DRIVER + ["--entropy_weight", "0", "--log_dir", str(tmp_path / "b")])
    on = main(DRIVER + ["--entropy_weight", "0.05", "--log_dir", str(tmp_path / "c")])
    strip = lambda h: [{k: v for k, v in rec.items() if k not in WALL_CLOCK} for rec in h]
    assert strip(zero["history"]) == strip(plain["history"]) and all("entropy" not in rec for rec in zero["history"])
    assert torch.equal(zero["model"].flat_params, plain["model"].flat_params)
    assert len(on["history"]) == 3
    for rec in on["history"]:
        assert np.isfinite(rec["entropy"]) and rec["entropy"] > 0 and np.isfinite(rec["train_loss"])
    assert not torch.equal(on["model"].flat_params, plain["model"].flat_params)      # the term reaches the parameters
