"""The single-evaluation grid training iteration (afx_march_train_step_mse_single_eval, GridTrainGraph(single_eval=True), --single-eval): the
training step's forward half over the march's candidates doubles as the alpha pass.  Its raw output against afx_mlp_infer, the counters / pixels /
loss against the two-evaluation capturable step, the gradient against the exact-fp32 operator sequence with many dropped samples, graph replay
against eager calls, and the driver (run with -m gpu on an MI355X)."""
import pytest
import torch

from conftest import rel_l2
from test_gpu_parity import DEV, TOL
from test_gpu_grid_graph import AABB, NEAR, FAR, SPR, EPS, THRE, _capturable, _grid, _mask, _model, _rays

pytestmark = pytest.mark.gpu
SINGLE_EVAL_GRAD_TOL = 2e-2          # relative L2 of the gradient against the two-evaluation step (the sums run in another order)


def _single(m, grid, o, d, tgt, grad, **kw):
    return m.engine.march_train_step_mse_single_eval(m._prepared(), o, d, tgt, 1.0 / o.shape[0], grad, "f16s8", AABB, NEAR, FAR,
                                                     (FAR - NEAR) / SPR, EPS, THRE, grid_bits=grid.bits, grid_aabb=grid._aabb_host,
                                                     grid_res=grid._res_host, **kw)


def _rup(x):
    return (x + 255) // 256 * 256


def _workspace_views(eng, n_rays, max_steps):
    """The candidates' offsets, group offsets, t_starts / t_ends and the per-row raw output the forward half wrote, read from the workspace of
    the last call - the carving order of carve_single_eval (csrc/afx_api.hip)."""
    ws = eng._ws
    R, n, g = n_rays, max(n_rays * max_steps, 1), max(n_rays * ((max_steps + 31) // 32), 1)
    sizes = [("counts", R * 4), ("offsets", (R + 1) * 8), ("totals", 32), ("goff", (R + 1) * 8), ("counts2", R * 4), ("off2", (R + 1) * 8),
             ("goff2", (R + 1) * 8), ("dsz", 64), ("pix", R * 4), ("ri", n * 4), ("ts", n * 4), ("te", n * 4), ("keep", n),
             ("tsp", g * 128), ("tep", g * 128), ("gray", g * 4), ("raw", g * 128)]
    at, off = {}, 0
    for name, b in sizes:
        at[name] = (off, b)
        off += _rup(b)

    def view(name, dtype, count):
        o = at[name][0]
        return ws[o:o + count * torch.tensor([], dtype=dtype).element_size()].view(dtype)

    offsets = view("offsets", torch.int64, R + 1)
    n_c = int(offsets[-1])
    goff = view("goff", torch.int64, R + 1)
    return offsets, goff, view("ts", torch.float32, n_c), view("te", torch.float32, n_c), view("raw", torch.float32, g * 32)


def _max_steps(m, o, d):
    import ctypes as C
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.engine import _fill_march_args
    a = _lib.MarchArgs()
    _fill_march_args(a, o, d, AABB, NEAR, FAR, (FAR - NEAR) / SPR, None, None, None)
    return int(m.engine.lib.afx_march_max_steps(C.byref(a)))


@pytest.mark.parametrize("kind,n_rays", [("full", 1500), ("sphere", 5625), ("sparse", 5625)])
def test_forward_half_raw_equals_mlp_infer(kind, n_rays):
    """The raw output the forward half writes for each candidate is afx_mlp_infer's at the march's mid-points, bit for bit - so the kept set it
    decides is the alpha pass's."""
    m = _model(4, 128, "none")
    grid = _grid(kind)
    o, d, tgt = _rays(n_rays, 17)
    grad = torch.zeros(m.engine.param_count, device=DEV)
    _, counts, _ = _single(m, grid, o, d, tgt, grad)
    torch.cuda.synchronize()
    offsets, goff, ts, te, raw_rows = _workspace_views(m.engine, n_rays, _max_steps(m, o, d))
    n_c = ts.numel()
    assert n_c == int(counts[0]) > 0
    cnt = offsets[1:] - offsets[:-1]
    ri = torch.repeat_interleave(torch.arange(n_rays, device=DEV), cnt)
    rows = goff[:-1].repeat_interleave(cnt) * 32 + (torch.arange(n_c, device=DEV) - offsets[:-1].repeat_interleave(cnt))
    raw = raw_rows[rows]
    pts = o[ri] + (d[ri] * (ts + te)[:, None]) / 2.0      # k_march_write's mid-points
    ref = m.engine.infer(m._prepared(), pts, "f16s8", apply_sigmoid=False).reshape(-1)
    assert torch.equal(raw, ref), (raw != ref).sum().item()


@pytest.mark.parametrize("kind", ["full", "sphere", "sparse"])
@pytest.mark.parametrize("layers,width", [(4, 128), (8, 256)])
def test_single_eval_equals_the_two_evaluation_step(layers, width, kind):
    """Counters (candidates, kept, kept groups), pixels, loss and skip flag equal afx_march_train_step_mse_capturable's bit for bit; the
    gradients agree to the f16s8 tolerance (the sums run over the candidate rows in another order)."""
    o, d, tgt = _rays(1500 if kind == "full" else 5625, 17)
    grid = _grid(kind)
    m1 = _model(layers, width, "none")
    g1 = torch.zeros(m1.engine.param_count, device=DEV)
    pix1, counts1, skip1 = _capturable(m1, grid, o, d, tgt, g1)
    m2 = _model(layers, width, "none")
    g2 = torch.zeros(m2.engine.param_count, device=DEV)
    pix2, counts2, skip2 = _single(m2, grid, o, d, tgt, g2)
    torch.cuda.synchronize()
    assert counts1.tolist() == counts2.tolist() and int(counts2[1]) > 0, (counts1.tolist(), counts2.tolist())
    assert torch.equal(skip1, skip2) and float(skip2) == 0.0
    assert torch.equal(pix1, pix2)
    assert torch.equal(torch.nn.functional.mse_loss(pix1, tgt), torch.nn.functional.mse_loss(pix2, tgt))
    assert rel_l2(g2.cpu().numpy(), g1.cpu().numpy()) < SINGLE_EVAL_GRAD_TOL


def test_gradient_with_many_dropped_samples_vs_fp32_operator_sequence():
    """Early-stop-heavy: the output bias raised so that rays terminate after a few dozen samples - the candidates far outnumber the kept samples.
    The single-evaluation gradient (dropped rows contribute nothing) against get_predictions + acc_render_volume_density + mse_loss + backward at
    the exact-fp32 kernels on the kept samples."""
    from nerf_for_angiography_amd.render import march_train_step_mse
    from nerf_for_angiography_amd.nerf.nerf_helpers import get_predictions
    from nerf_for_angiography_amd.nerf.nerf_helpers_acc import acc_ray_marching, acc_render_volume_density
    n = 5625
    o, d, tgt = _rays(n, 23)
    grid = _grid("full")
    m = _model(4, 128, "none")
    with torch.no_grad():
        m.output_linear[0].bias.fill_(-1.0)
    m.zero_grad(set_to_none=True)
    loss, pix, n_kept = march_train_step_mse(m, grid, AABB, o, d, SPR, NEAR, FAR, EPS, THRE, tgt, single_eval=True)
    g8 = torch.cat([p.grad.reshape(-1) for p in m._hip_params()]).double()
    counts = m.engine.last_single_eval_counts
    assert n_kept == counts[1] >= 100000 and counts[0] >= 5 * counts[1], counts
    with torch.no_grad():
        ri, ts, te = acc_ray_marching(m, grid, torch.tensor(AABB, device=DEV), o, d, SPR, NEAR, FAR, EPS, THRE)
    assert ri.numel() == n_kept
    m.precision = "f32"
    m.zero_grad(set_to_none=True)
    pos = o[ri.long()] + d[ri.long()] * (ts + te) / 2.0
    pred, _ = acc_render_volume_density(get_predictions(m, pos, 131072), ri, ts, te, n, SPR)
    loss32 = torch.nn.functional.mse_loss(pred, tgt)
    loss32.backward()
    g32 = torch.cat([p.grad.reshape(-1) for p in m._hip_params()]).double()
    e = float((g8 - g32).norm() / g32.norm())
    assert e < TOL["f16s8"]["grad"], e
    assert rel_l2(pix.cpu().numpy(), pred.detach().cpu().numpy()) < 2e-3
    assert abs(float(loss) - float(loss32)) < 2e-3 * float(loss32)


def test_graph_replay_equals_eager_single_eval_calls():
    """A captured GridTrainGraph(single_eval=True) replayed over full -> sphere -> sparse grids and new rays equals eager single-evaluation
    iterations with the same fused Adam bit for bit: pixels, gradients, counters and the weights after each step.  An empty grid then sets the
    skip flag and Adam leaves the weights unchanged."""
    from nerf_for_angiography_amd.render import GridTrainGraph, march_train_step_mse
    n = 1024
    grid = _grid("full")
    mg, me = _model(4, 128, "none"), _model(4, 128, "none")
    opt_g = torch.optim.Adam(mg.parameters(), lr=1e-3, fused=True, capturable=True)
    opt_e = torch.optim.Adam(me.parameters(), lr=1e-3, fused=True, capturable=True)
    gtg = GridTrainGraph(mg, opt_g, grid, AABB, n, SPR, NEAR, FAR, EPS, THRE, single_eval=True)
    kept = []
    for i, kind in enumerate(["full", "sphere", "sparse"]):
        grid._binary = _mask(kind).to(DEV)      # in place: the captured march reads the bitfield by address
        o, d, tgt = _rays(n, 60 + i)
        opt_e.zero_grad()
        loss_e, pix_e, kept_e = march_train_step_mse(me, grid, AABB, o, d, SPR, NEAR, FAR, EPS, THRE, tgt, single_eval=True)
        grads_e = [p.grad.clone() for p in me._hip_params()]
        opt_e.step()
        loss_g, pix_g, counts_g = gtg.step(o, d, tgt)
        torch.cuda.synchronize()
        assert tuple(counts_g.tolist()) == me.engine.last_single_eval_counts and float(gtg.skip) == 0.0, kind
        assert torch.equal(pix_g, pix_e) and torch.equal(loss_g, loss_e), kind
        for pg, ge in zip(mg._hip_params(), grads_e):
            assert torch.equal(pg.grad, ge), kind
        for pg, pe in zip(mg._hip_params(), me._hip_params()):
            assert torch.equal(pg.detach(), pe.detach()), kind
        kept.append(kept_e)
    assert kept[0] > kept[1] > kept[2] > 0
    grid._binary = _mask("empty").to(DEV)
    before = [p.detach().clone() for p in mg._hip_params()]
    o, d, tgt = _rays(n, 70)
    _, _, counts = gtg.step(o, d, tgt)
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0, 0] and float(gtg.skip) == 1.0
    for p, b in zip(mg._hip_params(), before):
        assert torch.equal(p.detach(), b)


def test_driver_single_eval_modes_train(tmp_path):
    """--march grid --single-eval, eager and under --graph, on the small synthetic configuration of the driver tests: the loss falls, the test
    PSNR is finite and the final loss is within 30 % of --march grid."""
    import math
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    base = ["--synthetic", "--img_size", "20", "--number_angles", "1", "--limited_size", "90", "--n_iters", "96", "--display_every", "16",
            "--sample_size", "16", "--depth_samples", "100", "--num_layers", "4", "--num_hidden_units", "64", "--sampling_strategy", "segmentation",
            "--march", "grid", "--precision", "f16s8"]
    h_ref = main(base + ["--log_dir", str(tmp_path / "grid")])["history"]
    for extra in (["--single-eval"], ["--graph", "--single-eval"]):
        h = main(base + extra + ["--log_dir", str(tmp_path / "_".join(extra))])["history"]
        assert [r["iter"] for r in h] == list(range(0, 97, 16)), extra
        assert h[-1]["train_loss"] < h[0]["train_loss"], extra
        assert all(math.isfinite(r["test_psnr"]) for r in h), extra
        assert abs(h[-1]["train_loss"] - h_ref[-1]["train_loss"]) <= 0.3 * h_ref[-1]["train_loss"], (extra, h[-1], h_ref[-1])
