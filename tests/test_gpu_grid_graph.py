"""The graph-capturable grid training iteration (afx_march_train_step_mse_capturable, render.GridTrainGraph): device-resident sizes, no host
read-back.  Bit-for-bit against the one-call step, replays over stale buffer contents, the skipped empty step, graph training against eager
training (run with -m gpu on an MI355X)."""
import pytest
import torch

from test_gpu_parity import DEV, make_model
from test_gpu_round3 import _ref_iteration_problem

pytestmark = pytest.mark.gpu

AABB = [-100.0, -100, -100, 100, 100, 100]
RES = 64
NEAR, FAR, SPR, EPS, THRE = 1400.0, 1600.0, 300, 1e-2, 1e-4


def _mask(kind):
    c = (torch.stack(torch.meshgrid(*[torch.arange(RES)] * 3, indexing="ij"), -1).float() + 0.5) / RES * 200 - 100
    if kind == "full":
        return torch.ones(RES, RES, RES, dtype=torch.bool)
    if kind == "sphere":
        return c.norm(dim=-1) < 55
    if kind == "sparse":       # a thin shell: few kept samples, many rays without any
        return (c.norm(dim=-1) < 30) & (c.norm(dim=-1) > 26)
    return torch.zeros(RES, RES, RES, dtype=torch.bool)


def _grid(kind):
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    grid = OccupancyGrid(roi_aabb=torch.tensor(AABB, device=DEV), resolution=RES).to(DEV)
    grid._binary = _mask(kind).to(DEV)
    return grid


def _model(layers, width, enc, seed=8):
    torch.manual_seed(seed)
    m = make_model(layers, width, pos_enc=enc, precision="f16s8")
    if enc == "barf":
        m.update_barf_alpha(2.5, "pts")
    with torch.no_grad():
        m.output_linear[0].bias.fill_(-3.0)
    return m


def _capturable(m, grid, o, d, tgt, grad, **kw):
    return m.engine.march_train_step_mse_capturable(m._prepared(), o, d, tgt, 1.0 / o.shape[0], grad, "f16s8", AABB, NEAR, FAR,
                                                    (FAR - NEAR) / SPR, EPS, THRE, grid_bits=grid.bits, grid_aabb=grid._aabb_host,
                                                    grid_res=grid._res_host, **kw)


def _rays(n, seed):
    o, d, tgt = _ref_iteration_problem(n, seed=seed)
    return o.to(DEV), d.to(DEV), tgt.to(DEV)


@pytest.mark.parametrize("kind", ["sphere", "full"])
@pytest.mark.parametrize("layers,width,enc", [(4, 128, "none"), (8, 256, "none"), (4, 128, "barf")])
def test_capturable_call_equals_the_one_call_step(layers, width, enc, kind):
    """The capturable call issued eagerly gives the one-call step's pixels, gradients, loss and counters bit for bit."""
    from nerf_for_angiography_amd.render import march_train_step_mse
    o, d, tgt = _rays(1500, 17)
    grid = _grid(kind)
    m1 = _model(layers, width, enc)
    loss1, pix1, kept1 = march_train_step_mse(m1, grid, AABB, o, d, SPR, NEAR, FAR, EPS, THRE, tgt)
    g1 = torch.cat([p.grad.reshape(-1) for p in m1._hip_params()])
    counts1 = m1.engine.last_march_counts
    m2 = _model(layers, width, enc)
    grad2 = torch.zeros(m2.engine.param_count, device=DEV)
    pix2, counts2, skip2 = _capturable(m2, grid, o, d, tgt, grad2)
    loss2 = torch.nn.functional.mse_loss(pix2, tgt)
    assert kept1 > 1000
    assert tuple(counts2.tolist()) == counts1 and float(skip2) == 0.0
    assert torch.equal(pix1, pix2) and torch.equal(g1, grad2) and torch.equal(loss1, loss2)


def test_graph_replay_tracks_rays_and_grid_over_stale_buffers():
    """One capture, three replays with new rays and a grid changed in place (full -> sphere -> sparse shell): every replay equals a fresh eager
    call bit for bit.  The dense replay leaves valid-looking data beyond the later, smaller counts: a read past a device count shows here."""
    m = _model(4, 128, "none")
    grid = _grid("full")
    n = 1024
    o, d, tgt = _rays(n, 3)
    eng = m.engine
    grad_g = torch.zeros(eng.param_count, device=DEV)
    pix_g = torch.empty(n, device=DEV)
    counts_g = torch.empty(3, dtype=torch.int64, device=DEV)
    skip_g = torch.empty(1, device=DEV)
    so, sd, st = o.clone(), d.clone(), tgt.clone()
    _capturable(m, grid, so, sd, st, grad_g, pixel=pix_g, counts=counts_g, skip=skip_g)      # sizes the workspace
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            grad_g.zero_()
            _capturable(m, grid, so, sd, st, grad_g, pixel=pix_g, counts=counts_g, skip=skip_g)
    torch.cuda.current_stream().wait_stream(side)
    kept = []
    for i, kind in enumerate(["full", "sphere", "sparse"]):
        grid._binary = _mask(kind).to(DEV)         # in place: the captured march reads the bitfield by address
        o, d, tgt = _rays(n, 40 + i)
        so.copy_(o), sd.copy_(d), st.copy_(tgt)
        graph.replay()
        torch.cuda.synchronize()
        res_g = (pix_g.clone(), grad_g.clone(), counts_g.clone(), skip_g.clone())
        grad_e = torch.zeros(eng.param_count, device=DEV)
        pix_e, counts_e, skip_e = _capturable(m, grid, o, d, tgt, grad_e)
        assert torch.equal(res_g[2], counts_e) and torch.equal(res_g[3], skip_e), kind
        assert torch.equal(res_g[0], pix_e) and torch.equal(res_g[1], grad_e), kind
        kept.append(int(counts_e[1]))
    assert kept[0] > kept[1] > kept[2] > 0


def test_empty_grid_skips_the_whole_step():
    """Nothing survives the march: counts are zero, the skip flag is 1, pixel and gradient are untouched - and in a GridTrainGraph the fused
    Adam step is skipped: parameters, moments and `step` bit-identical."""
    from nerf_for_angiography_amd.render import GridTrainGraph
    m = _model(4, 128, "none")
    grid = _grid("empty")
    o, d, tgt = _rays(512, 5)
    grad = torch.full((m.engine.param_count,), 7.0, device=DEV)
    pixel = torch.full((512,), -3.0, device=DEV)
    _, counts, skip = _capturable(m, grid, o, d, tgt, grad, pixel=pixel)
    assert counts.tolist() == [0, 0, 0] and float(skip) == 1.0
    assert bool((grad == 7.0).all()) and bool((pixel == -3.0).all())
    grid._binary = _mask("sphere").to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, fused=True, capturable=True)
    gtg = GridTrainGraph(m, opt, grid, AABB, 512, SPR, NEAR, FAR, EPS, THRE)
    gtg.step(o, d, tgt)                 # one real step: moments and step non-trivial
    torch.cuda.synchronize()
    assert float(gtg.skip) == 0.0 and int(gtg.counts[1]) > 0
    grid._binary = _mask("empty").to(DEV)
    before = [p.detach().clone() for p in m._hip_params()]
    st_before = {id(p): {k: v.clone() for k, v in opt.state[p].items()} for p in m._hip_params()}
    pix_before = gtg.pixel.clone()
    o2, d2, t2 = _rays(512, 6)
    _, pix, counts = gtg.step(o2, d2, t2)
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0, 0] and float(gtg.skip) == 1.0 and torch.equal(pix, pix_before)
    for p, b in zip(m._hip_params(), before):
        assert torch.equal(p.detach(), b)
        for k, v in opt.state[p].items():
            assert torch.equal(v, st_before[id(p)][k]), k


def test_graph_training_equals_eager_training():
    """20 iterations of GridTrainGraph against 20 eager iterations of march_train_step_mse + the same fused, capturable Adam: identical loss
    history and final weights.  After the replays an eager render of the graph-trained module equals a fresh module loaded with its weights
    (the cached prepared weights do not go stale)."""
    from nerf_for_angiography_amd.render import GridTrainGraph, march_train_step_mse, render_rays
    n, iters = 1024, 20
    pool_o, pool_d, pool_t = _rays(4000, 21)
    g = torch.Generator().manual_seed(0)
    picks = [torch.randperm(4000, generator=g)[:n].to(DEV) for _ in range(iters)]
    grid = _grid("sphere")
    me = _model(4, 128, "none")
    opt_e = torch.optim.Adam(me.parameters(), lr=1e-3, fused=True, capturable=True)
    loss_e = []
    for idx in picks:
        opt_e.zero_grad()
        loss, _, kept = march_train_step_mse(me, grid, AABB, pool_o[idx], pool_d[idx], SPR, NEAR, FAR, EPS, THRE, pool_t[idx])
        assert kept > 0
        opt_e.step()
        loss_e.append(loss.item())
    mg = _model(4, 128, "none")
    opt_g = torch.optim.Adam(mg.parameters(), lr=1e-3, fused=True, capturable=True)
    gtg = GridTrainGraph(mg, opt_g, grid, AABB, n, SPR, NEAR, FAR, EPS, THRE)
    loss_g = []
    for idx in picks:
        loss, _, _ = gtg.step(pool_o[idx], pool_d[idx], pool_t[idx])
        loss_g.append(loss.clone())
    loss_g = [x.item() for x in loss_g]
    assert loss_g == loss_e
    for pe, pg in zip(me._hip_params(), mg._hip_params()):
        assert torch.equal(pe.detach(), pg.detach())
    fresh = _model(4, 128, "none")
    fresh.load_state_dict(mg.state_dict())
    with torch.no_grad():
        a = render_rays(mg, pool_o[:777], pool_d[:777], 128, NEAR, FAR).rgb_map
        b = render_rays(fresh, pool_o[:777], pool_d[:777], 128, NEAR, FAR).rgb_map
    assert torch.equal(a, b)


def test_driver_graph_mode_matches_the_eager_grid_loop(tmp_path):
    """nerf/run_nerf_acc.py --march grid --graph against --march grid on the small synthetic configuration of the driver tests: the logged
    losses agree and the march keeps the same samples."""
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    base = ["--synthetic", "--img_size", "20", "--number_angles", "1", "--limited_size", "90", "--n_iters", "96", "--display_every", "16",
            "--sample_size", "16", "--depth_samples", "100", "--num_layers", "4", "--num_hidden_units", "64", "--sampling_strategy", "segmentation",
            "--march", "grid", "--precision", "f16s8"]
    h_e = main(base + ["--log_dir", str(tmp_path / "eager")])["history"]
    h_g = main(base + ["--graph", "--log_dir", str(tmp_path / "graph")])["history"]
    assert [r["iter"] for r in h_g] == [r["iter"] for r in h_e] == list(range(0, 97, 16))
    for re_, rg in zip(h_e, h_g):
        assert rg["marched_samples_per_iter"] == re_["marched_samples_per_iter"] > 0
        assert abs(rg["train_loss"] - re_["train_loss"]) <= 1e-5 * abs(re_["train_loss"])
