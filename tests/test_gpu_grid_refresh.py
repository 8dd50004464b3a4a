"""The occupancy-grid refresh on the device (afx_grid_select_cells, afx_grid_refresh, OccupancyGrid.refresh, render.GridUpdateGraph, the
driver's --graph-grid-update): the draw against its restatement, the refresh bit for bit against the composition of the existing entry points,
graph replays against eager refreshes, no host wait (run with -m gpu on an MI355X)."""
import numpy as np
import pytest
import torch

from test_gpu_parity import DEV, make_model
from test_grid_refresh_cpu import JITTER_TAG, SELECT_TAG, philox_u24, select_rule

pytestmark = pytest.mark.gpu

AABB = [-100.0, -100, -100, 100, 100, 100]


def _res3(res):
    return [res] * 3 if isinstance(res, int) else list(res)


def _mask(res, kind):
    r = _res3(res)
    c = torch.stack(torch.meshgrid(*[(torch.arange(n).float() + 0.5) / n * 2 - 1 for n in r], indexing="ij"), -1).norm(dim=-1)
    if kind == "empty":
        return torch.zeros(*r, dtype=torch.bool)
    if kind == "shell":        # n_occ < num_cells / 4
        return (c < 0.55) & (c > 0.45)
    return c < 1.2             # dense: n_occ > num_cells / 4


def _grid(res, kind, seed=0):
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    g = OccupancyGrid(roi_aabb=torch.tensor(AABB, device=DEV), resolution=res, seed=seed).to(DEV)
    g._binary = _mask(res, kind).to(DEV)
    return g


def _restated(grid, step, n):
    u = _engine().philox_uniform(grid.seed, SELECT_TAG | step, 2 * n, DEV)
    u24 = (u.double() * (1 << 24)).long().cpu()
    occupied = torch.nonzero(grid._binary_u8.cpu())[:, 0]
    return select_rule(u24, occupied, grid.num_cells, n), u24


def _engine():
    from nerf_for_angiography_amd import engine
    return engine


@pytest.mark.parametrize("res", [64, 128, (37, 29, 23)])
@pytest.mark.parametrize("kind", ["empty", "shell", "dense"])
def test_selection_equals_its_restatement(res, kind):
    """cells_out[:count] and the device count are the restatement of the draw rule from engine.philox_uniform and torch.nonzero(binary),
    with the step given on the host and as a device tensor; the numpy Philox of the CPU tests is the library's generator."""
    eng = _engine()
    grid = _grid(res, kind, seed=5)
    n = grid.num_cells // 4
    for step, step_arg in ((256, 256), (4096, torch.tensor(4096, device=DEV))):
        cells, count = eng.grid_select_cells(grid._aabb_host, grid._res_host, grid.bits, n, grid.seed, step_arg)
        want, u24 = _restated(grid, step, n)
        assert int(count) == want.numel()
        n_occ = int(grid._binary_u8.sum())
        assert want.numel() == n + min(n, n_occ)
        assert (n_occ < n) == (kind == "shell") or kind == "empty"
        assert torch.equal(cells[:int(count)].long().cpu(), want)
        assert np.array_equal(u24[:4096].numpy(), philox_u24(grid.seed, SELECT_TAG | step, min(4096, 2 * n)))


def _eager_refresh(grid, model, step, all_cells, occ_thre, ema_decay=0.95):
    """The refresh composed from the existing entry points on the cells the draw selects."""
    eng = _engine()
    if all_cells:
        cells, n = None, grid.num_cells
    else:
        cells, count = eng.grid_select_cells(grid._aabb_host, grid._res_host, grid.bits, grid.num_cells // 4, grid.seed, step)
        n = int(count)
        cells = cells[:n].contiguous()
    x = eng.grid_points(grid._aabb_host, grid._res_host, cells, n, seed=grid.seed, stream_id=JITTER_TAG | step, device=grid.occs.device)
    occ = model.engine.infer(model._prepared(), x, model.precision, apply_sigmoid=True)
    eng.grid_update(grid._aabb_host, grid._res_host, grid.occs, cells, occ, ema_decay, grid._scratch)
    eng.grid_binarize(grid._aabb_host, grid._res_host, grid.occs, occ_thre, grid._binary_u8, grid._bits, grid._partial)


def _twin(grid):
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    t = OccupancyGrid(roi_aabb=torch.tensor(AABB, device=DEV), resolution=grid._res_host, seed=grid.seed).to(DEV)
    t.occs.copy_(grid.occs)
    t._binary_u8.copy_(grid._binary_u8)
    t._bits.copy_(grid._bits)
    return t


def _assert_same(a, b):
    assert torch.equal(a.occs, b.occs)
    assert torch.equal(a._binary_u8, b._binary_u8)
    assert torch.equal(a._bits, b._bits)


def _model(layers, width, prec, seed=3):
    torch.manual_seed(seed)
    m = make_model(layers, width, precision=prec)
    with torch.no_grad():
        m.output_linear[0].bias.fill_(-4.0)
    return m


@pytest.mark.parametrize("prec", ["f16s8", "f32"])
@pytest.mark.parametrize("layers,width", [(4, 128), (8, 256)])
@pytest.mark.parametrize("phase", ["warmup", "post", "post_dev_step"])
def test_refresh_equals_the_eager_composition(prec, layers, width, phase):
    """occs, binary and bits after afx_grid_refresh equal grid_points -> infer(apply_sigmoid) -> grid_update -> grid_binarize on the same
    cells, bit for bit; with occupancies already in the grid so that the EMA and the threshold both act."""
    m = _model(layers, width, prec)
    grid = _grid(64, "dense", seed=2)
    with torch.no_grad():
        g = torch.Generator(device=DEV).manual_seed(1)
        grid.occs.copy_(torch.rand(grid.num_cells, device=DEV, generator=g) * 0.03)
    _engine().grid_binarize(grid._aabb_host, grid._res_host, grid.occs, 1e-2, grid._binary_u8, grid._bits, grid._partial)
    for step in (0, 256, 272) if phase == "warmup" else (256, 272, 288):
        all_cells = phase == "warmup" and step < 256
        twin = _twin(grid)
        step_arg = torch.tensor(step, device=DEV) if phase == "post_dev_step" else step
        grid.refresh(m, step_arg, occ_thre=5e-2, all_cells=all_cells if phase == "post_dev_step" else None)
        _eager_refresh(twin, m, step, all_cells, 5e-2)
        _assert_same(grid, twin)
    n_occ = int(grid._binary_u8.sum())
    assert 0 < n_occ < grid.num_cells      # (threshold = the mean occupancy: neither empty nor full)


def test_graph_replays_track_step_weights_and_counts():
    """One GridUpdateGraph captured once, replayed at 256, 272, 288, ... with an optimizer step (and an in-place write) on the model between
    replays and the grid going from full to sparse: every replay equals the eager refresh at that step from the same grid state.  Catches a
    frozen step, stale weights, and stale counts left by a larger earlier selection."""
    from nerf_for_angiography_amd.render import GridUpdateGraph
    m = _model(4, 128, "f16s8")
    opt = torch.optim.Adam(m.parameters(), lr=1e-2, fused=True)
    grid = _grid(64, "dense", seed=7)
    grid._binary = torch.ones(64, 64, 64, dtype=torch.bool, device=DEV)      # full
    upd = GridUpdateGraph(m, [(grid, 1e-2)])
    n = grid.num_cells // 4
    regimes = set()
    for it in range(256, 256 + 16 * 6 + 1):
        if it % 16 == 0:
            if it == 288:      # the grid turns sparse in place: the replay must draw from the new bitfield with a smaller count
                grid._binary = _mask(64, "shell").to(DEV)
            regimes.add(int(grid._binary_u8.sum()) > n)
            twin = _twin(grid)
            upd.step(it)      # (first: the eager refresh re-tiles the shared prepared buffer, which would hide a graph that does not)
            twin.refresh(m, it, occ_thre=1e-2)
            _assert_same(grid, twin)
        else:
            upd.step(it)      # (no refresh step: nothing happens)
        for p in m.parameters():
            p.grad = torch.randn_like(p) * 0.1
        opt.step()
        if it % 32 == 0:
            with torch.no_grad():
                m.output_linear[0].bias.add_(0.5)
    assert regimes == {True, False}
    assert len(upd._graphs) == 1


def test_no_host_wait_in_the_graph_loop():
    """32 post-warm-up driver-style iterations (GridUpdateGraph.step, GridTrainGraph.step, the lr fill_) under
    torch.cuda.set_sync_debug_mode("error"); the eager every_n_step - torch.nonzero and len() on its result - raises in the same mode."""
    from test_gpu_grid_graph import _rays
    from nerf_for_angiography_amd.render import GridTrainGraph, GridUpdateGraph
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    m = make_model(4, 128, precision="f16s8")
    with torch.no_grad():
        m.output_linear[0].bias.fill_(-3.0)
    lr = torch.tensor(1e-3, device=DEV)
    opt = torch.optim.Adam(m.parameters(), lr=lr, fused=True, capturable=True)
    grids = [OccupancyGrid(roi_aabb=torch.tensor(AABB, device=DEV), resolution=128, seed=s).to(DEV) for s in (0, 1)]
    for g in grids:
        g._binary = torch.ones(128, 128, 128, dtype=torch.bool, device=DEV)
    n_rays = 1024
    gtg = GridTrainGraph(m, opt, grids[0], AABB, n_rays, 300, 1400.0, 1600.0, 1e-2, 1e-4)
    upd = GridUpdateGraph(m, [(grids[0], 1e-4), (grids[1], 5e-2)])
    upd.step(0)
    upd.step(256)      # both graphs captured (a capture synchronises) before the mode is switched on
    o, d, t = _rays(4000, 3)
    batches = [(o[i * 97 % 2900:][:n_rays], d[i * 97 % 2900:][:n_rays], t[i * 97 % 2900:][:n_rays]) for i in range(32)]
    torch.cuda.synchronize()
    losses = []
    try:
        torch.cuda.set_sync_debug_mode("error")
        for k, it in enumerate(range(257, 289)):
            upd.step(it)
            loss, _, _ = gtg.step(*batches[k])
            losses.append(loss.clone())
            lr.fill_(1e-3 * 0.999 ** k)
        with pytest.raises(RuntimeError):
            grids[1].train()
            grids[1].every_n_step(288, lambda x: torch.sigmoid(m(x)))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(torch.stack(losses)).all()
    for g in grids:      # the replays refreshed both grids
        assert float(g.occs.max()) > 0


def test_driver_graph_grid_update(tmp_path):
    """--march grid --graph --graph-grid-update on the small synthetic configuration of the driver tests, past the warm-up (two post-warm-up
    refreshes at 272 and 288): finite losses, marched samples, and a final test PSNR within the spread that two seeds of the eager loop show
    of the --graph run (the refresh draws other cells than the eager torch draw: a different, equally valid random sequence)."""
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    base = ["--synthetic", "--img_size", "20", "--number_angles", "1", "--limited_size", "90", "--n_iters", "288", "--display_every", "96",
            "--sample_size", "16", "--depth_samples", "100", "--num_layers", "4", "--num_hidden_units", "64", "--sampling_strategy", "segmentation",
            "--march", "grid", "--precision", "f16s8"]
    h0 = main(base + ["--log_dir", str(tmp_path / "e0")])["history"]
    h1 = main(base + ["--seed", "1", "--log_dir", str(tmp_path / "e1")])["history"]
    hg = main(base + ["--graph", "--log_dir", str(tmp_path / "g")])["history"]
    r = main(base + ["--graph", "--graph-grid-update", "--log_dir", str(tmp_path / "gu")])
    hu = r["history"]
    assert [x["iter"] for x in hu] == [0, 96, 192, 288]
    for x in hu:
        assert np.isfinite(x["train_loss"]) and x["marched_samples_per_iter"] > 0
    spread = abs(h0[-1]["test_psnr"] - h1[-1]["test_psnr"])
    gap = abs(hu[-1]["test_psnr"] - hg[-1]["test_psnr"])
    print(f"final test PSNR: eager seeds {h0[-1]['test_psnr']:.3f} / {h1[-1]['test_psnr']:.3f}, graph {hg[-1]['test_psnr']:.3f}, "
          f"graph + graph grid update {hu[-1]['test_psnr']:.3f}")
    assert gap <= 2.0 * spread + 0.5
    for g in (r["acc_grid"], r["vessel_acc_grid"]):      # both grids were refreshed
        assert float(g.occs.max()) > 0
