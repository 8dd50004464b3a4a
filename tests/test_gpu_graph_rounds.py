"""Whole grid-training rounds from one graph (afx_sample_batches_dev, afx_train_round_advance, render.GridTrainRoundGraph, the driver's
--graph-rounds) against the per-iteration loop they replace - RayBatchSampler.draw, GridUpdateGraph.step, GridTrainGraph.step, the lr fill_.
Same kernels, same order, same inputs: every comparison in this file is bit for bit (run with -m gpu on an MI355X)."""
import json

import pytest
import torch

from test_gpu_parity import DEV, make_model
from test_gpu_grid_graph import _rays

pytestmark = pytest.mark.gpu

AABB = [-100.0, -100, -100, 100, 100, 100]
NEAR, FAR, SPR, EPS = 1400.0, 1600.0, 100, 1e-2
THRE, VESSEL_THRE = 1e-4, 5e-2      # the driver's thresholds: the marched grid's and the second grid's
K, SEED = 256, 11                   # rays per batch, sampler seed
LR0, DECAY, DECAY_STEPS = 1e-3, 0.1, 100.0      # a schedule that moves the float32 learning rate on every iteration


def _lr(i):
    return LR0 * (DECAY ** (i / DECAY_STEPS))      # the driver's expression (nerf/run_nerf_acc.py)


def _table(n=6000, seed=21, miss=False):
    o, d, p = _rays(n, seed)
    if miss:      # every ray passes the scene box at x = 1000
        o = o + torch.tensor([1000.0, 0, 0], device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.rand(n, device=DEV, generator=g) + 0.05
    w[::7] = 0.0      # rays that are never drawn (keys of -inf)
    return o.contiguous(), d.contiguous(), p.contiguous(), w


def _sample_batches_host_id(w, seed, sid, B, k):
    from nerf_for_angiography_amd import _lib
    lib = _lib.load()
    out = torch.empty(B, k, dtype=torch.int64, device=DEV)
    ws = torch.empty(int(lib.afx_sample_batches_workspace_bytes(w.numel(), B)), dtype=torch.uint8, device=DEV)
    _lib.check(lib.afx_sample_batches(w.data_ptr(), w.numel(), seed, sid, B, k, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream), "afx_sample_batches")
    return out


COUNTERS = [0, 7, 4096, 1 << 31]


@pytest.mark.parametrize("n_batches", [1, 16])
def test_device_draw_equals_the_host_id_draw(n_batches):
    """afx_sample_batches_dev == afx_sample_batches with the same id, index for index: eagerly, and from ONE captured graph replayed after
    step_dev.fill_() with each value (a capture that baked the value in shows here)."""
    from nerf_for_angiography_amd import engine
    w = _table(20000)[3]
    want = {v: _sample_batches_host_id(w, SEED, v, n_batches, K) for v in COUNTERS}
    assert not torch.equal(want[0], want[7])
    step_dev = torch.zeros((), dtype=torch.int64, device=DEV)
    for v in COUNTERS:
        step_dev.fill_(v)
        got = engine.sample_batches_dev(w, SEED, step_dev, n_batches, K)
        assert torch.equal(got, want[v]), v
    if n_batches == 16:      # row b of a block is the single draw of id + b (what RayBatchSampler hands out)
        assert torch.equal(want[0][7], want[7][0])
        assert torch.equal(want[0][7], engine.sample_rays(*_table(20000), K, seed=SEED, stream_id=7)[3])
    out = torch.zeros(n_batches, K, dtype=torch.int64, device=DEV)
    ws = torch.empty(engine.sample_batches_workspace_bytes(w.numel(), n_batches), dtype=torch.uint8, device=DEV)
    step_dev.fill_(COUNTERS[-1])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            engine.sample_batches_dev(w, SEED, step_dev, n_batches, K, out_idx=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    for v in COUNTERS:
        step_dev.fill_(v)
        out.zero_()
        graph.replay()
        assert torch.equal(out, want[v]), v


def test_advance_kernel_on_its_own():
    """afx_train_round_advance against its specification, value for value: table clamp, history slot, last_loss under a skip, the totals."""
    from nerf_for_angiography_amd import engine
    L = 4
    i64 = dict(dtype=torch.int64, device=DEV)
    step = torch.tensor(6, **i64)
    tab = torch.tensor([0.5, 0.25, 0.125], device=DEV)
    lr, skip, loss = torch.zeros((), device=DEV), torch.zeros(1, device=DEV), torch.tensor(3.0, device=DEV)
    counts = torch.tensor([9, 5, 2], **i64)
    lh, ch, sh = torch.full((L,), -1.0, device=DEV), torch.full((L, 3), -1, **i64), torch.full((L,), -1.0, device=DEV)
    last, total = torch.tensor(7.5, device=DEV), torch.tensor(100, **i64)
    engine.train_round_advance(step, tab, lr, skip, loss, counts, lh, ch, sh, last, total)
    assert int(step) == 7 and float(lr) == 0.125 and float(last) == 3.0 and int(total) == 105      # (6 clamps to the table's last entry)
    assert lh.tolist() == [-1.0, -1.0, 3.0, -1.0] and sh.tolist() == [-1.0, -1.0, 0.0, -1.0]
    assert ch.tolist() == [[-1] * 3, [-1] * 3, [9, 5, 2], [-1] * 3]
    step.fill_(1)
    skip.fill_(1.0)
    loss.fill_(4.0)
    counts.zero_()
    engine.train_round_advance(step, tab, lr, skip, loss, counts, lh, ch, sh, last, total)
    assert int(step) == 2 and float(lr) == 0.25 and float(last) == 3.0 and int(total) == 105      # a skipped step keeps last_loss
    assert lh.tolist() == [-1.0, 4.0, 3.0, -1.0] and sh.tolist() == [-1.0, 1.0, 0.0, -1.0] and ch[1].tolist() == [0, 0, 0]


def _fresh(res, seeded):
    """(model, lr tensor, optimizer, two grids): identical for every call with the same arguments."""
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    torch.manual_seed(8)
    m = make_model(4, 64, precision="f16s8")
    with torch.no_grad():
        m.output_linear[0].bias.fill_(-3.0)
    lr = torch.tensor(LR0, device=DEV)
    opt = torch.optim.Adam(m.parameters(), lr=lr, fused=True, capturable=True)
    grids = [OccupancyGrid(roi_aabb=torch.tensor(AABB, device=DEV), resolution=res, seed=s).to(DEV) for s in (0, 1)]
    if seeded:      # grids that have history when the run starts late: occupancies and a sphere of occupied cells
        c = (torch.stack(torch.meshgrid(*[torch.arange(res)] * 3, indexing="ij"), -1).float() + 0.5) / res * 200 - 100
        for s, g in enumerate(grids):
            gen = torch.Generator(device=DEV).manual_seed(s)
            g.occs.copy_(torch.rand(g.num_cells, device=DEV, generator=gen) * 0.03)
            g._binary = (c.norm(dim=-1) < 60 + 10 * s).to(DEV)
    return m, lr, opt, grids


def _loop(table, start, n, single_eval, res, seeded):
    """The per-iteration sequence of the driver's --graph --graph-grid-update loop.  Returns the state and every iteration's (loss, counts, skip)."""
    from nerf_for_angiography_amd.engine import RayBatchSampler
    from nerf_for_angiography_amd.render import GridTrainGraph, GridUpdateGraph
    m, lr, opt, grids = _fresh(res, seeded)
    sampler = RayBatchSampler(*table, K, seed=SEED, prefetch=16)
    gtg = GridTrainGraph(m, opt, grids[0], AABB, K, SPR, NEAR, FAR, EPS, THRE, single_eval=single_eval)
    upd = GridUpdateGraph(m, [(grids[0], THRE), (grids[1], VESSEL_THRE)])
    if start:
        lr.fill_(_lr(start - 1))      # what iteration start - 1 left behind
    hist = []
    for i in range(start, start + n):
        o, d, p, _ = sampler.draw(i)
        upd.step(i)
        loss, _, counts = gtg.step(o, d, p)
        hist.append((loss.clone(), counts.clone(), gtg.skip.clone()))
        lr.fill_(_lr(i))
    torch.cuda.synchronize()
    return m, opt, grids, lr, hist


def _rounds(table, start, single_eval, res, seeded, **kw):
    from nerf_for_angiography_amd.render import GridTrainRoundGraph, lr_decay_table
    m, lr, opt, grids = _fresh(res, seeded)
    rg = GridTrainRoundGraph(m, opt, [(grids[0], THRE), (grids[1], VESSEL_THRE)], table, AABB, K, SPR, NEAR, FAR, EPS, THRE, seed=SEED,
                             lr_table=lr_decay_table(LR0, DECAY, DECAY_STEPS, 400), single_eval=single_eval, start_iter=start, **kw)
    return m, opt, grids, lr, rg


def _assert_same_state(a, b):
    (ma, oa, ga, lra), (mb, ob, gb, lrb) = a, b
    for pa, pb in zip(ma._hip_params(), mb._hip_params()):
        assert torch.equal(pa.detach(), pb.detach())
        sa, sb = oa.state[pa], ob.state[pb]
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(sa[key], sb[key]), key
    for x, y in zip(ga, gb):
        assert torch.equal(x.occs, y.occs) and torch.equal(x._binary_u8, y._binary_u8) and torch.equal(x._bits, y._bits)
    assert torch.equal(lra, lrb)


def _assert_history(rg, hist, first, last):
    """Iterations first..last (at most round_len of them) of the loop's history against the slots the replays wrote."""
    h = rg.history()
    assert last - first < rg.round_len
    for i in range(first, last + 1):
        loss, counts, skip = hist[i]
        slot = i % rg.round_len
        assert torch.equal(h["loss"][slot], loss), i
        assert torch.equal(h["counts"][slot], counts), i
        assert torch.equal(h["skip"][slot], skip[0]), i


@pytest.mark.parametrize("single_eval", [False, True])
@pytest.mark.parametrize("res", [32])
def test_warmup_rounds_equal_the_loop(single_eval, res):
    """Iterations 0..47 - three warm-up rounds, one graph launch each - against the loop: every iteration's loss, counts and skip flag, then
    parameters, Adam state, both grids and the learning rate."""
    table = _table()
    m, opt, grids, lr, hist = _loop(table, 0, 48, single_eval, res, False)
    m2, opt2, grids2, lr2, rg = _rounds(table, 0, single_eval, res, False)
    kept = 0
    for r in range(3):
        rg.run(16)
        torch.cuda.synchronize()
        _assert_history(rg, [None] * (16 * r) + hist[16 * r:16 * r + 16], 16 * r, 16 * r + 15)
        kept += sum(int(c[1]) for _, c, _ in hist[16 * r:16 * r + 16])
    assert set(rg._graphs) == {"warmup"} and rg.iter == 48 and int(rg.step_dev) == 48
    _assert_same_state((m, opt, grids, lr), (m2, opt2, grids2, lr2))
    assert int(rg.n_marched) == kept > 0
    last = [l for l, _, s in hist if float(s) == 0.0][-1]
    assert torch.equal(rg.last_loss, last)
    assert float(opt2.state[next(iter(m2._hip_params()))]["step"]) == sum(float(s) == 0.0 for _, _, s in hist) > 0
    assert len({float(l) for l, _, _ in hist}) > 40      # the run trains: the losses move


def test_late_start_crosses_the_warmup_and_ends_on_a_tail():
    """start_iter = 240 for 33 iterations in ONE run(): a warm-up round (240), a post-warm-up round (256: the device draw of cells) and a
    refresh + tail iteration (272), against the loop brought to step 240 the same way (same parameters, fresh Adam state, same grids, the
    learning rate iteration 239 leaves).  The history holds the last round_len iterations."""
    table = _table()
    m, opt, grids, lr, hist = _loop(table, 240, 33, False, 32, True)
    m2, opt2, grids2, lr2, rg = _rounds(table, 240, False, 32, True)
    assert float(lr2) == float(torch.tensor(_lr(239), dtype=torch.float32))
    rg.run(33)
    torch.cuda.synchronize()
    assert set(rg._graphs) == {"warmup", "round", "tail"} and rg.iter == 273 and int(rg.step_dev) == 273
    _assert_history(rg, {240 + j: h for j, h in enumerate(hist)}, 257, 272)
    _assert_same_state((m, opt, grids, lr), (m2, opt2, grids2, lr2))
    assert int(rg.n_marched) == sum(int(c[1]) for _, c, _ in hist) > 0


def test_tail_iterations_and_chunked_runs_equal_the_loop():
    """run() in uneven pieces from an odd start (5: tails to 15, a round at 16, refresh + tails from 32) gives the loop's state too."""
    table = _table()
    m, opt, grids, lr, hist = _loop(table, 5, 30, False, 32, True)
    m2, opt2, grids2, lr2, rg = _rounds(table, 5, False, 32, True)
    for n in (3, 0, 26, 1):
        rg.run(n)
    torch.cuda.synchronize()
    assert rg.iter == 35 and int(rg.step_dev) == 35
    _assert_history(rg, {5 + j: h for j, h in enumerate(hist)}, 19, 34)
    _assert_same_state((m, opt, grids, lr), (m2, opt2, grids2, lr2))


def test_empty_march_inside_a_round():
    """A ray table whose rays all miss the scene box: after run(16) the parameters and moments are unchanged, the counter is 16, every
    iteration was skipped, last_loss keeps its initial value and nothing was marched."""
    table = _table(miss=True)
    m, opt, grids, lr, rg = _rounds(table, 0, False, 32, False, last_loss=7.5)
    before = [p.detach().clone() for p in m._hip_params()]
    st_before = [{k: v.clone() for k, v in opt.state[p].items()} for p in m._hip_params()]
    rg.run(16)
    torch.cuda.synchronize()
    for p, b, sb in zip(m._hip_params(), before, st_before):
        assert torch.equal(p.detach(), b)
        for k, v in opt.state[p].items():
            assert torch.equal(v, sb[k]), k
    h = rg.history()
    assert int(h["step"]) == 16 and rg.iter == 16
    assert h["skip"].tolist() == [1.0] * 16
    assert h["counts"].tolist() == [[0, 0, 0]] * 16
    assert float(h["last_loss"]) == 7.5
    assert int(h["n_marched"]) == 0
    assert float(lr) == float(torch.tensor(_lr(15), dtype=torch.float32))      # the schedule advances all the same, as the loop's fill_ does
    for g in grids:      # the round refreshed both grids
        assert float(g.occs.max()) > 0


def test_no_host_wait_between_display_points():
    """Three rounds and a tail under torch.cuda.set_sync_debug_mode("error") once the graphs exist."""
    table = _table()
    m, opt, grids, lr, rg = _rounds(table, 240, False, 32, True)
    rg.run(33)      # captures all three graphs (a capture synchronises)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
        rg.run(15 + 32 + 1)      # tails to 287, rounds at 288 and 304, refresh + tail at 320
        h = rg.history()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert rg.iter == 321 and int(h["step"]) == 321
    assert torch.isfinite(h["loss"]).all()


def _records(path):
    with open(path) as f:
        return [json.loads(line) for line in f]


def test_driver_graph_rounds_logs_the_same_records(tmp_path):
    """--synthetic --march grid --graph --graph-grid-update --graph-rounds --n_iters 64 --display_every 32 leaves a train_log.jsonl whose
    records equal those of the same command without --graph-rounds, field for field (the wall-clock fields excepted)."""
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    base = ["--synthetic", "--march", "grid", "--graph", "--graph-grid-update", "--n_iters", "64", "--display_every", "32"]
    main(base + ["--log_dir", str(tmp_path / "loop")])
    r = main(base + ["--graph-rounds", "--log_dir", str(tmp_path / "rounds")])
    a, b = _records(tmp_path / "loop" / "train_log.jsonl"), _records(tmp_path / "rounds" / "train_log.jsonl")
    assert [x["iter"] for x in a] == [x["iter"] for x in b] == [0, 32, 64]
    wall_clock = {"sec", "it_per_s"}
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for key in x:
            if key not in wall_clock:
                assert x[key] == y[key] or (x[key] != x[key] and y[key] != y[key]), (x["iter"], key, x[key], y[key])      # (NaN == NaN)
        print({k: v for k, v in y.items() if k not in wall_clock})
    assert b[-1]["marched_samples_per_iter"] > 0 and b[-1]["train_loss"] == b[-1]["train_loss"]
    assert [h["iter"] for h in r["history"]] == [0, 32, 64]
