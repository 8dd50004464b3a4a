"""The occupancy-grid update on the device (afx_grid_points, afx_grid_update, afx_grid_binarize, afx_grid_pack, and afx_grid_refresh on top
of them) against the NumPy restatement of tests/grid_reference.py, whose problems' preconditions tests/test_grid_update_cpu.py asserts.
Every comparison is on the bits: floats as int32 views, masks and words as integers (run with -m gpu on an MI355X).

 a. points: every grid and both boxes, all cells and an index list with duplicates, supplied jitter (with rows of 0 and of 1 - 2^-24) and
    the Philox path every real refresh takes; a prefix of a longer Philox call equals the shorter call;
 b. update: the planted problems (cells drawn twice and three times, 0 / negative / -0.0 / NaN / +inf / denormal draws, a -0.0 cell, a denormal
    cell), all cells, the first n cells, the one-cell grid - each twice from the same start, and the snapshot left in the scratch buffer;
 c. binarize: exact problems with thousands of cells on the threshold, random ones, flat grids, the one-cell grid, on prefilled outputs;
 d. pack: bytes from {0, 1, 2, 255} into prefilled words; OccupancyGrid.set_binary on the ragged grids;
 e. the refresh at 37 x 29 x 23 against points -> the device's own MLP -> update -> binarize on the host;
 f. refusals before any launch."""
import numpy as np
import pytest
import torch

import grid_reference as gr
from test_gpu_parity import DEV
from test_grid_refresh_cpu import JITTER_TAG, SELECT_TAG, philox_u24, select_rule

pytestmark = pytest.mark.gpu

F32 = np.float32
BOX_IDS = ["box0", "box1"]
UPDATE_GRIDS = [r for r in gr.GRIDS if gr.num_cells(r) > 1]
BINARIZE_GRIDS = [r for r in gr.GRIDS if gr.num_cells(r) > 32]


def _eng():
    from nerf_for_angiography_amd import engine
    return engine


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cells_dev(cells):
    return None if cells is None else _dev(np.asarray(cells).astype(np.int32))


def _host_bits(t):
    assert t.dtype == torch.float32
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _assert_bits(got, want, what):
    g, w = _host_bits(got), gr.bits_of(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert bad.shape[0] == 0, (what, f"{bad.shape[0]} of {g.size} differ, first at {bad[0].tolist()}: "
                                     f"{got.detach().cpu().numpy()[tuple(bad[0])]!r} for {np.asarray(want)[tuple(bad[0])]!r}")


# --- a: points -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("box", gr.BOXES, ids=BOX_IDS)
@pytest.mark.parametrize("res", gr.GRIDS, ids=str)
def test_points_with_supplied_jitter(res, box):
    n = gr.num_cells(res)
    jit = gr.jitter_problem(n, 1)
    pts = _eng().grid_points(box, res, None, n, jitter=_dev(jit))
    _assert_bits(pts, gr.points(np.arange(n), jit, box, res), "all cells")
    cells = gr.index_list(res)
    jit = gr.jitter_problem(cells.size, 2)
    assert cells.size % 256 and np.unique(cells).size < cells.size
    pts = _eng().grid_points(box, res, _cells_dev(cells), cells.size, jitter=_dev(jit))
    _assert_bits(pts, gr.points(cells, jit, box, res), "index list")


@pytest.mark.parametrize("box", gr.BOXES, ids=BOX_IDS)
@pytest.mark.parametrize("res", gr.GRIDS, ids=str)
def test_points_on_the_philox_path(res, box):
    """jitter=None: u[i, a] is number 3 i + a of the stream (seed, AFX_GRID_JITTER_TAG | step), for the i-th DRAW (not the cell)."""
    eng, n, seed, stream = _eng(), gr.num_cells(res), 5, JITTER_TAG | 272
    pts = eng.grid_points(box, res, None, n, seed=seed, stream_id=stream, device=DEV)
    _assert_bits(pts, gr.points(np.arange(n), gr.philox_jitter(seed, stream, n), box, res), "all cells")
    m = (n + 1) // 2
    assert torch.equal(eng.grid_points(box, res, None, m, seed=seed, stream_id=stream, device=DEV).view(torch.int32), pts[:m].view(torch.int32))
    cells = gr.index_list(res)
    cd = _cells_dev(cells)
    pts = eng.grid_points(box, res, cd, cells.size, seed=seed, stream_id=stream)
    _assert_bits(pts, gr.points(cells, gr.philox_jitter(seed, stream, cells.size), box, res), "index list")
    m = cells.size * 2 // 3
    short = eng.grid_points(box, res, cd[:m].contiguous(), m, seed=seed, stream_id=stream)
    assert torch.equal(short.view(torch.int32), pts[:m].view(torch.int32))
    other = eng.grid_points(box, res, cd, cells.size, seed=seed, stream_id=JITTER_TAG | 288)
    assert not torch.equal(other, pts)


# --- b: update -------------------------------------------------------------------------------------------------------------------------------

def _update_twice(res, occs0, cells, occ_new, decay, what):
    """afx_grid_update twice from the same start: both runs equal the restatement (and so each other, whatever order the atomics took), and
    the scratch buffer holds the occupancies from before the call."""
    eng, n = _eng(), gr.num_cells(res)
    want = gr.update(occs0, cells, occ_new, decay)
    for run in range(2):
        occs, scratch = _dev(occs0), torch.full((n,), float("nan"), device=DEV)
        eng.grid_update(gr.BOXES[0], res, occs, _cells_dev(cells), _dev(occ_new), decay, scratch)
        _assert_bits(scratch, occs0, (what, "snapshot", run))
        _assert_bits(occs, want, (what, "occs", run))
    return want


@pytest.mark.parametrize("decay", gr.DECAYS)
@pytest.mark.parametrize("res", UPDATE_GRIDS, ids=str)
def test_update_planted_problems(res, decay):
    p = gr.update_problem(res)
    out = _update_twice(res, p.occs, p.cells, p.occ_new, decay, "planted")
    assert out[p.special["neg_zero_cell"]] == F32(0.25) and out[p.special["tiny_draw"]] == gr.TINY      # (what the restatement says of them)


@pytest.mark.parametrize("decay", gr.DECAYS)
@pytest.mark.parametrize("res", gr.GRIDS, ids=str)
def test_update_all_cells_and_first_cells(res, decay):
    n = gr.num_cells(res)
    occs0, v = gr.start_occs(n), gr.all_cells_draws(n)
    occs0[0], v[0] = -0.0, 0.5      # a cell at -0.0 must rise to its draw
    out = _update_twice(res, occs0, None, v, decay, "all cells")
    assert out[0] == F32(0.5)
    first = n // 2 + 1
    if first < n:
        out = _update_twice(res, occs0, None, v[:first], decay, "first cells")
        assert np.array_equal(gr.bits_of(out[first:]), gr.bits_of(occs0[first:]))


@pytest.mark.parametrize("decay,want", [(0.5, 0.7), (0.95, None)])
def test_update_one_cell_grid(decay, want):
    f = lambda *v: np.array(v, F32)
    out = _update_twice((1, 1, 1), f(0.8), np.array([0, 0, 0]), f(0.2, 0.7, 0.4), decay, "one cell, three draws")
    assert out[0] == (F32(want) if want else F32(F32(0.8) * F32(0.95)))
    out = _update_twice((1, 1, 1), f(gr.TINY), np.array([0, 0]), f(-0.0, np.nan), decay, "one denormal cell")
    assert 0 < out[0] < gr.TINY
    _update_twice((1, 1, 1), f(-0.0), np.array([0]), f(gr.TINY), decay, "one cell at -0.0")


# --- c: binarize -----------------------------------------------------------------------------------------------------------------------------

def _binarize(res, occs, occ_thre, what):
    """afx_grid_binarize on prefilled outputs (bits all ones, bytes 7, partial sums NaN) against the restatement."""
    n = gr.num_cells(res)
    b8 = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=DEV)
    part = torch.full((256,), float("nan"), dtype=torch.float64, device=DEV)
    _eng().grid_binarize(gr.BOXES[0], res, _dev(occs), occ_thre, b8, bits, part)
    got_b, got_w = b8.cpu().numpy(), bits.cpu().numpy().view(np.uint32)
    want_b, want_w = gr.binarize(occs, occ_thre)
    thr, mean = gr.threshold(occs, occ_thre)
    on_thr = occs == thr
    print(f"{what} {res} occ_thre {occ_thre}: thr {float(thr):.9g} (mean {float(mean):.9g}); device on / off / ties left off "
          f"{int((got_b == 1).sum())} / {int((got_b == 0).sum())} / {int((on_thr & (got_b == 0)).sum())}, restatement "
          f"{gr.decision_counts(occs, occ_thre)}")
    assert set(np.unique(got_b).tolist()) <= {0, 1}, (what, np.unique(got_b))
    assert np.array_equal(got_b, want_b), (what, "bytes", int((got_b != want_b).sum()))
    assert np.array_equal(got_w, want_w), (what, "words", int((got_w != want_w).sum()))
    assert n % 32 == 0 or int(got_w[-1]) >> (n % 32) == 0, (what, "spare bits", hex(int(got_w[-1])))
    return part.cpu().numpy()


@pytest.mark.parametrize("occ_thre", gr.EXACT_THRESHOLDS)
@pytest.mark.parametrize("res", BINARIZE_GRIDS, ids=str)
def test_binarize_exact_problems(res, occ_thre):
    occs, n = gr.exact_binarize_problem(res), gr.num_cells(res)
    part = _binarize(res, occs, occ_thre, "exact")
    assert not np.isnan(part).any() and float(part.sum()) == n / 4      # every partial sum written (the empty slices as 0), the total exact


@pytest.mark.parametrize("res", BINARIZE_GRIDS, ids=str)
def test_binarize_flat_grids(res):
    n = gr.num_cells(res)
    for occs in (np.zeros(n, F32), np.full(n, 0.3, F32)):      # the mean is the value itself: nothing lies above it
        _binarize(res, occs, 0.5, "flat")
        assert not gr.binarize(occs, 0.5)[0].any()


@pytest.mark.parametrize("res", BINARIZE_GRIDS, ids=str)
def test_binarize_random_problems(res):
    _binarize(res, gr.random_binarize_problem(res), gr.RANDOM_THRE, "random")


@pytest.mark.parametrize("occ_thre,on", [(0.25, 1), (0.75, 0)])
def test_binarize_one_cell_grid(occ_thre, on):
    """One cell at 0.5: above a threshold of 0.25; with 0.75 the mean 0.5 decides and the cell lies on it (off)."""
    _binarize((1, 1, 1), np.array([0.5], F32), occ_thre, "one cell")
    assert int(gr.binarize(np.array([0.5], F32), occ_thre)[1][0]) == on


# --- d: pack ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("res", gr.GRIDS, ids=str)
def test_pack(res):
    n = gr.num_cells(res)
    b = gr.pack_problem(res)
    bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=DEV)
    b8 = _dev(b)
    _eng().grid_pack(gr.BOXES[0], res, b8, bits)
    got = bits.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, gr.pack(b)), int((got != gr.pack(b)).sum())
    assert n % 32 == 0 or int(got[-1]) >> (n % 32) == 0
    assert np.array_equal(b8.cpu().numpy(), b)      # the bytes are read only


@pytest.mark.parametrize("res", gr.RAGGED, ids=str)
def test_set_binary_packs_a_ragged_grid(res):
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    grid = OccupancyGrid(roi_aabb=torch.tensor(gr.BOXES[0]), resolution=list(res)).to(DEV)
    grid._bits.fill_(-1)
    b = gr.pack_problem(res, seed=1)
    grid.set_binary(torch.from_numpy(b).view(*res))
    assert np.array_equal(grid._binary_u8.cpu().numpy(), (b != 0).astype(np.uint8))
    assert np.array_equal(grid.bits.cpu().numpy().view(np.uint32), gr.pack(b))
    assert np.array_equal(grid.binary.cpu().numpy().reshape(-1), b != 0)


# --- e: the refresh --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["f32", "f16s8"])
def test_refresh_equals_the_restatement(prec):
    """afx_grid_refresh at 37 x 29 x 23 (4 x 64 model, output bias -4): a warm-up refresh over all cells, one at step 272 from a dense mask
    and, on the same grid and workspace, one at 288 from a shell mask with n_occ < n, so that the device count lies below the capacity and
    the slots behind it still hold the draw of 272.  Expected: the cells of the draw rule, points on the Philox jitter, the device's own MLP
    on those points (not under test: it is the same on both sides), then update and binarize on the host."""
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    from test_gpu_grid_refresh import AABB, _mask, _model
    res, seed, occ_thre, decay = (37, 29, 23), 5, 5e-2, 0.95
    nc = gr.num_cells(res)
    n = nc // 4
    model = _model(4, 64, prec)
    grid = OccupancyGrid(roi_aabb=torch.tensor(AABB, device=DEV), resolution=list(res), seed=seed).to(DEV)
    occs = gr.random_binarize_problem(res, seed=3)
    grid.occs.copy_(_dev(occs))
    for step, kind in ((0, None), (272, "dense"), (288, "shell")):
        if kind is None:
            cells, count = None, nc
        else:
            mask = _mask(res, kind)
            grid._binary = mask.to(DEV)
            occupied = np.nonzero(mask.reshape(-1).numpy())[0]
            assert (occupied.size > n) == (kind == "dense") and occupied.size > 0
            cells = select_rule(philox_u24(seed, SELECT_TAG | step, 2 * n), occupied, nc, n).numpy()
            count = cells.size
            assert count == n + min(n, occupied.size) and (kind == "dense") == (count == 2 * n)
            if step == 272:
                assert np.bincount(cells, minlength=nc).max() > 1      # a cell drawn more than once
        pts = gr.points(np.arange(nc) if cells is None else cells, gr.philox_jitter(seed, JITTER_TAG | step, count), AABB, res)
        occ = model.engine.infer(model._prepared(), _dev(pts), model.precision, apply_sigmoid=True).reshape(-1).cpu().numpy()
        assert occ.dtype == np.float32 and occ.shape == (count,)
        occs = gr.update(occs, cells, occ, decay)
        margin, bound = gr.mean_margin(occs)
        assert margin > bound      # (the order of the device's fp64 sum cannot move the fp32 mean)
        want_b, want_w = gr.binarize(occs, occ_thre)
        grid.refresh(model, step, occ_thre=occ_thre, ema_decay=decay, all_cells=kind is None)
        _assert_bits(grid.occs, occs, (prec, step, "occs"))
        assert np.array_equal(grid._binary_u8.cpu().numpy(), want_b), (prec, step, "binary")
        assert np.array_equal(grid._bits.cpu().numpy().view(np.uint32), want_w), (prec, step, "bits")
        print(f"{prec} step {step}: {count} draws, on / off / ties {gr.decision_counts(occs, occ_thre)}, thr {gr.threshold(occs, occ_thre)}")
        assert 0 < int(want_b.sum()) < nc


# --- f: refusals -----------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    """A tensor of the wrong dtype, size, layout or device is a ValueError naming the argument, raised before the library is called: the
    sentinel-filled buffers are unchanged afterwards."""
    eng, box, res = _eng(), gr.BOXES[0], (5, 3, 7)
    n, words = 105, 4
    occs, scratch = torch.full((n,), 0.625, device=DEV), torch.full((n,), -3.0, device=DEV)
    b8, bits = torch.full((n,), 7, dtype=torch.uint8, device=DEV), torch.full((words,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    part = torch.full((256,), -1.0, dtype=torch.float64, device=DEV)
    cells, new = torch.arange(9, dtype=torch.int32, device=DEV), torch.full((9,), 0.9, device=DEV)
    jit = torch.full((9, 3), 0.5, device=DEV)
    keep = [t.clone() for t in (occs, scratch, b8, bits, part)]
    cases = [("cell_idx", lambda: eng.grid_update(box, res, occs, cells.long(), new, 0.95, scratch)),
             ("cell_idx", lambda: eng.grid_update(box, res, occs, cells[:8], new, 0.95, scratch)),
             ("cell_idx", lambda: eng.grid_update(box, res, occs, torch.arange(18, dtype=torch.int32, device=DEV)[::2], new, 0.95, scratch)),
             ("cell_idx", lambda: eng.grid_update(box, res, occs, cells.view(3, 3), new, 0.95, scratch)),
             ("cell_idx", lambda: eng.grid_update(box, res, occs, cells.cpu(), new, 0.95, scratch)),
             ("occs", lambda: eng.grid_update(box, res, occs.double(), cells, new, 0.95, scratch)),
             ("occs", lambda: eng.grid_update(box, res, occs[:-1], cells, new, 0.95, scratch)),
             ("scratch", lambda: eng.grid_update(box, res, occs, cells, new, 0.95, scratch[:-1])),
             ("scratch", lambda: eng.grid_update(box, res, occs, cells, new, 0.95, scratch.cpu())),
             ("occ_new", lambda: eng.grid_update(box, res, occs, None, torch.zeros(n + 1, device=DEV), 0.95, scratch)),
             ("occ_new", lambda: eng.grid_update(box, res, occs, cells, new.half(), 0.95, scratch)),
             ("bits", lambda: eng.grid_binarize(box, res, occs, 1e-2, b8, bits[:3], part)),
             ("bits", lambda: eng.grid_binarize(box, res, occs, 1e-2, b8, bits.long(), part)),
             ("binary_u8", lambda: eng.grid_binarize(box, res, occs, 1e-2, b8.bool(), bits, part)),
             ("binary_u8", lambda: eng.grid_binarize(box, res, occs, 1e-2, b8[:-1], bits, part)),
             ("occs", lambda: eng.grid_binarize(box, res, occs[:-1], 1e-2, b8, bits, part)),
             ("partial_ws", lambda: eng.grid_binarize(box, res, occs, 1e-2, b8, bits, part[:255])),
             ("partial_ws", lambda: eng.grid_binarize(box, res, occs, 1e-2, b8, bits, part.float())),
             ("partial_ws", lambda: eng.grid_binarize(box, res, occs, 1e-2, b8, bits, part.cpu())),
             ("bits", lambda: eng.grid_pack(box, res, b8, bits[:3])),
             ("bits", lambda: eng.grid_pack(box, res, b8, bits.long())),
             ("binary_u8", lambda: eng.grid_pack(box, res, b8[:-1], bits)),
             ("binary_u8", lambda: eng.grid_pack(box, res, b8.to(torch.int8), bits)),
             ("jitter", lambda: eng.grid_points(box, res, cells, 9, jitter=jit.reshape(-1))),
             ("jitter", lambda: eng.grid_points(box, res, cells, 9, jitter=jit[:8])),
             ("jitter", lambda: eng.grid_points(box, res, cells, 9, jitter=jit.double())),
             ("jitter", lambda: eng.grid_points(box, res, cells, 9, jitter=jit.cpu())),
             ("cell_idx", lambda: eng.grid_points(box, res, cells.long(), 9)),
             ("cell_idx", lambda: eng.grid_points(box, res, cells, 10)),
             ("cell_idx", lambda: eng.grid_points(box, res, cells.view(3, 3), 9))]
    for name, call in cases:
        with pytest.raises(ValueError, match=name):
            call()
    torch.cuda.synchronize()
    for t, k in zip((occs, scratch, b8, bits, part), keep):
        assert torch.equal(t, k)
    # the conforming calls go through
    eng.grid_update(box, res, occs, cells, new, 0.95, scratch)
    eng.grid_binarize(box, res, occs, 1e-2, b8, bits, part)
    eng.grid_pack(box, res, b8, bits)
    assert tuple(eng.grid_points(box, res, cells, 9, jitter=jit).shape) == (9, 3)
    assert float(occs[0]) == float(F32(0.9)) and float(occs[9]) == 0.625 and int(b8.sum()) == n
