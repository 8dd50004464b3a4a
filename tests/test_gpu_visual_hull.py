"""The visual hull on the GPU (afx_visual_hull, afx_grid_apply_mask, OccupancyGrid.carve / carve_from_views, the driver's --grid_init hull,
sweep.reconstruction_hull_metrics): the votes equal the NumPy restatement exactly, a carved grid equals an uncarved one followed by the
mask, an uncarved grid is what it was (run with -m gpu on an MI355X)."""
import json

import numpy as np
import pytest
import torch

import hull_reference as hr
from test_gpu_parity import DEV, make_model
from test_visual_hull_cpu import EXCHANGE, SRC

pytestmark = pytest.mark.gpu

AABB = [-100.0, -100, -100, 100, 100, 100]
BOX = (2.0, 0.0, 0.0, -9.0, 0.0, 1.5, 0.0, 4.0, 0.0, 0.0, 0.5, -7.0)      # axis-aligned, three spacings
SHAPES = [(1, 1, 1), (3, 5, 70), (17, 16, 33)]      # 70 and 33: no multiple of the wavefront; 17 16 33 = 8976 points: 36 workgroups
DETECTORS = [(1, 1), (9, 13), (13, 9)]              # (W, H)
N_VIEWS = [1, 3, 65]


def _engine():
    from nerf_for_angiography_amd import engine
    return engine


def _views_for(x, n_views, width, height, case):
    """Poses and focal lengths laid out around the lattice x: one with its source inside the lattice (part of it has d <= rho), one so
    close that the lattice leaves the detector over all four edges, the rest far and oblique (source_matrix) with focal lengths that put
    part of the lattice off the detector; a single view takes each kind in turn."""
    from nerf_for_angiography_amd.phantomdata.proj_helpers import source_matrix
    rng = np.random.RandomState(100 + case)
    centre = 0.5 * (x.min(0) + x.max(0))
    s = max(float(0.5 * (x.max(0) - x.min(0)).max()), 1.0)
    big = float(max(width, height))
    poses, focal = [], []
    for v in range(n_views):
        theta, phi = rng.uniform(-180, 180), rng.uniform(-80, 80)
        kind = (v + case) % 3 if v < 3 else 2
        if kind == 0:
            poses.append(source_matrix(np.array([0.0, 0.0, 0.3 * s]), theta, phi, translation=centre))
            focal.append(0.8 * big)
        elif kind == 1:
            poses.append(source_matrix(np.array([0.0, 0.0, 3.0 * s]), theta, phi, translation=centre))
            focal.append(3.0 * big)
        else:
            poses.append(source_matrix(np.array([0.0, 0.0, 6.0 * s]), theta, phi, translation=centre))
            focal.append(rng.uniform(2.0, 5.0) * big)
    return np.stack(poses), np.asarray(focal)


def _masks(n_views, width, height, case):
    """A single pixel, a full image and a random 10 % (at least one pixel), in turn."""
    rng = np.random.RandomState(200 + case)
    masks = np.zeros((n_views, height, width), bool)
    for v in range(n_views):
        kind = (v + case) % 3
        if kind == 0:
            masks[v, rng.randint(height), rng.randint(width)] = True
        elif kind == 1:
            masks[v] = True
        else:
            masks[v] = rng.uniform(size=(height, width)) < 0.1
            masks[v, rng.randint(height), rng.randint(width)] = True
    return masks


CASES = [(shape, det, v) for shape in SHAPES for det in DETECTORS for v in N_VIEWS]


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"{s}-{d[0]}x{d[1]}-V{v}" for s, d, v in CASES])
def test_votes_equal_the_restatement(case):
    """seen and rejects equal tests/hull_reference.py exactly - and so does the stack of distance images they were taken from."""
    eng = _engine()
    shape, (width, height), n_views = CASES[case]
    a12 = EXCHANGE if case % 2 == 0 else BOX
    radius = (eng.hull_default_radius(a12), 0.0, 0.4)[case % 3]
    margin = (1.0, 0.0, 2.5)[(case // 3) % 3]
    x = hr.lattice_points(shape, a12)
    poses, focal = _views_for(x, n_views, width, height, case)
    masks = _masks(n_views, width, height, case)
    views = eng.visual_hull_views(poses, torch.from_numpy(masks).to(DEV), focal, margin_px=margin)
    dist = hr.distance_stack(masks)
    assert np.array_equal(views["dist"].cpu().numpy(), dist)
    seen, rejects = eng.visual_hull_record(views, shape, a12, radius)
    want_seen, want_rejects = hr.hull_counts(x, radius, poses, focal, width, height, margin, dist)
    assert seen.dtype == torch.uint16 and tuple(seen.shape) == shape
    assert np.array_equal(seen.cpu().numpy().reshape(-1), want_seen)
    assert np.array_equal(rejects.cpu().numpy().reshape(-1), want_rejects)
    hull = eng.visual_hull(views, shape, a12, radius, max_rejects=1, min_seen=2)
    assert np.array_equal(hull.cpu().numpy().reshape(-1), (want_rejects <= 1) & (want_seen >= 2))
    if shape == (17, 16, 33) and n_views >= 3 and width > 1:      # the cases are what they claim to be
        assert int((want_seen < n_views).sum()) > 0 and int(want_seen.max()) > 0
        assert int(want_rejects.min()) < int(want_rejects.max())
        for v in range(3):
            u, w, d = hr.project(x, poses[v], focal[v], width, height)
            kind = (v + case) % 3
            if kind == 0:
                assert ((d - radius) <= 0).any() and ((d - radius) > 0).any()
            if kind == 1:
                ok = d - radius > 0
                assert (u[ok] < 0).any() and (u[ok] > width - 1).any() and (w[ok] < 0).any() and (w[ok] > height - 1).any()


def test_repeatable_and_capturable():
    """A second launch and a replay from a captured graph give the same bytes; the replay follows the contents of the view buffers."""
    eng = _engine()
    shape, width, height = (17, 16, 33), 13, 9
    x = hr.lattice_points(shape, EXCHANGE)
    radius = eng.hull_default_radius(EXCHANGE)
    sets = []
    for case in (0, 1):
        poses, focal = _views_for(x, 65, width, height, case)
        sets.append(eng.visual_hull_views(poses, torch.from_numpy(_masks(65, width, height, case)).to(DEV), focal))
    eager = [eng.visual_hull_record(v, shape, EXCHANGE, radius) for v in sets]
    again = eng.visual_hull_record(sets[0], shape, EXCHANGE, radius)
    as_bytes = lambda t: t.view(torch.int16)
    assert torch.equal(as_bytes(eager[0][0]), as_bytes(again[0])) and torch.equal(as_bytes(eager[0][1]), as_bytes(again[1]))
    assert not torch.equal(as_bytes(eager[0][1]), as_bytes(eager[1][1]))
    static = dict(sets[0], records=sets[0]["records"].clone(), dist=sets[0]["dist"].clone())
    seen = torch.zeros(shape, dtype=torch.int16, device=DEV).view(torch.uint16)
    rejects = torch.zeros(shape, dtype=torch.int16, device=DEV).view(torch.uint16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            eng.visual_hull_record(static, shape, EXCHANGE, radius, seen=seen, rejects=rejects)
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 0):
        static["records"].copy_(sets[k]["records"])
        static["dist"].copy_(sets[k]["dist"])
        as_bytes(seen).fill_(7)
        as_bytes(rejects).fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(as_bytes(seen), as_bytes(eager[k][0])) and torch.equal(as_bytes(rejects), as_bytes(eager[k][1]))


def _raw_hull(n0, n1, n2, a12, radius, views, n_views, width, height, margin, dist, seen, rejects):
    """afx_visual_hull as C sees it -> (return code, afx_last_error)."""
    import ctypes as C
    from nerf_for_angiography_amd import _lib
    lib = _lib.load()
    a = None if a12 is None else (C.c_double * 12)(*[float(v) for v in np.asarray(a12, np.float64).reshape(-1)])
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = lib.afx_visual_hull(n0, n1, n2, a, radius, ptr(views), n_views, width, height, margin, ptr(dist), ptr(seen), ptr(rejects), None)
    return rc, (lib.afx_last_error() or b"").decode()


def test_entry_point_refuses_bad_arguments():
    """Null pointers, a view count outside 1..65535, a non-positive extent and 2^31 points are refused before any launch, by name."""
    rec = torch.zeros(1, 16, dtype=torch.float64, device=DEV)
    rec[0, [0, 4, 8]] = 1.0
    rec[0, 11], rec[0, 12] = 50.0, 10.0
    dist = torch.zeros(1, 4, 4, dtype=torch.float64, device=DEV)
    out = [torch.full((8,), 7, dtype=torch.int16, device=DEV) for _ in range(2)]
    good = dict(n0=2, n1=2, n2=2, a12=BOX, radius=1.0, views=rec, n_views=1, width=4, height=4, margin=1.0, dist=dist, seen=out[0], rejects=out[1])
    assert _raw_hull(**good)[0] == 0
    torch.cuda.synchronize()
    assert int(out[0].max()) <= 1 and int(out[1].max()) <= 1
    for change, word in ((dict(a12=None), "index_to_world"), (dict(views=None), "views"), (dict(dist=None), "dist"), (dict(seen=None), "seen"),
                         (dict(rejects=None), "rejects"), (dict(n_views=0), "n_views"), (dict(n_views=65536), "n_views"),
                         (dict(n1=0), "positive"), (dict(n2=-3), "positive"), (dict(width=0), "width"), (dict(height=0), "height"),
                         (dict(n0=2048, n1=2048, n2=512), "2^31"), (dict(radius=-1.0), "radius"), (dict(radius=float("nan")), "radius"),
                         (dict(margin=-0.5), "margin_px"), (dict(a12=(float("inf"),) + BOX[1:]), "finite")):
        rc, msg = _raw_hull(**dict(good, **change))
        assert rc != 0 and word in msg and msg.startswith("afx_visual_hull"), (change, rc, msg)
    eng = _engine()
    views = dict(records=rec, dist=dist, n_views=1, width=4, height=4, margin_px=1.0)
    with pytest.raises(ValueError, match="seen"):
        eng.visual_hull_record(views, (2, 2, 2), BOX, 1.0, seen=out[0][:4].view(torch.uint16))
    with pytest.raises(ValueError, match="12 numbers"):
        eng.visual_hull_record(views, (2, 2, 2), BOX[:9], 1.0)


# ---- afx_grid_apply_mask and OccupancyGrid.carve ----
def _pack(binary_u8):
    """The march's bitfield restated: bit b of word w = binary[32 w + b] != 0, as non-negative int64 words."""
    on = (binary_u8.cpu().reshape(-1) != 0).to(torch.int64)
    on = torch.cat([on, torch.zeros((-on.numel()) % 32, dtype=torch.int64)]).view(-1, 32)
    return (on << torch.arange(32)).sum(dim=1)


def _words(bits):
    return bits.cpu().to(torch.int64) & 0xFFFFFFFF


def _apply_mask_restated(mask_u8, occs, binary_u8):
    keep = mask_u8 != 0
    return torch.where(keep, occs, torch.zeros_like(occs)), torch.where(keep, binary_u8, torch.zeros_like(binary_u8))


@pytest.mark.parametrize("with_occs", [True, False])
def test_apply_mask_equals_the_torch_restatement(with_occs):
    """5 x 6 x 7 = 210 cells, no multiple of 32: occs, binary and the bitfield; the spare bits of the last word stay zero."""
    eng = _engine()
    res, n = [5, 6, 7], 210
    g = torch.Generator().manual_seed(11)
    occs = torch.rand(n, generator=g).to(DEV)
    binary = torch.tensor([0, 1, 3], dtype=torch.uint8)[torch.randint(3, (n,), generator=g)].to(DEV)
    mask = torch.tensor([0, 1, 5], dtype=torch.uint8)[torch.randint(3, (n,), generator=g)].to(DEV)
    bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=DEV)
    want_occs, want_binary = _apply_mask_restated(mask, occs, binary)
    occs_in = occs.clone()
    eng.grid_apply_mask(AABB, res, mask, occs if with_occs else None, binary, bits)
    assert torch.equal(binary, want_binary)
    assert torch.equal(occs, want_occs if with_occs else occs_in)
    assert torch.equal(_words(bits), _pack(want_binary))
    assert int(_words(bits)[-1]) >> (n % 32) == 0
    assert 0 < int((want_binary != 0).sum()) < int((binary != 0).sum() + (mask == 0).sum())
    with pytest.raises(ValueError, match="mask"):
        eng.grid_apply_mask(AABB, res, mask[:-1], None, binary, bits)


def _grid(res, seed=0):
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    return OccupancyGrid(roi_aabb=torch.tensor(AABB, device=DEV), resolution=res, seed=seed).to(DEV)


def _twin(grid):
    t = _grid(grid._res_host, grid.seed)
    t.occs.copy_(grid.occs)
    t._binary_u8.copy_(grid._binary_u8)
    t._bits.copy_(grid._bits)
    return t


def _assert_same(a, b):
    assert torch.equal(a.occs, b.occs)
    assert torch.equal(a._binary_u8, b._binary_u8)
    assert torch.equal(a._bits, b._bits)


def _model(bias, prec="f16s8", seed=3):
    torch.manual_seed(seed)
    m = make_model(4, 128, precision=prec)
    with torch.no_grad():
        m.output_linear[0].bias.fill_(bias)
    return m


def _random_mask(res, seed, share=0.4):
    r = [res] * 3 if isinstance(res, int) else list(res)
    return torch.rand(*r, generator=torch.Generator().manual_seed(seed)) < share


def test_carve_is_the_ceiling_of_every_update():
    """A model whose output bias makes every cell occupied: after a warm-up refresh (the device path) and after a warm-up every_n_step
    (the eager path) binary == mask exactly and occs is 0 outside the mask."""
    m = _model(4.0)
    res = (17, 16, 33)
    mask = _random_mask(res, 5)
    for path in ("refresh", "every_n_step"):
        grid = _grid(res, seed=2)
        grid.carve(mask)
        assert int(grid._binary_u8.sum()) == 0 and torch.equal(grid._carve_u8.cpu(), mask.reshape(-1).to(torch.uint8))
        if path == "refresh":
            grid.refresh(m, 0)
        else:
            grid.train()
            grid.every_n_step(0, lambda x: torch.sigmoid(m(x)))
        assert torch.equal(grid.binary.cpu(), mask), path
        assert float(grid.occs[~mask.reshape(-1).to(DEV)].abs().max()) == 0.0
        assert float(grid.occs[mask.reshape(-1).to(DEV)].min()) > 0.5
        assert torch.equal(_words(grid.bits), _pack(mask.reshape(-1).to(torch.uint8)))
        grid.carve(None)      # the mask is gone: the next update fills the grid again
        grid.refresh(m, 0)
        assert bool(grid.binary.all())


def test_masked_refresh_is_the_unmasked_refresh_then_the_mask():
    """On the same state, step and seed: refresh of the carved grid == refresh of an uncarved twin followed by the torch restatement of
    afx_grid_apply_mask, bit for bit, in the warm-up phase and after it."""
    eng = _engine()
    m = _model(-4.0)
    grid = _grid(64, seed=2)
    mask = _random_mask(64, 9, share=0.6)
    with torch.no_grad():
        grid.occs.copy_(torch.rand(grid.num_cells, generator=torch.Generator().manual_seed(1)).to(DEV) * 0.03)
    eng.grid_binarize(grid._aabb_host, grid._res_host, grid.occs, 1e-2, grid._binary_u8, grid._bits, grid._partial)
    grid.carve(mask)
    mask_u8 = mask.reshape(-1).to(torch.uint8).to(DEV)
    for step in (0, 256, 272):
        twin = _twin(grid)
        grid.refresh(m, step, occ_thre=5e-2)
        twin.refresh(m, step, occ_thre=5e-2)
        assert int((twin._binary_u8 != 0)[mask_u8 == 0].sum()) > 0      # (the mask has something to remove)
        occs, binary = _apply_mask_restated(mask_u8, twin.occs, twin._binary_u8)
        assert torch.equal(grid.occs, occs) and torch.equal(grid._binary_u8, binary)
        assert torch.equal(_words(grid.bits), _pack(binary))
    assert 0 < int(grid._binary_u8.sum()) < int(mask.sum())


def test_uncarved_grid_is_what_it_was():
    """The no-change guarantee: a grid that is not carved - never, or no longer - refreshes exactly as the composition of the entry
    points that made up a refresh before carving existed, and its training state carries no carve entry."""
    from test_gpu_grid_refresh import _eager_refresh
    m = _model(-4.0)
    fresh, was_carved, composed = _grid(64, seed=4), _grid(64, seed=4), _grid(64, seed=4)
    was_carved.carve(_random_mask(64, 13))
    was_carved.carve(None)
    assert fresh._carve_u8 is None and was_carved._carve_u8 is None
    assert "carve" not in fresh.training_state() and "carve" not in was_carved.training_state()
    for step, all_cells in ((0, True), (16, True), (256, False), (272, False)):
        fresh.refresh(m, step, occ_thre=5e-2)
        was_carved.refresh(m, step, occ_thre=5e-2)
        _eager_refresh(composed, m, step, all_cells, 5e-2)
        _assert_same(fresh, was_carved)
        _assert_same(fresh, composed)
    assert 0 < int(fresh._binary_u8.sum()) < fresh.num_cells


def test_update_graph_over_a_carved_grid():
    """GridUpdateGraph captured over a grid carved beforehand: two replays equal the eager carved refreshes from the same states."""
    from nerf_for_angiography_amd.render import GridUpdateGraph
    m = _model(-4.0)
    mask = _random_mask(64, 21, share=0.5)
    grid = _grid(64, seed=7)
    grid._binary = torch.ones(64, 64, 64, dtype=torch.bool, device=DEV)
    grid.carve(mask)
    upd = GridUpdateGraph(m, [(grid, 1e-2)])
    for it in (256, 272):
        twin = _twin(grid)
        twin.carve(mask)
        upd.step(it)
        twin.refresh(m, it, occ_thre=1e-2)
        _assert_same(grid, twin)
        assert int((grid._binary_u8 != 0)[mask.reshape(-1).to(DEV) == 0].sum()) == 0
    assert int(grid._binary_u8.sum()) > 0


def test_training_state_round_trips_the_mask():
    m = _model(4.0)
    mask = _random_mask(32, 31)
    grid = _grid(32, seed=1)
    grid.carve(mask)
    grid.refresh(m, 0)
    state = grid.training_state()
    assert torch.equal(state["carve"], mask.reshape(-1).to(torch.uint8))
    other = _grid(32, seed=1)
    other.load_training_state(state)
    _assert_same(grid, other)
    assert torch.equal(other._carve_u8, grid._carve_u8) and other._carve_u8.device == other.occs.device
    other.carve(None)
    other.refresh(m, 0)
    assert bool(other.binary.all())
    other.load_training_state(state)      # the restored mask acts again
    other.refresh(m, 16)
    assert torch.equal(other.binary.cpu(), mask)


def test_march_through_a_carved_grid_is_a_subset():
    """The carved march returns a subset of the uncarved march's samples: the same (ray, t_start) pairs, fewer of them."""
    from nerf_for_angiography_amd.nerf.occupancy import ray_marching
    full, carved = _grid(32), _grid(32)
    for g in (full, carved):
        g._binary = torch.ones(32, 32, 32, dtype=torch.bool, device=DEV)
    carved.carve(_random_mask(32, 41, share=0.3))
    gen = torch.Generator().manual_seed(2)
    o = (torch.tensor([0.0, 0.0, 300.0]) + torch.randn(257, 3, generator=gen) * 5).to(DEV)
    d = (torch.rand(257, 3, generator=gen) * 160 - 80).to(DEV) - o
    d = (d / d.norm(dim=-1, keepdim=True)).contiguous()
    box = torch.tensor(AABB, device=DEV)
    pairs = []
    for g in (full, carved):
        ri, ts, te = ray_marching(o, d, scene_aabb=box, grid=g, render_step_size=1.7)
        pairs.append(set(zip(ri.tolist(), ts[:, 0].tolist())))
        assert len(pairs[-1]) == ri.numel()
    assert pairs[1] < pairs[0] and 0.15 * len(pairs[0]) < len(pairs[1]) < 0.45 * len(pairs[0])


# ---- the hull of the synthetic dataset's training views ----
@pytest.fixture(scope="module")
def capsule_views():
    """9 training views of 32^2 of the synthetic capsule dataset (binary, 'segmentation'), masks pixel_value < 1; made once."""
    from nerf_for_angiography_amd.nerf.run_nerf_acc import training_view_masks
    from nerf_for_angiography_amd.phantomdata import dataset as ds
    proj_df, ray_df = ds.make_synthetic_dataset(ds.angle_grid(180, 2), img_size=32, sampling_strategy="segmentation", device=DEV, seed=0,
                                                binary=True)
    held_out = proj_df.index[-1]
    poses, masks, focal = training_view_masks(proj_df, ray_df[ray_df["image_id"] != held_out], held_out, 1.0, DEV)
    assert tuple(masks.shape) == (9, 32, 32) and bool(masks.reshape(9, -1).any(dim=1).all())
    for v in (0, 4, 8):      # the scatter by image_id / y_position / x_position puts every pixel where the image has it
        assert np.array_equal(masks[v].cpu().numpy(), np.asarray(proj_df["image_data"].iloc[v]) < np.asarray(proj_df["image_data"].iloc[v]).max())
    return dict(poses=poses, masks=masks, focal=focal, views=_engine().visual_hull_views(poses, masks, focal, margin_px=1.0))


def test_carve_from_views(capsule_views):
    """A 32^3 grid carved by the hull of the 9 training views at margin 1: the votes equal the restatement over the cell centres, the
    mask after a warm-up refresh with an all-occupying model is <= the hull, and every cell whose centre lies in the vessel and is seen
    by all views stays."""
    from nerf_for_angiography_amd.phantomdata.helpers import capsule_mu, capsule_tree
    eng = _engine()
    grid = _grid(32, seed=3)
    hull, seen, rejects = grid.carve_from_views(capsule_views["views"], return_counts=True)
    a12, rho = eng.grid_cell_lattice(grid._aabb_host, grid._res_host)
    x = hr.lattice_points((32,) * 3, a12)
    want_seen, want_rejects = hr.hull_counts(x, rho, capsule_views["poses"], capsule_views["focal"], 32, 32, 1.0,
                                             hr.distance_stack(capsule_views["masks"].cpu().numpy()))
    assert np.array_equal(seen.cpu().numpy().reshape(-1), want_seen) and np.array_equal(rejects.cpu().numpy().reshape(-1), want_rejects)
    assert np.array_equal(hull.cpu().numpy().reshape(-1), (want_rejects == 0) & (want_seen >= 1))
    grid.refresh(_model(4.0), 0)
    assert not bool((grid.binary & ~hull).any()) and torch.equal(grid.binary, hull)
    truth = capsule_mu(torch.from_numpy(x), capsule_tree(levels=5, seed=0)).numpy() > 0
    must_stay = truth & (want_seen == 9)
    share = float(hull.float().mean())
    print(f"hull share {share:.4f}, vessel cells seen by all views {int(must_stay.sum())}, of which outside the hull "
          f"{int((must_stay & ~hull.cpu().numpy().reshape(-1)).sum())}")
    assert must_stay.sum() >= 10
    assert not (must_stay & ~hull.cpu().numpy().reshape(-1)).any()
    assert 0.02 < share < 0.5


@pytest.mark.parametrize("flags", [[], ["--graph", "--graph-grid-update", "--graph-rounds"]], ids=["eager", "graph-rounds"])
def test_driver_trains_inside_the_hull(tmp_path, flags):
    """--grid_init hull for 48 iterations: a finite loss, both saved grid masks and both live grids <= the saved hull, the hull in the log."""
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    out = main(["--synthetic", "--binary", "True", "--march", "grid", "--grid_init", "hull", "--img_size", "32", "--number_angles", "2",
                "--n_iters", "48", "--display_every", "16", "--sample_size", "24", "--depth_samples", "100", "--num_layers", "4",
                "--num_hidden_units", "64", "--save_hull", str(tmp_path / "votes.npy"), "--log_dir", str(tmp_path / "run")] + flags)
    h = out["history"]
    assert [r["iter"] for r in h] == [0, 16, 32, 48] and all(np.isfinite(r["train_loss"]) for r in h)
    hull = np.load(tmp_path / "run" / "hull.npy")
    votes = np.load(tmp_path / "votes.npy")
    assert hull.shape == (128, 128, 128) and hull.dtype == bool and votes.shape == (2, 128, 128, 128) and votes.dtype == np.uint16
    assert np.array_equal(hull, (votes[1] == 0) & (votes[0] >= 1))
    info = out["hull_info"]
    assert info["n_views"] == 9 and 0.0 < info["share"] < 0.5 and info["share"] == hull.mean() and info["min_seen"] >= 1
    for name in ("acc_grid_binary.npy", "vessel_acc_grid_binary.npy"):
        saved = np.load(tmp_path / "run" / name)
        assert not (saved & ~hull).any(), name
    for g in (out["acc_grid"], out["vessel_acc_grid"]):
        live = g.binary.cpu().numpy()
        assert not (live & ~hull).any() and float(g.occs[torch.from_numpy(~hull.reshape(-1)).to(DEV)].abs().max()) == 0.0
    assert out["acc_grid"].binary.any()
    log = [json.loads(line) for line in open(tmp_path / "run" / "train_log.jsonl")]
    assert all(rec["hull"] == dict(share=info["share"], min_seen=info["min_seen"], n_views=9) for rec in log) and len(log) == 4


def test_hull_metrics(golden):
    """reconstruction_hull_metrics on the capsule phantom at n = 33: three finite numbers that equal the restatement's counts; a
    'reconstruction' that is the truth itself has nothing outside the hull of its own silhouettes; the sweep tabulates the columns."""
    from nerf_for_angiography_amd.phantomdata.dataset import angle_grid
    from nerf_for_angiography_amd.phantomdata.helpers import VoxelVolume, capsule_mu, capsule_tree
    from nerf_for_angiography_amd.phantomdata.proj_helpers import source_matrix
    from nerf_for_angiography_amd.visualization import sweep
    eng = _engine()
    t = np.linspace(-100.0, 100.0, 65)
    nodes = np.stack(np.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)
    mu = capsule_mu(torch.from_numpy(nodes), capsule_tree(levels=5, seed=0)).numpy().reshape(65, 65, 65)
    vol = VoxelVolume(t, t, t, mu, fill_value=0.0, device=DEV)
    poses = np.stack([source_matrix(SRC, th, ph) for th, ph in angle_grid(180, 2)[:-1]])
    masks, _ = hr.masks_from_points(nodes[mu.reshape(-1) > 0], poses, 13.0 * 48, 48, 48)      # the silhouettes of the phantom's own voxels
    views = eng.visual_hull_views(poses, torch.from_numpy(masks).to(DEV), 13.0 * 48)
    m = _model(-5.0, prec="f32")
    n = 33
    scores, hull, pred, gt = sweep.reconstruction_hull_metrics(m, vol, 100.0, n, views)
    a12 = sweep.grid_index_to_world(100.0, n)
    seen, rejects = hr.hull_counts(hr.lattice_points((n,) * 3, a12), eng.hull_default_radius(a12), poses, 13.0 * 48, 48, 48, 1.0,
                                   hr.distance_stack(masks))
    want_hull = ((rejects == 0) & (seen >= 1)).reshape(n, n, n)
    assert np.array_equal(hull.cpu().numpy(), want_hull)
    thr = float(torch.mean(gt))
    a, b = pred.cpu().numpy() >= np.float32(thr), gt.cpu().numpy() >= np.float32(thr)
    want = sweep.hull_scores(int(a.sum()), int((a & ~want_hull).sum()), int(want_hull.sum()), int(b.sum()), int((b & want_hull).sum()))
    print(f"hull metrics: {scores}")
    for key in ("outside_hull", "dice_hull", "hull_ratio"):
        assert np.isfinite(scores[key]) and scores[key] == want[key], key
    assert scores["n_gt"] == int(b.sum()) >= 10 and scores["hull_ratio"] > 1.0
    truth = sweep.reconstruction_hull_metrics(None, vol, 100.0, n, views, grids=(gt, gt))[0]
    assert truth["outside_hull"] == 0.0 and truth["n_pred"] == scores["n_gt"] and truth["dice_hull"] == scores["dice_hull"]
    # the sweep's columns, last in the table, repeated on every row
    from test_gpu_sweep_metrics import BASE, _sweep_setup
    g, gvol, gm, ggt, angles, geo = _sweep_setup(golden)
    sweep_poses = sweep._poses(angles, geo[3], (0.0, 0.0, 0.0), DEV)
    full = eng.visual_hull_views(sweep_poses, torch.ones(len(angles), geo[1], geo[0], dtype=torch.bool, device=DEV), geo[2])
    with pytest.raises(ValueError, match="hull_views"):
        sweep.evaluation_sweep(gm, ggt, angles, *geo, metrics=["PSNR", "OUTSIDE HULL 3D"], volume=gvol)
    df, _ = sweep.evaluation_sweep(gm, ggt, angles, *geo, metrics=["HULL RATIO 3D", "PSNR", "OUTSIDE HULL 3D", "DICE 3D HULL"], volume=gvol,
                                   volume_outside=100.0, volume_points=25, hull_views=full)
    assert list(df.columns) == BASE + ["PSNR"] + list(sweep.HULL_METRICS)
    ref = sweep.reconstruction_hull_metrics(gm, gvol, 100.0, 25, full)[0]
    for col, key in zip(sweep.HULL_METRICS, ("outside_hull", "dice_hull", "hull_ratio")):
        v = df[col].to_numpy()
        assert len(v) == len(angles) and ((v == ref[key]).all() or (np.isnan(v).all() and ref[key] != ref[key])), col
