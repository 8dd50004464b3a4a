"""The two-level scans past 1024 partials (k_cc_scan, k_cg_scan_chunks, k_iso_scan, k_sel_offsets, k_grid_occ_scan, the chunked launches of
the thinning): every family of kernels on the cases of tests/many_chunks_cases.py, where each thread of the one scanning workgroup walks
a run of two or three partials, against the reference and with the equality helper of the family's own test module - bit for bit, as at
the small shapes.  A wrong run bound, a wrong exclusive prefix for a thread's second partial or a total read from the wrong thread
shifts every label, vertex id, branch offset or selected index behind the first 1024 chunks (tests/test_many_chunks_cpu.py shows it on a
model of the scan).  Run with -m gpu on an MI355X."""
import functools

import numpy as np
import pytest
import torch

import components_reference as cr
import graph_reference as gr
import many_chunks_cases as mc
import skeleton_reference as sk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = sorted(mc.VOLUMES)


def _on_dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _skeleton(name):
    """(reference skeleton, reference record) of a volume, once per session"""
    return sk.skeletonize(mc.volume(name))


@functools.lru_cache(maxsize=None)
def _device_d2(name):
    """The device's squared EDT of a volume (int64 ndarray), checked against SciPy by test_edt_and_surface_metrics."""
    from nerf_for_angiography_amd.engine import distance_transform_edt_3d
    return distance_transform_edt_3d(_on_dev(mc.volume(name)), return_squared=True)[1].cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_components(name):
    from nerf_for_angiography_amd.engine import filter_components_3d
    from test_gpu_components import _check
    m = mc.volume(name)
    for c in (1, 2, 3):
        want, k = _check(m, c, name)
        assert k > mc.SCAN_THREADS
    x = _on_dev(m)
    sizes = cr.sizes(want)                                   # of the 26-connected labelling
    big, n_big, _ = cr.largest(want)
    size_of = sizes[np.maximum(want, 1) - 1]
    assert n_big > 1000 and (sizes == 1).sum() > mc.SCAN_THREADS
    assert np.array_equal(filter_components_3d(x, 3, largest_only=True).cpu().numpy(), want == big)
    assert np.array_equal(filter_components_3d(x, 3, min_size=2).cpu().numpy(), (want != 0) & (size_of >= 2))
    assert np.array_equal(filter_components_3d(x, 3, largest_only=True, min_size=2).cpu().numpy(), want == big)
    assert np.array_equal(filter_components_3d(x, 3).cpu().numpy(), m)


@pytest.mark.parametrize("name", NAMES)
def test_edt_and_surface_metrics(name):
    from test_gpu_surface_metrics import _check_edt, _check_scores
    m = mc.volume(name)
    _check_edt(m.copy(), name)                               # d2 and dist against SciPy, bit for bit
    assert np.array_equal(_device_d2(name), gr.squared_edt(m))
    shifted = np.zeros_like(m)
    shifted[:, :, 1:] = m[:, :, :-1]                         # the volume against a copy shifted by one voxel
    got = _check_scores(m.astype(np.float32), shifted.astype(np.float32), 0.5, 0.5)
    assert got["n_pred"] == int(m.sum()) and 0.0 < got["dice_vessel"] < 1.0 and got["hd"] >= 1.0


@pytest.mark.parametrize("name", NAMES)
def test_thinning(name):
    from test_gpu_skeleton import _gpu, _record, _want_record
    m = mc.volume(name)
    want, rec = _skeleton(name)
    got, grec = _gpu(m.copy())
    assert grec == _want_record(rec, m), (grec, rec)
    assert np.array_equal(got, want), int((got != want).sum())
    assert rec["passes"] >= 3 and rec["converged"] == 1
    full = sk.record_list(rec, m.sum())
    for sync in (2, 3):                                      # the fixed-pass form: exactly the reference's passes, read back every `sync`
        s, r = _record(m, rec["passes"], sync)
        assert r == full and np.array_equal(s, want.astype(np.uint8)), (sync, r, full)


@pytest.mark.parametrize("name", NAMES)
def test_centreline_graph(name):
    from test_gpu_centreline_graph import _check
    s = _skeleton(name)[0]
    d2 = _device_d2(name)
    want, _ = _check(s, d2, what=name, max_branches=4096)    # room for every branch
    nb = want["record"]["branches"]
    assert mc.SCAN_THREADS < nb <= 4096 and want["record"]["deg0"] > mc.SCAN_THREADS      # the specks: one-voxel branches in nearly every chunk
    _, (_, _, _, _, rec) = _check(s, d2, what=name + ", too few rows", max_branches=1000)
    assert int(rec[11]) == 1 and int(rec[4]) == nb


@pytest.mark.parametrize("name", NAMES)
def test_spur_pruning(name):
    from nerf_for_angiography_amd.engine import prune_spurs
    from test_gpu_centreline_graph import _prune_raw
    s = _skeleton(name)[0]
    d2 = _device_d2(name)
    want, rec = gr.prune(s, d2, 1.0)
    assert rec["branches"] > 0 and rec["rounds"] >= 2
    full = gr.prune_record_slots(rec)
    for sync, rounds in ((0, rec["rounds"]), (1, rec["rounds"] + 3)):
        got, r = _prune_raw(s, d2, 1.0, rounds, sync)
        assert r == full and np.array_equal(got, want.astype(np.uint8)), (sync, rounds, r, full)
    p, prec = prune_spurs(_on_dev(s), _on_dev(d2), 1.0, return_record=True)
    assert np.array_equal(p.cpu().numpy(), want) and list(prec.values()) == full[:7]


@functools.lru_cache(maxsize=None)
def _mesh(name, cap):
    """(float32 field, affine, reference mesh) of a volume's mask at level 0.5, once per session"""
    from test_gpu_isosurface import _reference
    from test_isosurface_cpu import SWAPPED
    f = mc.volume(name).astype(np.float32)
    affine = SWAPPED if cap else None
    return f, affine, _reference(f, 0.5, affine, cap, 0.0)


@pytest.mark.parametrize("cap", [False, True], ids=["open", "capped"])
@pytest.mark.parametrize("name", NAMES)
def test_isosurface(name, cap):
    from test_gpu_isosurface import _extract, _same_mesh
    f, affine, want = _mesh(name, cap)
    assert want["V"] > 50_000 and want["T"] > 100_000
    got = _extract(f, 0.5, affine, cap, fill=0.0)
    _same_mesh(got, want, (name, cap))
    assert (got[2]["B"] == 0) == cap


@pytest.mark.parametrize("name", NAMES)
def test_isosurface_capacities_one_below_the_counts(name):
    """As test_capacities_are_respected_and_counts_stay_true: the counts stay true, the status bits are set, what fits is what a full call
    writes and nothing is written beyond."""
    from nerf_for_angiography_amd.engine import isosurface_record
    f, affine, want = _mesh(name, False)
    x = _on_dev(f)
    V, T = want["V"], want["T"]
    counts = [V, T, want["E"], want["B"], want["n22"]]
    full = isosurface_record(x, 0.5, affine, V, T)
    assert full[2].cpu().tolist() == counts + [0, 0, 0]
    assert full[0].cpu().numpy().tobytes() == want["vertices"].tobytes()
    assert isosurface_record(x, 0.5, affine)[2].cpu().tolist() == counts + [3, 0, 0]
    guard = 64
    for cap_v, cap_t, status in ((V - 1, T, 1), (V, T - 1, 2), (V - 1, T - 1, 3)):
        verts = torch.full((cap_v + guard, 3), -7.0, dtype=torch.float32, device=DEV)
        tris = torch.full((cap_t + guard, 3), -7, dtype=torch.int32, device=DEV)
        rec = isosurface_record(x, 0.5, affine, cap_v, cap_t, vertices=verts, triangles=tris)[2].cpu().tolist()
        assert rec == counts + [status, 0, 0], (cap_v, cap_t)
        assert torch.equal(verts[:cap_v], full[0][:cap_v]) and torch.equal(tris[:cap_t], full[1][:cap_t])
        assert (verts[cap_v:] == -7.0).all() and (tris[cap_t:] == -7).all(), (cap_v, cap_t)


@pytest.mark.parametrize("kind", ["bernoulli", "few"])
def test_grid_draw(kind):
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    from test_gpu_grid_refresh import AABB, _restated
    from test_grid_refresh_cpu import SELECT_TAG, philox_u24
    grid = OccupancyGrid(roi_aabb=torch.tensor(AABB, device=DEV), resolution=list(mc.GRID_RES), seed=5).to(DEV)
    mask = mc.grid_mask(kind)
    grid._binary = _on_dev(mask)
    n_occ = int(mask.sum())
    for n in mc.GRID_DRAWS:
        for step, step_arg in ((256, 256), (4096, torch.tensor(4096, device=DEV))):
            cells, count = engine.grid_select_cells(grid._aabb_host, grid._res_host, grid.bits, n, grid.seed, step_arg)
            want, u24 = _restated(grid, step, n)
            assert int(count) == want.numel() == n + min(n, n_occ), (n, step)
            assert torch.equal(cells[:int(count)].long().cpu(), want), (n, step)
            assert np.array_equal(u24[:4096].numpy(), philox_u24(grid.seed, SELECT_TAG | step, 4096))
            if n_occ <= n:                                   # all of them, in index order
                assert np.array_equal(want[n:].numpy(), np.flatnonzero(mask))


@pytest.mark.parametrize("n", mc.SAMPLER_SIZES)
def test_topk(n):
    from nerf_for_angiography_amd.engine import topk_indices
    keys = mc.sampler_keys(n)
    order = mc.descending_order(keys)
    kd = _on_dev(keys)
    for k in mc.sampler_ks(n):
        idx = topk_indices(kd, k)
        assert idx.dtype == torch.int64 and idx.shape == (k,)
        assert np.array_equal(idx.cpu().numpy(), mc.topk_reference(keys, k, order)), (n, k)
        assert torch.equal(idx, topk_indices(kd, k)), (n, k)
    ties = mc.tie_keys(n)                                    # 5 values: the k-th largest one is cut in index order
    order = mc.descending_order(ties)
    td = _on_dev(ties)
    for k in (1, n // 5, n // 2 + 1, n - 3):
        assert ties[order[k - 1]] == ties[order[k]]          # the cut lies inside a tie class
        idx = topk_indices(td, k)
        assert np.array_equal(idx.cpu().numpy(), mc.topk_reference(ties, k, order)), (n, k)
        assert torch.equal(idx, topk_indices(td, k)), (n, k)


def test_batched_draw_equals_the_per_iteration_draw():
    from nerf_for_angiography_amd.engine import RayBatchSampler, sample_rays
    n, k, seed, first = mc.SAMPLER_SIZES[0], 5625, 11, 40
    g = torch.Generator().manual_seed(n)
    w = torch.rand(n, generator=g) + 0.05
    w[::7] = 0.0
    o, d, pix = torch.randn(n, 3, generator=g).to(DEV), torch.randn(n, 3, generator=g).to(DEV), torch.rand(n, generator=g).to(DEV)
    w = w.to(DEV)
    sampler = RayBatchSampler(o, d, pix, w, k, seed=seed, prefetch=3)
    rows = []
    for b in range(3):
        bo, bd, bp, bidx = sampler.draw(first + b)
        so, sd, sp, sidx = sample_rays(o, d, pix, w, k, seed=seed, stream_id=first + b)
        assert torch.equal(bidx, sidx), b
        assert torch.equal(bo, so) and torch.equal(bd, sd) and torch.equal(bp, sp), b
        assert bool((sidx[1:] > sidx[:-1]).all()) and bool((w[sidx] > 0).all()) and int(sidx.max()) > mc.SCAN_THREADS * mc.SEL_PER_BLOCK
        rows.append(sidx)
    assert sampler._first == first                           # one launch sequence served the three draws
    assert not torch.equal(rows[0], rows[1]) and not torch.equal(rows[1], rows[2])
