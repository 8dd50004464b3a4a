"""Host side of the device-side occupancy-grid refresh (afx_grid_select_cells, afx_grid_refresh; no GPU needed): the restatement of the cell
draw rule of include/afx.h that the GPU tests compare the kernels with, checked on hand-made bitfields; the workspace formula; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

SELECT_TAG = 0x53454C43 << 32
JITTER_TAG = 0x47524944 << 32
M32 = 0xFFFFFFFF


def philox_u24(seed: int, stream: int, n: int) -> np.ndarray:
    """Top 24 bits of numbers 0..n-1 of the Philox4x32-10 stream (seed, stream): the generator of afx_philox_uniform, restated in numpy."""
    i = np.arange(n, dtype=np.uint64)
    c = [(i >> np.uint64(2)) & np.uint64(M32), (i >> np.uint64(34)) & np.uint64(M32), np.full(n, stream & M32, np.uint64),
         np.full(n, stream >> 32, np.uint64)]
    k0, k1 = np.uint64(seed & M32), np.uint64(seed >> 32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & np.uint64(M32), p1 & np.uint64(M32), ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & np.uint64(M32),
             p0 & np.uint64(M32)]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(M32), (k1 + np.uint64(0xBB67AE85)) & np.uint64(M32)
    out = np.stack(c, 1)[np.arange(n), (i & np.uint64(3)).astype(np.int64)]
    return (out >> np.uint64(8)).astype(np.int64)


def select_rule(u24, occupied, num_cells: int, n: int):
    """The draw rule of include/afx.h: u24 [2n] (int64, the stream's top 24 bits), occupied = the occupied cells in index order.  Returns the
    selected cells (int64), n + min(n, n_occ) of them."""
    u24 = torch.as_tensor(u24, dtype=torch.int64)
    occupied = torch.as_tensor(occupied, dtype=torch.int64)
    uniform = (u24[:n] * num_cells) >> 24
    n_occ = occupied.numel()
    occ = occupied[(u24[n:2 * n] * n_occ) >> 24] if n < n_occ else occupied
    return torch.cat([uniform, occ])


def _bits_of(mask: np.ndarray) -> np.ndarray:
    m = np.zeros((mask.size + 31) // 32 * 32, np.uint64)
    m[:mask.size] = mask.reshape(-1)
    return (m.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def _occupied_from_bits(bits: np.ndarray, num_cells: int) -> np.ndarray:
    """The occupied cells of a packed bitfield, in index order (what the kernels rank)."""
    flat = ((bits[:, None].astype(np.uint64) >> np.arange(32, dtype=np.uint64)) & np.uint64(1)).reshape(-1)[:num_cells]
    return np.nonzero(flat)[0]


@pytest.mark.parametrize("res", [(8, 8, 8), (37, 29, 23), (5, 3, 7)])
@pytest.mark.parametrize("density", [0.0, 0.05, 0.2, 0.6, 1.0])
def test_draw_rule_on_hand_made_bitfields(res, density):
    """The restated rule on bitfields built by hand: n uniform cells in range; the occupied part is a draw among the occupied cells when there
    are more than n of them, else all of them in index order; the total is n + min(n, n_occ).  Bits past the last cell are ignored."""
    nc = res[0] * res[1] * res[2]
    rng = np.random.default_rng(int(density * 100) + nc)
    mask = rng.random(nc) < density
    bits = _bits_of(mask)
    if nc % 32:
        bits[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(nc % 32)      # junk past the last cell
    occupied = _occupied_from_bits(bits, nc)
    assert np.array_equal(occupied, np.nonzero(mask)[0])
    n = nc // 4
    u24 = philox_u24(3, SELECT_TAG | 272, 2 * n)
    assert u24.min() >= 0 and u24.max() < (1 << 24)
    cells = select_rule(u24, occupied, nc, n)
    n_occ = occupied.size
    assert cells.numel() == n + min(n, n_occ)
    assert int(cells[:n].min()) >= 0 and int(cells[:n].max()) < nc
    occ_part = cells[n:].numpy()
    assert mask[occ_part].all()
    if n_occ <= n:
        assert np.array_equal(occ_part, occupied)
    # exact in float64 for N < 2^29: floor(u * N) with u = u24 / 2^24
    u = u24.astype(np.float64) / (1 << 24)
    assert np.array_equal(np.floor(u[:n] * nc).astype(np.int64), cells[:n].numpy())


def test_philox_restatement_is_the_uniform_generator():
    """philox_u24 / 2^24 is afx_philox_uniform's u: a restatement independent of the library (the GPU tests compare the two); here the
    stream's statistics and its dependence on every argument."""
    a = philox_u24(0, SELECT_TAG | 256, 4096)
    assert abs(a.mean() / (1 << 24) - 0.5) < 0.02
    assert not np.array_equal(a, philox_u24(1, SELECT_TAG | 256, 4096))
    assert not np.array_equal(a, philox_u24(0, SELECT_TAG | 272, 4096))
    assert not np.array_equal(a, philox_u24(0, JITTER_TAG | 256, 4096))
    assert np.array_equal(a[:100], philox_u24(0, SELECT_TAG | 256, 100))


def _rup(v, a=256):
    return (v + a - 1) // a * a


def _expected_ws(res, n_draw, all_cells):
    nc = res[0] * res[1] * res[2]
    cap = nc if all_cells else 2 * n_draw
    words = (nc + 31) // 32
    nb = (words + 255) // 256
    sel = _rup(words * 4) + 2 * _rup(nb * 4) + _rup(8)
    o = _rup(0 if all_cells else cap * 4)
    o = _rup(o + cap * 12)
    o = _rup(o + cap * 4)
    o = _rup(o + nc * 4)
    o = _rup(o + 256 * 8)
    o = _rup(o + (0 if all_cells else 8))
    return o + (0 if all_cells else sel), sel


@pytest.mark.parametrize("res", [(128, 128, 128), (64, 64, 64), (37, 29, 23), (1, 1, 1)])
def test_workspace_formula(res):
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd import _lib
    nc = res[0] * res[1] * res[2]
    n = max(nc // 4, 1)
    for all_cells in (True, False):
        want, sel = _expected_ws(res, n, all_cells)
        assert engine.grid_refresh_workspace_bytes([-1.0, -1, -1, 1, 1, 1], res, n, all_cells) == want
    assert engine.grid_select_workspace_bytes([-1.0, -1, -1, 1, 1, 1], res) == sel
    if res == (128, 128, 128):      # the post-warm-up refresh needs less than the warm-up one; both well under 100 MiB
        assert _lib.load() is not None
        assert engine.grid_refresh_workspace_bytes([-1.0, -1, -1, 1, 1, 1], res, n, False) < \
            engine.grid_refresh_workspace_bytes([-1.0, -1, -1, 1, 1, 1], res, n, True) < 100 << 20


def _grid(_lib, res=(16, 16, 16)):
    g = _lib.GridDesc()
    for i, v in enumerate([-1.0, -1, -1, 1, 1, 1]):
        g.roi_aabb[i] = v
    for i, v in enumerate(res):
        g.resolution[i] = v
    return g


def test_refusals():
    """Invalid sizes and null pointers return AFX_E_INVALID, a short workspace AFX_E_WORKSPACE - all before anything is launched; host tensors
    raise AfxError in the Python wrappers."""
    from nerf_for_angiography_amd import _lib, engine
    from nerf_for_angiography_amd._lib import AfxError
    from nerf_for_angiography_amd.engine import Engine
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    lib = _lib.load()
    fake = 1 << 40      # never dereferenced: every refusal happens before a launch
    g = _grid(_lib)
    nc = 16 ** 3
    ws = int(lib.afx_grid_select_workspace_bytes(C.byref(g)))
    sel = lambda n, bits=fake, cells=fake, count=fake, wsb=ws, step=0: lib.afx_grid_select_cells(
        C.byref(g), bits, n, 0, step, None, cells, count, fake, wsb, None)
    assert sel(0) == -1 and b"n_draw" in lib.afx_last_error()
    assert sel(nc + 1) == -1
    assert sel(-3) == -1
    assert sel(16, bits=None) == -1 and b"null" in lib.afx_last_error()
    assert sel(16, count=None) == -1
    assert sel(16, step=-1) == -1 and b"step" in lib.afx_last_error()
    assert sel(16, step=1 << 32) == -1
    assert sel(16, wsb=ws - 1) == -2 and b"workspace" in lib.afx_last_error()
    assert lib.afx_grid_refresh_workspace_bytes(C.byref(g), 0, 0) == -1
    assert lib.afx_grid_refresh_workspace_bytes(C.byref(g), nc + 1, 0) == -1
    assert lib.afx_grid_refresh_workspace_bytes(C.byref(g), 0, 1) > 0      # (warm-up: n_draw unused)
    big = _grid(_lib, (2048, 2048, 2048))      # 2^33 cells: beyond the int32 cell lists and afx_mlp_infer's per-call limit
    assert lib.afx_grid_refresh_workspace_bytes(C.byref(big), 1 << 20, 1) == -1
    assert lib.afx_grid_refresh_workspace_bytes(C.byref(big), 1 << 20, 0) == -1
    wide = _grid(_lib, (2048, 2048, 256))      # 2^30 cells: fits int32, but a draw of 2^30 cells is a capacity of 2^31 points
    assert lib.afx_grid_refresh_workspace_bytes(C.byref(wide), 1 << 30, 0) == -1 and b"2^31" in lib.afx_last_error()
    assert lib.afx_grid_refresh_workspace_bytes(C.byref(wide), 1 << 28, 0) > 0

    eng = Engine(64, 4)
    need = int(lib.afx_grid_refresh_workspace_bytes(C.byref(g), nc // 4, 0))
    a = _lib.GridRefreshArgs()
    a.grid = g
    a.occs = a.binary = a.bits = a.workspace = fake
    a.n_draw, a.all_cells, a.occ_thre, a.ema_decay = nc // 4, 0, 0.01, 0.95
    a.workspace_bytes = need - 1
    p = _lib.PREC["f16s8"]
    assert lib.afx_grid_refresh(eng.h, p, fake, C.byref(a), None) == -2 and b"workspace" in lib.afx_last_error()
    a.workspace_bytes = need
    assert lib.afx_grid_refresh(eng.h, 99, fake, C.byref(a), None) == -1
    assert lib.afx_grid_refresh(eng.h, p, None, C.byref(a), None) == -1
    assert lib.afx_grid_refresh(None, p, fake, C.byref(a), None) == -1
    a.step = -5
    assert lib.afx_grid_refresh(eng.h, p, fake, C.byref(a), None) == -1 and b"step" in lib.afx_last_error()
    a.step, a.bits = 0, None
    assert lib.afx_grid_refresh(eng.h, p, fake, C.byref(a), None) == -1 and b"null" in lib.afx_last_error()
    a.bits, a.n_draw = fake, 0
    assert lib.afx_grid_refresh(eng.h, p, fake, C.byref(a), None) == -1

    with pytest.raises(AfxError):
        engine.grid_select_cells([-1.0, -1, -1, 1, 1, 1], (16, 16, 16), torch.zeros(128, dtype=torch.int32), 16, 0, 0)
    host_grid = OccupancyGrid(roi_aabb=[-1.0, -1, -1, 1, 1, 1], resolution=16)
    with pytest.raises(AfxError):
        host_grid.refresh(None, 300)
    prepared = torch.zeros(int(lib.afx_query(eng.h, _lib.Q_PREPARED_BYTES, p, 0, 0)), dtype=torch.uint8)      # (well-formed but for the device)
    with pytest.raises(AfxError, match="no CPU path"):
        engine.grid_refresh(eng, prepared, "f16s8", [-1.0, -1, -1, 1, 1, 1], (16, 16, 16), host_grid.occs,
                            host_grid._binary_u8, host_grid._bits, nc // 4, False, 0, 300, 0.01, 0.95, torch.zeros(need, dtype=torch.uint8))


def test_driver_flag_requires_graph():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    with pytest.raises(ValueError, match="--graph-grid-update"):
        main(["--synthetic", "--march", "grid", "--graph-grid-update", "--n_iters", "0"])


def test_update_graph_refuses_a_host_model():
    """GridUpdateGraph checks the module like the other graph helpers before it touches a GPU."""
    from nerf_for_angiography_amd import render
    from nerf_for_angiography_amd.model.CPPN import CPPN
    md = dict(num_early_layers=4, num_late_layers=0, num_filters=64, num_input_channels=3, num_output_channels=1, num_input_channels_views=0,
              use_bias=True, pos_enc="none", pos_enc_basis=5, act_func="relu", fourier_sigma=5, num_img=1, device=torch.device("cpu"),
              precision="f16s8")
    with pytest.raises(Exception):
        render.GridUpdateGraph(CPPN(md), [])
