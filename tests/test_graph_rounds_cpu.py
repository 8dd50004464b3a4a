"""Whole grid-training rounds from one graph (afx_sample_batches_dev, afx_train_round_advance, render.GridTrainRoundGraph, the driver's
--graph-rounds): exports, argument refusals, the driver's flag checks, the learning-rate table and the host-side round scheduler - no GPU."""
import ctypes as C

import numpy as np
import pytest

FAKE = 1 << 40      # never dereferenced: every refusal happens before a launch


def test_library_exports_the_entry_points():
    from nerf_for_angiography_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("afx_sample_batches_dev", "afx_train_round_advance"):
        assert hasattr(lib, name), name
        assert name in _lib.exported_symbols()
    for variant in ("safe", "h6"):      # every build variant is bound through the same table
        assert hasattr(_lib.load(variant), "afx_sample_batches_dev")


def test_sample_batches_dev_refusals():
    from nerf_for_angiography_amd import _lib
    lib = _lib.load()
    n, k, B = 1000, 10, 16
    ws = int(lib.afx_sample_batches_workspace_bytes(n, B))

    def call(n=n, k=k, B=B, step=FAKE, out=FAKE, w=FAKE, wsb=ws, weights=FAKE):
        return lib.afx_sample_batches_dev(weights, n, 0, step, B, k, out, w, wsb, None)

    assert call(step=None) == -1 and b"null" in lib.afx_last_error()
    assert call(out=None) == -1 and b"null" in lib.afx_last_error()
    assert call(w=None) == -1 and b"null" in lib.afx_last_error()
    for bad in (0, -1, 65536):
        assert call(B=bad, wsb=1 << 40) == -1 and b"n_batches" in lib.afx_last_error(), bad
    assert call(n=1 << 32, wsb=1 << 62) == -1 and b"2^32" in lib.afx_last_error()
    assert call(n=(1 << 32) + 5, wsb=1 << 62) == -1
    assert call(n=0) == -1
    assert call(k=n + 1) == -1 and b"k" in lib.afx_last_error()
    assert call(k=-1) == -1
    assert call(wsb=ws - 1) == -2 and b"workspace" in lib.afx_last_error()
    # the host-id entry point keeps its own rules (an empty request is a no-op there)
    assert lib.afx_sample_batches(FAKE, n, 0, 0, 0, k, FAKE, FAKE, ws, None) == 0


def _round_args(_lib, **over):
    a = _lib.TrainRoundArgs()
    for name, _ in a._fields_:
        setattr(a, name, FAKE)
    a.n_table, a.round_len = 8, 16
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_train_round_advance_refusals():
    from nerf_for_angiography_amd import _lib
    lib = _lib.load()
    assert lib.afx_train_round_advance(None, None) == -1 and b"null" in lib.afx_last_error()
    pointers = [name for name, t in _lib.TrainRoundArgs._fields_ if t is C.c_void_p]
    assert len(pointers) == 11
    for name in pointers:
        assert lib.afx_train_round_advance(C.byref(_round_args(_lib, **{name: None})), None) == -1, name
        assert b"null" in lib.afx_last_error()
    assert lib.afx_train_round_advance(C.byref(_round_args(_lib, n_table=0)), None) == -1 and b"n_table" in lib.afx_last_error()
    assert lib.afx_train_round_advance(C.byref(_round_args(_lib, round_len=0)), None) == -1 and b"round_len" in lib.afx_last_error()


def test_wrappers_refuse_host_tensors():
    import torch
    from nerf_for_angiography_amd import engine
    from nerf_for_angiography_amd._lib import AfxError
    with pytest.raises(AfxError):
        engine.sample_batches_dev(torch.ones(100), 0, torch.zeros((), dtype=torch.int64), 4, 10)
    z = torch.zeros(1)
    with pytest.raises(AfxError):
        engine.train_round_advance(torch.zeros((), dtype=torch.int64), z, z, z, z, torch.zeros(3, dtype=torch.int64), z, torch.zeros(1, 3, dtype=torch.int64),
                                   z, z, torch.zeros((), dtype=torch.int64))


def test_driver_flag_checks():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser, check_args, main
    base = ["--synthetic", "--march", "grid", "--n_iters", "0"]
    with pytest.raises(ValueError, match="--graph-rounds"):
        main(base + ["--graph-rounds"])
    with pytest.raises(ValueError, match="--graph-rounds"):
        main(base + ["--graph", "--graph-rounds"])
    with pytest.raises(ValueError, match="--graph-grid-update"):      # (the older check comes first)
        main(base + ["--graph-grid-update", "--graph-rounds"])
    with pytest.raises(ValueError, match="--host_sampler"):
        main(base + ["--graph", "--graph-grid-update", "--graph-rounds", "--host_sampler"])
    ok = build_parser().parse_args(base + ["--graph", "--graph-grid-update", "--graph-rounds", "--single-eval"])
    check_args(ok)      # composes with --single-eval
    assert ok.graph_rounds and ok.single_eval
    assert not build_parser().parse_args(base).graph_rounds      # opt-in


def test_lr_table_is_the_drivers_expression():
    from nerf_for_angiography_amd.render import lr_decay_table
    n = 5001
    tab = lr_decay_table(1e-4, 0.1, 500 * 1000, n)
    assert tab.dtype == np.float32 and tab.shape == (n,)
    for i in (0, 1, 15, 16, 4999, n - 1):
        want = np.float32(1e-4 * 0.1 ** (i / 500000))
        assert tab[i].tobytes() == want.tobytes(), i
    assert tab[0] == np.float32(1e-4) and tab[-1] < tab[0]


def _expand(ops, round_len):
    """(iterations in order, {step: refresh count}, op kinds in order)"""
    its, refreshes = [], {}
    for op in ops:
        if op[0] == "round":
            assert op[1] % round_len == 0
            its += list(range(op[1], op[1] + round_len))
            refreshes[op[1]] = refreshes.get(op[1], 0) + 1
        elif op[0] == "refresh":
            refreshes[op[1]] = refreshes.get(op[1], 0) + 1
        else:
            assert op[0] == "tail"
            its.append(op[1])
    return its, refreshes


@pytest.mark.parametrize("start,n", [(0, 48), (240, 33), (5, 30), (0, 2001)])
def test_round_schedule(start, n):
    from nerf_for_angiography_amd.render import grid_round_schedule
    L, W = 16, 256
    ops = grid_round_schedule(start, n, L, W)
    assert ops == grid_round_schedule(start, n, L, W)      # a pure function
    its, refreshes = _expand(ops, L)
    assert its == list(range(start, start + n))
    assert refreshes == {s: 1 for s in range(start, start + n) if s % L == 0}      # every multiple of round_len, exactly once
    for op in ops:
        if op[0] in ("round", "refresh"):
            assert op[2] == (op[1] < W)      # warm-up is step < 256
    for i, op in enumerate(ops):             # a refresh on its own is followed by the tail iteration of the same step
        if op[0] == "refresh":
            assert ops[i + 1] == ("tail", op[1])
    expected = {
        (0, 48): [("round", 0, True), ("round", 16, True), ("round", 32, True)],
        (240, 33): [("round", 240, True), ("round", 256, False), ("refresh", 272, False), ("tail", 272)],
        (5, 30): [("tail", s) for s in range(5, 16)] + [("round", 16, True)] + [("refresh", 32, True)] + [("tail", s) for s in range(32, 35)],
        (0, 2001): [("round", s, s < 256) for s in range(0, 2000, 16)] + [("refresh", 2000, False), ("tail", 2000)],
    }[(start, n)]
    assert ops == expected


def test_round_schedule_edges():
    from nerf_for_angiography_amd.render import grid_round_schedule
    assert grid_round_schedule(7, 0) == []
    assert grid_round_schedule(16, 15) == [("refresh", 16, True)] + [("tail", s) for s in range(16, 31)]      # a short remainder never replays a round
    assert grid_round_schedule(0, 1) == [("refresh", 0, True), ("tail", 0)]
    assert grid_round_schedule(256, 16) == [("round", 256, False)]
    assert grid_round_schedule(8, 8, round_len=4, warmup=12) == [("round", 8, True), ("round", 12, False)]
    with pytest.raises(ValueError):
        grid_round_schedule(-1, 4)


def test_round_graph_refuses_a_host_model():
    """GridTrainRoundGraph makes the checks of the other graph helpers before it touches a GPU."""
    import torch
    from nerf_for_angiography_amd import render
    from nerf_for_angiography_amd.model.CPPN import CPPN
    md = dict(num_early_layers=4, num_late_layers=0, num_filters=64, num_input_channels=3, num_output_channels=1, num_input_channels_views=0,
              use_bias=True, pos_enc="none", pos_enc_basis=5, act_func="relu", fourier_sigma=5, num_img=1, device=torch.device("cpu"),
              precision="f16s8")
    m = CPPN(md)
    tab = (torch.zeros(8, 3), torch.zeros(8, 3), torch.zeros(8), torch.ones(8))
    with pytest.raises(ValueError, match="Adam"):      # not the fused, capturable Adam
        render.GridTrainRoundGraph(m, torch.optim.Adam(m.parameters(), lr=1e-3), [], tab, None, 4, 100, 0.0, 1.0, 1e-2, 1e-4,
                                   lr_table=np.ones(4, np.float32))
