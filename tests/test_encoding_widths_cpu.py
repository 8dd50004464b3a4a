"""CPU-only: the input encodings at every band count afx_create admits (L = 1 ... 10, K0 = 3 + 6 L = 9 ... 63 first-layer columns).
The library's queries against their closed forms, the model class's gate (CPPN.fused_forward) against afx_create, and the exact-fp32
kernels' LDS refusal for encoded width-256 models, which launch_chain decides before it looks for a device.  No kernel is launched here."""
import ctypes as C

import pytest
import torch

from conftest import rel_l2
from test_host_cpu import model_def

ENCS = ("barf", "fourier")
WIDTHS = (64, 128, 256)
BANDS = range(0, 13)
PRECS16 = ("bf16x3", "bf16", "f16", "f16s8")
N_HIDDEN = 4
# (n_rays, n_samples) of the rays-mode workspace queries and (0, n_points) of the points-mode ones: the GPU tests' own problems
PROBLEMS = ((300, 40), (37, 33), (0, 3001))


def admitted(n_freq: int, width: int) -> bool:
    """What include/afx.h states for an encoded model: 1 ... 10 bands, and the K0 + 1 = 4 + 6 L columns fit the layer."""
    return 1 <= n_freq <= 10 and 4 + 6 * n_freq <= width


def _create(lib, enc, n_freq, width, n_hidden=N_HIDDEN):
    from nerf_for_angiography_amd import _lib
    h = C.c_void_p()
    d = _lib.ModelDesc(3, _lib.ENC[enc], n_freq, width, n_hidden)
    rc = lib.afx_create(C.byref(d), C.byref(h))
    return rc, h


@pytest.fixture(scope="module")
def lib():
    from nerf_for_angiography_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("enc", ENCS)
def test_afx_create_takes_1_to_10_bands_and_the_layouts_follow_k0(lib, enc):
    from nerf_for_angiography_amd import _lib
    from nerf_for_angiography_amd.model.CPPN import CPPN
    n_ok = 0
    for width in WIDTHS:
        for n_freq in BANDS:
            rc, h = _create(lib, enc, n_freq, width)
            assert (rc == 0) == admitted(n_freq, width), (enc, n_freq, width, lib.afx_last_error())
            if rc != 0:
                assert rc == -1 and lib.afx_last_error()
                continue
            n_ok += 1
            k0, f = 3 + 6 * n_freq, width
            assert lib.afx_query(h, _lib.Q_K0, 0, 0, 0) == k0
            n_params = f * k0 + f + N_HIDDEN * (f * f + f) + f + 1
            assert lib.afx_query(h, _lib.Q_PARAM_COUNT, 0, 0, 0) == n_params
            layout, total = CPPN(model_def(N_HIDDEN, width, pos_enc=enc, pos_enc_basis=n_freq))._layout()
            assert total == n_params
            for layer, want in enumerate(layout):
                wo, bo, r, c = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
                assert lib.afx_param_layout(h, layer, C.byref(wo), C.byref(bo), C.byref(r), C.byref(c)) == 0
                assert (wo.value, bo.value, r.value, c.value) == want, (enc, n_freq, width, layer)
            assert layout[0] == (0, f * k0, f, k0)
            lib.afx_destroy(h)
    assert n_ok == 3 * 10      # every width takes all ten: at width 64, L = 10 fills the layer exactly (k0pad == width)


@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("width", WIDTHS)
def test_sizes_grow_with_the_band_count_at_f32_only(lib, enc, width):
    """The exact-fp32 kernels keep rows of k0pad = K0 + 1 columns (prepared first-layer slab, encoded-input stash): their sizes never
    decrease in L.  The 16-bit kernels keep 64-column rows (four k-steps of 16) for any encoding: their workspaces do not depend on L."""
    from nerf_for_angiography_amd import _lib
    queries = (_lib.Q_BWD_WORKSPACE_MIN, _lib.Q_BWD_WORKSPACE_FULL, _lib.Q_BWD_INPUTS_WORKSPACE_MIN, _lib.Q_BWD_INPUTS_WORKSPACE_FULL)
    rows = {}
    for n_freq in [n for n in BANDS if admitted(n, width)]:
        rc, h = _create(lib, enc, n_freq, width)
        assert rc == 0
        row = {}
        for prec, p in _lib.PREC.items():
            row["prepared", prec] = lib.afx_query(h, _lib.Q_PREPARED_BYTES, p, 0, 0)
            for q in queries:
                for a0, a1 in PROBLEMS:
                    row[q, prec, a0, a1] = lib.afx_query(h, q, a0, a1, p)
        lib.afx_destroy(h)
        assert all(v > 0 for v in row.values()), (n_freq, row)
        rows[n_freq] = row
    bands = sorted(rows)
    assert bands[0] == 1 and len(bands) >= 9
    grew = False
    for lo, hi in zip(bands, bands[1:]):
        for key, v in rows[lo].items():
            prec = key[1]
            if prec == "f32":
                assert rows[hi][key] >= v, (key, lo, hi)
                grew = grew or rows[hi][key] > v
            elif key[0] != "prepared":
                assert rows[hi][key] == v, (key, lo, hi)
    assert grew
    # a FULL workspace is never smaller than the MIN one the same call accepts ... for the inputs' backward, whose MIN is one tile
    for n_freq, row in rows.items():
        for prec in _lib.PREC:
            for a0, a1 in PROBLEMS:
                assert row[_lib.Q_BWD_INPUTS_WORKSPACE_FULL, prec, a0, a1] >= row[_lib.Q_BWD_INPUTS_WORKSPACE_MIN, prec, a0, a1]


# ---------------------------------------------------------------- the model class's gate
@pytest.mark.parametrize("enc", ENCS)
def test_fused_gate_is_afx_create_s(lib, enc):
    """CPPN.fused_forward is True exactly where afx_create takes the geometry: a model the library refuses must never reach Engine(...)."""
    from nerf_for_angiography_amd.model.CPPN import CPPN
    for width in WIDTHS:
        for n_freq in BANDS:
            rc, h = _create(lib, enc, n_freq, width)
            if rc == 0:
                lib.afx_destroy(h)
            m = CPPN(model_def(N_HIDDEN, width, pos_enc=enc, pos_enc_basis=n_freq))
            assert m.fused_forward == (rc == 0), (enc, n_freq, width)
            assert m.fused == (rc == 0)
            assert (m.flat_params is not None) == (rc == 0)


@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("n_freq", [0, 11, 12])
def test_band_counts_outside_the_library_run_through_the_operators(enc, n_freq):
    """4 + 6 L <= 128 holds for L = 0, 11 and 12, but afx_create refuses them: such a model is not fused, and on host tensors its
    forward (the module's PyTorch operators) is the oracle's."""
    from nerf_for_angiography_amd.model.CPPN import CPPN
    from oracle import angio_oracle as orc
    torch.manual_seed(40 + n_freq)
    m = CPPN(model_def(3, 128, pos_enc=enc, pos_enc_basis=n_freq))
    assert not m.fused_forward and not m.fused and m.flat_params is None
    if enc == "barf":
        m.update_barf_alpha(n_freq - 0.5, "pts")
    else:
        with torch.no_grad():
            m.fourier_coefficients.mul_(0.1)
    assert m.early_pts_layers[0].weight.shape == (128, 3 + 6 * n_freq)
    x = torch.rand(257, 3) * 2 - 1
    cfg = dict(num_early_layers=3, num_filters=128, pos_enc=enc, pos_enc_basis=n_freq)
    params = {k: v.detach() for k, v in m.state_dict().items()}
    with torch.no_grad():
        y = m(x)
    assert y.shape == (257, 1)
    assert rel_l2(y.numpy(), orc.cppn_forward(x, cfg, params).numpy()) < 2e-6
    # ... and with gradients: the operators are differentiable as usual
    m(x).sum().backward()
    assert m.early_pts_layers[0].weight.grad is not None


# ---------------------------------------------------------------- the exact-fp32 kernels' LDS
def _f32_chain_lds(width, n_hidden, n_freq, bwd, enc="barf"):
    """launch_chain's own sum for the exact-fp32 kernels at width 256 (one workgroup per CU): the small parameters (biases, output
    layer, encoding tables) padded to 1 KiB, two stream slots of max(first-layer slab, hidden slab), and for the backward pass one
    ReLU-mask KiB per layer and tile pair plus 256 B of per-group optical depths."""
    nt, nq = width // 32, (3 + 6 * n_freq + 1) // 2
    naux = (6 if enc == "barf" else 3) * n_freq
    small = -(-((n_hidden + 2) * width + 4 + naux) // 4) * 4 * 4
    small = -(-small // 1024) * 1024
    slab0 = -(-nq * nt * 256 // 4096) * 4096
    slabh = nt * 4 * 1024
    lds = small + 2 * max(slab0, slabh)
    if bwd:
        lds += (n_hidden + 1) * ((nt + 1) // 2) * 1024 + 256
    return lds


def test_f32_lds_arithmetic_of_encoded_width_256_models():
    limit = 160 * 1024
    assert _f32_chain_lds(256, 8, 10, True) == 179456 > limit
    assert _f32_chain_lds(256, 8, 9, True) == 171264 > limit
    assert all(_f32_chain_lds(256, 8, n, True) <= limit for n in range(1, 9))
    assert _f32_chain_lds(256, 2, 10, True) == 148736 <= limit
    assert _f32_chain_lds(256, 8, 10, False) == 142336 <= limit


@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("n_freq", [9, 10])
def test_f32_backward_of_an_8x256_model_with_9_or_10_bands_is_refused_for_lds(lib, enc, n_freq):
    """launch_chain compares the LDS a launch needs with the 160 KiB of a CU before it looks for a device or touches a pointer: the refusal
    is reachable on a machine without a GPU, with placeholder pointers (never dereferenced).  Only refused launches can be pinned this way - an admitted one
    goes on to the device - so that L <= 8 trains and the forward pass of L = 9, 10 runs is left to tests/test_gpu_encoding_widths.py."""
    from nerf_for_angiography_amd import _lib
    assert _f32_chain_lds(256, 8, n_freq, True, enc) > 160 * 1024      # (no call at all if this file's own arithmetic said it fits)
    rc, h = _create(lib, enc, n_freq, 256, 8)
    assert rc == 0
    n_pts, f32 = 1000, _lib.PREC["f32"]
    ws_bytes = int(lib.afx_query(h, _lib.Q_BWD_WORKSPACE_FULL, 0, n_pts, f32))
    if torch.cuda.is_available():
        # where there is a device, the buffers are real ones of the sizes the call asks for: should the sizing ever change so that the
        # launch fits, the call runs on them (and this test fails on rc) instead of launching kernels on a placeholder address
        dev = torch.device("cuda:0")
        sizes = (int(lib.afx_query(h, _lib.Q_PREPARED_BYTES, f32, 0, 0)), 12 * n_pts, 4 * n_pts,
                 4 * int(lib.afx_query(h, _lib.Q_PARAM_COUNT, 0, 0, 0)), ws_bytes)
        bufs = [torch.zeros(n, dtype=torch.uint8, device=dev) for n in sizes]
        prepared, pts, d_out, grad, ws = (b.data_ptr() for b in bufs)
        rc = lib.afx_mlp_backward(h, f32, prepared, pts, n_pts, d_out, grad, ws, ws_bytes, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    else:
        p = 4096      # a placeholder for every pointer (aligned as a workspace must be): without a device no launch can follow
        rc = lib.afx_mlp_backward(h, f32, p, p, n_pts, p, p, p, ws_bytes, None)
    msg = lib.afx_last_error()
    lib.afx_destroy(h)
    assert rc == -1 and b"LDS" in msg, (rc, msg)
    assert str(_f32_chain_lds(256, 8, n_freq, True, enc)).encode() in msg, msg
