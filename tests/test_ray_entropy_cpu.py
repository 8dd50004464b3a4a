"""Host-side checks of the ray-entropy regulariser (afx_ray_entropy_*, engine.ray_entropy_*, acc_ray_entropy, ray_entropy,
--entropy_weight): the exported symbols and their refusals, the wrappers' refusal of host tensors, the driver's argument check, and the
fp64 torch restatement of tests/ray_entropy_reference.py against the reference's own outputs and autograd gradient (fixture g12) - the
yardstick of the GPU tests."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ray_entropy_reference as rer
from nerf_for_angiography_amd import _lib, engine
from nerf_for_angiography_amd._lib import AfxError

AFX_E_INVALID = -1
FAKE = C.c_void_p(1 << 20)      # a non-null pointer the host checks never dereference
SYMBOLS = ("afx_ray_entropy_packed", "afx_ray_entropy_packed_backward", "afx_ray_entropy_dense", "afx_ray_entropy_dense_backward")


def test_symbols_exported():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.exported_symbols()
        assert getattr(lib, name) is not None
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "afx.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(" in header


def test_entry_points_refuse_null_and_negative_arguments():
    lib = _lib.load()
    assert lib.afx_ray_entropy_packed(None, FAKE, 10, FAKE, 4, 0.4, FAKE, FAKE, None) == AFX_E_INVALID
    assert "afx_ray_entropy_packed" in lib.afx_last_error().decode()
    assert lib.afx_ray_entropy_packed(FAKE, FAKE, 10, FAKE, 4, 0.4, None, FAKE, None) == AFX_E_INVALID
    assert lib.afx_ray_entropy_packed(FAKE, FAKE, 10, FAKE, 4, 0.4, FAKE, None, None) == AFX_E_INVALID
    assert lib.afx_ray_entropy_packed(FAKE, FAKE, -1, FAKE, 4, 0.4, FAKE, FAKE, None) == AFX_E_INVALID
    assert lib.afx_ray_entropy_packed(FAKE, FAKE, 10, FAKE, -4, 0.4, FAKE, FAKE, None) == AFX_E_INVALID
    assert lib.afx_ray_entropy_packed(FAKE, FAKE, 10, FAKE, 1 << 31, 0.4, FAKE, FAKE, None) == AFX_E_INVALID
    assert lib.afx_ray_entropy_packed(FAKE, FAKE, 10, FAKE, 0, 0.4, FAKE, FAKE, None) == 0      # no rays: nothing to do
    assert lib.afx_ray_entropy_packed_backward(FAKE, None, 10, FAKE, 0.4, FAKE, FAKE, 0, FAKE, None) == AFX_E_INVALID
    assert "afx_ray_entropy_packed_backward" in lib.afx_last_error().decode()
    assert lib.afx_ray_entropy_packed_backward(FAKE, FAKE, 10, FAKE, 0.4, FAKE, FAKE, 1, None, None) == AFX_E_INVALID
    assert lib.afx_ray_entropy_packed_backward(FAKE, FAKE, -10, FAKE, 0.4, FAKE, FAKE, 0, FAKE, None) == AFX_E_INVALID
    assert lib.afx_ray_entropy_packed_backward(None, None, 0, None, 0.4, None, None, 0, None, None) == 0      # no samples
    assert lib.afx_ray_entropy_dense(None, 4, 8, FAKE, 0.4, FAKE, FAKE, None) == AFX_E_INVALID
    assert "afx_ray_entropy_dense" in lib.afx_last_error().decode()
    assert lib.afx_ray_entropy_dense(FAKE, 4, 0, FAKE, 0.4, FAKE, FAKE, None) == AFX_E_INVALID
    assert lib.afx_ray_entropy_dense(FAKE, -4, 8, FAKE, 0.4, FAKE, FAKE, None) == AFX_E_INVALID
    assert lib.afx_ray_entropy_dense_backward(FAKE, 4, 8, FAKE, 0.4, None, FAKE, 0, FAKE, None) == AFX_E_INVALID
    assert "afx_ray_entropy_dense_backward" in lib.afx_last_error().decode()
    assert lib.afx_ray_entropy_dense_backward(FAKE, 4, 8, FAKE, 0.4, FAKE, FAKE, 0, None, None) == AFX_E_INVALID
    assert lib.afx_ray_entropy_dense_backward(FAKE, 4, -8, FAKE, 0.4, FAKE, FAKE, 0, FAKE, None) == AFX_E_INVALID


def test_wrappers_refuse_host_tensors():
    from nerf_for_angiography_amd.nerf.nerf_helpers import ray_entropy
    from nerf_for_angiography_amd.nerf.nerf_helpers_acc import acc_ray_entropy
    pred, ri, rgb = torch.zeros(6), torch.tensor([0, 0, 1, 1, 1, 2], dtype=torch.int32), torch.full((3,), 0.2)
    sums, d_ent = torch.ones(3, 2), torch.ones(3)
    with pytest.raises(AfxError, match="no CPU path"):
        engine.ray_entropy_packed(pred, ri, rgb, 3)
    with pytest.raises(AfxError, match="no CPU path"):
        engine.ray_entropy_packed_backward(pred, ri, rgb, sums, d_ent)
    with pytest.raises(AfxError, match="no CPU path"):
        engine.ray_entropy_dense(pred.reshape(3, 2), rgb)
    with pytest.raises(AfxError, match="no CPU path"):
        engine.ray_entropy_dense_backward(pred.reshape(3, 2), rgb, sums, d_ent)
    with pytest.raises(AfxError, match="no CPU fallback"):
        acc_ray_entropy(pred, ri, rgb, 3)
    with pytest.raises(AfxError, match="no CPU fallback"):
        ray_entropy(pred.reshape(3, 2), rgb)


def test_driver_argument_check():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser, check_args
    parse = build_parser().parse_args
    assert parse([]).entropy_weight == 0.0
    check_args(parse([]))
    check_args(parse(["--march", "grid"]))      # weight 0: every march as before
    args = parse(["--entropy_weight", "0.1", "--march", "grid_ops"])
    check_args(args)
    assert args.entropy_weight == 0.1
    for flags in (["--march", "dense"], ["--march", "grid"], [], ["--march", "grid", "--graph"],
                  ["--march", "grid", "--graph", "--graph-grid-update"], ["--march", "grid", "--graph", "--graph-grid-update", "--graph-rounds"],
                  ["--march", "grid", "--single-eval"]):
        with pytest.raises(ValueError, match="grid_ops"):
            check_args(parse(["--entropy_weight", "0.1"] + flags))
    with pytest.raises(ValueError, match="entropy_weight"):
        check_args(parse(["--entropy_weight", "-0.1", "--march", "grid_ops"]))


def test_fingerprint_names_the_weight_only_when_set():
    """A state file written without the flag keeps its fingerprint; a run with the term does not resume as one without."""
    from nerf_for_angiography_amd.nerf import checkpoint as ck
    from nerf_for_angiography_amd.nerf.run_nerf_acc import build_parser
    table = [torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5), torch.ones(5)]
    off = ck.config_fingerprint(build_parser().parse_args(["--march", "grid_ops"]), {}, table)
    on = ck.config_fingerprint(build_parser().parse_args(["--march", "grid_ops", "--entropy_weight", "0.05"]), {}, table)
    assert "entropy_weight" not in off and on["entropy_weight"] == 0.05
    with pytest.raises(ValueError, match="entropy_weight"):
        ck.compare_fingerprints(off, on)


def test_restatement_reproduces_the_reference_fixture(golden):
    """The fp64 restatement against the reference's render_volume_density entropy and its autograd gradient: same formula in the same
    precision, so they agree to fp64 rounding (1e-12 relative)."""
    g = golden("g12_ray_entropy")
    raw, rgb = torch.from_numpy(g["raw"]), torch.from_numpy(g["rgb_map"])
    assert raw.shape == (48, 33) and raw.dtype == torch.float32 and rgb.dtype == torch.float64
    assert g["dirs"].shape == (48, 3) and g["z"].shape == (33,) and g["d_raw"].shape == (48, 33)
    thr = float(g["threshold"])
    assert thr == 0.4
    margin = np.abs(1.0 - g["rgb_map"] - thr)
    assert margin.min() >= 1e-3      # fp32 and fp64 agree on the mask
    mask = (1.0 - g["rgb_map"]) > thr
    assert 0 < mask.sum() < mask.size      # both mask states occur
    e, d = rer.value_and_grad(rer.entropy_dense, raw.double(), rgb, thr)
    assert rer.rel_l2(e, torch.from_numpy(g["entropy"])) < 1e-12
    assert rer.rel_l2(d, torch.from_numpy(g["d_raw"])) < 1e-12
    assert bool((e[torch.from_numpy(~mask)] == 0).all()) and bool((d[torch.from_numpy(~mask)] == 0).all())
    # the packed restatement is the dense one on the flattened list (so the fixture pins it too) ...
    ri = torch.arange(48, dtype=torch.int32).repeat_interleave(33)
    ep, dp = rer.value_and_grad(rer.entropy_packed, raw.double().reshape(-1), rgb, ri, 48, thr)
    assert rer.rel_l2(ep, e) < 1e-12 and rer.rel_l2(dp, d.reshape(-1)) < 1e-12
    # ... and the closed-form gradient the kernels evaluate is the autograd one
    sg = torch.sigmoid(raw.double())
    D = sg.sum(-1, keepdim=True) + 1e-10
    p = sg / D
    u = torch.log(p + 1e-10) + p / (p + 1e-10)
    closed = -(u - (p * u).sum(-1, keepdim=True)) / D * sg * (1 - sg) * torch.from_numpy(mask)[:, None]
    assert rer.rel_l2(closed, d) < 1e-12
