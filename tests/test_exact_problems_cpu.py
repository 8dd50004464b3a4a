"""The generator of the exact points-mode problems (tests/exact_problems.py) keeps its guarantees for every shape the GPU test uses, and its
float64 reference agrees with the oracle's CPU autograd."""
import numpy as np
import pytest
import torch

import exact_problems
from test_gpu_backward_exact import SHAPES, CHUNKED


@pytest.mark.parametrize("layers,width,n_pts", SHAPES + [CHUNKED])
def test_generator_guarantees(layers, width, n_pts):
    p = exact_problems.make(layers, width, n_pts, seed=1)
    assert exact_problems.check(p)
    assert p["pts"].dtype == np.float32 and p["d_out"].dtype == np.float32 and p["pts"].shape == (n_pts, 3)
    k = np.log2(np.abs(p["d_out"].astype(np.float64)))
    assert np.array_equal(k, np.round(k))                                       # powers of two
    if n_pts >= 1024:
        assert k.max() - k.min() >= 10                                          # the f16 path's scales vary


@pytest.mark.parametrize("layers,width,n_pts", [(1, 64, 31), (4, 64, 255), (12, 64, 257), (4, 256, 33)])
def test_reference_matches_oracle_autograd(layers, width, n_pts):
    from oracle import angio_oracle as orc
    p = exact_problems.make(layers, width, n_pts, seed=1)
    params = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in p["params"].items()}
    cfg = dict(num_early_layers=layers, num_filters=width)
    raw = orc.cppn_forward(torch.from_numpy(p["pts"]).double(), cfg, params).reshape(-1)
    assert np.array_equal(raw.detach().numpy(), p["raw"])
    (raw * torch.from_numpy(p["d_out"]).double()).sum().backward()
    for k, want in p["grads"].items():
        assert np.array_equal(params[k].grad.numpy(), want), k
