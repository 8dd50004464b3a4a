"""The two-level scans AT 1024 partials (csrc/afx_scan.h and its users): the many-chunk cases start at 1027 partials and every other test
module stays far below 1024, so nothing else runs the one scanning workgroup with exactly 1024 partials - per = 1, no thread idle - or
with 1025 - per = 2, the threads from 513 on with empty runs.  The top-k selection (k_sel_offsets), the component labelling (k_cc_scan) and
the march's offsets (k_ray_offsets) on the boundary cases of tests/many_chunks_cases.py, against the references of their own test
modules, bit for bit; tests/test_scan_boundary_cpu.py asserts that the cases hold the partial counts they are there for.
Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch

import many_chunks_cases as mc
import march_reference as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n", mc.BOUNDARY_SAMPLER_SIZES)
def test_topk(n):
    from nerf_for_angiography_amd.engine import topk_indices
    for keys in (mc.sampler_keys(n), mc.tie_keys(n)):
        order = mc.descending_order(keys)
        kd = torch.from_numpy(keys).to(DEV)
        for k in (1, 5625, n):
            idx = topk_indices(kd, k)
            assert idx.dtype == torch.int64 and idx.shape == (k,)
            assert np.array_equal(idx.cpu().numpy(), mc.topk_reference(keys, k, order)), (n, k)


@pytest.mark.parametrize("shape", mc.BOUNDARY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_components(shape):
    from test_gpu_components import _check
    m = mc.sparse_volume(shape)
    for c in (1, 3):
        _, k = _check(m, c, shape)                           # labels, sizes and the record against the reference
        assert k > mc.SCAN_THREADS


@pytest.mark.parametrize("n_rays", mc.BOUNDARY_RAY_COUNTS)
def test_march_offsets(n_rays):
    from test_gpu_march import _march
    p = mr.chunk_problem(n_rays, "alternate")
    want = mr.march64(p).packed()
    ri, _, _, _, off = _march(p, want_points=False)
    assert off.dtype == torch.int64 and torch.equal(off.cpu(), torch.from_numpy(want[4])), n_rays
    assert int(off[-1]) == ri.numel() > n_rays and torch.equal(ri.cpu(), torch.from_numpy(want[0])), n_rays
