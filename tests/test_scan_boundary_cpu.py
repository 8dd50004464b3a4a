"""The inputs of tests/test_gpu_scan_boundary.py (no GPU needed) sit where they are meant to: exactly 1024 partials, where every thread of
the scanning workgroup holds one, and 1025, where the runs are two long and the threads from 513 on hold none."""
import numpy as np
import pytest

import components_reference as cr
import many_chunks_cases as mc
import march_reference as mr


def _runs(nb):
    """(per, the threads of the scanning workgroup whose run is not empty)"""
    per = mc.run_length(nb)
    return per, mc._ceil_div(nb, per)


def test_the_boundary_cases_have_1024_and_1025_partials():
    assert [mc.partials_volume(s[0] * s[1] * s[2]) for s in mc.BOUNDARY_SHAPES] == [1024, 1025]
    assert [mc.partials_sampler(n) for n in mc.BOUNDARY_SAMPLER_SIZES] == [1024, 1025]
    assert mc.BOUNDARY_SAMPLER_SIZES[0] == mc.SCAN_THREADS * mc.SEL_PER_BLOCK
    assert _runs(1023) == (1, 1023) and _runs(1024) == (1, 1024) and _runs(1025) == (2, 513) and _runs(2049) == (3, 683)
    assert mc.BOUNDARY_RAY_COUNTS == (1023, 1024, 1025, 2049)          # one partial per ray
    assert not set(mc.BOUNDARY_SHAPES) & set(mc.VOLUMES.values()) and not set(mc.BOUNDARY_SAMPLER_SIZES) & set(mc.SAMPLER_SIZES)


@pytest.mark.parametrize("shape", mc.BOUNDARY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_boundary_volumes_fill_their_chunks(shape):
    m = mc.sparse_volume(shape)
    assert m.shape == shape and m.dtype == bool and max(shape) <= 1024 and m.flat[0] and m.flat[-1]
    occupied = mc.chunk_occupancy(m, mc.CC_CHUNK)
    assert occupied.size == mc.partials_volume(m.size) and 2 * occupied.sum() >= occupied.size and occupied[-1]
    assert cr.label(m, 3)[1] > mc.SCAN_THREADS and m.sum() < 0.02 * m.size


@pytest.mark.parametrize("n_rays", mc.BOUNDARY_RAY_COUNTS)
def test_boundary_rays_hold_samples(n_rays):
    """One ray in nine has no step; the others keep samples, up to the last runs of the scanning workgroup."""
    off = mr.march64(mr.chunk_problem(n_rays, "alternate")).packed()[4]
    assert off.size == n_rays + 1 and np.count_nonzero(np.diff(off)) >= n_rays * 8 // 9 - 1
    assert off[-1] > off[-4] > off[n_rays // 2] > 0
