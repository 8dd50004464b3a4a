"""The restatement of the ray sampler's draw (tests/sampler_reference.py; no GPU needed): the exact inclusion probabilities of weighted
sampling without replacement, the restated draw against torch.topk on fp64 keys, the restated draw's own frequencies on the seeds and
stream ids of the GPU distribution test - so that test's inputs are known to pass for a correct kernel before it ever runs - and the
refusals of the sampler's entry points that happen before any launch."""
import numpy as np
import pytest
import torch

import sampler_reference as sref

FAKE = 1 << 40      # never dereferenced: every refusal happens before a launch


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_enumeration_sums_to_k_and_follows_the_weights(k):
    w = sref.DIST_WEIGHTS
    p, sets = sref.inclusion_probabilities(w, k)
    assert abs(p.sum() - k) <= 1e-14 * k and abs(sum(sets.values()) - 1.0) <= 1e-14
    assert p[4] == 0.0 and all(4 not in s and len(s) == k for s in sets)               # the zero weight is never drawn
    order = sorted(range(len(w)), key=lambda i: w[i])
    assert all(p[a] < p[b] for a, b in zip(order, order[1:])) or k == 5                # a larger weight: more likely to be in the batch
    if k == 5:                                                                          # all five positive weights, always
        assert np.allclose(p, [1, 1, 1, 1, 0, 1], atol=1e-14) and len(sets) == 1
    if k == 1:
        assert np.allclose(p, np.asarray(w) / sum(w), atol=1e-16)
    if k == 2:                                                                          # the closed form of a pair
        W = sum(w)
        for s, prob in sets.items():
            i, j = sorted(s)
            assert abs(prob - (w[i] / W * w[j] / (W - w[i]) + w[j] / W * w[i] / (W - w[j]))) <= 1e-15
        assert len(sets) == 10


def test_uniforms_lie_on_the_lattice_inside_the_unit_interval():
    u = sref.uniforms(3, (7 << 32) | 5, 100_000)
    assert u.min() >= 2.0 ** -24 and u.max() <= 1.0 - 2.0 ** -24
    assert np.array_equal(u * sref.LATTICE, np.rint(u * sref.LATTICE)) and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert np.array_equal(u[:10], sref.uniforms(3, (7 << 32) | 5, 10))                  # counter-based: a prefix is a prefix
    assert not np.array_equal(u[:100], sref.uniforms(3, (7 << 32) | 6, 100)) and not np.array_equal(u[:100], sref.uniforms(3, 5, 100))
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / u.size)


def test_keys_pattern():
    u = np.array([0.5, 0.5, 0.5, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -24])
    w = np.array([1.0, 0.0, -2.0, np.nan, 1e-6, 1e3])
    k = sref.keys(u, w)
    assert k[0] == np.log(0.5) and np.isneginf(k[1:4]).all() and np.isfinite(k[4:]).all() and (k[np.isfinite(k)] <= 0).all()
    assert sref.select(k, 3).tolist() == [0, 4, 5] and sref.select(k, 4).tolist() == [0, 1, 4, 5]      # then the lowest-index -inf


@pytest.mark.parametrize("n,k", [(7, 3), (64, 64), (1025, 100), (5000, 4999)])
def test_restated_draw_equals_topk_on_fp64_keys(n, k):
    rng = np.random.default_rng(n + k)
    for stream in (0, 17, (0x53 << 32) | 9):
        w = rng.random(n) + 0.01
        key = sref.keys(sref.uniforms(n, stream, n), w)
        assert np.unique(key).size == n                                                 # no two keys tie: the k largest are one set
        want = torch.topk(torch.from_numpy(key), k).indices.sort().values.numpy()
        assert np.array_equal(sref.draw(n, stream, w, k), want)
        assert np.array_equal(sref.draws(n, stream, 2, w, k)[1], sref.draw(n, stream + 1, w, k))


@pytest.mark.parametrize("k", [2, 3])
def test_restated_draw_has_the_distribution_of_sampling_without_replacement(k):
    """The inputs of the GPU distribution test, through the restatement: within 4 sigma here, so 5 sigma there leaves the kernel room for
    nothing but being right (its draws are these draws unless a float32 key ties or swaps order with its neighbour)."""
    w, B = sref.DIST_WEIGHTS, sref.DIST_DRAWS
    rows = sref.draws(sref.DIST_SEED, sref.DIST_STREAM0, B, w, k)
    assert rows.shape == (B, k) and (np.diff(rows, axis=1) > 0).all()
    p, sets = sref.inclusion_probabilities(w, k)
    f, fsets = sref.frequencies(rows, len(w))
    print(f"k = {k}: f {f}\n p {p}\n |f - p| / sigma {np.abs(f - p)[p > 0] / sref.frequency_bound(p, B, 1.0)[p > 0]}")
    assert f[4] == 0.0
    assert (np.abs(f - p) <= sref.frequency_bound(p, B, 4.0)).all()
    assert set(fsets) <= set(sets)
    for s, prob in sets.items():
        assert abs(fsets.get(s, 0.0) - prob) <= sref.frequency_bound(prob, B, 4.0), (sorted(s), fsets.get(s, 0.0), prob)


def test_refusals_before_any_launch():
    from nerf_for_angiography_amd import _lib, engine
    from nerf_for_angiography_amd._lib import AfxError
    lib = _lib.load()
    n = 100
    ws = int(lib.afx_sample_batches_workspace_bytes(n, 4))
    assert lib.afx_sample_batches(FAKE, n, 0, 0, 4, n + 1, FAKE, FAKE, ws, None) == -1                  # k > n
    assert lib.afx_topk_indices(FAKE, n, n + 1, FAKE, FAKE, 1 << 20, None) == -1
    assert lib.afx_topk_indices(FAKE, n, -1, FAKE, FAKE, 1 << 20, None) == -1
    assert lib.afx_topk_indices(FAKE, n, 5, FAKE, FAKE, int(lib.afx_topk_workspace_bytes(n)) - 1, None) == -2
    o, d, p, w = torch.zeros(n, 3), torch.zeros(n, 3), torch.zeros(n), torch.ones(n)                     # host tensors
    with pytest.raises(AfxError, match="no CPU path"):
        engine.sample_rays(o, d, p, w, 10, seed=1, stream_id=2)
    with pytest.raises(AfxError, match="no CPU path"):
        engine.topk_indices(w, 10)
    with pytest.raises(AfxError, match="no CPU path"):
        engine.RayBatchSampler(o, d, p, w, 10)
    with pytest.raises(AfxError, match="no CPU path"):
        engine.sample_batches_dev(w, 0, torch.zeros((), dtype=torch.int64), 4, 10)
