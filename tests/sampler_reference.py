"""The ray sampler's Philox-mode draw restated from its definition (include/afx.h: afx_sample_keys, afx_topk_indices, afx_sample_batches;
the comment above k_sample_keys), and the distribution it must have: the yardstick of tests/test_sampler_cpu.py and
tests/test_gpu_sampler.py.

  u_i   = max(u24_i, 1) / 2^24, u24_i = the top 24 bits of number i of the Philox4x32-10 stream (seed, stream id)
  key_i = log(u_i) / w_i for w_i > 0, else -inf                                    (Efraimidis-Spirakis, log form)
  draw  = the k largest keys, ties to the lowest index, in ascending index order

The k largest keys of independent u are a weighted sample without replacement: k successive draws, each with probabilities
proportional to the weights of what is left.  inclusion_probabilities() enumerates that process exactly."""
import functools
import itertools

import numpy as np

from test_grid_refresh_cpu import philox_u24

LATTICE = 1 << 24
DIST_WEIGHTS = (1.0, 2.0, 3.0, 4.0, 0.0, 10.0)      # the distribution test: n = 6, one zero weight, k = 2 and k = 3
DIST_DRAWS = 20000                                  # draws of consecutive stream ids in one afx_sample_batches call
DIST_SEED, DIST_STREAM0 = 2024, 1000


def uniforms(seed, stream, n):
    """float64 [n]: the sampler's u - the stream's numbers on the 2^-24 lattice, 0 replaced by 2^-24.  Every value is a float32 too."""
    return np.maximum(philox_u24(seed, stream, n), 1).astype(np.float64) / LATTICE


def keys(u, w):
    """float64 keys log(u) / w; -inf where the weight is zero, negative or NaN."""
    u, w = np.asarray(u, np.float64), np.asarray(w, np.float64)
    ok = w > 0                                        # False for NaN
    out = np.full(u.shape, -np.inf)
    out[ok] = np.log(u[ok]) / w[ok]
    return out


def select(key, k):
    """The k largest keys, ties to the lowest index, in ascending index order (int64).  The keys hold no NaN."""
    order = np.argsort(-np.asarray(key, np.float64), kind="stable")
    return np.sort(order[:k]).astype(np.int64)


def draw(seed, stream, w, k):
    """The restated draw of stream (seed, stream) from the weights w, with fp64 keys."""
    w = np.asarray(w)
    return select(keys(uniforms(seed, stream, w.size), w), k)


@functools.lru_cache(maxsize=4)
def batch_uniforms(seed, stream0, n_batches, n):
    """float64 [n_batches, n]: row b holds the u of stream id stream0 + b (afx_sample_batches)."""
    return np.stack([uniforms(seed, stream0 + b, n) for b in range(n_batches)])


def draws(seed, stream0, n_batches, w, k):
    """int64 [n_batches, k]: row b is draw(seed, stream0 + b, w, k)."""
    w = np.asarray(w)
    key = keys(batch_uniforms(seed, stream0, n_batches, w.size), np.broadcast_to(w, (n_batches, w.size)))
    return np.sort(np.argsort(-key, axis=1, kind="stable")[:, :k], axis=1).astype(np.int64)


def inclusion_probabilities(w, k):
    """Successive weighted sampling without replacement, enumerated in fp64: every ordered k-tuple of distinct indices with positive
    weight has probability prod_j w_(i_j) / (W - w_(i_1) - ... - w_(i_(j-1))).  -> (p [n]: the probability that index i is among the k,
    sets: {frozenset of k indices: probability})."""
    w = [float(x) for x in w]
    positive = [i for i, x in enumerate(w) if x > 0]
    assert k <= len(positive)
    p, sets = np.zeros(len(w)), {}
    for seq in itertools.permutations(positive, k):
        left, prob = sum(w[i] for i in positive), 1.0
        for i in seq:
            prob *= w[i] / left
            left -= w[i]
        for i in seq:
            p[i] += prob
        sets[frozenset(seq)] = sets.get(frozenset(seq), 0.0) + prob
    return p, sets


def frequency_bound(p, n_draws, sigmas=5.0):
    """|f - p| of a frequency over n_draws independent draws lies within `sigmas` standard deviations sqrt(p (1 - p) / n_draws) with
    probability 1 - 6e-7 at 5 sigma (the normal tail; the exact binomial tail is no heavier at these p and n_draws).  The 2^-24 lattice
    of u moves p by less than n 2^-24, four orders below the bound at 20 000 draws."""
    p = np.asarray(p, np.float64)
    return sigmas * np.sqrt(p * (1.0 - p) / n_draws)


def frequencies(rows, n):
    """(f [n]: the share of rows that hold index i, {frozenset(row): share}) of an int [B, k] array of draws."""
    rows = np.asarray(rows)
    f = np.bincount(rows.reshape(-1), minlength=n) / rows.shape[0]
    sets = {}
    for r in rows:
        key = frozenset(int(x) for x in r)
        sets[key] = sets.get(key, 0) + 1
    return f, {s: c / rows.shape[0] for s, c in sets.items()}
