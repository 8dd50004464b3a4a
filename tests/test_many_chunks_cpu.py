"""The inputs of tests/test_gpu_many_chunks.py (tests/many_chunks_cases.py; no GPU needed) reach what they are there for: every case leaves
MORE THAN 1024 PARTIALS to the one scanning workgroup of its kernels, so each of its 1024 threads walks a run of per > 1 partials, and the
partials are not empty.  The chunk sizes are read from the kernel sources: a change there cannot silently put the cases back under 1024.
A Python model of the two-level scan shows that a wrong prefix for a thread's second partial changes the answer at these sizes and at
none of the sizes the other test modules use."""
import numpy as np
import pytest

import components_reference as cr
import many_chunks_cases as mc


@pytest.mark.parametrize("name", sorted(mc.CHUNKS))
def test_chunk_constants_are_those_of_the_sources(name):
    assert mc.source_constant(name) == mc.CHUNKS[name][1], name


def test_the_scanning_workgroups_have_1024_threads():
    """The launches of the scans: dim3(1024), or ISO_SCAN = 1024, with one run of ceil(nb / 1024) partials per thread."""
    for file, kernel in (("afx_kernels_metrics.hip", "k_cc_scan"), ("afx_kernels_graph.hip", "k_cg_scan_chunks"), ("afx_api.hip", "k_sel_offsets"),
                         ("afx_api.hip", "k_grid_occ_scan")):
        text = (mc.CSRC / file).read_text()
        launches = [line for line in text.splitlines() if "hipLaunchKernelGGL(" + kernel + "," in line]
        assert launches and all(f"dim3({mc.SCAN_THREADS})" in line for line in launches), (kernel, launches)
    mesh = (mc.CSRC / "afx_kernels_mesh.hip").read_text()
    assert f"constexpr int ISO_SCAN = {mc.SCAN_THREADS};" in mesh and "hipLaunchKernelGGL(k_iso_scan, dim3(1), dim3(ISO_SCAN)" in mesh


def test_partial_count_formulas():
    assert mc.partials_volume(2048) == 1 and mc.partials_volume(2049) == 2 and mc.partials_isosurface(1025) == 2
    assert mc.partials_sampler(900_000) == 879 and mc.partials_grid(128 ** 3) == 256 and mc.partials_volume(65 * 64 * 63) == 128
    assert mc.partials_grid(33) == 1 and mc.partials_grid(32 * 256 + 1) == 2
    assert mc.run_length(1024) == 1 and mc.run_length(1025) == 2 and mc.run_length(2049) == 3


@pytest.mark.parametrize("name", sorted(mc.VOLUMES))
def test_volumes_have_more_than_1024_partials_and_fill_them(name):
    m = mc.volume(name)
    assert m.shape == mc.VOLUMES[name] and m.dtype == bool and max(m.shape) <= 1024
    nb, nb_iso = mc.partials_volume(m.size), mc.partials_isosurface(m.size)
    assert nb > mc.SCAN_THREADS and mc.run_length(nb) == 2
    assert nb_iso > 2 * mc.SCAN_THREADS and mc.run_length(nb_iso) == 3
    assert m.flat[0] and m.flat[-1]
    occupied = mc.chunk_occupancy(m, mc.CC_CHUNK)
    assert occupied.size == nb and 2 * occupied.sum() >= nb, (int(occupied.sum()), nb)
    assert occupied[mc.SCAN_THREADS:].all() and occupied[-1]           # the chunks behind the first 1024, and the last one
    assert cr.label(m, 3)[1] > mc.SCAN_THREADS                         # components at 26 neighbours (fewer than at 18 or 6)
    assert m.sum() < 0.02 * m.size                                     # sparse: the host references stay at a second
    if name == "3x700x1001":                                           # a ragged last chunk; the last scanning thread's run is short
        assert m.size % mc.CC_CHUNK and m.size % mc.ISO_CHUNK
        per = mc.run_length(nb_iso)
        last_thread = (nb_iso - 1) // per
        assert 0 < nb_iso - last_thread * per < per


def test_grid_case_has_more_than_1024_workgroup_totals():
    n = mc.GRID_RES[0] * mc.GRID_RES[1] * mc.GRID_RES[2]
    assert n == 8_454_144 and mc.partials_grid(n) == 1032 and mc.run_length(mc.partials_grid(n)) == 2
    dense, few = mc.grid_mask("bernoulli"), mc.grid_mask("few")
    assert dense.size == few.size == n
    small, large = mc.GRID_DRAWS
    assert small < int(dense.sum()) < large == n // 4                  # a ranked draw at the small n_draw, all of them at the large one
    assert int(few.sum()) == mc.GRID_FEW < small and few[0] and few[-1]      # "all of them, in index order" at both
    for m in (dense, few):                                             # occupied cells behind the first 1024 workgroup totals
        assert m[mc.SCAN_THREADS * mc.SEL_WORDS * 32:].any()
    occupied = mc.chunk_occupancy(dense, mc.SEL_WORDS * 32)
    assert occupied.all()


@pytest.mark.parametrize("n", mc.SAMPLER_SIZES)
def test_sampler_sizes_have_more_than_1024_partials(n):
    nb = mc.partials_sampler(n)
    assert nb > mc.SCAN_THREADS and mc.run_length(nb) == (2 if n == mc.SAMPLER_SIZES[0] else 3)
    assert n % mc.SEL_PER_BLOCK and n % 4                               # a ragged last block, a ragged last thread in it
    if n == mc.SAMPLER_SIZES[1]:
        per = mc.run_length(nb)
        assert 0 < nb - (nb - 1) // per * per < per                    # the last run is short
    for k in mc.sampler_ks(n):
        assert 1 <= k <= n


def test_topk_reference_on_a_hand_made_array():
    keys = np.array([1.0, 3.0, 3.0, -np.inf, 2.0, 3.0, -np.inf], np.float32)
    assert mc.topk_reference(keys, 2).tolist() == [1, 2]               # the tie is cut in index order
    assert mc.topk_reference(keys, 4).tolist() == [1, 2, 4, 5]
    assert mc.topk_reference(keys, 6).tolist() == [0, 1, 2, 3, 4, 5] and mc.topk_reference(keys, 7).tolist() == list(range(7))


# ---- a model of the two-level scan: what a wrong second level does, and where it shows
def _scan_model(partials, wrong=None):
    """The exclusive scan of `partials` as the one scanning workgroup forms it: thread t sums its run of per = ceil(nb / 1024) partials, the
    1024 thread sums are scanned, and the thread walks its run again from its exclusive prefix.  wrong = "prefix": every partial of a
    run gets the run's prefix (the second chunk starts where the first did); wrong = "bound": per is taken as 1."""
    partials = np.asarray(partials, np.int64)
    nb = partials.size
    per = 1 if wrong == "bound" else mc.run_length(nb)
    out = np.zeros(nb, np.int64)
    sums = [int(partials[t * per:(t + 1) * per].sum()) for t in range(mc.SCAN_THREADS)]
    prefix = np.concatenate([[0], np.cumsum(sums)[:-1]])
    for t in range(mc.SCAN_THREADS):
        p = int(prefix[t])
        for b in range(min(t * per, nb), min((t + 1) * per, nb)):
            out[b] = p
            if wrong != "prefix":
                p += int(partials[b])
    return out


def _roots_per_chunk(mask, c, chunk):
    """What k_cc_flatten leaves per chunk: the components whose first voxel in raster order lies in it."""
    labels, k = cr.label(mask, c)
    flat = labels.reshape(-1)
    first = np.full(k + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    return np.bincount(first[1:] // chunk, minlength=mc.partials_volume(flat.size))


@pytest.mark.parametrize("name", sorted(mc.VOLUMES))
def test_a_wrong_second_level_changes_the_labels_here_and_nowhere_else(name):
    roots = _roots_per_chunk(mc.volume(name), 3, mc.CC_CHUNK)
    want = np.concatenate([[0], np.cumsum(roots)[:-1]])
    assert np.array_equal(_scan_model(roots), want)
    for wrong in ("prefix", "bound"):
        got = _scan_model(roots, wrong)
        bad = (got != want) & (roots > 0)                              # a chunk with a root and a wrong prefix: wrong labels from there on
        assert bad.any(), wrong
    rng = np.random.default_rng(1)
    for nb in (128, 256, 879, 1024):                                   # the most partials the other test modules reach: the model cannot tell
        small = rng.integers(0, 9, nb)
        for wrong in ("prefix", "bound"):
            assert np.array_equal(_scan_model(small, wrong), _scan_model(small)), (nb, wrong)
