"""Time of the feature transform and of the per-label overlap counts at 201^3 voxels (the reference's depth_samples_per_ray + 1) on the
GPU, against the 3-D EDT of the same inputs in the same run and against SciPy's distance_transform_edt(return_indices=True) on the host.

What is measured: `afx_feature_transform_3d` (engine.feature_transform_record into caller buffers: three launches, nothing allocated) on a
centreline-like site set (`--segments` straight voxel lines, a few thousand sites) and on a dense one (every second voxel at random);
`afx_distance_transform_edt_3d` on the inverted masks, called with its own caller buffers and no fp64 output, so that both write their
integer results only; `afx_label_overlap_3d` (engine.label_overlap_record) over the territories of the centreline-like set with one label
per segment and with a single label.  The two transforms alternate inside one loop.  Every repetition is bracketed by device events;
the report gives the median, the minimum and the maximum over `--reps` repetitions after `--warmup` calls.  The host runs SciPy once.
Bytes per voxel are counted from the kernels' loads and stores (every element a kernel addresses once, whatever the caches absorb).
Writes a small report (default profiles/r29_branch_territories.md) and prints the same numbers as one JSON line.
    python tools/branch_territories_timing.py [--reps 50] [--warmup 3] [--points 201] [--segments 50] [--out profiles/r29_branch_territories.md]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_for_angiography_amd import _lib                                                         # noqa: E402
from nerf_for_angiography_amd.engine import Engine, feature_transform_record, label_overlap_record      # noqa: E402

# bytes a voxel costs, counted from the kernels (axis 2: both sweeps; then the two line passes), against the least a transform could move
FT_BYTES = {"axis 2": 1 + 8 + 1 + 4 + 8, "axis 1": 8 + 8, "axis 0": 8 + 8, "least": 1 + 8}
EDT_BYTES = {"axis 2": 1 + 2 + 2 + 2, "axis 1": 2 + 4, "axis 0": 4 + 4, "least": 1 + 4}


def stats(fns, reps, warmup):
    """Median, minimum and maximum device time (ms) of each function of `fns`, the functions alternating inside one loop."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}


def segments(n, count, seed=0):
    """`count` straight voxel lines through the middle of an n^3 box -> int32 [n, n, n]: 0, or the number (1..count) of the line."""
    rng = np.random.default_rng(seed)
    labels = np.zeros((n, n, n), np.int32)
    for s in range(1, count + 1):
        p, q = rng.uniform(0.15 * n, 0.85 * n, 3), rng.uniform(0.15 * n, 0.85 * n, 3)
        t = np.linspace(0.0, 1.0, 2 * n)[:, None]
        v = np.rint(p + t * (q - p)).astype(np.int64)
        labels[v[:, 0], v[:, 1], v[:, 2]] = s
    return labels


def edt_call(lib, fg, d2, ws):
    n0, n1, n2 = fg.shape
    ptr = lambda t: C.c_void_p(t.data_ptr())
    def run():
        _lib.check(lib.afx_distance_transform_edt_3d(ptr(fg), n0, n1, n2, ptr(d2), None, ptr(ws), ws.numel(), None, Engine._stream(fg.device)),
                   "afx_distance_transform_edt_3d")
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=201)
    ap.add_argument("--segments", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_branch_territories.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("branch_territories_timing: needs a GPU; a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = a.points
    shape = (n, n, n)
    seg = segments(n, a.segments)
    dense = np.random.default_rng(1).random(shape) < 0.5
    res = {"points": n, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "sites_centreline": int((seg > 0).sum()),
           "sites_dense": int(dense.sum())}
    d2, near, d2_edt = (torch.empty(shape, dtype=torch.int32, device=dev) for _ in range(3))
    ws = torch.empty(int(lib.afx_distance_transform_edt_3d_workspace_bytes(n, n, n)), dtype=torch.uint8, device=dev)
    for name, sites_np in (("centreline", seg > 0), ("dense", dense)):
        sites = torch.from_numpy(sites_np).to(dev).to(torch.uint8)
        inverted = (1 - sites).contiguous()
        got = stats({"ft": lambda: feature_transform_record(sites, d2, near), "edt": edt_call(lib, inverted, d2_edt, ws)}, a.reps, a.warmup)
        res[f"ft_{name}_ms"], res[f"edt_{name}_ms"] = got["ft"], got["edt"]
        res[f"ratio_{name}"] = round(got["ft"]["median"] / got["edt"]["median"], 3)
        res[f"d2_equal_{name}"] = bool(torch.equal(d2, d2_edt))
        flat, lin = near.reshape(-1).to(torch.int64), torch.arange(n ** 3, device=dev)
        away = (lin // (n * n) - flat // (n * n)) ** 2 + (lin // n % n - flat // n % n) ** 2 + (lin % n - flat % n) ** 2
        res[f"nearest_is_a_site_at_d2_{name}"] = bool(sites.reshape(-1)[flat].all()) and bool(torch.equal(away, d2.reshape(-1).to(torch.int64)))
        t = time.perf_counter()
        from scipy import ndimage
        dist, idx = ndimage.distance_transform_edt(~sites_np, return_indices=True)
        res[f"host_scipy_{name}_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        host_d2 = np.rint(dist ** 2).astype(np.int64)
        res[f"d2_equals_scipy_{name}"] = bool(np.array_equal(d2.cpu().numpy().astype(np.int64) & 0xffffffff, host_d2))
        lin = np.ravel_multi_index(tuple(idx), shape)
        res[f"nearest_differs_from_scipy_{name}"] = int((near.cpu().numpy() != lin).sum())      # ties only: SciPy's rule is not the lowest index
    # the overlap counts over the territories of the centreline-like set
    sites = torch.from_numpy(seg > 0).to(dev).to(torch.uint8)
    feature_transform_record(sites, d2, near)
    a_mask = ((d2 >= 0) & (d2 <= 9)).to(torch.uint8)
    b_mask = torch.roll(a_mask, 1, 0).contiguous()
    terr = torch.empty(shape, dtype=torch.int32, device=dev)
    for name, labels_np, n_labels in (("50", seg, a.segments), ("1", (seg > 0).astype(np.int32), 1)):
        labels = torch.from_numpy(labels_np).to(dev)
        counts = torch.empty((n_labels + 1, 4), dtype=torch.int64, device=dev)
        got = stats({"overlap": lambda: label_overlap_record(labels, a_mask, n_labels, b_mask, near, d2, 400, counts, terr)}, a.reps, a.warmup)
        res[f"overlap_{name}_labels_ms"] = got["overlap"]
        res[f"overlap_{name}_rows_sum"] = int(counts[:, 0].sum())
    res["overlap_bytes_per_voxel"] = 4 + 4 + 4 + 1 + 1 + 4      # index, d2, one label, a, b, territory
    nvox = n ** 3
    ft_b, edt_b = sum(v for k, v in FT_BYTES.items() if k != "least"), sum(v for k, v in EDT_BYTES.items() if k != "least")
    res["ft_bytes_per_voxel"], res["edt_bytes_per_voxel"] = ft_b, edt_b
    row = lambda what, s: f"| {what} | {s['median']} | {s['min']} | {s['max']} |"
    gbs = lambda b, s: round(b * nvox / (s["median"] * 1e-3) / 1e9, 1)
    lines = [f"# Feature transform and label overlap at {n}^3 voxels", "",
             f"`tools/branch_territories_timing.py --reps {a.reps} --warmup {a.warmup} --points {n} --segments {a.segments}` on {res['device']}.",
             f"Device times are per call between two device events, median / minimum / maximum over {a.reps} repetitions after {a.warmup}",
             "warm-up calls, the feature transform and the EDT alternating in one loop, all buffers allocated beforehand; the EDT writes its",
             "integer output only.  Host times are one run of SciPy.  No gate depends on these numbers.", "",
             "| what | median (ms) | min | max |", "|---|---|---|---|",
             row(f"feature transform, centreline-like ({res['sites_centreline']} sites)", res["ft_centreline_ms"]),
             row("3-D EDT, same input", res["edt_centreline_ms"]),
             row(f"feature transform, dense ({res['sites_dense']} sites)", res["ft_dense_ms"]),
             row("3-D EDT, same input", res["edt_dense_ms"]),
             row(f"label overlap, {a.segments} labels (index, d2, a, b, territory)", res[f"overlap_50_labels_ms"]),
             row("label overlap, 1 label", res["overlap_1_labels_ms"]), "",
             f"Ratio feature transform / EDT (medians): centreline-like {res['ratio_centreline']}, dense {res['ratio_dense']}.",
             f"SciPy `distance_transform_edt(return_indices=True)` on the host: {res['host_scipy_centreline_ms']} ms (centreline-like), "
             f"{res['host_scipy_dense_ms']} ms (dense).", "",
             f"Bytes addressed per voxel, counted from the kernels: feature transform {ft_b} (axis 2: {FT_BYTES['axis 2']}, the two line passes "
             f"{FT_BYTES['axis 1']} each) against {FT_BYTES['least']} at the least (the mask in, two 4-byte fields out); EDT {edt_b} against "
             f"{EDT_BYTES['least']}; label overlap {res['overlap_bytes_per_voxel']}, all of them needed.  At the medians that is "
             f"{gbs(ft_b, res['ft_centreline_ms'])} / {gbs(ft_b, res['ft_dense_ms'])} GB/s for the feature transform (centreline-like / dense), "
             f"{gbs(edt_b, res['edt_centreline_ms'])} / {gbs(edt_b, res['edt_dense_ms'])} GB/s for the EDT, "
             f"{gbs(res['overlap_bytes_per_voxel'], res['overlap_50_labels_ms'])} / {gbs(res['overlap_bytes_per_voxel'], res['overlap_1_labels_ms'])} "
             f"GB/s for the overlap ({a.segments} labels / 1 label).", "",
             f"d2 equals the EDT's: {res['d2_equal_centreline']} / {res['d2_equal_dense']}; every nearest site is a site at exactly d2: "
             f"{res['nearest_is_a_site_at_d2_centreline']} / {res['nearest_is_a_site_at_d2_dense']}; d2 equals SciPy's squared: "
             f"{res['d2_equals_scipy_centreline']} / {res['d2_equals_scipy_dense']}; voxels whose nearest site differs from SciPy's (ties: SciPy "
             f"does not take the lowest index): {res['nearest_differs_from_scipy_centreline']} / {res['nearest_differs_from_scipy_dense']}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
