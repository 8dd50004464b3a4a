"""Time of the surface-distance scores at 201^3 points (the reference's depth_samples_per_ray + 1) on the GPU against their SciPy
restatement on the host (tests/surface_reference.py: two distance_transform_edt, two binary_erosion, one np.percentile).

What is measured: two synthetic vessel trees (a few tubes, the second one moved by a voxel or two) as fp32 density grids resident on the
device; `engine.surface_metrics_3d` - the whole call, its 128-byte read-back included - as wall time around a synchronised loop of
`--reps` calls after one warm-up; `engine.distance_transform_edt_3d` alone on the distance-to-surface mask the same way; the host
restatement once, wall time.  It also compares the scores of both.  Writes a small report (default profiles/r12_surface_metrics.md)
and prints the same numbers as one JSON line.
    python tools/surface_metrics_timing.py [--reps 10] [--points 201] [--out profiles/r12_surface_metrics.md]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import surface_reference as sr                                                                    # noqa: E402
from nerf_for_angiography_amd.engine import distance_transform_edt_3d, surface_metrics_3d        # noqa: E402


def gpu_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def tree(n, shift, seed=0):
    """A density grid [n, n, n] (fp32, 0..1) of six smooth-edged tubes through the middle of the box, moved by `shift` voxels."""
    ax = np.arange(n, dtype=np.float32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    rng = np.random.default_rng(seed)
    mu = np.zeros((n, n, n), np.float32)
    for _ in range(6):
        p = rng.uniform(0.35 * n, 0.65 * n, 3).astype(np.float32) + np.asarray(shift, np.float32)
        d = rng.normal(size=3).astype(np.float32)
        d /= np.linalg.norm(d)
        vx, vy, vz = x - p[0], y - p[1], z - p[2]
        along = vx * d[0] + vy * d[1] + vz * d[2]
        r = np.sqrt(np.maximum(vx * vx + vy * vy + vz * vz - along * along, 0))
        mu = np.maximum(mu, 1 / (1 + np.exp(np.minimum((r - np.float32(rng.uniform(1.5, 4))) / np.float32(0.7), 60))))      # exp(60) stays in fp32
    return mu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=201)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_surface_metrics.md"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.points
    pred, gt = tree(n, (1.3, -0.8, 2.1)), tree(n, (0.0, 0.0, 0.0))
    dp, dg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    res = {"points": n, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    res["device_surface_metrics_ms"] = round(gpu_ms(lambda: surface_metrics_3d(dp, dg, 0.5, 0.5), a.reps), 3)
    not_surface = torch.from_numpy(~sr.surface(gt >= 0.5)).to(dev)
    res["device_edt_3d_ms"] = round(gpu_ms(lambda: distance_transform_edt_3d(not_surface), a.reps), 3)
    got = surface_metrics_3d(dp, dg, 0.5, 0.5)
    t = time.perf_counter()
    want = sr.surface_metrics(pred, gt, 0.5, 0.5)
    res["host_scipy_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    t = time.perf_counter()
    host_edt = sr.edt(not_surface.cpu().numpy())
    res["host_scipy_one_edt_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    res["edt_bit_identical"] = bool(np.array_equal(distance_transform_edt_3d(not_surface).cpu().numpy(), host_edt))
    res["vessel_fraction"] = got["n_gt"] / n ** 3
    for key in ("dice_vessel", "assd", "hd", "hd_percentile"):
        res[key], res[key + "_host"] = got[key], want[key]
    res["counts_equal"] = all(got[k] == want[k] for k in ("n_pred", "n_gt", "n_overlap", "n_surface_pred", "n_surface_gt"))
    lines = [f"# Surface-distance scores at {n}^3 points: GPU against the SciPy restatement", "",
             f"`tools/surface_metrics_timing.py --reps {a.reps} --points {n}` on {res['device']}.  Two synthetic vessel trees (six tubes, the",
             f"prediction moved by (1.3, -0.8, 2.1) voxels), thresholds 0.5; the vessel class fills {100 * res['vessel_fraction']:.2f} % of the grid.",
             "Device times are wall time per call over a synchronised loop after one warm-up (allocations and, for the metric, the 128-byte",
             "read-back included); host times are one run of tests/surface_reference.py.  No gate depends on these numbers.", "",
             "| what | GPU (ms) | host SciPy (ms) |", "|---|---|---|",
             f"| surface metrics (2 EDTs, surfaces, sums, maxima, percentile) | {res['device_surface_metrics_ms']} | {res['host_scipy_ms']} |",
             f"| one 3-D EDT (`distance_transform_edt_3d`, fp64 out) | {res['device_edt_3d_ms']} | {res['host_scipy_one_edt_ms']} |", "",
             "| score | GPU | host |", "|---|---|---|"]
    lines += [f"| {k} | {res[k]!r} | {res[k + '_host']!r} |" for k in ("dice_vessel", "assd", "hd", "hd_percentile")]
    lines += ["", f"Counts equal: {res['counts_equal']}; EDT bit-identical to SciPy: {res['edt_bit_identical']}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
