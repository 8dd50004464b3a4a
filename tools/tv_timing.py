"""Times of afx_tv_denoise_3d, its traffic against the minimum, the NumPy restatement on the host, and SIRT against SIRT-TV on the synthetic
phantom.

Parts (--parts, default kernel,host,phantom):
  kernel   at 64^3 and at 201^3 (the evaluation grid over the +-100 box; the volume is the capsule phantom's density plus Gaussian noise):
           engine.tv_denoise_3d with out and workspace passed, at 10 and at 40 iterations, device events around --reps back-to-back calls
           after two warm-up calls, the median of five such series (min .. max).  Time per iteration = (t40 - t10) / 30 - the last launch,
           which writes out, drops out of the difference.  The least an iteration can move is 56 bytes a voxel (x and three p read,
           three p written); "share" is that traffic over the time against 6.3 TB/s, the HBM rate a streaming copy reaches on the MI355X.
  host     64^3, 10 iterations: tests/tv_reference.py on the host, once, against the device call (host clock around the call and a
           synchronise, median of five); the two volumes must be equal bit for bit.
  phantom  the synthetic capsule phantom's 25 training views of 64^2 (--binary True, angle_grid(180, 4) without the held-out pose), SIRT
           and SIRT-TV at 50 iterations on 101^3 points (rays of 160 samples between 1400 and 1600), no mask: the vessel Dice at the
           threshold 0.1 (half the vessel's density) and at mean(gt), and Pearson's correlation with the truth
           (sweep.reconstruction_sirt_metrics), from the clean line integrals and with Gaussian noise of 10 % of the largest line
           integral added to them, at three weights, 10 inner iterations.  One seed.
  traffic  four iterations at 201^3, once, and nothing else: the run to put under a counter collection, one counter per run
           (rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d DIR -- python tools/tv_timing.py --parts traffic, the same
           with WRITE_SIZE); --counters DIR [DIR ...] then reads the per-dispatch values of k_tv_iterate from the CSV files.
Prints the numbers as one JSON line and, with --out, writes them as a report.

    python tools/tv_timing.py [--reps 5] [--parts kernel,host,phantom] [--counters DIR ...] [--out profiles/tv_numbers.md]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sirt_reference as sr                                                                        # noqa: E402
import tv_reference as tv                                                                          # noqa: E402
from nerf_for_angiography_amd import engine                                                        # noqa: E402
from nerf_for_angiography_amd.phantomdata.helpers import VoxelVolume, capsule_mu, capsule_tree     # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12
MIN_BYTES_PER_VOXEL = 56


def spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def event_ms(fn, reps, series=5):
    """ms per call from device events around `reps` back-to-back calls; the median, min and max of `series` such series."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(series):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return spread(out)


def noisy_phantom(n, sigma=0.04, seed=0):
    """The capsule phantom's density (0.2 in the vessel) on n^3 points over the +-100 box plus Gaussian noise, float64 on the device."""
    from nerf_for_angiography_amd.visualization.sweep import grid_index_to_world
    caps = capsule_tree(levels=5, seed=0)
    x = torch.from_numpy(sr.lattice_points((n,) * 3, grid_index_to_world(100.0, n))).to(DEV)
    mu = torch.cat([capsule_mu(x[i:i + (1 << 20)], caps) for i in range(0, x.shape[0], 1 << 20)]).to(torch.float64).reshape(n, n, n)
    g = torch.Generator(device=DEV).manual_seed(seed)
    return mu + sigma * torch.randn(mu.shape, dtype=torch.float64, device=DEV, generator=g)


def part_kernel(reps):
    rows = []
    for n in (64, 201):
        x = noisy_phantom(n)
        out, work = torch.empty_like(x), engine.tv_denoise_3d_workspace(x.shape, DEV)
        t10 = event_ms(lambda: engine.tv_denoise_3d(x, 0.02, 10, out=out, workspace=work), reps)
        t40 = event_ms(lambda: engine.tv_denoise_3d(x, 0.02, 40, out=out, workspace=work), reps)
        t0 = event_ms(lambda: engine.tv_denoise_3d(x, 0.02, 0, out=out), reps)
        engine.tv_denoise_3d(x, 0.02, 40, out=out, workspace=work)
        per_iteration_ms = (t40["median"] - t10["median"]) / 30.0
        rate = MIN_BYTES_PER_VOXEL * x.numel() / (per_iteration_ms * 1e-3)
        rows.append(dict(points=n, voxels=x.numel(), volume_mb=round(x.numel() * 8 / 1e6, 1), working_set_mb=round(x.numel() * 56 / 1e6, 1),
                         call_10_iterations_ms=t10, call_40_iterations_ms=t40, last_launch_alone_ms=t0,
                         per_iteration_us=round(per_iteration_ms * 1e3, 2), min_bytes_per_voxel=MIN_BYTES_PER_VOXEL,
                         min_traffic_tb_per_s=round(rate / 1e12, 3), share_of_hbm_rate=round(rate / HBM_BYTES_PER_S, 3),
                         tv_before=float(engine.total_variation_3d(x)), tv_after_40=float(engine.total_variation_3d(out))))
        print(rows[-1], flush=True)
    return rows


def part_host(n=64, iterations=10):
    x = noisy_phantom(n)
    out, work = torch.empty_like(x), engine.tv_denoise_3d_workspace(x.shape, DEV)
    times = []
    for _ in range(6):
        torch.cuda.synchronize()
        t = time.perf_counter()
        engine.tv_denoise_3d(x, 0.02, iterations, out=out, workspace=work)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    host = x.cpu().numpy()
    t = time.perf_counter()
    want = tv.tv_denoise(host, 0.02, iterations)
    host_ms = (time.perf_counter() - t) * 1e3
    equal = bool(np.array_equal(out.cpu().numpy().view(np.int64), want.view(np.int64)))
    row = dict(points=n, iterations=iterations, device_ms=spread(times[1:], 3), host_ms=round(host_ms, 1), bit_equal=equal)
    print(row, flush=True)
    return row


def part_phantom(n=101, iterations=50, weights=(1e-4, 3e-4, 1e-3), tv_iterations=10):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import training_view_images
    from nerf_for_angiography_amd.phantomdata import dataset as ds
    from nerf_for_angiography_amd.visualization import sweep
    proj_df, ray_df = ds.make_synthetic_dataset(ds.angle_grid(180.0, 4, [90, 0]), img_size=64, sampling_strategy="segmentation", device=DEV, seed=0,
                                                binary=True)
    held_out = proj_df.index[-1]
    poses, images, focal = training_view_images(proj_df, ray_df[ray_df["image_id"] != held_out], held_out, DEV)
    views = engine.xray_views(poses, focal, images.shape[2], images.shape[1], 1400.0, 1600.0, 160, device=DEV)
    t = np.linspace(-100.0, 100.0, 129)
    nodes = torch.from_numpy(np.stack(np.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)).to(DEV)
    caps = capsule_tree(levels=5, seed=0)
    mu = torch.cat([capsule_mu(nodes[i:i + (1 << 20)], caps) for i in range(0, nodes.shape[0], 1 << 20)]).cpu().numpy().reshape(129, 129, 129)
    gt = sweep.ground_truth_grid(VoxelVolume(t, t, t, mu, fill_value=0.0, device=DEV), 100.0, n)
    clean = engine.line_integrals(images)
    g = torch.Generator(device=DEV).manual_seed(0)
    noise = 0.1 * float(clean.max()) * torch.randn(clean.shape, dtype=torch.float64, device=DEV, generator=g)
    rows = []
    for name, b in (("clean", clean), ("noise of 10 % of the largest line integral", clean + noise)):
        an = sweep.GridAnalysis(gt, gt, 100.0, n)          # (no model: the truth stands in for the predicted grid, whose scores are not read)
        for threshold in (0.1, None):
            for w in weights:
                s = sweep.reconstruction_sirt_metrics(None, None, 100.0, n, views, b, iterations=iterations, threshold=threshold, grids=an,
                                                      tv_weight=w, tv_iterations=tv_iterations)[0]
                rows.append(dict(images=name, threshold=s["threshold"], tv_weight=w, tv_iterations=tv_iterations, iterations=iterations,
                                 dice_sirt=s["dice_sirt"], dice_sirt_tv=s["dice_sirt_tv"], tv_gain=s["tv_gain"], corr_sirt=s["corr_sirt"],
                                 corr_sirt_tv=s["corr_sirt_tv"], n_gt=s["n_gt"], n_sirt=s["n_sirt"], n_sirt_tv=s["n_sirt_tv"]))
                print(rows[-1], flush=True)
    return dict(points=n, views=int(views["n_views"]), detector=int(images.shape[2]), rows=rows)


def part_traffic(n=201, iterations=4):
    x = noisy_phantom(n)
    out, work = torch.empty_like(x), engine.tv_denoise_3d_workspace(x.shape, DEV)
    engine.tv_denoise_3d(x, 0.02, iterations, out=out, workspace=work)
    torch.cuda.synchronize()
    return dict(points=n, iterations=iterations)


def read_counters(dirs, voxels=201 ** 3):
    """Per dispatch of k_tv_iterate: the values of every counter in the counter_collection CSV files under `dirs`, as rocprofv3 gives
    them, and per voxel.  (FETCH_SIZE and WRITE_SIZE count kilobytes at the L2's memory side.)"""
    per = {}
    for d in dirs:
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(f) as fh:
                for row in csv.DictReader(fh):
                    if "k_tv_iterate" in row.get("Kernel_Name", ""):
                        per.setdefault(row["Counter_Name"], {}).setdefault(row.get("Dispatch_Id", "?"), 0.0)
                        per[row["Counter_Name"]][row.get("Dispatch_Id", "?")] += float(row["Counter_Value"])
    return {name: dict(dispatches=len(v), per_dispatch=[round(x, 1) for x in v.values()],
                       kb_per_dispatch_median=statistics.median(v.values()),
                       bytes_per_voxel_median=round(statistics.median(v.values()) * 1024 / voxels, 2)) for name, v in per.items()}


def main_cli():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="kernel,host,phantom")
    ap.add_argument("--counters", nargs="*", default=None, metavar="DIR")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {}
    if args.counters is not None:
        result["counters"] = read_counters(args.counters)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("tv_timing: needs an MI355X; nothing is measured without one")
        parts = args.parts.split(",")
        if "kernel" in parts:
            result["kernel"] = part_kernel(args.reps)
        if "host" in parts:
            result["host"] = part_host()
        if "phantom" in parts:
            result["phantom"] = part_phantom()
        if "traffic" in parts:
            result["traffic"] = part_traffic()
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# TV denoising numbers (tools/tv_timing.py)\n\n```json\n" + json.dumps(result, indent=1) + "\n```\n")


if __name__ == "__main__":
    main_cli()
