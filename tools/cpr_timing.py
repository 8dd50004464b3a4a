"""Time of the curved-planar reformation (afx_reformat_planes) on the GPU.

Two inputs: the capsule tree of the skeleton tests at --points^3 (default 201, the evaluation grid's size) and the 64^3 tree.  The volume
is the tree's mask averaged over 3 x 3 x 3 voxels (a density with a soft wall), the path the main path of the pruned skeleton of the mask
read as a graph (`engine.centreline_main_path`), smoothed (8 passes) and resampled at one voxel; step half a voxel, K = 65 samples across.
Reported per input:
  * the straightened volume [P, 65, 65] and the four longitudinal images [4, P, 65] (0, 45, 90, 135 degrees): `engine.reformat_planes_record`
    on buffers allocated once - the launch only - and `engine.straighten_volume` / `engine.cpr_images` as a user calls them (frames on the
    host, upload, allocation, launch, and for the volume the un-permutation); samples per second of the launch, the share of samples
    inside the box;
  * the cross-section table in row order against 8 x 8 tiles, the launch only, three medians each, the two alternating - on the path's
    planes, and on the same planes 32 times over in one launch (the path alone is a launch of a few microseconds of work);
  * the longitudinal images with half_slab 0 against 4 (9 lookups per sample), mean mode;
  * at 64^3: one run of the NumPy restatement on the host (tests/reformat_reference.py), and whether the device equals it.
Every GPU time is the median of --reps calls (min .. max), each call timed by a host clock around the call and a device synchronise, after
two warm-up calls.  Writes a small report (default profiles/r27_cpr.md) and prints the same numbers as one JSON line.

    python tools/cpr_timing.py [--reps 20] [--points 201] [--out profiles/r27_cpr.md]"""
import argparse
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
import reformat_reference as rr                                                                    # noqa: E402
import skeleton_reference as sk                                                                    # noqa: E402
from nerf_for_angiography_amd.engine import (centreline_graph, centreline_main_path, cpr_images, distance_transform_edt_3d,  # noqa: E402
                                             lumen_world_to_index, polyline_resample, polyline_smooth, prune_spurs, reformat_planes_record,
                                             reformat_table_cpr, reformat_table_grid, rotation_minimising_frames, skeletonize_3d,
                                             straighten_volume)

HALF_WIDTH, STEP, ANGLES, REPEAT = 32, 0.5, (0.0, 45.0, 90.0, 135.0), 32


def median_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return {"median": round(statistics.median(times), 3), "min": round(min(times), 3), "max": round(max(times), 3)}


def measure(mask, reps, dev, host):
    m = torch.from_numpy(mask).to(dev)
    vol = torch.nn.functional.avg_pool3d(m[None, None].float(), 3, 1, 1, count_include_pad=True)[0, 0].contiguous()
    d2 = distance_transform_edt_3d(m, return_squared=True)[1]
    graph = centreline_graph(prune_spurs(skeletonize_3d(m), d2, 1.0), d2)
    t = time.perf_counter()
    path = centreline_main_path(graph, None, d2=d2)
    points = polyline_resample(polyline_smooth(path["points"], 8), 1.0)
    _, u, v, flags = rotation_minimising_frames(points, 3)
    geometry_ms = (time.perf_counter() - t) * 1e3
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    planes_host = np.concatenate([points, u, v], axis=1)
    planes, w = up(planes_host), lumen_world_to_index(None)
    p = planes.shape[0]
    tables = {"rows": reformat_table_grid(HALF_WIDTH, STEP, tiled=False)[0], "tiles": reformat_table_grid(HALF_WIDTH, STEP, tiled=True)[0],
              "cpr": reformat_table_cpr(HALF_WIDTH, STEP, ANGLES)}
    dt = {k: up(x) for k, x in tables.items()}
    out = {k: torch.empty((p, x.shape[0]), dtype=torch.float64, device=dev) for k, x in dt.items()}
    launch = lambda k, h=0: reformat_planes_record(vol, planes, dt[k], w, 0.0, h, "mean", out=out[k])
    res = {"shape": list(mask.shape), "mask_voxels": int(mask.sum()), "branches": graph["n_branches"], "path_branches": len(path["branches"]),
           "path_voxels": int(path["voxels"].size), "P": p, "rows_flagged": int(flags.sum()), "host_geometry_ms": round(geometry_ms, 1)}
    res["volume_launch_ms"] = median_ms(lambda: launch("rows"), reps)
    res["volume_samples"] = p * tables["rows"].shape[0]
    res["volume_samples_per_s"] = round(res["volume_samples"] / (res["volume_launch_ms"]["median"] * 1e-3))
    res["volume_wall_ms"] = median_ms(lambda: straighten_volume(vol, points, None, HALF_WIDTH, STEP), reps)
    res["images_launch_ms"] = median_ms(lambda: launch("cpr"), reps)
    res["images_samples"] = p * tables["cpr"].shape[0]
    res["images_wall_ms"] = median_ms(lambda: cpr_images(vol, points, None, ANGLES, HALF_WIDTH, STEP), reps)
    res["images_slab4_launch_ms"] = median_ms(lambda: launch("cpr", 4), reps)
    rows, tiles = [], []
    for _ in range(3):                                                                # alternating, so that a drift of the machine hits both
        rows.append(median_ms(lambda: launch("rows"), reps)["median"])
        tiles.append(median_ms(lambda: launch("tiles"), reps)["median"])
    res["table_rows_ms"], res["table_tiles_ms"] = rows, tiles
    # the same comparison out of the launch-latency regime: the path's planes REPEAT times over, one launch
    many = planes.repeat(REPEAT, 1).contiguous()
    big = torch.empty((many.shape[0], tables["rows"].shape[0]), dtype=torch.float64, device=dev)
    rows, tiles, slab = [], [], []
    for _ in range(3):
        rows.append(median_ms(lambda: reformat_planes_record(vol, many, dt["rows"], w, out=big), reps)["median"])
        tiles.append(median_ms(lambda: reformat_planes_record(vol, many, dt["tiles"], w, out=big), reps)["median"])
        slab.append(median_ms(lambda: reformat_planes_record(vol, many, dt["rows"], w, half_slab=4, out=big), reps)["median"])
    res["many_samples"], res["many_rows_ms"], res["many_tiles_ms"], res["many_rows_slab4_ms"] = big.numel(), rows, tiles, slab
    res["many_samples_per_s"] = round(big.numel() / (min(statistics.median(rows), statistics.median(tiles)) * 1e-3))
    del many, big
    launch("rows")
    torch.cuda.synchronize()
    # the volume is >= 0 everywhere: with fill -1 the samples that are not -1 are those inside the box
    res["inside_share"] = round(float((reformat_planes_record(vol, planes, dt["rows"], w, -1.0) != -1.0).float().mean()), 4)
    if host:
        t = time.perf_counter()
        want = rr.reformat_planes(vol.cpu().numpy(), w, planes_host, tables["rows"])
        res["host_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        res["equals_host"] = bool(np.array_equal(want, out["rows"].cpu().numpy()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=201)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_cpr.md"))
    args = ap.parse_args()
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "tree": measure(sk.capsule_tree(args.points), args.reps, dev, host=False),
           "tree64": measure(sk.capsule_tree(64), args.reps, dev, host=True)}
    k = 2 * HALF_WIDTH + 1
    lines = ["# Curved-planar reformation: times", "",
             f"`tools/cpr_timing.py --reps {args.reps} --points {args.points}` on {res['device']}; medians of {args.reps} calls (min .. max), each "
             "call timed by a host clock around the call and a device synchronise, after two warm-up calls.  float32 volume (the mask averaged "
             f"over 3^3 voxels), the main path smoothed (8 passes) and resampled at one voxel, step {STEP} voxels, K = {k} samples across, fill 0.",
             "", "The capability is new: there is no time of an earlier commit to compare with.", ""]
    for key, title in (("tree", f"capsule tree, {args.points}^3"), ("tree64", "capsule tree, 64^3")):
        r = res[key]
        lines += [f"## {title}", "",
                  f"{r['mask_voxels']} mask voxels, {r['branches']} branches after pruning; the main path crosses {r['path_branches']} of them "
                  f"({r['path_voxels']} voxels) and gives P = {r['P']} rows, {r['rows_flagged']} of them flagged; the host geometry (path, smoothing, "
                  f"resampling, frames) takes {r['host_geometry_ms']} ms once.  {100 * r['inside_share']:.1f} % of the volume's samples lie inside "
                  "the box.", "",
                  "| call | samples | ms |", "|---|---|---|"]
        for name, label, cnt in (("volume_launch_ms", f"straightened volume [P, {k}, {k}], the launch only (row table)", r["volume_samples"]),
                                 ("volume_wall_ms", "`straighten_volume`, as called", r["volume_samples"]),
                                 ("images_launch_ms", f"four longitudinal images [4, P, {k}], the launch only", r["images_samples"]),
                                 ("images_wall_ms", "`cpr_images`, as called", r["images_samples"]),
                                 ("images_slab4_launch_ms", "the images with half_slab 4 (9 lookups per sample), the launch only", r["images_samples"])):
            t = r[name]
            lines.append(f"| {label} | {cnt} | {t['median']} ({t['min']} .. {t['max']}) |")
        lines += ["", f"The volume's launch: {r['volume_samples_per_s']:.3e} samples per second (8 loads each).", "",
                  f"Cross-section table, the launch only, three medians each, alternating: row order {r['table_rows_ms']} ms; 8 x 8 tiles "
                  f"{r['table_tiles_ms']} ms.", "",
                  f"The same with the path's planes {REPEAT} times over in one launch ({r['many_samples']} samples, 8 bytes written each): row "
                  f"order {r['many_rows_ms']} ms; 8 x 8 tiles {r['many_tiles_ms']} ms - {r['many_samples_per_s']:.3e} samples per second for "
                  f"the faster; row order with half_slab 4 (9 lookups per sample) {r['many_rows_slab4_ms']} ms.  Faster there by the median of "
                  f"the three: {'8 x 8 tiles' if statistics.median(r['many_tiles_ms']) < statistics.median(r['many_rows_ms']) else 'row order'}."]
        if "host_ms" in r:
            lines += ["", f"NumPy restatement of the volume, one run on the host: {r['host_ms']} ms.  Device result equal to it: {r['equals_host']}."]
        lines.append("")
    lines += ["`engine.REFORMAT_TILED` follows the larger input's repeated launch, the only one of these that is not launch latency; the two orders "
              "lie within a few per cent of each other, and at 64^3, where the volume fits the caches, neither is ahead by more than the spread of the medians.", "",
              "Not measured: fp64 volumes, anisotropic affines, mode max, tables beyond K = 65, paths of more than a few hundred rows (at these "
              "sizes the launch is a few workgroups per CU and much of its time is launch latency, so neither the achieved gather rate nor the "
              "table order is settled for large P), and replay from a captured graph.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
