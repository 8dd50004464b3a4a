"""Time of the lumen cross-sections along a centreline (afx_lumen_profile) on the GPU.

Two inputs: the capsule tree of the skeleton tests at --points^3 (default 201, the evaluation grid's size) and the 64^3 tree.  The volume
is the tree's mask averaged over 3 x 3 x 3 voxels (a density with a soft wall), the centreline the pruned skeleton of the mask read as a
graph, iso 0.5, 64 rays, the default step (half a voxel) and 32 steps.  Reported:
  * per input: `engine.lumen_profile_record` on buffers allocated once - the launch only - and `engine.centreline_lumen_profile` as a user
    calls it (world points on the host, upload, allocation, launch); P, the valid points and the mean number of march steps per ray;
  * at 64^3 with 16 rays: the launch with four points per wavefront (the library) against one point per wavefront with 48 idle lanes
    (`python -m nerf_for_angiography_amd.build --variant=lumidle`; skipped when that library has not been built), the two alternating;
  * at 64^3: one run of the NumPy restatement on the host (tests/lumen_reference.py), and whether the device equals it.
Every GPU time is the median of --reps calls (min .. max), each call timed by a host clock around the call and a device synchronise, after
two warm-up calls.  Writes a small report (default profiles/r20_lumen_profile.md) and prints the same numbers as one JSON line.

    python tools/lumen_profile_timing.py [--reps 20] [--points 201] [--out profiles/r20_lumen_profile.md]"""
import argparse
import ctypes as C
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
import lumen_reference as lr                                                                       # noqa: E402
import skeleton_reference as sk                                                                    # noqa: E402
from nerf_for_angiography_amd import _lib                                                          # noqa: E402
from nerf_for_angiography_amd.build import lib_path                                                # noqa: E402
from nerf_for_angiography_amd.engine import (Engine, centreline_graph, centreline_lumen_profile, centreline_segments,  # noqa: E402
                                             centreline_world_points, distance_transform_edt_3d, lumen_default_step, lumen_profile_record,
                                             lumen_ray_table, lumen_world_to_index, prune_spurs, skeletonize_3d)

ISO, MAX_STEPS = 0.5, 32


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


def raw_call(lib, vol, pts, first, last, w, n_rays, cs, coef, step, profile, flags):
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    _lib.check(lib.afx_lumen_profile(vol.data_ptr(), 0, *vol.shape, dp(w), pts.data_ptr(), first.data_ptr(), last.data_ptr(), pts.shape[0], 3,
                                     n_rays, dp(cs), coef, ISO, step, MAX_STEPS, profile.data_ptr(), flags.data_ptr(), None,
                                     Engine._stream(vol.device)), "afx_lumen_profile", lib)


def measure(mask, reps, dev, host):
    lib = _lib.load()
    m = torch.from_numpy(mask).to(dev)
    vol = torch.nn.functional.avg_pool3d(m[None, None].float(), 3, 1, 1, count_include_pad=True)[0, 0].contiguous()
    d2 = distance_transform_edt_3d(m, return_squared=True)[1]
    graph = centreline_graph(prune_spurs(skeletonize_3d(m), d2, 1.0), d2)
    points, offsets = centreline_world_points(graph, np.eye(3, 4))
    seg_first, seg_last, _, _ = centreline_segments(points, offsets)
    pts, first, last = (torch.from_numpy(x).to(dev) for x in (points, seg_first, seg_last))
    p, w, step = pts.shape[0], lumen_world_to_index(None), lumen_default_step(None)
    profile, flags = torch.empty((p, 8), dtype=torch.float64, device=dev), torch.empty(p, dtype=torch.int32, device=dev)
    radii = torch.empty((p, 64), dtype=torch.float64, device=dev)
    res = {"shape": list(mask.shape), "mask_voxels": int(mask.sum()), "branches": graph["n_branches"], "P": p}
    res["launch_ms"] = median_ms(lambda: lumen_profile_record(vol, pts, first, last, w, ISO, 64, step, MAX_STEPS, profile=profile, flags=flags), reps)
    res["wall_ms"] = median_ms(lambda: centreline_lumen_profile(graph, vol, None, ISO), reps)
    lumen_profile_record(vol, pts, first, last, w, ISO, 64, step, MAX_STEPS, profile=profile, flags=flags, radii=radii)
    ok = flags == 0
    res["valid"] = int(ok.sum())
    res["open_rays"] = int(((flags >> 8) & 0xff).sum())
    # a closed ray crossed at step floor(r / ds) + 1, an open one took all of them
    took = torch.clamp(torch.floor(radii[ok] / step) + 1.0, max=float(MAX_STEPS))
    res["mean_steps_per_ray"] = round(float(took.mean()), 2) if res["valid"] else float("nan")
    if host:
        cs16, coef16 = lumen_ray_table(16)
        packed, idle = [], []
        other = _lib.load("lumidle") if os.path.exists(lib_path("lumidle")) else None
        for _ in range(3):                                                            # alternating, so that a drift of the machine hits both
            packed.append(median_ms(lambda: raw_call(lib, vol, pts, first, last, w, 16, cs16, coef16, step, profile, flags), reps)["median"])
            if other is not None:
                idle.append(median_ms(lambda: raw_call(other, vol, pts, first, last, w, 16, cs16, coef16, step, profile, flags), reps)["median"])
        res["r16_four_points_per_wave_ms"], res["r16_one_point_per_wave_ms"] = packed, idle
        cs, coef = lumen_ray_table(64)
        t = time.perf_counter()
        want = lr.lumen_profile(vol.cpu().numpy(), w, points, seg_first, seg_last, 3, 64, cs, coef, ISO, step, MAX_STEPS)
        res["host_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        got = lumen_profile_record(vol, pts, first, last, w, ISO, 64, step, MAX_STEPS, want_radii=True)
        res["equals_host"] = bool(all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(want, got)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=201)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_lumen_profile.md"))
    args = ap.parse_args()
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "tree": measure(sk.capsule_tree(args.points), args.reps, dev, host=False),
           "tree64": measure(sk.capsule_tree(64), args.reps, dev, host=True)}
    lines = ["# Lumen cross-sections along the centreline: times", "",
             f"`tools/lumen_profile_timing.py --reps {args.reps} --points {args.points}` on {res['device']}; medians of {args.reps} calls "
             "(min .. max), each call timed by a host clock around the call and a device synchronise, after two warm-up calls.  float32 volume "
             f"(the mask averaged over 3^3 voxels), iso {ISO}, 64 rays, step half a voxel, {MAX_STEPS} steps at most, window +-3 points.", ""]
    for key, title in (("tree", f"capsule tree, {args.points}^3"), ("tree64", "capsule tree, 64^3")):
        r = res[key]
        lines += [f"## {title}", "",
                  f"{r['mask_voxels']} mask voxels, {r['branches']} branches after pruning, P = {r['P']} centreline points, {r['valid']} of them valid, "
                  f"{r['open_rays']} open rays; a ray of a valid point takes {r['mean_steps_per_ray']} march steps in the mean (8 loads each).", "",
                  "| call | ms |", "|---|---|"]
        for name, label in (("launch_ms", "`lumen_profile_record`, the launch only"), ("wall_ms", "`centreline_lumen_profile`, as called")):
            t = r[name]
            lines.append(f"| {label} | {t['median']} ({t['min']} .. {t['max']}) |")
        if "host_ms" in r:
            lines += [f"| NumPy restatement, one run | {r['host_ms']} |", "", f"Device result equal to the restatement: {r['equals_host']}.", "",
                      f"16 rays, the launch only, three medians each, alternating: four points per wavefront (the library) "
                      f"{r['r16_four_points_per_wave_ms']} ms; one point per wavefront, 48 lanes idle (variant lumidle) "
                      f"{r['r16_one_point_per_wave_ms'] or 'not measured: the variant was not built'} ms."]
        lines.append("")
    lines += ["Not measured: fp64 volumes, fewer than 64 rays at scale (the 16-ray comparison above is the 64^3 tree only), the achieved gather "
              "rate (bytes per second of the scattered 4-byte loads), and replay from a captured graph.", ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
