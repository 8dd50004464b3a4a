"""Times of the view map (afx_view_map): culled against brute, and the share of pixel-segment pairs the cull leaves.

Trees: the pruned centreline of the skeleton tests' capsule tree at --points^3 (201: the reference's evaluation grid) in the +-100 box
with the radii voxel x sqrt(d2), and a denser synthetic tree of 5 000 segments in 40 branches (the wavy lines of the view-map tests
scaled to +-80, radii 1.2 .. 2.4) - about the segment count of a clinical coronary tree at this sampling.  View sets: the 1 369 angles of
the evaluation sweep (sweep_angles(180, 5)) on a 100^2 detector and 25 angles (sweep_angles(180, 45)) on 512^2, source 1 500 from the
centre, focal length 13 x the detector.  Per tree and view set: ms per call of `engine.view_map_record` into preallocated buffers
(device events around --reps back-to-back calls after two warm-up calls; the median of five such series, min .. max), culled and brute
(brute: one call per series), counts alone and foreshortening alone; the pairs the cull leaves, counted on the host with the kernel's
own box test; and the host restatement (tests/viewmap_reference.py) on 25 views of 40 x 23, host clock, as a baseline.
Writes a report (default profiles/r26_view_map.md) and prints the same numbers as one JSON line.

    python tools/view_map_timing.py [--reps 5] [--points 201] [--out profiles/r26_view_map.md]"""
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
import skeleton_reference as sk                                                                    # noqa: E402
import viewmap_reference as vr                                                                     # noqa: E402
from nerf_for_angiography_amd import engine                                                        # noqa: E402
from nerf_for_angiography_amd.visualization.sweep import grid_index_to_world, sweep_angles         # noqa: E402

DEV = "cuda:0"
SRC = (0.0, 0.0, 1500.0)


def spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def event_ms(fn, reps, series=5):
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


def capsule_tree_segments(points):
    """(segments, seg_branch) of the pruned centreline of the capsule tree at points^3 over the +-100 box."""
    a12 = grid_index_to_world(100.0, points)
    voxel = 200.0 / (points - 1)
    mask = torch.from_numpy(sk.capsule_tree(points)).to(DEV)
    d2 = engine.distance_transform_edt_3d(mask, return_squared=True)[1]
    graph = engine.centreline_graph(engine.prune_spurs(engine.skeletonize_3d(mask), d2), d2, a12)
    pts, offsets = engine.centreline_world_points(graph, a12)
    vox = graph["path_voxels"].cpu().numpy()
    radius = np.sqrt((d2.reshape(-1).cpu().numpy().astype(np.int64) & 0xffffffff)[vox].astype(np.float64)) * voxel
    return engine.view_map_segments(pts, offsets, radius)


def dense_tree_segments():
    seg, br = vr.wavy_tree(5000, 40, 0)
    seg[:, 0:6] *= 8.0
    seg[:, 6] = np.random.RandomState(1).uniform(1.2, 2.4, seg.shape[0])
    return seg, br


def pairs_kept(seg, rec, width, height, tile=16):
    """The share of (tile pixel, segment) pairs the cull leaves: per view and tile the visible segments whose box, padded by rho + 1,
    meets the tile's pixel centres - the kernel's test, in NumPy - over all the segments."""
    kept = total = 0
    tx0 = np.arange(0, width, tile, dtype=np.float64)
    ty0 = np.arange(0, height, tile, dtype=np.float64)
    tx1, ty1 = np.minimum(tx0 + tile - 1, width - 1), np.minimum(ty0 + tile - 1, height - 1)
    for v in range(rec.shape[0]):
        u0, w0, d0 = vr.project(seg[:, 0:3], rec[v], width, height)
        u1, w1, d1 = vr.project(seg[:, 3:6], rec[v], width, height)
        ok = (d0 > 0) & (d1 > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            pad = (rec[v, 12] * seg[:, 6]) / (0.5 * (d0 + d1)) + 1.0
        in_x = ~((np.maximum(u0, u1) + pad)[:, None] < tx0[None]) & ~((np.minimum(u0, u1) - pad)[:, None] > tx1[None])
        in_y = ~((np.maximum(w0, w1) + pad)[:, None] < ty0[None]) & ~((np.minimum(w0, w1) - pad)[:, None] > ty1[None])
        kept += int(np.einsum("sx,sy->", (in_x & ok[:, None]).astype(np.int64), in_y.astype(np.int64)))
        total += seg.shape[0] * tx0.size * ty0.size
    return kept / total


def measure(name, seg, br, angles, size, reps):
    rec = engine.view_angles_records(angles, SRC, 13.0 * size)
    dev = [torch.from_numpy(x).to(DEV) for x in (seg, br, rec)]
    nb = int(br[-1])
    out = engine.view_map_record(*dev, size, size, n_branches=nb)
    torch.cuda.synchronize()
    row = dict(tree=name, segments=int(seg.shape[0]), branches=nb, views=int(rec.shape[0]), detector=size)
    call = lambda **kw: (lambda: engine.view_map_record(*dev, size, size, n_branches=nb, out=out, **kw))
    row["culled_ms"] = event_ms(call(), reps)
    row["brute_ms"] = event_ms(call(brute=True), 1, series=3)
    row["counts_only_ms"] = event_ms(call(foreshortening=False), reps)
    row["foreshortening_only_ms"] = event_ms(call(counts=False), reps)
    tree = out["tree"].cpu().numpy()
    pairs = float(seg.shape[0]) * rec.shape[0] * size * size
    row.update(pairs=pairs, pairs_kept_share=round(pairs_kept(seg, rec, size, size), 5), speedup=round(row["brute_ms"]["median"] / row["culled_ms"]["median"], 1),
               views_with_shared_pixels=int((tree[:, 1] > 0).sum()), mean_union_px=round(float(tree[:, 0].mean()), 1))
    return row


def host_baseline():
    seg, br = vr.wavy_tree(600, 4, 0)
    rec = engine.hull_view_records(*vr.scene_views(25, 40, 23, 0))
    t = time.perf_counter()
    vr.view_map(seg, br, rec, 40, 23)
    host = time.perf_counter() - t
    dev = [torch.from_numpy(x).to(DEV) for x in (seg, br, rec)]
    out = engine.view_map_record(*dev, 40, 23, n_branches=4)
    gpu = event_ms(lambda: engine.view_map_record(*dev, 40, 23, n_branches=4, out=out), 20)
    return dict(segments=600, views=25, detector="40 x 23", host_restatement_ms=round(host * 1e3, 1), device_ms=gpu)


def fmt(t):
    return f"{t['median']} ({t['min']} .. {t['max']})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=201)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_view_map.md"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": []}
    trees = ((f"capsule tree {args.points}^3, pruned centreline", *capsule_tree_segments(args.points)), ("dense synthetic tree", *dense_tree_segments()))
    for name, seg, br in trees:
        for angles, size in ((sweep_angles(180, 5), 100), (sweep_angles(180, 45), 512)):
            res["rows"].append(measure(name, seg, br, angles, size, args.reps))
            print(json.dumps(res["rows"][-1]), flush=True)
    res["baseline"] = host_baseline()
    lines = ["# The view map (afx_view_map): culled against brute", "", f"`tools/view_map_timing.py --reps {args.reps} --points {args.points}` on {res['device']}.",
             "", "ms per call of `engine.view_map_record` into preallocated buffers, device events around back-to-back calls after two warm-up calls; "
             "median of five series (min .. max); brute: three series of one call.  Pairs kept: the share of (tile pixel, segment) pairs that "
             "pass the tile's box test, counted on the host.", "",
             "| tree | segments | branches | views | detector | culled, ms | brute, ms | brute / culled | pairs | pairs kept | counts alone, ms | foreshortening alone, ms | views with shared pixels |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["rows"]:
        lines.append(f"| {r['tree']} | {r['segments']} | {r['branches']} | {r['views']} | {r['detector']}^2 | {fmt(r['culled_ms'])} | {fmt(r['brute_ms'])} | "
                     f"{r['speedup']} | {r['pairs']:.3g} | {r['pairs_kept_share']} | {fmt(r['counts_only_ms'])} | {fmt(r['foreshortening_only_ms'])} | "
                     f"{r['views_with_shared_pixels']} |")
    b = res["baseline"]
    lines += ["", "## The host restatement, as a baseline", "",
              f"{b['segments']} segments, {b['views']} views of {b['detector']}: tests/viewmap_reference.py {b['host_restatement_ms']} ms (one run, host clock); "
              f"the device {fmt(b['device_ms'])} ms.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
