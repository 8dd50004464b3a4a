"""Times of the visual hull (afx_visual_hull), of carving an occupancy grid with it, and what the carved grid buys the training loop.

Parts (--parts, default all of them):
  kernel   afx_visual_hull over the 128^3 cell centres of the +-100 box for 4, 25 and 1 369 views of 100^2 (angle_grid(180, 1 / 4 / 36)
           without the held-out pose) and over the 201^3 evaluation grid for 25 views; masks = the rounded projections of 50 000 points of
           the capsule tree, margin 1.  Kernel time from device events around --reps back-to-back launches after two warm-up launches,
           the median of five such series (min .. max); points x views per second; the hull's share of the lattice.
  edt      the D-stack build (`engine.distance_transform_edt` of the complements of the masks) for the same view sets, timed likewise.
  refresh  `OccupancyGrid.refresh` of a 128^3 grid (4 x 128 f16s8 model), warm-up phase and afterwards: uncarved against uncarved first
           (the run-to-run band of what the parent does), then carved against uncarved, alternating, medians of --reps calls timed by a
           host clock around the call and a device synchronise; and the afx_grid_apply_mask launch alone.
  driver   the driver's first 2 048 iterations on the synthetic capsule phantom (--binary True, 26 views of 64^2, 4 x 128, f16s8) with
           --march grid and with --march grid --graph --graph-grid-update --graph-rounds, each without and with --grid_init hull, same
           seed: iterations per second over the window (the evaluations at the display points included, alike in both arms), samples
           marched per iteration in the windows that end at iterations 0, 256 and 1 024, and the held-out view's PSNR at the end.
Writes a report (default profiles/r21_visual_hull.md) and prints the same numbers as one JSON line.

    python tools/hull_timing.py [--reps 20] [--parts kernel,edt,refresh,driver] [--out profiles/r21_visual_hull.md]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hull_reference as hr                                                                        # noqa: E402
from nerf_for_angiography_amd import engine                                                        # noqa: E402
from nerf_for_angiography_amd.phantomdata.dataset import angle_grid                                # noqa: E402
from nerf_for_angiography_amd.phantomdata.helpers import capsule_mu, capsule_tree                  # noqa: E402
from nerf_for_angiography_amd.phantomdata.proj_helpers import source_matrix                        # noqa: E402

DEV = "cuda:0"
AABB = [-100.0, -100, -100, 100, 100, 100]
SIZE, FOCAL = 100, 1300.0


def spread(xs, digits=3):
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
    return spread(out, 4)


def host_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return spread(times)


def vessel_points(n, seed=0):
    caps = capsule_tree(levels=5, seed=0)
    rng = np.random.RandomState(seed)
    i = rng.randint(len(caps), size=4 * n)
    a, b, r = caps[i, :3].astype(np.float64), caps[i, 3:6].astype(np.float64), caps[i, 6:7].astype(np.float64)
    p = a + rng.uniform(size=(len(i), 1)) * (b - a) + rng.uniform(-1, 1, size=(len(i), 3)) * r
    return p[capsule_mu(torch.from_numpy(p), caps).numpy() > 0][:n]


def view_set(number_angles, points):
    poses = np.stack([source_matrix(np.array([0.0, 0.0, 1500.0]), th, ph) for th, ph in angle_grid(180, number_angles)[:-1]])
    masks, _ = hr.masks_from_points(points, poses, FOCAL, SIZE, SIZE)
    return poses, torch.from_numpy(masks).to(DEV)


def part_kernel(reps, sets):
    from nerf_for_angiography_amd.visualization.sweep import grid_index_to_world
    rows = []
    cells, rho = engine.grid_cell_lattice(AABB, [128] * 3)
    metric = grid_index_to_world(100.0, 201)
    for name, shape, a12, radius, number_angles in (("128^3 cell centres", (128,) * 3, cells, rho, 1), ("128^3 cell centres", (128,) * 3, cells, rho, 4),
                                                    ("128^3 cell centres", (128,) * 3, cells, rho, 36),
                                                    ("201^3 evaluation grid", (201,) * 3, metric, engine.hull_default_radius(metric), 4)):
        poses, masks = sets[number_angles]
        views = engine.visual_hull_views(poses, masks, FOCAL, margin_px=1.0)
        seen = torch.empty(shape, dtype=torch.uint16, device=DEV)
        rejects = torch.empty(shape, dtype=torch.uint16, device=DEV)
        n_views = len(poses)
        t = event_ms(lambda: engine.visual_hull_record(views, shape, a12, radius, seen=seen, rejects=rejects), max(2, reps if n_views < 100 else reps // 5))
        hull = (rejects.to(torch.int32) == 0) & (seen.to(torch.int32) >= 1)
        pv = float(np.prod(shape)) * n_views
        rows.append(dict(lattice=name, views=n_views, ms=t, point_views_per_s=round(pv / (t["median"] * 1e-3), -6), hull_share=round(float(hull.float().mean()), 4),
                         min_seen_kept=int(seen.to(torch.int32)[hull].min()) if bool(hull.any()) else 0))
    return rows


def part_edt(reps, sets):
    rows = []
    for number_angles in (1, 4, 36):
        _, masks = sets[number_angles]
        x = (~masks).to(torch.float64)
        rows.append(dict(views=int(masks.shape[0]), ms=event_ms(lambda: engine.distance_transform_edt(x), max(2, reps // 2))))
    return rows


def part_refresh(reps, sets):
    from nerf_for_angiography_amd.model.CPPN import CPPN
    from nerf_for_angiography_amd.nerf.occupancy import OccupancyGrid
    torch.manual_seed(0)
    model = CPPN(dict(num_early_layers=4, num_late_layers=0, num_filters=128, num_input_channels=3, num_output_channels=1, num_input_channels_views=0,
                      use_bias=True, pos_enc="none", pos_enc_basis=5, act_func="relu", fourier_sigma=5, num_img=1, device=torch.device(DEV),
                      precision="f16s8")).to(DEV)
    with torch.no_grad():
        model.output_linear[0].bias.fill_(-4.0)
    poses, masks = sets[4]
    views = engine.visual_hull_views(poses, masks, FOCAL, margin_px=1.0)
    grids = [OccupancyGrid(roi_aabb=torch.tensor(AABB, device=DEV), resolution=128, seed=0).to(DEV) for _ in range(3)]
    hull = grids[2].carve_from_views(views)
    out = {"hull_share": round(float(hull.float().mean()), 4)}
    for phase, step in (("warm-up (every cell)", 16), ("after warm-up (the draw)", 512)):
        for g in grids:
            g.refresh(model, 0)      # a common, full start
        series = {"parent_a": [], "parent_b": [], "carved": []}
        for _ in range(3):      # alternating, so that a drift of the machine hits all three
            for name, g in zip(("parent_a", "parent_b", "carved"), grids):
                series[name].append(host_ms(lambda: g.refresh(model, step), reps)["median"])
        out[phase] = {k: spread(v) for k, v in series.items()}
    g = grids[2]
    out["apply_mask_launch_ms"] = event_ms(lambda: engine.grid_apply_mask(g._aabb_host, g._res_host, g._carve_u8, g.occs, g._binary_u8, g._bits), reps * 5)
    return out


def part_driver():
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main
    rows = []
    base = ["--synthetic", "--binary", "True", "--n_iters", "2048", "--display_every", "256", "--seed", "0"]
    for body, flags in (("--march grid", ["--march", "grid"]),
                        ("--march grid --graph --graph-grid-update --graph-rounds", ["--march", "grid", "--graph", "--graph-grid-update", "--graph-rounds"])):
        for hull in (False, True):
            with tempfile.TemporaryDirectory() as tmp:
                out = main(base + flags + (["--grid_init", "hull"] if hull else []) + ["--log_dir", tmp])
            h = {r["iter"]: r for r in out["history"]}
            window = sum(r["sec"] for it, r in h.items() if it > 0)
            rows.append(dict(body=body, hull=hull, it_per_s=round(2048 / window, 1), window_s=round(window, 3),
                             marched={"0": h[0]["marched_samples_per_iter"] * 256, "256": h[256]["marched_samples_per_iter"],
                                      "1024": h[1024]["marched_samples_per_iter"]},
                             psnr=round(h[2048]["test_psnr"], 3), vessel_psnr=round(h[2048]["test_vessel_psnr"], 3),
                             hull_share=round(out["hull_info"]["share"], 4) if hull else None,
                             occupied_share_end=round(float(out["acc_grid"].binary.float().mean()), 4)))
    return rows


def fmt(t):
    return f"{t['median']} ({t['min']} .. {t['max']})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parts", default="kernel,edt,refresh,driver")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_visual_hull.md"))
    args = ap.parse_args()
    parts = args.parts.split(",")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    points = vessel_points(50000)
    sets = {k: view_set(k, points) for k in (1, 4, 36)} if set(parts) & {"kernel", "edt", "refresh"} else {}
    lines = ["# Visual hull of the training views: times and what carving buys", "",
             f"`tools/hull_timing.py --reps {args.reps} --parts {args.parts}` on {res['device']}.", ""]
    if "kernel" in parts:
        res["kernel"] = part_kernel(args.reps, sets)
        lines += ["## afx_visual_hull", "",
                  "Views of 100^2, f = 1300, margin 1; masks = the rounded projections of 50 000 points of the capsule tree.  ms per launch from "
                  "device events around back-to-back launches; median of five series (min .. max).", "",
                  "| lattice | views | ms | points x views / s | hull share | fewest views seeing a kept point |", "|---|---|---|---|---|---|"]
        lines += [f"| {r['lattice']} | {r['views']} | {fmt(r['ms'])} | {r['point_views_per_s']:.3g} | {r['hull_share']} | {r['min_seen_kept']} |" for r in res["kernel"]]
        lines.append("")
    if "edt" in parts:
        res["edt"] = part_edt(args.reps, sets)
        lines += ["## The D stack (`distance_transform_edt` of the complements of the masks), 100^2 images", "", "| views | ms |", "|---|---|"]
        lines += [f"| {r['views']} | {fmt(r['ms'])} |" for r in res["edt"]] + [""]
    if "refresh" in parts:
        r = res["refresh"] = part_refresh(args.reps, sets)
        lines += ["## A carved refresh against the parent's refresh", "",
                  f"128^3 grid, 4 x 128 f16s8 model, hull of 25 views (share {r['hull_share']}).  `OccupancyGrid.refresh`, host clock around the call "
                  f"and a device synchronise; each entry: median (min .. max) of three medians of {args.reps} calls, the three grids alternating.  "
                  "parent a / parent b are two uncarved grids: their difference is the run-to-run band.", "",
                  "| phase | parent a, ms | parent b, ms | carved, ms |", "|---|---|---|---|"]
        for phase in ("warm-up (every cell)", "after warm-up (the draw)"):
            p = r[phase]
            lines.append(f"| {phase} | {fmt(p['parent_a'])} | {fmt(p['parent_b'])} | {fmt(p['carved'])} |")
        lines += ["", f"The afx_grid_apply_mask launch alone, back to back (device events): {fmt(r['apply_mask_launch_ms'])} ms.", ""]
    if "driver" in parts:
        res["driver"] = part_driver()
        lines += ["## The driver's first 2 048 iterations, without and with --grid_init hull", "",
                  "Synthetic capsule phantom, --binary True, 26 views of 64^2 (25 train), 4 x 128, f16s8, seed 0, display every 256 iterations.  "
                  "it/s over iterations 1 .. 2 048, the eight evaluations of the held-out view included.  Samples marched per iteration: the mean "
                  "over the 256 iterations that end at the named one (iteration 0: that iteration alone).", "",
                  "| body | hull | it/s | marched @0 | @256 | @1024 | PSNR | vessel PSNR | hull share | occupied share at the end |", "|---|---|---|---|---|---|---|---|---|---|"]
        lines += [f"| {r['body']} | {'yes' if r['hull'] else 'no'} | {r['it_per_s']} | {r['marched']['0']} | {r['marched']['256']} | {r['marched']['1024']} | "
                  f"{r['psnr']} | {r['vessel_psnr']} | {r['hull_share']} | {r['occupied_share_end']} |" for r in res["driver"]]
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
