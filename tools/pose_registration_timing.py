"""Times of the 2D-3D pose registration (afx_pose_chamfer, afx_pose_lm_step) and one end-to-end run of the driver with noisy poses.

Scene: the wavy tree of the view-map tests (points = the first end of every segment, radii as given) seen by oblique views of 64 x 64 at
distance 60, focal 2.4 x the detector, the silhouettes rasterised at the true poses; poses perturbed by up to +-0.5 degrees and +-0.5
units per axis.  Measured, ms per call into preallocated buffers (device events around --reps back-to-back calls after two warm-up
calls; the median of five such series, min .. max):
  search      the cost-only score of 25 views x 729 candidates x 2 000 points (one launch) -> point evaluations per second
  iteration   one LM iteration (the full score of the trial and the step: two launches) at V = 9 and 25, N = 2 000, against two
              launches of afx_pose_compose on one record (launch latency) and against the host restatement (tests/pose_reference.py)
  slices      the full score at V = 9 over S = 1 .. 64 slices, at N = 2 000 and N = 100 000
  driver      (--driver_iters > 0) nerf/run_nerf_acc.py --synthetic --binary True --pose_noise on one seed, then the registration of
              its training views to the final model's centreline: CHAMFER 2D before and after, and the mean reprojection error of the
              centreline (of the density grid cut at 0.3 x its maximum) against unshifted_tform_cam2world before and after; and the
              same views against the centreline of the phantom itself (what the registration gives when the reconstruction is right)
Writes a report (default profiles/r28_pose_registration.md) and prints the same numbers as one JSON line.

    python tools/pose_registration_timing.py [--reps 20] [--driver_iters 3000] [--no_timing] [--out profiles/r28_pose_registration.md]"""
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
import pose_reference as pr                                                                       # noqa: E402
from nerf_for_angiography_amd import engine                                                        # noqa: E402

DEV = torch.device("cuda:0")
W = 64


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


def fmt(t):
    return f"{t['median']} ({t['min']} .. {t['max']})"


def scene(n_points, n_views):
    pts, rad, seg = pr.tree_points(n_points, 3, 1)
    poses, focal = pr.oblique_views(n_views, W)
    rec = engine.hull_view_records(poses, focal)
    small = pr.tree_points(600, 3, 1)[2]                       # the silhouettes do not need the dense tree
    masks = torch.from_numpy(pr.silhouettes(small, rec, W, W)).to(DEV)
    views = engine.pose_views(poses, masks, focal)
    pert = np.stack([pr.compose(r, x) for r, x in zip(rec, pr.perturbation(n_views, 11))])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return views, up(pts), up(rad), up(pert), (pts, rad, rec, pert)


def time_search(reps):
    views, pts, rad, pert, _ = scene(2000, 25)
    offsets = torch.from_numpy(engine.pose_search_offsets(2.0, 1.0, 9)).to(DEV)
    m = offsets.shape[0]
    buf = engine.register_poses_buffers(25, m, 1, DEV)
    engine.pose_compose(pert, offsets, outer=True, out=buf["cand"])
    cand = buf["cand"].view(25 * m, 16)
    ms = event_ms(lambda: engine.pose_chamfer_record(views, pts, rad, None, cand, buf["cand_view"], 8.0, 1, True, buf["cand_sums"], buf["cand_counts"]), reps)
    evals = 25 * m * 2000
    return dict(views=25, candidates=m, points=2000, ms=ms, point_evaluations_per_s=round(evals / (ms["median"] * 1e-3), 0))


def time_iteration(n_views, reps):
    from nerf_for_angiography_amd import _lib
    lib = _lib.load()
    views, pts, rad, pert, host = scene(2000, n_views)
    s = engine.pose_default_slices(2000, n_views)
    row = dict(views=n_views, points=2000, default_slices=s)
    for name, slices in (("s1", 1), ("default", s)):
        buf = engine.register_poses_buffers(n_views, 0, slices, DEV)
        engine.register_poses_record(views, pts, rad, None, pert, 2, 8.0, 63, None, slices, buffers=buf)
        stream = engine.Engine._stream(DEV)

        def iteration():
            engine.pose_chamfer_record(views, pts, rad, None, buf["trial_records"], buf["rec_view"], 8.0, slices, False, buf["sums"], buf["counts"])
            _lib.check(lib.afx_pose_lm_step(engine._ptr(buf["state"]), n_views, engine._ptr(buf["sums"]), slices, engine.POSE_LM_UPDATE, 63, 1e-3, None,
                                            engine._ptr(buf["trial_records"]), stream))
        row[f"iteration_{name}_ms"] = event_ms(iteration, reps)
    one, xi, out = pert[:1].contiguous(), torch.zeros(1, 6, dtype=torch.float64, device=DEV), torch.empty(1, 16, dtype=torch.float64, device=DEV)

    def two_launches():
        engine.pose_compose(one, xi, out=out)
        engine.pose_compose(one, xi, out=out)
    row["two_small_launches_ms"] = event_ms(two_launches, reps)
    pts_h, rad_h, rec_h, pert_h = host
    field = views["field"].cpu().numpy()
    t = time.perf_counter()
    sums, _ = pr.chamfer(field, pts_h, rad_h, None, pert_h, np.arange(n_views), 8.0, 1)
    state = np.zeros((n_views, 64))
    pr.lm_step(state, sums, pr.LM_INIT, records_in=pert_h)
    row["host_restatement_ms"] = round((time.perf_counter() - t) * 1e3, 2)
    return row


def time_slices(n_points, reps):
    views, pts, rad, pert, _ = scene(n_points, 9)
    rec_view = torch.arange(9, dtype=torch.int32, device=DEV)
    out = {}
    for s in (1, 2, 4, 8, 16, 32, 64):
        if s > -(-n_points // 256):
            continue
        sums = torch.empty(9, s, 32, dtype=torch.float64, device=DEV)
        counts = torch.empty(9, s, 4, dtype=torch.int32, device=DEV)
        out[str(s)] = event_ms(lambda: engine.pose_chamfer_record(views, pts, rad, None, pert, rec_view, 8.0, s, False, sums, counts), reps)
    return dict(views=9, points=n_points, ms_by_slices=out)


def driver_run(iters, log_dir):
    """One seed of the synthetic driver with noisy poses, then the registration of its training views against the final centreline."""
    from nerf_for_angiography_amd.nerf import run_nerf_acc as drv
    from nerf_for_angiography_amd.phantomdata import dataset as ds
    from nerf_for_angiography_amd.render import density_grid
    noise, size, depth = (0.3, 2.0), 64, 128
    argv = ["--synthetic", "--binary", "True", "--img_size", str(size), "--depth_samples", str(depth), "--n_iters", str(iters), "--display_every",
            str(max(iters // 2, 1)), "--pose_noise", str(noise[0]), str(noise[1]), "--log_dir", log_dir, "--seed", "0"]
    out = drv.main(argv)
    args = drv.build_parser().parse_args(argv)
    proj_df, ray_df = ds.make_synthetic_dataset(ds.angle_grid(180.0, 4, [90, 0]), img_size=size, sampling_strategy="segmentation", device=DEV, seed=0,
                                                binary=True, pose_noise=noise)
    test_id = proj_df.index[-1]
    train = ray_df[ray_df["image_id"] != test_id]
    poses, masks, focal = drv.training_view_masks(proj_df, train, test_id, args.hull_threshold, DEV)
    true = np.asarray([proj_df.loc[i, "unshifted_tform_cam2world"] for i in proj_df.index if i != test_id], np.float64)
    grid = density_grid(out["model"], 100, depth)
    thr = 0.3 * float(grid.max())                                # the model's own scale: a third of its densest voxel
    tree, a = drv._export_tree(grid, 100, depth + 1, thr, 1.0)
    points, rad = engine.centreline_pose_points(tree["graph"], a, d2=tree["d2"], voxel_size=200.0 / depth)
    row = dict(iterations=iters, pose_noise=noise, detector=size, views=int(len(poses)), test_psnr=round(float(out.get("best_psnr", float("nan"))), 2))
    views = engine.pose_views(poses, masks, focal)
    true_rec = engine.hull_view_records(true, focal)
    given_rec = views["records"].cpu().numpy()

    def score(points, rad, **kw):
        if points.shape[0] == 0:
            return dict(points=0, note="no centreline at this threshold")
        reg = engine.register_poses(points, rad, views, **kw)
        err = lambda rec: round(float(np.mean(engine.pose_projection_shift(points, true_rec, rec, size, size))), 4)
        return dict(points=int(points.shape[0]), chamfer_before=round(float(np.mean(reg["mean_residual_before"])), 4),
                    chamfer_after=round(float(np.mean(reg["mean_residual_after"])), 4), reprojection_error_before_px=err(given_rec),
                    reprojection_error_after_px=err(reg["records"]), accepted_mean=round(float(np.mean(reg["accepted"])), 1))
    row["model"] = dict(score(points, rad), threshold=round(thr, 4))
    # the same views against the centreline of the phantom itself: what the registration gives when the reconstruction is right
    from nerf_for_angiography_amd.phantomdata.helpers import capsule_mu, capsule_tree
    n = depth + 1
    ijk = torch.stack(torch.meshgrid(*(torch.arange(n, dtype=torch.float64, device=DEV),) * 3, indexing="ij"), dim=-1).reshape(-1, 3)
    a34 = torch.tensor(a, dtype=torch.float64, device=DEV).reshape(3, 4)
    truth = capsule_mu(ijk @ a34[:, :3].T + a34[:, 3], capsule_tree(levels=5, seed=0)).reshape(n, n, n).float()
    tree, _ = drv._export_tree(truth, 100, n, 0.1, 1.0)
    points, rad = engine.centreline_pose_points(tree["graph"], a, d2=tree["d2"], voxel_size=200.0 / depth)
    row["phantom"] = score(points, rad)
    row["phantom_inplane_search"] = score(points, rad, dof="inplane", search=(0.5, 3.0, 5))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--driver_iters", type=int, default=0)
    ap.add_argument("--no_timing", action="store_true", help="the driver run alone (no report is written)")
    ap.add_argument("--log_dir", default=os.path.join(ROOT, "runs", "pose_timing"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_pose_registration.md"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    if args.no_timing:
        res["driver"] = driver_run(args.driver_iters, args.log_dir)
        print(json.dumps(res))
        return
    res["search"] = time_search(max(args.reps // 4, 2))
    print(json.dumps(res["search"]), flush=True)
    res["iteration"] = [time_iteration(v, args.reps) for v in (9, 25)]
    print(json.dumps(res["iteration"]), flush=True)
    res["slices"] = [time_slices(n, args.reps) for n in (2000, 100000)]
    print(json.dumps(res["slices"]), flush=True)
    if args.driver_iters > 0:
        res["driver"] = driver_run(args.driver_iters, args.log_dir)
    s = res["search"]
    lines = ["# 2D-3D pose registration (afx_pose_chamfer, afx_pose_lm_step)", "",
             f"`tools/pose_registration_timing.py --reps {args.reps} --driver_iters {args.driver_iters}` on {res['device']}.", "",
             "ms per call into preallocated buffers, device events around back-to-back calls after two warm-up calls; median of five series "
             "(min .. max).", "", "## The cost-only search", "",
             f"{s['views']} views x {s['candidates']} candidates x {s['points']} points, one launch of {s['views'] * s['candidates']} workgroups: "
             f"{fmt(s['ms'])} ms, {s['point_evaluations_per_s']:.3g} point evaluations per second.", "", "## One LM iteration (two launches)", "",
             "| views | points | S = 1, ms | default S | default S, ms | two small launches, ms | host restatement, ms |", "|---|---|---|---|---|---|---|"]
    for r in res["iteration"]:
        lines.append(f"| {r['views']} | {r['points']} | {fmt(r['iteration_s1_ms'])} | {r['default_slices']} | {fmt(r['iteration_default_ms'])} | "
                     f"{fmt(r['two_small_launches_ms'])} | {r['host_restatement_ms']} |")
    lines += ["", "## The slice count (full score, 9 views)", "", "| points | " + " | ".join(f"S = {k}" for k in res["slices"][1]["ms_by_slices"]) + " |",
              "|---|" + "---|" * len(res["slices"][1]["ms_by_slices"])]
    for r in res["slices"]:
        lines.append(f"| {r['points']} | " + " | ".join(fmt(r["ms_by_slices"][k]) if k in r["ms_by_slices"] else "-" for k in res["slices"][1]["ms_by_slices"]) + " |")
    if "driver" in res:
        lines += ["", "## The synthetic driver with noisy poses, one seed", "", "```", json.dumps(res["driver"], indent=1), "```"]
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
