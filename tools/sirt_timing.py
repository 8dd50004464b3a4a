"""Times of the SIRT operators (afx_xray_project, afx_xray_backproject), of a whole reconstruction against the NumPy restatement, and what
the classical baseline achieves on the synthetic phantom.

Parts (--parts, default all of them):
  kernel   at 201^3 points (the evaluation grid over the +-100 box) against 25 views of 512^2 with S = 256, and at the 128^3 cell centres
           of that box against 25 views of 100^2 with S = 128 (angle_grid(180, 4) without the held-out pose, source distance 1500,
           f = 13 W, near / far 1400 / 1600; the volume is the capsule phantom's density): the plain projection, the fused residual, the
           fused backproject-update and one iteration (the two fused launches).  Time from device events around --reps back-to-back
           launches after two warm-up launches, the median of five such series (min .. max).  Counted from the shapes and from a
           projection of ones: samples tested (rays x S), samples interpolated (those inside the lattice), point-views gathered (the sum
           of `seen`); effective gathered bytes = 64 per interpolated sample, 32 per gathered point-view.
  recon    engine.sirt_reconstruct, 50 iterations at 64^3 against 9 views of 64^2 with S = 128, by a host clock around the call and a
           device synchronise (median of five), against tests/sirt_reference.py's iteration on the host, once; the two volumes must be
           equal bit for bit.
  phantom  the driver's first 2 048 iterations on the synthetic capsule phantom (--binary True, 26 views of 64^2, 4 x 128, f16s8,
           --march grid --grid_init hull), then on 101^3 points: the vessel Dice of SIRT (50 iterations) from the 25 training views with
           and without the hull as its mask, the hull's own Dice and the trained model's (sweep.reconstruction_sirt_metrics,
           reconstruction_hull_metrics; the SIRT rays take 160 samples between 1400 and 1600), at the threshold mean(gt) and at 0.1, half
           the phantom's vessel density.  One seed.
Prints the numbers as one JSON line and, with --out, writes them as a report.

    python tools/sirt_timing.py [--reps 10] [--parts kernel,recon,phantom] [--out profiles/sirt_numbers.md]"""
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
import sirt_reference as sr                                                                        # noqa: E402
from nerf_for_angiography_amd import engine                                                        # noqa: E402
from nerf_for_angiography_amd.phantomdata.dataset import angle_grid                                # noqa: E402
from nerf_for_angiography_amd.phantomdata.helpers import VoxelVolume, capsule_mu, capsule_tree     # noqa: E402
from nerf_for_angiography_amd.phantomdata.proj_helpers import source_matrix                        # noqa: E402

DEV = "cuda:0"
AABB = [-100.0, -100, -100, 100, 100, 100]
SRC = np.array([0.0, 0.0, 1500.0])


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


def phantom_on(shape, a12, chunk=1 << 20):
    """The capsule phantom's density at the lattice points, float64 on the device."""
    caps = capsule_tree(levels=5, seed=0)
    x = torch.from_numpy(sr.lattice_points(shape, a12)).to(DEV)
    mu = torch.cat([capsule_mu(x[i:i + chunk], caps) for i in range(0, x.shape[0], chunk)])
    return mu.to(torch.float64).reshape(shape)


def training_poses(number_angles):
    return np.stack([source_matrix(SRC, th, ph) for th, ph in angle_grid(180, number_angles)[:-1]])


def part_kernel(reps):
    from nerf_for_angiography_amd.visualization.sweep import grid_index_to_world
    rows = []
    poses = training_poses(4)
    for name, shape, a12, size, s in (("201^3 evaluation grid", (201,) * 3, grid_index_to_world(100.0, 201), 512, 256),
                                      ("128^3 cell centres", (128,) * 3, engine.grid_cell_lattice(AABB, [128] * 3)[0], 100, 128)):
        views = engine.xray_views(poses, 13.0 * size, size, size, 1400.0, 1600.0, s, device=DEV)
        x = phantom_on(shape, a12)
        rays = len(poses) * size * size
        ones = engine.xray_project(torch.ones_like(x), views, a12)
        b = engine.xray_project(x, views, a12)
        rec = views["records"].cpu().numpy()
        iw, iu = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing="ij")
        length = np.stack([np.sqrt(((iu - size / 2) / r[12]) ** 2 + ((iw - size / 2) / r[12]) ** 2 + 1.0) for r in rec])      # |d| (R orthonormal)
        inside = int(np.rint(ones.cpu().numpy() / ((200.0 / s) * length)).sum())
        weight = torch.where(ones > 0, 1.0 / ones, torch.zeros_like(ones))
        out = torch.empty_like(b)
        y = torch.zeros_like(x)
        _, seen = engine.xray_backproject(b, views, shape, a12)
        gathered = int(seen.to(torch.int64).sum())
        t_plain = event_ms(lambda: engine.xray_project(x, views, a12, out=out), reps)
        t_fused = event_ms(lambda: engine.xray_project(x, views, a12, target=b, weight=weight, out=out), reps)
        t_back = event_ms(lambda: engine.xray_backproject(out, views, shape, a12, x_inout=y, relax=1.0, nonneg=True), reps)

        def iteration():
            engine.xray_project(y, views, a12, target=b, weight=weight, out=out)
            engine.xray_backproject(out, views, shape, a12, x_inout=y, relax=1.0, nonneg=True)
        t_iter = event_ms(iteration, reps)
        per_s = lambda count, t: float(f"{count / (t['median'] * 1e-3):.4g}")
        rows.append(dict(lattice=name, views=len(poses), detector=size, S=s, rays=rays, samples_tested=rays * s, samples_interpolated=inside,
                         point_views_gathered=gathered, project_ms=t_plain, residual_ms=t_fused, backproject_update_ms=t_back, iteration_ms=t_iter,
                         project_interpolations_per_s=per_s(inside, t_fused), project_samples_tested_per_s=per_s(rays * s, t_fused),
                         project_gathered_bytes_per_s=per_s(64 * inside, t_fused), backproject_point_views_per_s=per_s(gathered, t_back),
                         backproject_gathered_bytes_per_s=per_s(32 * gathered, t_back),
                         volume_mb=round(x.numel() * 8 / 1e6, 1), images_mb=round(b.numel() * 8 / 1e6, 1)))
        print(rows[-1], flush=True)
    return rows


def part_recon():
    n, size, s, iters = 64, 64, 128, 50
    shape = (n,) * 3
    a12 = engine.grid_cell_lattice(AABB, [n] * 3)[0]
    poses = training_poses(2)
    views = engine.xray_views(poses, 13.0 * size, size, size, 1400.0, 1600.0, s, device=DEV)
    b = engine.xray_project(phantom_on(shape, a12), views, a12)
    times = []
    for _ in range(6):
        torch.cuda.synchronize()
        t = time.perf_counter()
        x = engine.sirt_reconstruct(views, b, shape, a12, iterations=iters)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter()
    want, _ = sr.sirt(b.cpu().numpy(), shape, a12, views["records"].cpu().numpy(), size, size, 1400.0, 1600.0, s, iters)
    host_s = time.perf_counter() - t
    equal = bool(np.array_equal(x.cpu().numpy().view(np.int64), want.view(np.int64)))
    row = dict(lattice=f"{n}^3", views=len(poses), detector=size, S=s, iterations=iters, device_ms=spread(times[1:], 2), host_s=round(host_s, 1),
               bit_equal=equal)
    print(row, flush=True)
    return row


def part_phantom(n_iters=2048, n=101, iterations=50):
    from nerf_for_angiography_amd.nerf.run_nerf_acc import main, training_view_images, training_view_masks
    from nerf_for_angiography_amd.phantomdata import dataset as ds
    from nerf_for_angiography_amd.visualization import sweep
    with tempfile.TemporaryDirectory() as tmp:
        out = main(["--synthetic", "--binary", "True", "--march", "grid", "--grid_init", "hull", "--img_size", "64", "--number_angles", "4",
                    "--n_iters", str(n_iters), "--display_every", "512", "--num_layers", "4", "--num_hidden_units", "128",
                    "--log_dir", os.path.join(tmp, "run")])
    model = out["model"]
    proj_df, ray_df = ds.make_synthetic_dataset(ds.angle_grid(180.0, 4, [90, 0]), img_size=64, sampling_strategy="segmentation", device=DEV, seed=0,
                                                binary=True)
    held_out = proj_df.index[-1]
    train = ray_df[ray_df["image_id"] != held_out]
    poses, images, focal = training_view_images(proj_df, train, held_out, DEV)
    _, masks, _ = training_view_masks(proj_df, train, held_out, 1.0, DEV)
    views = engine.xray_views(poses, focal, images.shape[2], images.shape[1], 1400.0, 1600.0, 160, device=DEV)
    hull_views = engine.visual_hull_views(poses, masks, focal)
    t = np.linspace(-100.0, 100.0, 129)
    nodes = torch.from_numpy(np.stack(np.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)).to(DEV)
    caps = capsule_tree(levels=5, seed=0)
    mu = torch.cat([capsule_mu(nodes[i:i + (1 << 20)], caps) for i in range(0, nodes.shape[0], 1 << 20)]).cpu().numpy().reshape(129, 129, 129)
    vol = VoxelVolume(t, t, t, mu, fill_value=0.0, device=DEV)
    an = sweep.GridAnalysis(*sweep._reconstruction_grids(model, vol, 100.0, n), 100.0, n)
    b = engine.line_integrals(images)
    free = sweep.reconstruction_sirt_metrics(model, vol, 100.0, n, views, b, iterations=iterations, grids=an)[0]
    held = sweep.reconstruction_sirt_metrics(model, vol, 100.0, n, views, b, iterations=iterations, hull_views=hull_views, grids=an)[0]
    hull = sweep.reconstruction_hull_metrics(model, vol, 100.0, n, hull_views, grids=an)[0]
    row = dict(points=n, views=int(views["n_views"]), detector=int(images.shape[2]), iterations=iterations, train_iterations=n_iters,
               dice_sirt=free["dice_sirt"], dice_sirt_hull_mask=held["dice_sirt"], dice_hull=hull["dice_hull"], dice_model=free["dice_model"],
               corr_sirt=free["corr_sirt"], corr_sirt_hull_mask=held["corr_sirt"], residual=free["residual"], residual_hull_mask=held["residual"],
               n_gt=free["n_gt"], n_sirt=free["n_sirt"], n_sirt_hull_mask=held["n_sirt"], n_pred=free["n_pred"], threshold=free["threshold"],
               test_psnr=out["history"][-1]["test_psnr"])
    # the same at half the vessel's density (mu = 0.2): mean(gt) is so low here that any positive smear counts as vessel
    free = sweep.reconstruction_sirt_metrics(model, vol, 100.0, n, views, b, iterations=iterations, threshold=0.1, grids=an)[0]
    held = sweep.reconstruction_sirt_metrics(model, vol, 100.0, n, views, b, iterations=iterations, hull_views=hull_views, threshold=0.1, grids=an)[0]
    hull = sweep.reconstruction_hull_metrics(model, vol, 100.0, n, hull_views, threshold=0.1, grids=an)[0]
    row["at_threshold_0.1"] = dict(dice_sirt=free["dice_sirt"], dice_sirt_hull_mask=held["dice_sirt"], dice_hull=hull["dice_hull"],
                                   dice_model=free["dice_model"], n_gt=free["n_gt"], n_sirt=free["n_sirt"], n_sirt_hull_mask=held["n_sirt"],
                                   n_pred=free["n_pred"])
    print(row, flush=True)
    return row


def main_cli():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parts", default="kernel,recon,phantom")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sirt_timing: needs an MI355X; nothing is measured without one")
    parts = args.parts.split(",")
    result = {}
    if "kernel" in parts:
        result["kernel"] = part_kernel(args.reps)
    if "recon" in parts:
        result["recon"] = part_recon()
    if "phantom" in parts:
        result["phantom"] = part_phantom()
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# SIRT numbers (tools/sirt_timing.py)\n\n```json\n" + json.dumps(result, indent=1) + "\n```\n")


if __name__ == "__main__":
    main_cli()
