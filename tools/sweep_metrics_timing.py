"""Time of the evaluation sweep's SSIM and 3-D metrics on the GPU against their NumPy / SciPy restatement on the host:
afx_ssim (engine.ssim) on 1 369 views at 100^2 (the 37 x 37 sweep) and 25 views at 512^2 against tests/ssim_reference.py, and at 201^3
points (the reference's depth_samples_per_ray + 1) afx_volume_grid alone and reconstruction_metrics (density grid of a 4 x 64 model,
ground-truth grid, DICE 3D, DOT 3D) against scipy's RegularGridInterpolator plus the NumPy scores.  Prints one JSON line.
    python tools/sweep_metrics_timing.py [--reps 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.interpolate import RegularGridInterpolator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssim_reference as sr                                                   # noqa: E402
from nerf_for_angiography_amd.engine import ssim, volume_grid                 # noqa: E402
from nerf_for_angiography_amd.phantomdata.helpers import VoxelVolume          # noqa: E402
from nerf_for_angiography_amd.visualization.sweep import reconstruction_metrics  # noqa: E402


def gpu_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def phantom(n=121, half=60.0, seed=0):
    """A voxel phantom on [-half, half]^3: a few smooth-edged tubes, fp32 [n, n, n], and its axis."""
    ax = np.linspace(-half, half, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    rng = np.random.default_rng(seed)
    mu = np.zeros_like(x)
    for _ in range(6):
        p, d = rng.uniform(-30, 30, 3), rng.normal(size=3)
        d /= np.linalg.norm(d)
        v = np.stack([x - p[0], y - p[1], z - p[2]], -1)
        r = np.linalg.norm(v - (v @ d)[..., None] * d, axis=-1)
        mu = np.maximum(mu, 0.05 / (1 + np.exp((r - rng.uniform(2, 6)) / 0.7)))
    return ax, mu.astype(np.float32)


def model(dev):
    from nerf_for_angiography_amd.model.CPPN import CPPN
    torch.manual_seed(0)
    md = dict(num_early_layers=4, num_late_layers=0, num_filters=64, num_input_channels=3, num_output_channels=1, num_input_channels_views=0,
              use_bias=True, pos_enc="none", pos_enc_basis=5, act_func="relu", fourier_sigma=5, num_img=1, device=dev, precision="f32")
    return CPPN(md).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for tag, size, n in (("ssim_1369x100^2", 100, 1369), ("ssim_25x512^2", 512, 25)):
        x = torch.from_numpy(sr.vessel_views(n, size, size, seed=1)).to(dev)
        g = torch.Generator(device=dev).manual_seed(2)
        y = (x + 0.02 * torch.randn(x.shape, device=dev, generator=g)).contiguous()
        r = {"device_ms": round(gpu_ms(lambda: ssim(x, y), a.reps), 3)}
        hx, hy = x.cpu().numpy(), y.cpu().numpy()
        t = time.perf_counter()
        want = sr.ssim_batch(hx, hy)
        r["host_numpy_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        r["max_abs_diff"] = float(np.abs(ssim(x, y).cpu().numpy() - want).max())
        res[tag] = r
    pts, outside = 201, 100.0
    ax, mu = phantom()
    vol = VoxelVolume(ax, ax, ax, mu, device=dev)
    m = model(dev)
    r = {"device_volume_grid_ms": round(gpu_ms(lambda: volume_grid(vol.values, vol.origin, vol.spacing, vol.fill_value, -outside, outside,
                                                                     pts), a.reps), 3),
         "device_reconstruction_metrics_ms": round(gpu_ms(lambda: reconstruction_metrics(m, vol, outside, pts), a.reps), 3)}
    dice, dot, pred, gt = reconstruction_metrics(m, vol, outside, pts)
    pred = pred.cpu().numpy()
    t = time.perf_counter()
    tt = np.linspace(-outside, outside, pts)
    q = np.stack(np.meshgrid(tt, tt, tt), -1).astype(np.float32).reshape(-1, 3)
    ref = RegularGridInterpolator((ax,) * 3, mu.astype(np.float64), method="linear", bounds_error=False, fill_value=float(mu.min()))(q)
    ref = ref.astype(np.float32).reshape(pts, pts, pts)
    r["host_scipy_grid_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    thr = np.float32(ref.mean(dtype=np.float64))
    host_dice = float(np.mean((pred >= thr) == (ref >= thr)))
    host_dot = float(np.mean(pred.astype(np.float64) * ref))
    r["host_scipy_grid_and_scores_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    r["grid_max_abs_diff"] = float(np.abs(gt.cpu().numpy().astype(np.float64) - ref).max())
    r["dice_3d"], r["dice_3d_host"], r["dot_3d"], r["dot_3d_host"] = dice, host_dice, dot, host_dot
    res[f"3d_{pts}^3"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
