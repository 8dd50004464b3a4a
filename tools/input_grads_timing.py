"""Time of the backward with and without gradients with respect to the rays, at the bench shape (512^2 rays x 128 samples, 8 x 256,
f16s8) and at the reference's batch (5 625 rays x 300 samples, 4 x 128, f16s8): afx_render_backward alone (parameters), with input
gradients (afx_render_backward_inputs: parameters + origins + directions) and input-only (a frozen model: no weight-gradient kernels).
Device time per call from CUDA events, median of --reps calls after one warm-up.  Prints one JSON line; --out also writes it to a file.
    python tools/input_grads_timing.py [--reps 5] [--out profiles/input_grads_timing.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_for_angiography_amd.engine import RenderSpec                          # noqa: E402
from nerf_for_angiography_amd.model.CPPN import CPPN                           # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = (("bench 512^2x128, 8x256", 8, 256, 512 * 512, 128), ("reference batch 5625x300, 4x128", 4, 128, 5625, 300))


def events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return sorted(out)[len(out) // 2]


def run(layers, width, n_rays, n_samples, reps, prec="f16s8"):
    torch.manual_seed(0)
    md = dict(num_early_layers=layers, num_late_layers=0, num_filters=width, num_input_channels=3, num_output_channels=1,
              num_input_channels_views=0, use_bias=True, pos_enc="none", pos_enc_basis=5, act_func="relu", fourier_sigma=5, num_img=1,
              device=DEV, precision=prec)
    m = CPPN(md).to(DEV)
    o = (torch.randn(n_rays, 3, device=DEV) * 5 + torch.tensor([0.0, 0.0, -150.0], device=DEV)).contiguous()
    d = (torch.randn(n_rays, 3, device=DEV) * 0.1 + torch.tensor([0.0, 0.0, 1.0], device=DEV)).contiguous()
    spec = RenderSpec(n_rays=n_rays, n_samples=n_samples, origins=o, dirs=d, mode="acc", t_near=100.0, t_far=200.0)
    e, prep = m.engine, m._prepared()
    pixel, _, _ = e.render_forward(prep, spec, prec)
    dpix = torch.randn(n_rays, device=DEV)
    grad = torch.zeros(e.param_count, device=DEV)
    d_o, d_d = torch.empty(n_rays, 3, device=DEV), torch.empty(n_rays, 3, device=DEV)
    return {
        "params_only_ms": events_ms(lambda: e.render_backward(prep, spec, pixel, dpix, grad, prec), reps),
        "params_and_rays_ms": events_ms(lambda: e.render_backward_inputs(prep, spec, pixel, dpix, grad, d_o, d_d, prec), reps),
        "rays_only_ms": events_ms(lambda: e.render_backward_inputs(prep, spec, pixel, dpix, None, d_o, d_d, prec), reps),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "prec": "f16s8", "reps": args.reps}
    for name, layers, width, n_rays, s in SHAPES:
        res[name] = run(layers, width, n_rays, s, args.reps)
        print(name, res[name], flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
