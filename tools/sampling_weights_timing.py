"""Time of the projection ray-sampling weights on the GPU (dataset.sampling_weights_device: afx_sampling_weights plus the status
read-back) against the host SciPy segmentation path (dataset.sampling_weights per view), on capsule-tree projections:
1 369 views at 100^2 (the evaluation sweep's 37 x 37) and 25 views at 512^2.  Prints one JSON line.
    python tools/sampling_weights_timing.py [--reps 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_for_angiography_amd.phantomdata import dataset as ds            # noqa: E402
from nerf_for_angiography_amd.phantomdata.helpers import (capsule_mu, capsule_tree, get_depth_values, get_ray_values,  # noqa: E402
                                                          ray_tracing_fn)


def views(size, n_distinct, n, dev):
    caps = capsule_tree(levels=5, seed=0)
    z = get_depth_values(1400.0, 1600.0, 160, dev, stratified=False).float()
    out = []
    for k in range(n_distinct):
        o, d, _, _, _ = get_ray_values(60.0 + 60.0 * k / n_distinct, -30.0 + 60.0 * k / n_distinct, 0.0, np.array([0.0, 0.0, 1500.0]),
                                       size, size, 13.0 * size, dev)
        with torch.no_grad():
            out.append(ray_tracing_fn(lambda p: capsule_mu(p, caps), o.reshape(-1, 3).float(), d.reshape(-1, 3).float(), z).reshape(size, size))
    x = torch.stack(out).double()
    return x.repeat((n + n_distinct - 1) // n_distinct, 1, 1)[:n].contiguous()


def gpu_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for tag, size, n in (("1369x100^2", 100, 1369), ("25x512^2", 512, 25)):
        x = views(size, 37 if size == 100 else 25, n, dev)
        host = x.cpu().numpy()
        r = {}
        for strategy, binary in (("frangi", True), ("frangi", False), ("segmentation", True)):
            r[f"device_{strategy}{'' if binary else '_nonbinary'}_ms"] = round(gpu_ms(lambda: ds.sampling_weights_device(x, strategy, binary), a.reps), 3)
        t = time.perf_counter()
        for im in host:
            ds.sampling_weights(im, "segmentation")
        r["host_scipy_segmentation_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        res[tag] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
