"""Time of the 3-D Frangi vesselness (afx_frangi_3d) on the GPU.

What is measured, for sigmas = (1, 2, 3) on the capsule-tree phantom of the skeleton tests as a float32 0 / 1 volume at 64^3 and at
--points^3 (201: the reference's depth_samples_per_ray + 1):
  * `engine.frangi_3d_record` on buffers allocated once - launches only - and `engine.frangi_3d` as a user calls it (allocation included);
  * the same launches from the build variant that recomputes the eigenvalues in the vessel kernel instead of keeping them
    (`python -m nerf_for_angiography_amd.build --variant=f3drc`; skipped when that library has not been built), the two alternating;
  * at 64^3 the NumPy / SciPy restatement (tests/frangi3d_reference.py, one run) as a yardstick, and the device result against it;
  * tubular_fraction_gt of the phantom: the share of its voxels with vesselness >= 0.1.
Every device time is the MEDIAN of --reps calls, each timed on its own by a host clock around the call and a device synchronise, after
two warm-up calls.  The per-kernel split comes from a run of its own under the profiler (`rocprofv3 --kernel-trace --stats -- python
tools/frangi3d_timing.py --reps 5 --no-host --out <scratch>`): its kernel names are k_f3_gauss<axis>, k_f3_eigen, k_f3_vessel.
Writes a small report (default profiles/r19_frangi3d.md) and prints the same numbers as one JSON line.  The capability is new: the
numbers are a record, no gate depends on them.
    python tools/frangi3d_timing.py [--reps 20] [--points 201] [--no-host] [--out profiles/r19_frangi3d.md]"""
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
import frangi3d_reference as fr                                                                    # noqa: E402
import skeleton_reference as sk                                                                    # noqa: E402
from nerf_for_angiography_amd import _lib                                                          # noqa: E402
from nerf_for_angiography_amd.build import lib_path                                                # noqa: E402
from nerf_for_angiography_amd.engine import Engine, frangi_3d, frangi_3d_record                    # noqa: E402

SIGMAS = (1.0, 2.0, 3.0)


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


def raw_call(lib, x, out, idx, ws):
    sg = (C.c_double * len(SIGMAS))(*SIGMAS)
    _lib.check(lib.afx_frangi_3d(x.data_ptr(), int(x.dtype == torch.float64), *x.shape, sg, len(SIGMAS), 0.5, 0.5, 0.0, 0, out.data_ptr(),
                                 idx.data_ptr(), ws.data_ptr(), ws.numel(), None, Engine._stream(x.device)), "afx_frangi_3d", lib)


def measure(mask, reps, dev, host):
    lib = _lib.load()
    x = torch.from_numpy(mask.astype(np.float32)).to(dev)
    shape = tuple(x.shape)
    out, idx = torch.empty(shape, dtype=torch.float64, device=dev), torch.empty(shape, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(lib.afx_frangi_3d_workspace_bytes(*shape, len(SIGMAS))), dtype=torch.uint8, device=dev)
    res = {"shape": list(shape), "mask_voxels": int(mask.sum()), "workspace_mib": round(ws.numel() / 2 ** 20, 1)}
    res["launches_ms"] = median_ms(lambda: frangi_3d_record(x, SIGMAS, out=out, scale_index=idx, workspace=ws), reps)
    res["wall_ms"] = median_ms(lambda: frangi_3d(x, SIGMAS, return_scale=True), reps)
    v = out.clone()
    res["tubular_fraction_gt"] = float((v[x > 0] >= 0.1).double().mean())
    if os.path.exists(lib_path("f3drc")):
        rc = _lib.load("f3drc")
        ws2 = torch.empty(int(rc.afx_frangi_3d_workspace_bytes(*shape, len(SIGMAS))), dtype=torch.uint8, device=dev)
        keep, again = [], []
        for _ in range(3):                                                            # alternating, so that a drift of the machine hits both
            keep.append(median_ms(lambda: raw_call(lib, x, out, idx, ws), reps)["median"])
            again.append(median_ms(lambda: raw_call(rc, x, out, idx, ws2), reps)["median"])
        res["keep_eigenvalues_ms"], res["recompute_eigenvalues_ms"] = keep, again
        res["recompute_workspace_mib"] = round(ws2.numel() / 2 ** 20, 1)
        res["recompute_equals_keep"] = bool(torch.equal(out, v))
    if host:
        t = time.perf_counter()
        want, want_idx = fr.frangi_3d(mask.astype(np.float64), SIGMAS, return_scale=True)
        res["host_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        res["max_error_over_max"] = float(np.abs(v.cpu().numpy() - want).max() / want.max())
        res["zero_pattern_differences"] = int(((v.cpu().numpy() == 0) != (want == 0)).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=201)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_frangi3d.md"))
    args = ap.parse_args()
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "sigmas": SIGMAS,
           "tree64": measure(sk.capsule_tree(64), args.reps, dev, host=not args.no_host),
           "tree": measure(sk.capsule_tree(args.points), args.reps, dev, host=False)}
    lines = ["# 3-D Frangi vesselness: times", "",
             f"`tools/frangi3d_timing.py --reps {args.reps} --points {args.points}` on {res['device']}; sigmas {SIGMAS}, float32 input; medians of "
             f"{args.reps} calls (min .. max), each call timed by a host clock around the call and a device synchronise, after two warm-up calls.", ""]
    for key, title in (("tree64", "capsule tree, 64^3"), ("tree", f"capsule tree, {args.points}^3")):
        r = res[key]
        lines += [f"## {title}", "", f"{r['mask_voxels']} phantom voxels; tubular_fraction_gt (vesselness >= 0.1 on the phantom's own voxels) "
                  f"{r['tubular_fraction_gt']:.4f}; workspace {r['workspace_mib']} MiB.", "", "| call | ms |", "|---|---|"]
        for name, label in (("launches_ms", "`frangi_3d_record`, launches only"), ("wall_ms", "`frangi_3d`, as called")):
            t = r[name]
            lines.append(f"| {label} | {t['median']} ({t['min']} .. {t['max']}) |")
        if "keep_eigenvalues_ms" in r:
            lines += [f"| eigenvalues kept in the workspace, three medians | {r['keep_eigenvalues_ms']} |",
                      f"| eigenvalues recomputed by the vessel kernel (variant f3drc, workspace {r['recompute_workspace_mib']} MiB), three medians, "
                      f"alternating with the line above | {r['recompute_eigenvalues_ms']} |", "",
                      f"Recomputed result bit-identical to the kept one: {r['recompute_equals_keep']}."]
        else:
            lines += ["", "Kept against recomputed eigenvalues: not measured (the f3drc variant was not built)."]
        if "host_ms" in r:
            lines += ["", f"NumPy / SciPy restatement, one run: {r['host_ms']} ms; device against it: max |difference| / max = "
                      f"{r['max_error_over_max']:.2e}, zero-pattern differences {r['zero_pattern_differences']}."]
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
