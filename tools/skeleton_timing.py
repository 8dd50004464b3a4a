"""Time of 3-D thinning to medial curves (afx_skeletonize_3d) at 201^3 points (the reference's depth_samples_per_ray + 1) on the GPU, and
of the sequential host restatement (tests/skeleton_reference.py) at a size where that finishes.

What is measured:
  * the capsule-tree phantom of the tests scaled to --points (a trunk that splits twice, radii 7 to 18 voxels at 201), alone and with
    200 single-voxel floaters;
  * per mask: the passes needed; `engine.skeleton_record` with sync_every = 0 and exactly the passes needed, on buffers allocated once
    (launches only, nothing read back); `engine.skeletonize_3d` (allocations, a look at the record every 4 passes, the read-back);
  * the same phantom at --host-points (default 64) on the device and by the host restatement, the two results compared.
Every device time is the MEDIAN of --reps calls, each timed on its own by a host clock around the call and a device synchronise, after
two warm-up calls.  The launches of one call are timed once with torch's profiler (kernel names and device times, summed per kernel;
left out when the profiler gives none).  Writes a small report (default profiles/r14_skeleton.md) and prints the same numbers as one
JSON line.  The capability is new: the numbers are a record, no gate depends on them.
    python tools/skeleton_timing.py [--reps 20] [--points 201] [--host-points 64] [--out profiles/r14_skeleton.md]"""
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
from nerf_for_angiography_amd import _lib                                                          # noqa: E402
from nerf_for_angiography_amd.engine import skeleton_record, skeletonize_3d                       # noqa: E402

LAUNCHES = ("k_sk_reset", "k_sk_init", "k_sk_mark", "k_sk_subfield", "k_sk_advance")


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
    return statistics.median(times), min(times), max(times)


def launch_times(fn):
    """{kernel: (launches, device microseconds in all)} of one call of fn, from torch's profiler; {} when it reports no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for name in LAUNCHES:
                if name in ev.key:
                    us = getattr(ev, "device_time_total", None)
                    if us is None:
                        us = getattr(ev, "cuda_time_total", 0.0)
                    n, t = out.get(name, (0, 0.0))
                    out[name] = (n + int(ev.count), round(t + float(us), 1))
        return out
    except Exception as e:                                                                         # the numbers are a record, not a gate
        print("per-launch times not available:", repr(e), file=sys.stderr)
        return {}


def measure(mask, reps, dev, host=False):
    x = torch.from_numpy(mask.astype(np.uint8)).to(dev)
    ws = torch.empty(int(_lib.load().afx_skeletonize_3d_workspace_bytes(*x.shape)), dtype=torch.uint8, device=dev)
    skel = torch.empty_like(x)
    rec = torch.empty(8, dtype=torch.int64, device=dev)
    s, record = skeletonize_3d(x, return_record=True)
    passes = record["passes"]
    call = lambda: skeleton_record(x, passes, 0, skel=skel, record=rec, workspace=ws)                  # noqa: E731
    med, lo, hi = median_ms(call, reps)
    med2, lo2, hi2 = median_ms(lambda: skeletonize_3d(x), reps)
    border = int(sk.border(mask).sum())
    r = {"shape": list(mask.shape), "foreground": int(mask.sum()), "border_voxels_first_pass": border, "skeleton_voxels": record["remaining"],
         "passes": passes, "launches_per_call": 2 + 10 * passes,
         "device_launches_ms": {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)},
         "device_skeletonize_3d_ms": {"median": round(med2, 3), "min": round(lo2, 3), "max": round(hi2, 3)},
         "launch_us": launch_times(call)}
    call()
    r["fixed_form_equals_synchronised_form"] = bool(torch.equal(skel.bool(), s) and rec.cpu().tolist()[:6] == list(record.values()))
    if host:
        t = time.perf_counter()
        want, wrec = sk.skeletonize(mask)
        r["host_restatement_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        r["equal_to_host"] = bool(np.array_equal(s.cpu().numpy(), want) and wrec["passes"] == passes)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=201)
    ap.add_argument("--host-points", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_skeleton.md"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.points
    res = {"points": n, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "tree": measure(sk.capsule_tree(n), a.reps, dev),
           "tree_floaters": measure(sk.capsule_tree(n, floaters=200, seed=1), a.reps, dev),
           "host_size": measure(sk.capsule_tree(a.host_points, floaters=30, seed=1), a.reps, dev, host=True)}
    rows = (("tree", f"capsule tree, {n}^3"), ("tree_floaters", f"capsule tree + 200 floaters, {n}^3"),
            ("host_size", f"capsule tree + 30 floaters, {a.host_points}^3"))
    lines = [f"# Thinning to medial curves at {n}^3 points", "",
             f"`tools/skeleton_timing.py --reps {a.reps} --points {n} --host-points {a.host_points}` on {res['device']}.  Device times are the",
             "median (min - max) of that many calls, each timed on its own by a host clock around the call and a device synchronise, after two",
             "warm-up calls: `launches` is `engine.skeleton_record` with sync_every = 0 and exactly the passes needed on buffers allocated once",
             "(2 + 10 launches per pass, nothing read back), `skeletonize_3d` includes its allocations, a look at the record every 4 passes and",
             "the read-back.  The host time is one run of the sequential restatement.  No gate depends on these numbers.", "",
             "| mask | foreground | border voxels, pass 1 | skeleton | passes | launches (ms) | skeletonize_3d (ms) | host (ms) | equal to host |",
             "|---|---|---|---|---|---|---|---|---|"]
    for tag, name in rows:
        r = res[tag]
        d, e = r["device_launches_ms"], r["device_skeletonize_3d_ms"]
        lines.append(f"| {name} | {r['foreground']} | {r['border_voxels_first_pass']} | {r['skeleton_voxels']} | {r['passes']} | "
                     f"{d['median']} ({d['min']} - {d['max']}) | {e['median']} ({e['min']} - {e['max']}) | {r.get('host_restatement_ms', 'not run')} | "
                     f"{r.get('equal_to_host', 'not run')} |")
    lines += ["", "Device time of the launches of one call (torch profiler; launches x, microseconds in all):", "",
              "| kernel | " + " | ".join(name for _, name in rows) + " |", "|---|---|---|---|"]
    for k in LAUNCHES:
        cells = []
        for tag, _ in rows:
            n_us = res[tag]["launch_us"].get(k)
            cells.append("n/a" if n_us is None else f"{n_us[0]} x, {n_us[1]}")
        lines.append(f"| {k} | " + " | ".join(cells) + " |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
