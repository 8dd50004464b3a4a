"""Time of isosurface extraction (afx_isosurface_3d) and of the mesh measures (afx_mesh_measures) at 201^3 points (the reference's
depth_samples_per_ray + 1) on the GPU, against the NumPy restatement on the host (tests/isosurface_reference.py).

What is measured:
  * the capsule-tree phantom of the skeleton tests scaled to --points (a trunk that splits twice), its mask smoothed by a 3 x 3 x 3 mean
    into a density, meshed at 0.5 - a vessel surface: few of the cubes are crossed;
  * a dense random field (uniform in [0, 1), level 0.5) - the worst case: almost every tetrahedron is crossed;
  * per field: the counting call alone, the counting + emitting call on buffers allocated once (`engine.isosurface_record`, launches
    only), `engine.mesh_measures_record` on that mesh, and `engine.extract_isosurface` + `engine.mesh_measures` as a user calls them
    (the read-back of the record, the exact allocation, the cap);
  * the host restatement (isosurface + measures, one run) on the phantom at --points and on the random field at --host-points (it needs
    minutes and tens of GB for the random field at 201^3), and whether the device mesh equals it bit for bit.
Every device time is the MEDIAN of --reps calls, each timed on its own by a host clock around the call and a device synchronise, after
two warm-up calls.  The launches of one call are timed once with torch's profiler (left out when the profiler gives none).  Writes a
small report (default profiles/r16_isosurface.md) and prints the same numbers as one JSON line.  The capability is new: the numbers are
a record, no gate depends on them.
    python tools/isosurface_timing.py [--reps 20] [--points 201] [--host-points 64] [--out profiles/r16_isosurface.md]"""
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
import isosurface_reference as iso                                                                 # noqa: E402
import skeleton_reference as sk                                                                    # noqa: E402
from nerf_for_angiography_amd import _lib                                                          # noqa: E402
from nerf_for_angiography_amd.engine import (extract_isosurface, isosurface_record, mesh_measures,  # noqa: E402
                                             mesh_measures_record)

LAUNCHES = ("k_iso_classify", "k_iso_scan", "k_iso_emit", "k_mm_partial", "k_mm_finish")
AFFINE = (0.0, 1.0, 0.0, -100.0, 1.0, 0.0, 0.0, -100.0, 0.0, 0.0, 1.0, -100.0)      # the evaluation grid's exchange of two axes, unit step


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


def phantom(n, dev):
    mask = torch.from_numpy(sk.capsule_tree(n)).to(dev).float()
    return torch.nn.functional.avg_pool3d(mask[None, None], 3, stride=1, padding=1)[0, 0].contiguous()


def measure(x, level, reps, host):
    dev = x.device
    n_pts = x.numel()
    ws = torch.empty(int(_lib.load().afx_isosurface_3d_workspace_bytes(*x.shape)), dtype=torch.uint8, device=dev)
    rec = torch.empty(8, dtype=torch.int64, device=dev)
    isosurface_record(x, level, AFFINE, record=rec, workspace=ws)
    V, T, E, B, n22 = rec.cpu().tolist()[:5]
    verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
    tris = torch.empty(T, 3, dtype=torch.int32, device=dev)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    mws = torch.empty(int(_lib.load().afx_mesh_measures_workspace_bytes()), dtype=torch.uint8, device=dev)
    count = lambda: isosurface_record(x, level, AFFINE, record=rec, workspace=ws)                                    # noqa: E731
    emit = lambda: isosurface_record(x, level, AFFINE, V, T, vertices=verts, triangles=tris, record=rec, workspace=ws)      # noqa: E731
    meas = lambda: mesh_measures_record(verts, tris, rec, (0.0, 0.0, 0.0), out=out, workspace=mws)                  # noqa: E731

    def user():
        v, t, _ = extract_isosurface(x, level, AFFINE, cap=True, fill=0.0)
        return mesh_measures(v, t)
    r = {"shape": list(x.shape), "points": n_pts, "V": V, "T": T, "E": E, "B": B, "two_and_two": n22, "euler": V - E + T,
         "mesh_bytes": 12 * (V + T), "count_ms": median_ms(count, reps), "count_and_emit_ms": median_ms(emit, reps),
         "measures_ms": median_ms(meas, reps), "extract_isosurface_and_mesh_measures_ms": median_ms(user, reps),
         "launch_us": launch_times(lambda: (emit(), meas()))}
    emit()
    meas()
    r["area"], r["volume"] = out.cpu().tolist()
    if host:
        f = x.cpu().numpy()
        t = time.perf_counter()
        want = iso.isosurface(f, level, AFFINE)
        m = iso.measures(want["vertices"], want["triangles"])
        r["host_restatement_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        r["equal_to_host"] = bool(verts.cpu().numpy().tobytes() == want["vertices"].tobytes() and [V, T, E, B] == [want[k] for k in "VTEB"]
                                  and np.array_equal(iso.rotated_triangles(tris.cpu().numpy()), iso.rotated_triangles(want["triangles"])))
        r["host_area"], r["host_volume"] = m["area"], m["volume"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=201)
    ap.add_argument("--host-points", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_isosurface.md"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, h = a.points, a.host_points
    gen = torch.Generator(device=dev).manual_seed(0)
    res = {"points": n, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "tree": measure(phantom(n, dev), 0.5, a.reps, host=True),
           "random": measure(torch.rand(n, n, n, device=dev, generator=gen), 0.5, a.reps, host=False),
           "random_host_size": measure(torch.rand(h, h, h, device=dev, generator=gen), 0.5, a.reps, host=True)}
    rows = (("tree", f"vessel tree, {n}^3"), ("random", f"dense random, {n}^3"), ("random_host_size", f"dense random, {h}^3"))
    fmt = lambda d: f"{d['median']} ({d['min']} - {d['max']})"                                     # noqa: E731
    lines = [f"# Isosurface extraction and mesh measures at {n}^3 points", "",
             f"`tools/isosurface_timing.py --reps {a.reps} --points {n} --host-points {h}` on {res['device']}.  Device times are the median",
             "(min - max) of that many calls, each timed on its own by a host clock around the call and a device synchronise, after two warm-up",
             "calls.  `count` is the counting call (classify + scan), `count + emit` the full `engine.isosurface_record` call on buffers",
             "allocated once (launches only), `measures` is `engine.mesh_measures_record` on that mesh, `as a user calls it` is",
             "`engine.extract_isosurface(cap=True)` + `engine.mesh_measures`: the pad, the counting call, the read-back of the record, the exact",
             "allocation, the emitting call, the bounding box and the measures.  The host time is one run of the NumPy restatement (isosurface +",
             "measures) - a yardstick, not a tuned host code.  No gate depends on these numbers.", "",
             "| field | V | T | mesh (MB) | count (ms) | count + emit (ms) | measures (ms) | as a user calls it (ms) | host (ms) | equal to host |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for tag, name in rows:
        r = res[tag]
        lines.append(f"| {name} | {r['V']} | {r['T']} | {r['mesh_bytes'] / 1e6:.1f} | {fmt(r['count_ms'])} | {fmt(r['count_and_emit_ms'])} | "
                     f"{fmt(r['measures_ms'])} | {fmt(r['extract_isosurface_and_mesh_measures_ms'])} | {r.get('host_restatement_ms', 'not run')} | "
                     f"{r.get('equal_to_host', 'not run')} |")
    lines += ["", "Device time of the launches of one count + emit + measures call (torch profiler; launches x, microseconds in all):", "",
              "| kernel | " + " | ".join(name for _, name in rows) + " |", "|---|---|---|---|"]
    for k in LAUNCHES:
        cells = []
        for tag, _ in rows:
            n_us = res[tag]["launch_us"].get(k)
            cells.append("n/a" if n_us is None else f"{n_us[0]} x, {n_us[1]}")
        lines.append(f"| {k} | " + " | ".join(cells) + " |")
    lines += ["", "Bytes the launches have to move at the least (from the shapes: the volume read once by classify and once by emit, 5 bytes of",
              "workspace per point written and read, the mesh written once; the eight-fold corner reads are left to the L2):", ""]
    for tag, name in rows:
        r = res[tag]
        least = r["points"] * (4 + 4 + 5 + 5) + r["mesh_bytes"]
        lines.append(f"* {name}: {least / 1e6:.1f} MB; over the median of count + emit: {least / 1e6 / r['count_and_emit_ms']['median']:.1f} GB/s")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
