"""Time of the mesh -> signed-distance-field path (afx_mesh_sdf_3d, afx_mesh_point_distance) on the GPU, against the NumPy restatement on
the host (tests/mesh_sdf_reference.py).

The mesh is the capped surface of the capsule-tree phantom of tests/skeleton_reference.py at n^3 points (smoothed by a 3^3 box, meshed at
0.5 by engine.extract_isosurface); the field is computed on the same n^3 grid, n = 64 and n = 201 (the reference's depth_samples_per_ray + 1).
Per size: the grid call as `engine.mesh_sdf_record` issues it on buffers allocated once (launches only), culled (the default), with
AFX_MESH_SDF_CLOSED, and with AFX_MESH_SDF_BRUTE (the comparator; only up to --brute-points, its cost is N T exact distances), timed with
HIP events after a warm-up; the record's counts (which share of the N T pairs the distance pass evaluated, how many bricks were clear); and
the point call for the mesh-to-mesh scores (the vertices of that mesh against the triangles of the mesh at 0.4, and back).  A variant whose
first run takes longer than --once-above seconds is timed by that run alone.  The host restatement runs once at --host-points (about a
minute: it is the yardstick of the tests, not the code under test) and the GPU result is compared with it bit for bit.

Writes a small report (default profiles/r17_mesh_sdf.md) and prints the same numbers as one JSON line.  The capability is new: the numbers
are a record, not a gate.
    python tools/mesh_sdf_timing.py [--reps 5] [--points 64 201] [--brute-points 64] [--host-points 32] [--out profiles/r17_mesh_sdf.md]"""
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
import mesh_sdf_reference as ref                                                                    # noqa: E402
import skeleton_reference as sk                                                                     # noqa: E402
from nerf_for_angiography_amd import _lib                                                           # noqa: E402
from nerf_for_angiography_amd.engine import (MESH_SDF_BRUTE, MESH_SDF_CLOSED, extract_isosurface,   # noqa: E402
                                             mesh_point_distance_record, mesh_sdf_record)

# what hipcc -Rpass-analysis=kernel-resource-usage reports for the kernels of afx_kernels_sdf.hip (gfx950, -O3)
RESOURCES = {"k_sdf_prepare": "38 VGPRs, no LDS, 8 waves per SIMD", "k_sdf_grid": "114 VGPRs, no spills, 59 432 bytes of LDS, 4 waves per SIMD",
             "k_mesh_point_distance": "88 VGPRs, no spills, 19 488 bytes of LDS, 5 waves per SIMD"}


def affine(n):
    """the evaluation grid's exchange of two axes over [-100, 100]^3"""
    step = 200.0 / (n - 1)
    return (0.0, step, 0.0, -100.0, step, 0.0, 0.0, -100.0, 0.0, 0.0, step, -100.0)


def phantom_mesh(n, level, dev):
    mask = torch.from_numpy(sk.capsule_tree(n)).to(dev).float()
    x = torch.nn.functional.avg_pool3d(mask[None, None], 3, stride=1, padding=1)[0, 0].contiguous()
    v, t, info = extract_isosurface(x, level, affine(n), cap=True, fill=0.0)
    return v, t, info


def event_ms(fn, reps, once_above):
    """median / min / max of the device time of fn (HIP events); one warm-up run, which is the only run when it is a long one"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    first = start.elapsed_time(stop)
    if first > once_above * 1e3:
        return {"median": round(first, 1), "runs": 1}
    times = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return {"median": round(statistics.median(times), 3), "min": round(min(times), 3), "max": round(max(times), 3), "runs": reps}


def measure(n, reps, brute, once_above, dev):
    v, t, info = phantom_mesh(n, 0.5, dev)
    v2, t2, _ = phantom_mesh(n, 0.4, dev)
    shape, aff = (n, n, n), affine(n)
    sdf = torch.empty(shape, dtype=torch.float32, device=dev)
    rec = torch.empty(8, dtype=torch.int64, device=dev)
    ws = torch.empty(int(_lib.load().afx_mesh_sdf_3d_workspace_bytes(t.shape[0])), dtype=torch.uint8, device=dev)
    pairs = n ** 3 * t.shape[0]
    bricks = (-(-n // 8)) ** 3
    r = {"points": n ** 3, "V": int(v.shape[0]), "T": int(t.shape[0]), "B": info["B"], "pairs": pairs, "bricks": bricks, "variants": {}}
    results = {}
    for name, flags in (("culled", 0), ("closed", MESH_SDF_CLOSED)) + ((("brute", MESH_SDF_BRUTE),) if brute else ()):
        call = lambda: mesh_sdf_record(v, t, shape, aff, flags, sdf=sdf, record=rec, workspace=ws)          # noqa: E731
        ms = event_ms(call, reps, once_above)
        counts = rec.cpu().tolist()
        results[name] = sdf.clone()
        r["variants"][name] = {"ms": ms, "pairs_evaluated": counts[3], "share_of_pairs": counts[3] / pairs, "clear_bricks": counts[2],
                               "valid_triangles": counts[0]}
    r["closed_equals_culled"] = bool(torch.equal(results["closed"], results["culled"]))
    if brute:
        r["brute_equals_culled"] = bool(torch.equal(results["brute"], results["culled"]))
    r["inside_points"] = int((results["culled"] < 0).sum())
    d12 = torch.empty(v.shape[0], dtype=torch.float32, device=dev)
    d21 = torch.empty(v2.shape[0], dtype=torch.float32, device=dev)
    prec = torch.empty(8, dtype=torch.int64, device=dev)

    def both():
        mesh_point_distance_record(v, v2, t2, dist=d12, record=prec)
        mesh_point_distance_record(v2, v, t, dist=d21, record=prec)
    r["point_call"] = {"ms": event_ms(both, reps, once_above), "pairs": int(v.shape[0]) * int(t2.shape[0]) + int(v2.shape[0]) * int(t.shape[0]),
                       "assd": float((d12.double().mean() + d21.double().mean()) / 2), "hd": float(torch.maximum(d12.max(), d21.max()))}
    return r


def host(n, dev):
    v, t, _ = phantom_mesh(n, 0.5, dev)
    vh, th = v.cpu().numpy(), t.cpu().numpy()
    t0 = time.perf_counter()
    want = ref.mesh_sdf(vh, th, (n, n, n), affine(n))
    sec = time.perf_counter() - t0
    got, _ = mesh_sdf_record(v, t, (n, n, n), affine(n))
    return {"points": n ** 3, "T": int(t.shape[0]), "pairs": n ** 3 * int(t.shape[0]), "seconds": round(sec, 1),
            "equal_to_gpu": bool(got.cpu().numpy().tobytes() == want["sdf"].tobytes())}


def fmt(ms):
    return f"{ms['median']} ({ms['min']} .. {ms['max']}, {ms['runs']} runs)" if ms["runs"] > 1 else f"{ms['median']} (one run)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, nargs="+", default=[64, 201])
    ap.add_argument("--brute-points", type=int, default=64)
    ap.add_argument("--host-points", type=int, default=32)
    ap.add_argument("--once-above", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_mesh_sdf.md"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "sizes": {}}
    measure(16, 1, True, 1e9, dev)                                                                   # warm-up: the library, the allocator
    for n in a.points:
        res["sizes"][str(n)] = measure(n, a.reps, n <= a.brute_points, a.once_above, dev)
    if a.host_points:
        res["host"] = host(a.host_points, dev)
    lines = ["# Mesh to signed distance field: device times", "",
             f"`tools/mesh_sdf_timing.py --reps {a.reps} --points {' '.join(map(str, a.points))} --brute-points {a.brute_points} --host-points "
             f"{a.host_points}` on {res['device']}.  Device times in ms between two HIP events around the launches of one call, the median "
             "(min .. max) after a warm-up run; a call whose warm-up run took more than a second was timed by that run alone.  The mesh is "
             "the capped surface of the capsule-tree phantom at n^3 points, the field is computed on the same n^3 grid (N points, T "
             "triangles, N T pairs).  `share` is the record's count of exact point-triangle distances over N T: what the culling left.", "",
             "Brick: 8 x 8 x 8 points, one 512-thread workgroup.  Kernels (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): "
             + "; ".join(f"`{k}` {v}" for k, v in RESOURCES.items()) + ".", "",
             "| n | N | T | variant | ms | share of N T evaluated | clear bricks / bricks |", "|---|---|---|---|---|---|---|"]
    for n, r in res["sizes"].items():
        for name, v in r["variants"].items():
            lines.append(f"| {n} | {r['points']} | {r['T']} | {name} | {fmt(v['ms'])} | {v['share_of_pairs']:.4%} | {v['clear_bricks']} / {r['bricks']} |")
    lines += ["", "| n | point call: both directions of the mesh-to-mesh scores, ms | pairs | ASSD | HD |", "|---|---|---|---|---|"]
    for n, r in res["sizes"].items():
        p = r["point_call"]
        lines.append(f"| {n} | {fmt(p['ms'])} | {p['pairs']} | {p['assd']:.4f} | {p['hd']:.4f} |")
    lines += [""] + [f"n = {n}: closed equals culled bit for bit: {r['closed_equals_culled']}"
                     + (f"; brute equals culled bit for bit: {r['brute_equals_culled']}" if "brute_equals_culled" in r else "")
                     + f"; {r['inside_points']} points inside." for n, r in res["sizes"].items()]
    if "host" in res:
        h = res["host"]
        lines += ["", f"Host restatement (NumPy, all pairs, one run) at {a.host_points}^3 points against {h['T']} triangles ({h['pairs']} pairs): "
                      f"{h['seconds']} s; equal to the GPU result bit for bit: {h['equal_to_gpu']}."]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
