"""Time of the centreline graph (afx_centreline_graph) and of spur pruning (afx_prune_spurs) on the GPU.

What is measured:
  * the skeleton (engine.skeletonize_3d) of the capsule-tree phantom of the skeleton tests scaled to --points (201: the reference's
    depth_samples_per_ray + 1), with the squared distance transform of the phantom;
  * the skeleton of the 64^3 tree with 30 floaters, where the NumPy restatement (tests/graph_reference.py, one run) is timed next to it
    as a yardstick and the device result is compared with it;
  * per input: `engine.centreline_graph_record` and `engine.prune_record` (sync_every = 0, as many rounds as the pruning needs) on
    buffers allocated once - launches only - and `engine.centreline_graph` / `engine.prune_spurs` as a user calls them (allocation,
    the record's read-back, the retry of the branch table, one read-back per pruning round).
Every device time is the MEDIAN of --reps calls, each timed on its own by a host clock around the call and a device synchronise, after
two warm-up calls.  Writes a small report (default profiles/r18_centreline_graph.md) and prints the same numbers as one JSON line.  The
capability is new: the numbers are a record, no gate depends on them.
    python tools/centreline_graph_timing.py [--reps 20] [--points 201] [--out profiles/r18_centreline_graph.md]"""
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
import graph_reference as gr                                                                       # noqa: E402
import skeleton_reference as sk                                                                    # noqa: E402
from nerf_for_angiography_amd import _lib                                                          # noqa: E402
from nerf_for_angiography_amd.engine import (centreline_graph, centreline_graph_record, distance_transform_edt_3d,  # noqa: E402
                                             prune_record, prune_spurs, skeletonize_3d, _d2_u32)


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


def measure(mask, reps, dev, host):
    lib = _lib.load()
    m = torch.from_numpy(mask).to(dev)
    skel = skeletonize_3d(m)
    d2 = distance_transform_edt_3d(m, return_squared=True)[1]
    s8, d32 = skel.to(torch.uint8).contiguous(), _d2_u32(d2, skel, "timing")
    shape, n = tuple(mask.shape), mask.size
    pruned, rec = prune_spurs(skel, d2, 1.0, return_record=True)
    g = centreline_graph(skel, d2)
    out = {"shape": list(shape), "mask_voxels": int(mask.sum()), "skeleton_voxels": g["n_on"], "branches": g["n_branches"], "nodes": g["n_nodes"],
           "free_ends": g["n_free_ends"], "spurs": g["n_spurs"], "longest_branch": int(g["branch_size"].max()) if g["n_branches"] else 0,
           "prune_rounds": rec["rounds"], "spurs_removed": rec["branches"], "voxels_after_pruning": rec["remaining"]}
    cap = max(g["n_branches"], 1)
    bufs = dict(node_labels=torch.empty(shape, dtype=torch.int32, device=dev), branch_labels=torch.empty(shape, dtype=torch.int32, device=dev),
                path_voxels=torch.empty(n, dtype=torch.int32, device=dev), branches=torch.empty((cap, 16), dtype=torch.int64, device=dev),
                record=torch.empty(16, dtype=torch.int64, device=dev),
                workspace=torch.empty(int(lib.afx_centreline_graph_workspace_bytes(*shape)), dtype=torch.uint8, device=dev))
    out["graph_workspace_mib"] = round(bufs["workspace"].numel() / 2 ** 20, 1)
    out["graph_launches_ms"] = median_ms(lambda: centreline_graph_record(s8, d32, None, cap, **bufs), reps)
    out["graph_wall_ms"] = median_ms(lambda: centreline_graph(skel, d2), reps)
    pws = torch.empty(int(lib.afx_prune_spurs_workspace_bytes(*shape)), dtype=torch.uint8, device=dev)
    pout, prec = torch.empty(shape, dtype=torch.uint8, device=dev), torch.empty(8, dtype=torch.int64, device=dev)
    out["prune_workspace_mib"] = round(pws.numel() / 2 ** 20, 1)
    out["prune_launches_ms"] = median_ms(lambda: prune_record(s8, d32, 1.0, rec["rounds"], 0, out=pout, record=prec, workspace=pws), reps)
    out["prune_wall_ms"] = median_ms(lambda: prune_spurs(skel, d2, 1.0), reps)
    assert torch.equal(pout.bool(), pruned)
    if host:
        s_host, d_host = skel.cpu().numpy(), d2.cpu().numpy()
        t = time.perf_counter()
        want = gr.analyse(s_host, d_host)
        out["host_graph_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        t = time.perf_counter()
        want_p, want_rec = gr.prune(s_host, d_host, 1.0)
        out["host_prune_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        out["equals_host"] = bool(g["path_voxels"].tolist() == want["path_voxels"] and g["total_length"] == want["record"]["length"]
                                  and np.array_equal(pruned.cpu().numpy(), want_p) and rec["branches"] == want_rec["branches"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=201)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_centreline_graph.md"))
    args = ap.parse_args()
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "tree": measure(sk.capsule_tree(args.points), args.reps, dev, host=False),
           "tree64_floaters": measure(sk.capsule_tree(64, floaters=30, seed=1), args.reps, dev, host=True)}
    lines = ["# Centreline graph and spur pruning: times", "",
             f"`tools/centreline_graph_timing.py --reps {args.reps} --points {args.points}` on {res['device']}; medians of {args.reps} calls "
             "(min .. max), each call timed by a host clock around the call and a device synchronise, after two warm-up calls.", ""]
    for key, title in (("tree", f"capsule tree, {args.points}^3"), ("tree64_floaters", "capsule tree with 30 floaters, 64^3")):
        r = res[key]
        lines += [f"## {title}", "",
                  f"{r['mask_voxels']} mask voxels, {r['skeleton_voxels']} skeleton voxels, {r['branches']} branches (longest {r['longest_branch']} "
                  f"voxels), {r['nodes']} junction nodes, {r['free_ends']} free ends, {r['spurs']} spurs; pruning at factor 1: {r['prune_rounds']} "
                  f"rounds, {r['spurs_removed']} spurs removed, {r['voxels_after_pruning']} voxels left.", "",
                  "| call | ms |", "|---|---|"]
        for name, label in (("graph_launches_ms", "`centreline_graph_record`, launches only"), ("graph_wall_ms", "`centreline_graph`, as called"),
                            ("prune_launches_ms", f"`prune_record`, {r['prune_rounds']} rounds, launches only"), ("prune_wall_ms", "`prune_spurs`, as called")):
            t = r[name]
            lines.append(f"| {label} | {t['median']} ({t['min']} .. {t['max']}) |")
        if "host_graph_ms" in r:
            lines += [f"| NumPy restatement of the graph, one run | {r['host_graph_ms']} |",
                      f"| NumPy restatement of the pruning, one run | {r['host_prune_ms']} |", "",
                      f"Device result equal to the restatement: {r['equals_host']}."]
        lines += ["", f"Workspace: graph {r['graph_workspace_mib']} MiB, pruning {r['prune_workspace_mib']} MiB.", ""]
    lines += ["Not measured: the per-launch split (the two labellings, the walk), a mask with one very long branch (the walk's sequential worst "
              "case), shapes near 1024^3, and replay from a captured graph.", ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
