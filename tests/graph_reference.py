"""The yardstick of the centreline-graph tests (include/afx.h: afx_centreline_graph, afx_prune_spurs): a NumPy / scipy.ndimage.label
restatement of the definitions, with no bit tricks - neighbours found one offset after another, paths walked voxel by voxel, lengths and
radius sums added in plain Python floats (IEEE fp64, one rounding per operation) in the stated order.

deg(v) = the on voxels among v's 26 neighbours; J = on with deg >= 3, P = on with deg <= 2; junction nodes / branches = the 26-components
of J / P in scipy.ndimage.label's numbering.  A branch is a path, a single voxel or a cycle; see the header for path order, attachments,
step classes, lengths, radii and the pruning rule."""
import itertools
import math
import struct

import numpy as np
from scipy import ndimage

S26 = np.ones((3, 3, 3), bool)
OFFSETS = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]         # raster order: increasing linear index
RECORD_SLOTS = 16
BRANCH_SLOTS = 16
NONE = 0xffffffff


def step_class(d):
    """0..12: code - 14 of whichever of +-d has code = (d0 + 1) * 9 + (d1 + 1) * 3 + (d2 + 1) above 13."""
    code = (d[0] + 1) * 9 + (d[1] + 1) * 3 + (d[2] + 1)
    if code < 13:
        code = 26 - code
    assert 14 <= code <= 26
    return code - 14


def class_offset(c):
    code = c + 14
    return (code // 9 - 1, code // 3 % 3 - 1, code % 3 - 1)


def unit_lengths():
    return [math.sqrt(float(sum(x != 0 for x in class_offset(c)))) for c in range(13)]


def world_lengths(index_to_world):
    """|A d_c| for the 3 x 3 matrix of a [3, 4] index_to_world, as engine.centreline_graph forms it on the host."""
    a = np.asarray(index_to_world, np.float64).reshape(3, 4)[:, :3]
    return [float(np.sqrt(((a @ np.asarray(class_offset(c), np.float64)) ** 2).sum())) for c in range(13)]


def length_of(counts, lengths):
    acc = float(counts[0]) * lengths[0]
    for c in range(1, 13):
        acc = acc + float(counts[c]) * lengths[c]
    return acc


def degree(mask):
    mask = np.asarray(mask, bool)
    return np.where(mask, ndimage.convolve(mask.astype(np.int32), np.ones((3, 3, 3), np.int32), mode="constant") - 1, -1)


def f64_bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def analyse(skel, d2=None, step_lengths=None):
    """-> dict: node_labels, branch_labels (int32 volumes), path_voxels (int list), branches (list of dicts), record (dict)."""
    s = np.asarray(skel) != 0
    shape = s.shape
    L = unit_lengths() if step_lengths is None else [float(x) for x in step_lengths]
    deg = degree(s)
    J = s & (deg >= 3)
    P = s & (deg <= 2)
    jl, kj = ndimage.label(J, S26)
    bl, nb = ndimage.label(P, S26)
    lin = np.arange(s.size).reshape(shape)

    def neighbours(v, mask):
        out = []
        for o in OFFSETS:
            u = (v[0] + o[0], v[1] + o[1], v[2] + o[2])
            if all(0 <= u[a] < shape[a] for a in range(3)) and mask[u]:
                out.append(u)
        return out

    members = [[] for _ in range(nb)]
    for v in np.argwhere(P):                                                        # raster order
        members[bl[tuple(v)] - 1].append(tuple(int(x) for x in v))
    branches, path_voxels, total = [], [], [0] * 13
    for b in range(1, nb + 1):
        vox = members[b - 1]
        pn = {v: neighbours(v, P) for v in vox}
        assert all(len(x) <= 2 for x in pn.values()), "a P voxel with more than 2 P-neighbours"
        ends = [v for v in vox if len(pn[v]) < 2]
        cyc = not ends
        start = min(ends) if ends else min(vox)
        path, prev, cur = [start], None, start
        while len(path) < len(vox):
            nxt = [u for u in pn[cur] if u != prev]
            if prev is None:
                nxt = [min(nxt)]
            assert len(nxt) == 1 and nxt[0] != start, "not a path or a cycle"
            prev, cur = cur, nxt[0]
            path.append(cur)
        assert len(set(path)) == len(vox)
        if cyc:
            assert len(path) >= 3 and start in pn[path[-1]] and not any(neighbours(v, J) for v in path)
        else:
            assert len(pn[path[-1]]) < 2 and (len(path) == 1 or path[-1] > path[0])
        counts = [0] * 13
        for a, c in zip(path[:-1], path[1:]):
            counts[step_class(np.subtract(c, a))] += 1
        if cyc:
            counts[step_class(np.subtract(path[0], path[-1]))] += 1
        sides = [None, None]                                                        # the J voxel of the start and the end side
        if not cyc:
            if len(path) == 1:
                js = neighbours(path[0], J)
                assert len(js) <= 2
                for q, u in enumerate(js):
                    sides[q] = u
            else:
                for q, v in enumerate((path[0], path[-1])):
                    js = neighbours(v, J)
                    assert len(js) <= 1
                    if js:
                        sides[q] = js[0]
            for q, v in enumerate((path[0], path[-1])):
                if sides[q] is not None:
                    counts[step_class(np.subtract(sides[q], v))] += 1
        att = sum(u is not None for u in sides)
        free = (0 if cyc else 2) - att
        assert free >= 0
        row = {"n": len(path), "offset": len(path_voxels), "cycle": int(cyc), "spur": int(free == 1 and att == 1), "free": free, "att": att,
               "node_start": int(jl[sides[0]]) if sides[0] is not None else 0, "node_end": int(jl[sides[1]]) if sides[1] is not None else 0,
               "counts": counts, "length": length_of(counts, L), "first": int(lin[path[0]]), "last": int(lin[path[-1]]),
               "d2_min": 0, "d2_max": 0, "argmin": 0, "d2_start": 0, "d2_end": 0, "r_sum": 0.0, "path": path, "sides": sides}
        if d2 is not None:
            vals = [int(d2[v]) for v in path]
            row["d2_min"], row["d2_max"] = min(vals), max(vals)
            row["argmin"] = vals.index(min(vals))
            acc = 0.0
            for x in vals:
                acc = acc + math.sqrt(float(x))
            row["r_sum"] = acc
            row["d2_start"] = int(d2[sides[0]]) if sides[0] is not None else 0
            row["d2_end"] = int(d2[sides[1]]) if sides[1] is not None else 0
        branches.append(row)
        path_voxels.extend(int(lin[v]) for v in path)
        total = [x + y for x, y in zip(total, counts)]
    record = {"on": int(s.sum()), "j_voxels": int(J.sum()), "p_voxels": int(P.sum()), "nodes": int(kj), "branches": int(nb),
              "deg0": int((deg == 0).sum()), "deg1": int((deg == 1).sum()), "free_ends": sum(r["free"] for r in branches),
              "cycles": sum(r["cycle"] for r in branches), "spurs": sum(r["spur"] for r in branches), "length": length_of(total, L),
              "d2_min": min((r["d2_min"] for r in branches), default=NONE) if d2 is not None else NONE, "counts": total}
    return {"node_labels": jl.astype(np.int32), "branch_labels": bl.astype(np.int32), "path_voxels": path_voxels, "branches": branches,
            "record": record}


def row_slots(r):
    """The 16 slots of a branch row, as Python ints in 0..2^64 - 1 (fp64 slots as their bits)."""
    c = r["counts"] + [0]
    return ([r["n"] | r["offset"] << 32, (r["cycle"] | r["spur"] << 1 | r["free"] << 8 | r["att"] << 16) | r["argmin"] << 32,
             r["node_start"] | r["node_end"] << 32, r["d2_min"] | r["d2_max"] << 32, r["d2_start"] | r["d2_end"] << 32]
            + [c[2 * q] | c[2 * q + 1] << 32 for q in range(7)]
            + [f64_bits(r["length"]) & (2 ** 64 - 1), f64_bits(r["r_sum"]) & (2 ** 64 - 1), r["first"] | r["last"] << 32, 0])


def record_slots(rec, max_branches=None):
    """The 16 slots of the graph record."""
    over = int(max_branches is not None and rec["branches"] > max_branches)
    return [rec["on"], rec["j_voxels"], rec["p_voxels"], rec["nodes"], rec["branches"], rec["deg0"], rec["deg1"], rec["deg1"] + 2 * rec["deg0"],
            rec["cycles"], rec["spurs"], f64_bits(rec["length"]) & (2 ** 64 - 1), over, rec["d2_min"], 0, 0, 0]


def prune(skel, d2, factor=1.0, max_rounds=None):
    """-> (pruned bool mask, record dict): rounds (the one that deleted nothing included), branches, voxels (deleted), converged,
    remaining, input, last (voxels the last round run deleted)."""
    s = (np.asarray(skel) != 0).copy()
    rec = {"rounds": 0, "branches": 0, "voxels": 0, "converged": 0, "remaining": int(s.sum()), "input": int(s.sum()), "last": 0}
    while not rec["converged"] and (max_rounds is None or rec["rounds"] < max_rounds):
        g = analyse(s, d2)
        kill = [r for r in g["branches"] if r["spur"]
                and r["length"] <= float(factor) * math.sqrt(float(d2[r["sides"][0] if r["sides"][0] is not None else r["sides"][1]]))]
        gone = 0
        for r in kill:
            for v in r["path"]:
                s[v] = False
                gone += 1
        rec["rounds"] += 1
        rec["branches"] += len(kill)
        rec["voxels"] += gone
        rec["last"] = gone
        rec["remaining"] = rec["input"] - rec["voxels"]
        rec["converged"] = int(gone == 0)
    return s, rec


def prune_record_slots(rec):
    return [rec["rounds"], rec["branches"], rec["voxels"], rec["converged"], rec["remaining"], rec["input"], rec["last"], 0]


def squared_edt(mask):
    """The exact integer squared EDT of a mask (0xffffffff everywhere when it has no zero voxel), as afx_distance_transform_edt_3d writes it."""
    mask = np.asarray(mask, bool)
    if mask.all():
        return np.full(mask.shape, NONE, np.int64)
    return np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64)
