"""A NumPy restatement of the territories (include/afx.h: afx_feature_transform_3d, afx_label_overlap_3d) and of the per-branch scores
built on them (visualization/sweep.py: reconstruction_branch_metrics).  The feature transform is a brute-force arg-min over all sites - no
separable pass, no tile, no early stop - so it shares nothing with the kernels but the definition; keep voxels x sites below ~10^7."""
import numpy as np
from scipy import ndimage

import graph_reference as gr
import skeleton_reference as sr

NONE = 0xffffffff


def feature_transform(sites):
    """-> (d2 int64, nearest int64), both of the mask's shape: the smallest squared voxel distance to a site and the LOWEST linear index
    among the sites at that distance; (0xffffffff, -1) everywhere without a site."""
    s = np.asarray(sites) != 0
    shape = s.shape
    if not s.any():
        return np.full(shape, NONE, np.int64), np.full(shape, -1, np.int64)
    idx = np.flatnonzero(s)                                                         # ascending linear index
    sc = np.stack(np.unravel_index(idx, shape), axis=1).astype(np.int64)
    vc = np.stack(np.unravel_index(np.arange(s.size), shape), axis=1).astype(np.int64)
    d2, nearest = np.empty(s.size, np.int64), np.empty(s.size, np.int64)
    step = max(1, 2_000_000 // len(idx))
    for lo in range(0, s.size, step):
        dd = ((vc[lo:lo + step, None, :] - sc[None, :, :]) ** 2).sum(axis=2)
        k = np.argmin(dd, axis=1)                                                   # the first minimum: the lowest site index
        d2[lo:lo + step], nearest[lo:lo + step] = dd[np.arange(len(k)), k], idx[k]
    return d2.reshape(shape), nearest.reshape(shape)


def label_overlap(labels, a, b=None, index=None, d2=None, max_d2=None, n_labels=None):
    """-> (counts int64 [n_labels + 1, 4], territory int32 of labels' shape), voxel by voxel as include/afx.h states it."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    n = lab.size
    n_labels = max(int(lab.max()), 0) if n_labels is None else int(n_labels)
    s = np.arange(n) if index is None else np.asarray(index).astype(np.int64).reshape(-1)
    out = (s < 0) | (s >= n)
    if d2 is not None:
        out |= np.asarray(d2).astype(np.int64).reshape(-1) > int(max_d2)
    l = np.where(out, 0, lab[np.where(out, 0, s)])
    l = np.where((l < 1) | (l > n_labels), 0, l)
    ia = np.asarray(a).reshape(-1) != 0
    ib = np.zeros(n, bool) if b is None else np.asarray(b).reshape(-1) != 0
    counts = np.zeros((n_labels + 1, 4), np.int64)
    np.add.at(counts[:, 0], l, 1)
    np.add.at(counts[:, 1], l, ia.astype(np.int64))
    np.add.at(counts[:, 2], l, ib.astype(np.int64))
    np.add.at(counts[:, 3], l, (ia & ib).astype(np.int64))
    return counts, l.astype(np.int32).reshape(np.asarray(labels).shape)


def site_labels(graph):
    """The labels of the sites of a graph_reference.analyse result -> (labels int32 volume, B, K): branch b -> b, junction node k -> B + k."""
    bl, jl = graph["branch_labels"].astype(np.int64), graph["node_labels"].astype(np.int64)
    nb, nk = int(graph["record"]["branches"]), int(graph["record"]["nodes"])
    return np.where(bl > 0, bl, np.where(jl > 0, jl + nb, 0)).astype(np.int32), nb, nk


def tree(mask, index_to_world=None, prune_factor=1.0):
    """The centreline of a bool mask by the existing restatements -> {"d2", "skeleton", "pruned", "graph"}: the squared EDT, the thinned
    mask, its spurs pruned, and the pruned skeleton read as a graph (lengths in world units with index_to_world)."""
    mask = np.asarray(mask, bool)
    d2 = gr.squared_edt(mask)
    skeleton, _ = sr.skeletonize(mask)
    pruned, _ = gr.prune(skeleton, d2, prune_factor)
    lengths = None if index_to_world is None else gr.world_lengths(index_to_world)
    return {"d2": d2, "skeleton": skeleton, "pruned": pruned, "graph": gr.analyse(pruned, d2, lengths)}


def branch_table(a, b, tree_pred, tree_true, max_d2=None, found_at=0.5):
    """The per-branch table and the scores of reconstruction_branch_metrics, row by row in plain loops -> (scores, table): table[key][l - 1]
    for label l (branches, then junctions)."""
    nan = float("nan")
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    labels, nb, nk = site_labels(tree_true["graph"])
    d2, nearest = feature_transform(labels > 0)
    terr = label_overlap(labels, a, b, nearest, d2 if max_d2 is not None else None, max_d2, nb + nk)[1]
    d2_off, near_p = feature_transform(tree_pred["pruned"])
    have_pred = bool(np.asarray(tree_pred["pruned"]).any())
    keys = ("n_pred", "n_gt", "n_both", "dice", "sensitivity", "precision", "coverage", "length", "offset", "radius_true", "radius_pred", "found")
    table = {k: [] for k in keys}
    for l in range(1, nb + nk + 1):
        t = terr == l
        n_pred, n_gt, n_both = int((t & a).sum()), int((t & b).sum()), int((t & a & b).sum())
        own = np.flatnonzero(labels.reshape(-1) == l)                               # raster order
        table["n_pred"].append(n_pred), table["n_gt"].append(n_gt), table["n_both"].append(n_both)
        table["dice"].append(2.0 * n_both / (n_pred + n_gt) if n_pred + n_gt else nan)
        table["sensitivity"].append(n_both / n_gt if n_gt else nan)
        table["precision"].append(n_both / n_pred if n_pred else nan)
        table["coverage"].append(float(a.reshape(-1)[own].sum()) / len(own))
        table["length"].append(float(tree_true["graph"]["branches"][l - 1]["length"]) if l <= nb else 0.0)
        table["radius_true"].append(float(np.mean(np.sqrt(tree_true["d2"].reshape(-1)[own].astype(np.float64)))))
        if have_pred:
            table["offset"].append(float(np.mean(np.sqrt(d2_off.reshape(-1)[own].astype(np.float64)))))
            table["radius_pred"].append(float(np.mean(np.sqrt(tree_pred["d2"].reshape(-1)[near_p.reshape(-1)[own]].astype(np.float64)))))
        else:
            table["offset"].append(nan), table["radius_pred"].append(nan)
        table["found"].append(l <= nb and table["coverage"][-1] >= found_at)
    found = [l for l in range(nb) if table["found"][l]]
    total = found_length = 0.0                                                      # plain left-to-right sums
    for l in range(nb):
        total = total + table["length"][l]
        found_length = found_length + (table["length"][l] if table["found"][l] else 0.0)
    errs = [abs(table["radius_pred"][l] - table["radius_true"][l]) / table["radius_true"][l] for l in found if table["radius_true"][l] > 0]
    union = a | b
    scores = {"branch_recall": len(found) / nb if nb else nan,
              "branch_recall_length": found_length / total if nb and total > 0 else nan,
              "worst_branch_dice": min(table["dice"][:nb]) if nb else nan,
              "branch_radius_err": float(np.mean(errs)) if errs else nan,
              "unassigned": float((union & (terr == 0)).sum()) / float(union.sum()) if union.any() else nan,
              "n_branches": nb, "n_junctions": nk, "n_found": len(found)}
    return scores, table, terr


# ---- the hand-built scenes: a Y of three voxel tubes ----
N = 24                                # the scenes live on an N^3 grid
OUTSIDE = 11.5                        # +-OUTSIDE over N points: a grid step of exactly 1


def y_truth():
    """A trunk along axis 2 that forks into two arms in the plane of axes 0 and 2, tubes of radius 2.2 voxels."""
    shape = (N, N, N)
    m = sr.capsule(shape, (12, 12, 3), (12, 12, 11), 2.2)
    m |= sr.capsule(shape, (12, 12, 11), (5, 12, 20), 2.2)
    m |= sr.capsule(shape, (12, 12, 11), (19, 12, 20), 2.2)
    return m


def without_branch(truth, tree_true, branch):
    """The truth without the territory of one branch: every voxel that lies nearest to it is removed."""
    labels, nb, nk = site_labels(tree_true["graph"])
    d2, nearest = feature_transform(labels > 0)
    terr = label_overlap(labels, truth, None, nearest, None, None, nb + nk)[1]
    return truth & (terr != branch)


def dilated(truth):
    """The truth grown by one voxel along the 6 face directions."""
    return ndimage.binary_dilation(truth, ndimage.generate_binary_structure(3, 1))
