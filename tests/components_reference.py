"""The yardstick of the connected-component tests (include/afx.h: afx_label_components_3d): scipy.ndimage.label with
generate_binary_structure(3, c) - background 0, components 1..K numbered in raster order of their first voxel - its sizes by
np.bincount, and a plain breadth-first flood fill in raster order, written without SciPy, that pins SciPy's numbering on tiny volumes."""
from collections import deque

import numpy as np
from scipy import ndimage


def label(mask, c):
    """(labels int32, K) of mask != 0 with connectivity c = 1, 2, 3 (6, 18, 26 neighbours)."""
    labels, k = ndimage.label(np.asarray(mask) != 0, structure=ndimage.generate_binary_structure(3, c))
    return labels.astype(np.int32), int(k)


def sizes(labels):
    """sizes[l - 1] = the voxels of component l (int64 [K])."""
    return np.bincount(np.asarray(labels).ravel())[1:].astype(np.int64)


def label_flood(mask, c):
    """The same by flood fill: walk the voxels in raster order, give every unlabelled foreground voxel the next label and spread it
    breadth-first over the neighbours that differ by 1 along at most c axes."""
    mask = np.asarray(mask) != 0
    n0, n1, n2 = mask.shape
    steps = [(a, b, d) for a in (-1, 0, 1) for b in (-1, 0, 1) for d in (-1, 0, 1) if 0 < (a != 0) + (b != 0) + (d != 0) <= c]
    labels = np.zeros(mask.shape, np.int32)
    k = 0
    for i in range(n0):
        for j in range(n1):
            for l in range(n2):
                if not mask[i, j, l] or labels[i, j, l]:
                    continue
                k += 1
                labels[i, j, l] = k
                todo = deque([(i, j, l)])
                while todo:
                    x, y, z = todo.popleft()
                    for a, b, d in steps:
                        u, v, w = x + a, y + b, z + d
                        if 0 <= u < n0 and 0 <= v < n1 and 0 <= w < n2 and mask[u, v, w] and not labels[u, v, w]:
                            labels[u, v, w] = k
                            todo.append((u, v, w))
    return labels, k


def largest(labels):
    """(label, size, first linear index) of the largest component, ties to the smaller label; (0, 0, 0) without foreground."""
    s = sizes(labels)
    if s.size == 0:
        return 0, 0, 0
    l = int(np.argmax(s)) + 1                     # argmax returns the first maximum
    return l, int(s[l - 1]), int(np.flatnonzero(np.asarray(labels).ravel() == l)[0])


def record(labels, k):
    """The 8-slot record afx_label_components_3d writes."""
    l, n, first = largest(labels)
    return [int(np.count_nonzero(labels)), int(k), n, l, first, 0, 0, 0]


def edge_pair(shape=(3, 4, 5), at=(1, 1, 1)):
    """Two voxels that share only an edge: 2 / 1 / 1 components for c = 1 / 2 / 3."""
    m = np.zeros(shape, bool)
    m[at] = m[at[0], at[1] + 1, at[2] + 1] = True
    return m


def corner_pair(shape=(3, 4, 5), at=(0, 1, 1)):
    """Two voxels that share only a corner: 2 / 2 / 1."""
    m = np.zeros(shape, bool)
    m[at] = m[at[0] + 1, at[1] + 1, at[2] + 1] = True
    return m


def checkerboard(shape=(6, 7, 8)):
    """(i + j + k) % 2 == 0: 168 / 1 / 1 components on 6 x 7 x 8."""
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    return (i + j + k) % 2 == 0
