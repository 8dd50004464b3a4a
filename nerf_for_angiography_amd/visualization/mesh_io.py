"""Triangle meshes on disk: binary STL (what the LCA phantom comes as) and legacy VTK POLYDATA (what the reference's viewer reads).

Host plumbing: the arrays are what `engine.extract_isosurface` / `sweep.reconstruction_mesh` return (tensors on any device, or arrays).
Both writers write atomically, as nerf/checkpoint.py does: to a temporary name in the same directory, flushed, then os.replace - a
write that fails half-way leaves no partial file and keeps a previous file as it was."""
from __future__ import annotations

import os

import numpy as np


def _arrays(vertices, triangles, who):
    def host(x):
        return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    v = np.ascontiguousarray(host(vertices), dtype=np.float32)
    t = np.ascontiguousarray(host(triangles), dtype=np.int64)
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"{who}: vertices must have shape [V, 3] and triangles [T, 3], got {v.shape} and {t.shape}")
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError(f"{who}: a triangle names a vertex outside 0..{len(v) - 1}")
    if not np.isfinite(v).all():
        raise ValueError(f"{who}: a vertex is not finite")
    return v, t


def _write_atomically(path, chunks):
    path = str(path)
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            for c in chunks:
                f.write(c)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return path


def facet_normals(vertices, triangles):
    """Unit normals by the right-hand rule of (v0, v1, v2), fp64 -> float32 [T, 3]; (0, 0, 0) for a degenerate triangle."""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[triangles[:, 0]], v[triangles[:, 1]], v[triangles[:, 2]]
    n = np.cross(b - a, c - a)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(length > 0, n / np.where(length > 0, length, 1.0), 0.0).astype(np.float32)


def write_stl(path, vertices, triangles, header: str = "nerf_for_angiography_amd mesh"):
    """Binary STL: 80 bytes of header, uint32 T, then per triangle the facet normal (from the winding), the three corners (float32,
    little-endian) and a zero attribute word.  STL is a triangle soup: the welding is lost, the winding is not."""
    v, t = _arrays(vertices, triangles, "write_stl")
    if len(t) > 0xffffffff:
        raise ValueError("write_stl: more than 2^32 - 1 triangles")
    rec = np.zeros(len(t), dtype=np.dtype([("normal", "<f4", 3), ("corners", "<f4", (3, 3)), ("attr", "<u2")]))
    rec["normal"] = facet_normals(v, t)
    rec["corners"] = v[t]
    head = header.encode("ascii", "replace")[:80].ljust(80, b" ")
    if head.lstrip().lower().startswith(b"solid"):      # readers take such a file for ASCII STL
        raise ValueError("write_stl: the header must not start with 'solid'")
    return _write_atomically(path, [head, np.uint32(len(t)).astype("<u4").tobytes(), rec.tobytes()])


def write_vtk_polydata(path, vertices, triangles, binary: bool = True, title: str = "nerf_for_angiography_amd mesh"):
    """Legacy VTK (version 3.0) POLYDATA: POINTS as float, POLYGONS as (3, i, j, k) per triangle; binary = big-endian, as the format
    asks.  The welded, indexed mesh is kept as it is."""
    v, t = _arrays(vertices, triangles, "write_vtk_polydata")
    if len(v) > 2 ** 31 - 1:
        raise ValueError("write_vtk_polydata: more than 2^31 - 1 vertices")
    title = title.replace("\n", " ")[:255]
    cells = np.concatenate([np.full((len(t), 1), 3, dtype=np.int64), t], axis=1)
    chunks = [f"# vtk DataFile Version 3.0\n{title}\n{'BINARY' if binary else 'ASCII'}\nDATASET POLYDATA\nPOINTS {len(v)} float\n".encode("ascii")]
    if binary:
        chunks += [v.astype(">f4").tobytes(), f"\nPOLYGONS {len(t)} {4 * len(t)}\n".encode("ascii"), cells.astype(">i4").tobytes(), b"\n"]
    else:
        chunks += ["".join(f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n" for p in v).encode("ascii"),
                   f"POLYGONS {len(t)} {4 * len(t)}\n".encode("ascii"),
                   "".join(f"3 {c[1]} {c[2]} {c[3]}\n" for c in cells).encode("ascii")]
    return _write_atomically(path, chunks)


def write_mesh(path, vertices, triangles):
    """By the file name: .stl -> write_stl, .vtk -> write_vtk_polydata (binary)."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".stl":
        return write_stl(path, vertices, triangles)
    if ext == ".vtk":
        return write_vtk_polydata(path, vertices, triangles)
    raise ValueError(f"write_mesh: {path}: the name must end in .stl or .vtk")
