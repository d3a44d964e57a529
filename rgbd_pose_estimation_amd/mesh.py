"""Mesh files for the surface Context.volume_mesh extracts: binary little-endian PLY, numpy only."""
from __future__ import annotations

import numpy as np


def write_ply(path, vertices, triangles, normals=None):
    """Write a binary little-endian PLY: float x y z (and nx ny nz when normals are given) per vertex, a uchar-counted int list of 3
    vertex ids per face."""
    V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    T = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    props = ["x", "y", "z"]
    cols = [V]
    if normals is not None:
        N = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if len(N) != len(V):
            raise ValueError(f"write_ply: {len(N)} normals for {len(V)} vertices")
        props += ["nx", "ny", "nz"]
        cols.append(N)
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(V)}"]
    head += [f"property float {p}" for p in props]
    head += [f"element face {len(T)}", "property list uchar int vertex_indices", "end_header"]
    vert = np.concatenate(cols, 1).astype("<f4")
    face = np.zeros(len(T), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"] = 3
    face["v"] = T
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(vert.tobytes())
        f.write(face.tobytes())


def read_ply(path):
    """(vertices, triangles, normals or None) of a file write_ply wrote"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    if "format binary_little_endian 1.0" not in head:
        raise ValueError("read_ply: not a binary little-endian PLY")
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in head if h.startswith("element face")).split()[-1])
    ncol = sum(1 for h in head if h.startswith("property float"))
    vert = np.frombuffer(data, "<f4", nv * ncol, end).reshape(nv, ncol)
    face = np.frombuffer(data, [("n", "u1"), ("v", "<i4", (3,))], nf, end + vert.nbytes)
    if nf and not np.all(face["n"] == 3):
        raise ValueError("read_ply: only triangles")
    return vert[:, :3].copy(), face["v"].astype(np.int32), (vert[:, 3:6].copy() if ncol >= 6 else None)
