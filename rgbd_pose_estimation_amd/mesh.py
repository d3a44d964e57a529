"""Mesh files for the surface Context.volume_mesh extracts: binary little-endian PLY, numpy only."""
from __future__ import annotations

import numpy as np


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """Write a binary little-endian PLY: float x y z (and nx ny nz when normals are given), then uchar red green blue alpha when colors
    ((V, 4) uint8 RGBA, as Context.volume_mesh_colors returns them) are given, per vertex; a uchar-counted int list of 3 vertex ids per
    face."""
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
    fields = [(p, "<f4") for p in props]
    if colors is not None:
        Cl = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        if len(Cl) != len(V):
            raise ValueError(f"write_ply: {len(Cl)} colours for {len(V)} vertices")
        fields += [(p, "u1") for p in _COLOR_PROPS]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(V)}"]
    head += [f"property float {p}" for p in props]
    if colors is not None:
        head += [f"property uchar {p}" for p in _COLOR_PROPS]
    head += [f"element face {len(T)}", "property list uchar int vertex_indices", "end_header"]
    vert = np.zeros(len(V), dtype=fields)
    flt = np.concatenate(cols, 1)
    for i, p in enumerate(props):
        vert[p] = flt[:, i]
    if colors is not None:
        for i, p in enumerate(_COLOR_PROPS):
            vert[p] = Cl[:, i]
    face = np.zeros(len(T), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"] = 3
    face["v"] = T
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(vert.tobytes())
        f.write(face.tobytes())


_COLOR_PROPS = ("red", "green", "blue", "alpha")
_PLY_TYPES = {"float": "<f4", "uchar": "u1"}


def _read(path):
    """(vertex record array, face record array) of a file write_ply wrote"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    if "format binary_little_endian 1.0" not in head:
        raise ValueError("read_ply: not a binary little-endian PLY")
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in head if h.startswith("element face")).split()[-1])
    first_face = next(i for i, h in enumerate(head) if h.startswith("element face"))
    fields = []
    for h in head[:first_face]:
        w = h.split()
        if w[0] == "property":
            if w[1] not in _PLY_TYPES:
                raise ValueError(f"read_ply: vertex property type {w[1]} is not supported")
            fields.append((w[2], _PLY_TYPES[w[1]]))
    vert = np.frombuffer(data, fields, nv, end)
    face = np.frombuffer(data, [("n", "u1"), ("v", "<i4", (3,))], nf, end + vert.nbytes)
    if nf and not np.all(face["n"] == 3):
        raise ValueError("read_ply: only triangles")
    return vert, face


def read_ply(path):
    """(vertices, triangles, normals or None) of a file write_ply wrote (with or without colours: read_ply_colors has them)"""
    vert, face = _read(path)
    names = vert.dtype.names
    V = np.stack([vert[p] for p in ("x", "y", "z")], 1).astype(np.float32)
    N = np.stack([vert[p] for p in ("nx", "ny", "nz")], 1).astype(np.float32) if "nx" in names else None
    return V, face["v"].astype(np.int32), N


def read_ply_colors(path):
    """(V, 4) uint8 RGBA of a file write_ply wrote with colours, None without"""
    vert, _ = _read(path)
    if "red" not in vert.dtype.names:
        return None
    return np.stack([vert[p] for p in _COLOR_PROPS], 1).astype(np.uint8)
