"""Restatement of the mesh simplification specification (include/bnv_fusion.h, "Mesh simplification"): vertex clustering
on a uniform grid with quadric placement.  This file is the definition: plain Python loops over Python floats (IEEE
float64, one rounding per operation, correctly rounded sqrt and division), every sum in its stated order.  It is
written from the specification and not from mesh.simplify_mesh (no sort tricks, no vectorised rounds);
tests/test_mesh_simplify_cpu.py pins the host function to it bit for bit, tests/test_gpu_mesh_simplify.py the device."""
import math

import numpy as np

EXTENT = 2.0 ** 20


def check(vertices, faces, cell, placement, min_det):
    """The inputs every path refuses, as ValueError -> (v float32 [V, 3], f int64 [T, 3], h, min_det)."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    h, md = float(cell), float(min_det)
    if placement not in ("quadric", "mean"):
        raise ValueError(f"placement must be 'quadric' or 'mean' (got {placement!r})")
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError(f"cell must be finite and > 0 (got {h})")
    if not (math.isfinite(md) and md >= 0.0):
        raise ValueError(f"min_det must be finite and >= 0 (got {md})")
    if len(v) > 2 ** 31 - 2 or len(f) > 2 ** 30:
        raise ValueError("too many vertices or faces")
    if not np.isfinite(v).all():
        raise ValueError("vertices must be finite")
    if len(f) and (len(v) == 0 or f.min() < 0 or f.max() >= len(v)):
        raise ValueError("a face indexes a vertex outside [0, V)")
    for x in v.reshape(-1).tolist():
        if abs(x) / h >= EXTENT:
            raise ValueError("a coordinate is 2^20 cells or more from the origin")
    return v, f, h, md


def cell_index(x, h):
    return math.floor(x / h)


def cell_key(i):
    return (i[0] + 2 ** 20) << 42 | (i[1] + 2 ** 20) << 21 | (i[2] + 2 ** 20)


def corner_quadric(p0, p1, p2):
    """The contribution of one corner: (A00, A01, A02, A11, A12, A22, b0, b1, b2), or None when the face has no area."""
    e1 = [p1[a] - p0[a] for a in range(3)]
    e2 = [p2[a] - p0[a] for a in range(3)]
    n0 = e1[1] * e2[2] - e1[2] * e2[1]
    n1 = e1[2] * e2[0] - e1[0] * e2[2]
    n2 = e1[0] * e2[1] - e1[1] * e2[0]
    L = math.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    if L == 0.0:
        return None
    u0, u1, u2 = n0 / L, n1 / L, n2 / L
    w = 0.5 * L
    d = -((u0 * p0[0] + u1 * p0[1]) + u2 * p0[2])
    wu0, wu1, wu2, wd = w * u0, w * u1, w * u2, w * d
    return (wu0 * u0, wu0 * u1, wu0 * u2, wu1 * u1, wu1 * u2, wu2 * u2, wd * u0, wd * u1, wd * u2)


def solve(q, h, min_det):
    """x minimising the quadric, or None when it is not accepted."""
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = q
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    tr = (a00 + a11) + a22
    if det == 0.0:                    # (x would be infinite or NaN: never within the cell)
        return None
    r0, r1, r2 = -b0, -b1, -b2
    x0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det
    x1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det
    x2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det
    m = tr / 3.0
    if tr > 0.0 and abs(det) >= min_det * ((m * m) * m) and abs(x0) <= h and abs(x1) <= h and abs(x2) <= h:
        return (x0, x1, x2)
    return None


def face_step(c):
    """Faces as cluster triples [T, 3] -> the indices of the faces kept: two equal clusters drop a face; of faces with
    the same cyclic triple the first stays."""
    kept, seen = [], set()
    for t, (a, b, d) in enumerate(np.asarray(c).reshape(-1, 3).tolist()):
        if a == b or b == d or a == d:
            continue
        r = min((a, b, d), (b, d, a), (d, a, b))
        if r not in seen:
            seen.add(r)
            kept.append(t)
    return np.array(kept, dtype=np.int64)


def simplify(vertices, faces, cell, placement="quadric", min_det=1e-3, return_info=False):
    """-> (vertices [V', 3] float32, faces [T', 3] int64) per the specification.  ``return_info``: also a dict with the
    kept clusters' cell indices [V', 3] and whether each took its quadric position."""
    v, f, h, min_det = check(vertices, faces, cell, placement, min_det)
    V, T = len(v), len(f)
    vd = v.astype(np.float64).tolist()
    idx = [tuple(cell_index(x, h) for x in p) for p in vd]
    keys = sorted({cell_key(i) for i in idx})
    number = {k: n for n, k in enumerate(keys)}
    cl = [number[cell_key(i)] for i in idx]
    n_c = len(keys)
    cell_of = [None] * n_c
    for i, c in zip(idx, cl):
        cell_of[c] = i
    # mean: ascending vertex index
    s = [[0.0, 0.0, 0.0] for _ in range(n_c)]
    cnt = [0] * n_c
    for i in range(V):
        c = cl[i]
        for a in range(3):
            s[c][a] = s[c][a] + vd[i][a]
        cnt[c] += 1
    pos = [[s[c][a] / float(cnt[c]) for a in range(3)] for c in range(n_c)]
    took = [False] * n_c
    if placement == "quadric":
        fl = f.tolist()
        q = [[0.0] * 9 for _ in range(n_c)]
        for t in range(T):                                       # ascending corner id 3 t + k
            i0, i1, i2 = fl[t]
            if i0 == i1 or i1 == i2 or i0 == i2:
                continue
            for k in range(3):
                c = cl[fl[t][k]]
                ctr = [(cell_of[c][a] + 0.5) * h for a in range(3)]
                p = [[vd[i][a] - ctr[a] for a in range(3)] for i in (i0, i1, i2)]
                add = corner_quadric(*p)
                if add is not None:
                    for j in range(9):
                        q[c][j] = q[c][j] + add[j]
        for c in range(n_c):
            x = solve(q[c], h, min_det)
            if x is not None:
                pos[c] = [(cell_of[c][a] + 0.5) * h + x[a] for a in range(3)]
                took[c] = True
    fc = np.asarray(cl, dtype=np.int64)[f] if T else np.zeros((0, 3), np.int64)
    fc = fc[face_step(fc)].reshape(-1, 3)
    used = np.unique(fc)
    remap = np.full(n_c, -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    vout = np.asarray([pos[c] for c in used.tolist()], dtype=np.float64).reshape(-1, 3).astype(np.float32)
    out = (vout, remap[fc].reshape(-1, 3))
    if return_info:
        info = {"cells": np.asarray([cell_of[c] for c in used.tolist()], dtype=np.int64).reshape(-1, 3),
                "quadric": np.asarray([took[c] for c in used.tolist()], dtype=bool)}
        return out + (info,)
    return out


# ---- shared test meshes ---------------------------------------------------------------------------------------------
def tetrahedron():
    v = np.array([[0.1, 0.1, 0.1], [1.1, 0.2, 0.15], [0.3, 1.2, 0.2], [0.4, 0.3, 1.3]], dtype=np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int64)
    return v, f


def box(n=6, lo=(-0.31, -0.27, -0.22), hi=(0.33, 0.29, 0.24)):
    """An axis-aligned box, every side a grid of n x n quads: 12 n^2 faces (432 at n = 6), welded, outward winding."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    pts, index, faces = [], {}, []

    def vid(ijk):
        if ijk not in index:
            index[ijk] = len(pts)
            pts.append([lo[a] + (hi[a] - lo[a]) * ijk[a] / n for a in range(3)])
        return index[ijk]

    for axis in range(3):
        a1, a2 = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def at(di, dj):
                        ijk = [0, 0, 0]
                        ijk[axis], ijk[a1], ijk[a2] = side, i + di, j + dj
                        return vid(tuple(ijk))
                    quad = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]
                    if side == 0:
                        quad.reverse()
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return np.asarray(pts, dtype=np.float32), np.asarray(faces, dtype=np.int64)


def uv_sphere(radius=0.4, centre=(0.05, -0.03, 0.02), n_lat=24, n_lon=48):
    """A welded UV sphere: 2 n_lon (n_lat - 1) faces (2208 at 24 x 48)."""
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)),
                     np.outer(np.cos(th), np.ones_like(ph))], -1).reshape(-1, 3)
    p = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]])
    idx = 1 + np.arange(len(ring)).reshape(n_lat - 1, n_lon)
    nxt = np.roll(idx, -1, axis=1)
    f = [np.stack([np.zeros(n_lon, np.int64), idx[0], nxt[0]], -1),
         np.stack([idx[:-1], idx[1:], nxt[:-1]], -1).reshape(-1, 3),
         np.stack([nxt[:-1], idx[1:], nxt[1:]], -1).reshape(-1, 3),
         np.stack([np.full(n_lon, len(p) - 1), nxt[-1], idx[-1]], -1)]
    v = (p * radius + np.asarray(centre)).astype(np.float32)
    return v, np.concatenate(f).astype(np.int64)


def strip(n_vertices, step=0.013):
    """A zig-zag triangle strip of ``n_vertices`` vertices (n - 2 faces) that climbs slowly out of its plane."""
    i = np.arange(n_vertices)
    v = np.stack([i // 2 * step, (i % 2) * 0.021 + 0.003 * np.sin(i), 0.0007 * i], 1).astype(np.float32)
    t = np.arange(n_vertices - 2)
    f = np.where((t % 2 == 0)[:, None], np.stack([t, t + 1, t + 2], 1), np.stack([t + 1, t, t + 2], 1))
    return v, f.astype(np.int64)


def fan(n_faces=300, radius=0.04):
    """``n_faces`` faces around vertex 0, a shallow cone: with a cell over all of it, one cluster's run of corners is
    longer than a wave and a block."""
    a = np.linspace(0, 2 * np.pi, n_faces, endpoint=False)
    rim = np.stack([0.05 + radius * np.cos(a), 0.05 + radius * np.sin(a), 0.03 + 0.004 * np.cos(3 * a)], 1)
    v = np.concatenate([[[0.05, 0.05, 0.045]], rim]).astype(np.float32)
    k = np.arange(n_faces)
    f = np.stack([np.zeros(n_faces, np.int64), 1 + k, 1 + (k + 1) % n_faces], 1)
    return v, f.astype(np.int64)


def adversarial(h=0.125):
    """One mesh with the awkward inputs together, for a cell ``h``: negative coordinates, vertices exactly on cell
    faces (x = k h), duplicated faces in both orders, faces with a repeated index, zero-area faces, unreferenced
    vertices."""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(*[np.arange(-3, 4) * (h / 2)] * 3, indexing="ij"), -1).reshape(-1, 3)      # on cell faces
    r = rng.uniform(-0.4, 0.4, size=(80, 3))
    line = np.stack([np.linspace(-0.3, 0.3, 7), np.full(7, 0.11), np.full(7, -0.07)], 1)                # collinear
    v = np.concatenate([g, r, line, rng.uniform(-0.4, 0.4, size=(9, 3))]).astype(np.float32)             # last 9: unused
    n_ref = len(v) - 9
    f = rng.integers(0, n_ref, size=(400, 3))
    lo = len(g) + len(r)
    extra = [[lo, lo + 1, lo + 2], [lo + 2, lo + 4, lo + 6],                                            # zero area
             [5, 5, 9], [7, 300, 7], [12, 12, 12],                                                      # repeated index
             f[0].tolist(), f[1][[1, 2, 0]].tolist(), f[2][[2, 1, 0]].tolist(), f[3].tolist()]          # duplicates
    return v, np.concatenate([f, np.asarray(extra)]).astype(np.int64)
