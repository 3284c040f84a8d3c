"""Signed distance to a triangle mesh, restated from its definition (include/bnv_fusion.h: bnv_mesh_sdf_query): a
chunked brute force over ALL triangles in numpy, float64 unless asked otherwise, with pseudonormal signs and feature
codes.  It shares nothing with csrc/meshsdf.hip: no grid, no fixed point, no hash table.  Also the test meshes (a
tessellated box, a torus, an open height field) and their analytic distances.

Not a test module (no ``test_`` prefix): tests/test_mesh_sdf_cpu.py, tests/test_gpu_mesh_sdf.py and
tests/test_gpu_patches.py import it.
"""
import numpy as np

BOUNDARY, NONMANIFOLD = 0x10, 0x20
ULP32 = 2.0 ** -23


# --------------------------------------------------------------------------- #
# topology: valid faces, face / vertex / edge pseudonormals, boundary flags
# --------------------------------------------------------------------------- #
def valid_faces(V, F):
    """The faces the index keeps: indices in range, fp32 area 0.5 |e1 x e2| positive and finite (one rounding per
    operation, as bnv_mesh_sample_surface), and a cross product that is not exactly zero in float64."""
    V32 = np.asarray(V, np.float32)
    F = np.asarray(F, np.int64)
    ok = ((F >= 0) & (F < len(V32))).all(1)
    Fc = np.where(ok[:, None], F, 0)
    with np.errstate(all="ignore"):
        a, b, c = V32[Fc[:, 0]], V32[Fc[:, 1]], V32[Fc[:, 2]]
        e1, e2 = b - a, c - a
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = np.float32(0.5) * np.sqrt(((cx * cx + cy * cy) + cz * cz).astype(np.float64)).astype(np.float32)
        n64 = np.cross(b.astype(np.float64) - a.astype(np.float64), c.astype(np.float64) - a.astype(np.float64))
        ok &= (area > 0) & np.isfinite(area) & (np.linalg.norm(n64, axis=1) > 0)
    return ok


class Topology:
    """Of the valid faces of (V, F): ``faces`` [T] their indices into F, ``tri`` [T, 3] vertex indices, ``normal``
    [T, 3] unit normals, ``vertex_normal`` [NV, 3] angle-weighted sums, ``edge_of`` [T, 3] the edge id of edge
    (k, k + 1), ``edge_normal`` [E, 3] sums of the incident unit normals, ``edge_flag`` [E] and ``vertex_flag`` [NV]
    (BOUNDARY: an edge with one face / a vertex of such an edge; NONMANIFOLD: more than two faces)."""

    def __init__(self, V, F):
        self.V = np.asarray(V, np.float32).astype(np.float64)
        F = np.asarray(F, np.int64)
        self.faces = np.nonzero(valid_faces(V, F))[0]
        self.tri = F[self.faces]
        P = self.V[self.tri]                                        # [T, 3, 3]
        n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        self.normal = n / np.linalg.norm(n, axis=1, keepdims=True)
        self.vertex_normal = np.zeros((len(self.V), 3))
        for k in range(3):
            a, b = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
            angle = np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))
            np.add.at(self.vertex_normal, self.tri[:, k], angle[:, None] * self.normal)
        ends = np.stack([self.tri, np.roll(self.tri, -1, axis=1)], -1)   # [T, 3, 2]: edge k = (k, k + 1)
        ends = np.sort(ends, axis=-1).reshape(-1, 2)
        uniq, inv, count = np.unique(ends, axis=0, return_inverse=True, return_counts=True)
        self.edge_of = inv.reshape(-1, 3)
        self.edge_normal = np.zeros((len(uniq), 3))
        np.add.at(self.edge_normal, inv.reshape(-1), np.repeat(self.normal, 3, axis=0))
        self.edge_flag = np.where(count == 1, BOUNDARY, np.where(count > 2, NONMANIFOLD, 0)).astype(np.uint8)
        self.vertex_flag = np.zeros(len(self.V), np.uint8)
        for col in range(2):
            np.bitwise_or.at(self.vertex_flag, uniq[:, col], self.edge_flag)


# --------------------------------------------------------------------------- #
# closest point on a triangle: the seven regions
# --------------------------------------------------------------------------- #
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest_on_triangles(P, A, B, C):
    """Closest point of every triangle (A, B, C) [1, t, 3] to every point P [n, 1, 3], in the arrays' dtype -> (closest
    [n, t, 3], code [n, t]: 0 face | 1 edge ab, 2 edge bc, 3 edge ca | 4 vertex a, 5 vertex b, 6 vertex c).  The
    Voronoi region of the point decides: the projections d1 .. d6 onto ab and ac from the three corners select the
    vertex regions, the signs of the barycentric numerators va, vb, vc the edge regions, else the face."""
    ab, ac = B - A, C - A
    ap, bp, cp = P - A, P - B, P - C
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6),
             (vc <= 0) & (d1 >= 0) & (d3 <= 0), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    code = np.select(conds, [4, 5, 6, 1, 3, 2], 0)
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    with np.errstate(all="ignore"):
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = one / ((va + vb) + vc)
        s = np.select([code == 5, code == 1, code == 0], [one, d1 / (d1 - d3), vb * denom], zero)
        t = np.select([code == 6, code == 3, code == 0], [one, d2 / (d2 - d6), vc * denom], zero)
        closest = (A + s[..., None] * ab) + t[..., None] * ac
        closest = np.where((code == 5)[..., None], B, closest)
        closest = np.where((code == 6)[..., None], C, closest)
        closest = np.where((code == 2)[..., None], B + t_bc[..., None] * (C - B), closest)
    return closest, code


def mesh_sdf(P, V, F, dtype=np.float64, pairs=400000, topology=None):
    """Brute force over all valid triangles -> dict: ``sdf`` (negative inside), ``face`` (index into F, the lowest
    among equal d2), ``closest``, ``feature`` (0 face | 1 edge | 2 vertex, | BOUNDARY, | NONMANIFOLD), ``second`` (the
    second smallest distance over the triangles; inf with one triangle).  Closest points and d2 are computed in
    ``dtype`` (float32: one rounding per numpy operation, the precision the kernel works in); the sign is always
    (P - closest) . pseudonormal of the closest feature in float64.  A non-finite point gets (nan, -1, nan, 0)."""
    top = topology or Topology(V, F)
    P = np.asarray(P, np.float32)
    n, T = len(P), len(top.faces)
    out = {"sdf": np.full(n, np.nan, np.float64), "face": np.full(n, -1, np.int64),
           "closest": np.full((n, 3), np.nan, np.float64), "feature": np.zeros(n, np.uint8),
           "second": np.full(n, np.inf, np.float64)}
    if T == 0:
        return out
    tri = top.V[top.tri].astype(dtype)
    A, B, C = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    finite = np.isfinite(P).all(1)
    rows = np.nonzero(finite)[0]
    step = max(1, pairs // T)
    for s in range(0, len(rows), step):
        r = rows[s:s + step]
        p = P[r].astype(dtype)[:, None, :]
        closest, code = closest_on_triangles(p, A, B, C)
        d = p - closest
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        best = np.argmin(d2, axis=1)                                 # the first minimum: the lowest face index
        k = np.arange(len(r))
        bc, bcode = closest[k, best].astype(np.float64), code[k, best]
        dist = np.sqrt(d2[k, best].astype(np.float64))
        if dtype == np.float32:
            dist = dist.astype(np.float32).astype(np.float64)
        if T > 1:
            out["second"][r] = np.sqrt(np.partition(d2, 1, axis=1)[:, 1].astype(np.float64))
        # pseudonormal and flags of the closest feature
        tv = top.tri[best]
        normal = top.normal[best].copy()
        flag = np.zeros(len(r), np.uint8)
        cls = np.zeros(len(r), np.uint8)
        for e in (1, 2, 3):
            m = bcode == e
            eid = top.edge_of[best[m], e - 1]
            normal[m], flag[m], cls[m] = top.edge_normal[eid], top.edge_flag[eid], 1
        for c in (4, 5, 6):
            m = bcode == c
            vid = tv[m, c - 4]
            normal[m], flag[m], cls[m] = top.vertex_normal[vid], top.vertex_flag[vid], 2
        dot = ((P[r].astype(np.float64) - bc) * normal).sum(1)
        out["sdf"][r] = np.where(dot < 0, -dist, dist)
        out["face"][r] = top.faces[best]
        out["closest"][r] = bc
        out["feature"][r] = cls | flag
    return out


# --------------------------------------------------------------------------- #
# test meshes with analytic distances
# --------------------------------------------------------------------------- #
def rotation(seed):
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def box_mesh(center, R, half, n=6):
    """A closed box of half extents ``half`` at pose (R, center), every face ``n`` x ``n`` quads, vertices shared
    across faces, outward orientation -> (V float32 [*, 3], F int64 [*, 3], the shape for synthetic.shape_sdf)."""
    center, half = np.asarray(center, np.float64), np.asarray(half, np.float64)
    ids = -np.ones((n + 1, n + 1, n + 1), np.int64)
    verts = []
    for i in range(n + 1):
        for j in range(n + 1):
            for k in range(n + 1):
                if i in (0, n) or j in (0, n) or k in (0, n):
                    ids[i, j, k] = len(verts)
                    verts.append((np.array([i, j, k]) * (2.0 / n) - 1.0) * half)
    faces = []
    for axis in range(3):
        ua, va = (axis + 1) % 3, (axis + 2) % 3
        for side, idx in ((1, n), (-1, 0)):
            for u in range(n):
                for v in range(n):
                    def vid(du, dv):
                        c = [0, 0, 0]
                        c[axis], c[ua], c[va] = idx, u + du, v + dv
                        return ids[c[0], c[1], c[2]]
                    quad = [vid(0, 0), vid(1, 0), vid(1, 1), vid(0, 1)]
                    if side < 0:
                        quad = quad[::-1]
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    V = center + np.array(verts) @ np.asarray(R).T
    return V.astype(np.float32), np.array(faces, np.int64), {"kind": "box", "center": center, "rotation": np.asarray(R),
                                                            "half": half}


def torus_mesh(R=0.5, r=0.2, nu=48, nv=24, center=(0.3, -0.2, 0.4)):
    """A closed torus around the z axis through ``center``: ``nu`` segments around the axis, ``nv`` around the tube."""
    u = np.arange(nu) * (2 * np.pi / nu)
    v = np.arange(nv) * (2 * np.pi / nv)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    V = np.stack([(R + r * np.cos(vv)) * np.cos(uu), (R + r * np.cos(vv)) * np.sin(uu), r * np.sin(vv)], -1)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b = idx, np.roll(idx, -1, axis=0)
    c, d = np.roll(b, -1, axis=1), np.roll(a, -1, axis=1)
    F = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return (V.reshape(-1, 3) + np.asarray(center)).astype(np.float32), F.astype(np.int64)


def torus_sdf(p, R=0.5, r=0.2, center=(0.3, -0.2, 0.4)):
    p = np.asarray(p, np.float64) - np.asarray(center)
    return np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - R) ** 2 + p[:, 2] ** 2) - r


def torus_sagittas(R=0.5, r=0.2, nu=48, nv=24):
    """How far the chords of the two circles lie inside them: the mesh deviates from the torus by at most their sum."""
    return (R + r) * (1 - np.cos(np.pi / nu)) + r * (1 - np.cos(np.pi / nv))


def height_field(n=24, lo=(-0.6, -0.4), hi=(0.6, 0.4)):
    """An open surface z = f(x, y) over a rectangle, ``n`` x ``n`` quads, normals up -> (V float32, F, (lo, hi) of the
    rim as float32 values)."""
    x = np.linspace(lo[0], hi[0], n + 1).astype(np.float32)
    y = np.linspace(lo[1], hi[1], n + 1).astype(np.float32)
    xx, yy = np.meshgrid(x, y, indexing="ij")
    zz = 0.1 * np.sin(3.0 * xx) * np.cos(2.0 * yy) + 0.05 * xx
    V = np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    F = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return V, F.astype(np.int64), ((float(x[0]), float(y[0])), (float(x[-1]), float(y[-1])))


def on_rim(closest, rim):
    (x0, y0), (x1, y1) = rim
    c = np.asarray(closest, np.float64)
    return (c[:, 0] == x0) | (c[:, 0] == x1) | (c[:, 1] == y0) | (c[:, 1] == y1)


def largest_coordinate(V, P):
    V, P = np.asarray(V, np.float64), np.asarray(P, np.float64)
    return float(max(np.abs(V[np.isfinite(V).all(1)]).max(), np.abs(P[np.isfinite(P).all(1)]).max()))


# --------------------------------------------------------------------------- #
# the cases the kernel is pinned on (tests/test_gpu_mesh_sdf.py)
# --------------------------------------------------------------------------- #
def kernel_cases():
    """-> [(name, V float32 [*, 3], F int64 [*, 3], P float32 [*, 3] finite queries)]"""
    from bnv_fusion_amd import sequence, synthetic
    rng = np.random.default_rng(11)
    cases = []
    V, F, _ = box_mesh((1.0, -0.5, 2.0), rotation(3), (0.31, 0.22, 0.17), n=6)
    cases.append(("box", V, F, (np.array([1.0, -0.5, 2.0]) + rng.uniform(-0.5, 0.5, (20000, 3))).astype(np.float32)))
    Vt, Ft = torus_mesh()
    cases.append(("torus", Vt, Ft, (np.array([0.3, -0.2, 0.4]) + rng.uniform(-0.9, 0.9, (20000, 3)) *
                                    np.array([1.0, 1.0, 0.5])).astype(np.float32)))
    Vh, Fh, _ = height_field()
    cases.append(("height_field", Vh, Fh, (rng.uniform(-1.0, 1.0, (8000, 3)) * np.array([0.9, 0.7, 0.4])).astype(np.float32)))
    m = sequence.gt_mesh()
    lo, hi = m.vertices.min(0), m.vertices.max(0)
    cases.append(("sequence.gt_mesh", m.vertices, m.faces,
                  (lo + rng.uniform(-0.05, 1.05, (20000, 3)) * (hi - lo)).astype(np.float32)))
    m = synthetic.gt_mesh(step_px=8)
    near = m.vertices[rng.integers(0, len(m.vertices), 3000)] + rng.normal(scale=0.05, size=(3000, 3))
    cases.append(("synthetic.gt_mesh(8)", m.vertices, m.faces, near.astype(np.float32)))
    # duplicated faces, degenerate faces (a repeated index, collinear vertices), an index out of range, a NaN vertex
    Vd = np.concatenate([V, np.array([[1.0, -0.5, 2.0], [1.5, -0.5, 2.0], [2.0, -0.5, 2.0], [np.nan, 0.0, 0.0]], np.float32)])
    k = len(V)
    extra = np.array([[0, 0, 1], [k, k + 1, k + 2], [0, 1, k + 9], [0, 1, k + 3], [-1, 0, 1]], np.int64)
    Fd = np.concatenate([extra[:2], F[::3], F, extra[2:], F[5:40]])
    cases.append(("duplicates_and_degenerates", Vd, Fd,
                  (np.array([1.0, -0.5, 2.0]) + rng.uniform(-0.5, 0.5, (5000, 3))).astype(np.float32)))
    Vs = np.array([[0.2, 0.1, -0.3], [1.1, 0.3, 0.2], [0.4, 0.9, 0.5]], np.float32)
    cases.append(("single_triangle", Vs, np.array([[0, 1, 2]], np.int64), rng.uniform(-1.0, 2.0, (2000, 3)).astype(np.float32)))
    far = rng.normal(size=(2000, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(5.0, 50.0, (2000, 1))
    cases.append(("far_queries", Vt, Ft, (np.array([0.3, -0.2, 0.4]) + far).astype(np.float32)))
    return cases
