"""numpy restatement of the mesh components specification (include/bnv_fusion.h, "Mesh components"), written from the
specification and not from mesh.connected_components: min-label propagation over edge groups instead of scipy's
connected_components, Python integers for the area sums.  tests/test_mesh_components_cpu.py pins it to the host
functions bit for bit; the GPU tests hold the device to the host."""
import math

import numpy as np

import mesh_post_restatement as post_rs


def face_units(vertices, faces):
    """[T] Python ints: q = rint(area * 2^50), float64 from the float32 coordinates, one rounding per operation."""
    out = []
    for t in np.asarray(faces, np.int64).reshape(-1, 3):
        a, b, c = (np.asarray(vertices, np.float32)[i].astype(np.float64) for i in t)
        e1, e2 = b - a, c - a
        cx = e1[1] * e2[2] - e1[2] * e2[1]
        cy = e1[2] * e2[0] - e1[0] * e2[2]
        cz = e1[0] * e2[1] - e1[1] * e2[0]
        area = 0.5 * math.sqrt((cx * cx + cy * cy) + cz * cz)
        out.append(int(np.rint(area * 2.0 ** 50)))
    return out


def components(vertices, faces):
    """-> (labels [T] int32, n_faces [C] int64, areas [C] float64) per the specification; ValueError for refused
    input."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    T = len(f)
    if not np.isfinite(v).all():
        raise ValueError("non-finite vertex")
    if T and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("face index out of range")
    q = face_units(v, f)
    if sum(q) >= 2 ** 62:
        raise ValueError("total area reaches 2^12")
    groups = {}
    for t, (a, b, c) in enumerate(f.tolist()):
        for x, y in ((a, b), (b, c), (c, a)):
            if x != y:
                groups.setdefault((min(x, y), max(x, y)), []).append(t)
    # min-label propagation: every face on an edge takes the smallest label on that edge, until nothing changes
    pairs = [(m[0], t) for m in groups.values() for t in m[1:]]
    lab = post_rs.components(T, np.array(pairs, dtype=np.int64).reshape(-1, 2)).tolist()
    roots = sorted(set(lab))                                  # ascending smallest face
    number = {r: k for k, r in enumerate(roots)}
    labels = np.array([number[r] for r in lab], dtype=np.int32).reshape(-1)
    n_faces = np.zeros(len(roots), np.int64)
    sums = [0] * len(roots)
    for t in range(T):
        n_faces[labels[t]] += 1
        sums[labels[t]] += q[t]
    areas = np.array([s / 2 ** 50 for s in sums], dtype=np.float64).reshape(-1)   # int / int: correctly rounded
    return labels, n_faces, areas


def remove_small(vertices, faces, min_area=0.0, min_faces=0, keep_largest=None):
    """-> (vertices [V', 3] float32, faces [T', 3] int64) per the specification."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    labels, n_faces, areas = components(v, f)
    C = len(areas)
    ranked = sorted(range(C), key=lambda c: (-areas[c], c))
    top = set(ranked[:keep_largest]) if keep_largest else set(range(C))
    kept = [c in top and areas[c] >= min_area and n_faces[c] >= min_faces for c in range(C)]
    new_index, out_v, out_f = {}, [], []
    used = sorted({int(i) for t in range(len(f)) if kept[labels[t]] for i in f[t]})
    for i in used:
        new_index[i] = len(out_v)
        out_v.append(v[i])
    for t in range(len(f)):
        if kept[labels[t]]:
            out_f.append([new_index[int(i)] for i in f[t]])
    return (np.array(out_v, dtype=np.float32).reshape(-1, 3), np.array(out_f, dtype=np.int64).reshape(-1, 3))


# ---- shared test meshes ---------------------------------------------------------------------------------------------
def isolated_triangles(n):
    """n unit right triangles, each with its own three vertices, one unit apart along x."""
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    v = (base[None] + np.arange(n, dtype=np.float32)[:, None, None] * np.array([2, 0, 0], np.float32)).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int64).reshape(-1, 3)


def strip(n_faces):
    """A triangle strip on the unit lattice: vertices (k // 2, k % 2, 0), face k = (k, k + 1, k + 2); every face has
    area exactly 0.5."""
    k = np.arange(n_faces + 2)
    v = np.stack([k // 2, k % 2, np.zeros_like(k)], 1).astype(np.float32)
    f = np.stack([k[:-2], k[:-2] + 1, k[:-2] + 2], 1).astype(np.int64)
    return v, f


def tetrahedron(centre, size):
    v = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64) * size + np.asarray(centre)).astype(np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)


def sphere_and_strays():
    """A welded soup_sphere through the restated post-processing (1 component) plus three stray tetrahedra of sizes
    0.05, 0.1 and 0.2 -> (vertices, faces, the strays' areas ascending as the specification computes them)."""
    v, f = post_rs.post_process(*post_rs.soup_sphere(0.1, [0.05, -0.02, 0.01], n_lat=10, n_lon=16), 0.025)
    vs, fs = [v], [f]
    n = len(v)
    for centre, size in (([2, 0, 0], 0.1), ([0, 2, 0], 0.2), ([0, 0, 2], 0.05)):
        tv, tf = tetrahedron(centre, size)
        vs.append(tv)
        fs.append(tf + n)
        n += len(tv)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int64)


def adversarial_cases():
    """[(name, vertices f32 [V, 3], faces i64 [T, 3], [filter keyword sets to try])]"""
    rng = np.random.default_rng(11)
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 1], [2, 2, 2], [3, 2, 2], [2, 3, 2]], np.float32)
    plain = [dict(), dict(min_area=0.6), dict(min_faces=2), dict(keep_largest=1)]
    cases = [
        ("one_face", tri[:3], [[0, 1, 2]], plain),
        ("edge_same_winding", tri[:4], [[0, 1, 2], [1, 2, 3]], plain),
        ("edge_opposite_winding", tri[:4], [[0, 1, 2], [2, 1, 3]], plain),
        ("bow_tie", tri, [[0, 1, 2], [2, 3, 4]], plain),
        ("three_faces_one_edge", tri, [[0, 1, 2], [1, 0, 3], [0, 1, 4]], plain),
        ("degenerate_beside_neighbour", tri, [[0, 1, 2], [1, 1, 2], [5, 6, 7]], plain + [dict(min_faces=2, min_area=0.5)]),
        ("duplicate_face", tri, [[0, 1, 2], [0, 1, 2], [5, 6, 7]], plain),
        ("unreferenced_and_trailing", tri, [[1, 2, 3], [5, 6, 7]], plain + [dict(keep_largest=2)]),
    ]
    for n in (255, 256, 257):
        v, f = isolated_triangles(n)
        cases.append((f"isolated_{n}", v, f, [dict(), dict(min_area=0.5), dict(keep_largest=n - 1), dict(min_faces=2)]))
    v, f = strip(4097)
    cases.append(("strip_4097_shuffled", v, f[np.random.default_rng(3).permutation(len(f))],
                  [dict(), dict(min_area=2048.5), dict(min_area=np.nextafter(2048.5, 4096.0))]))
    # the strip cut in two (face 2000 removed: faces 1999 and 2001 share only a vertex); the part with face 0 last in memory
    cut = np.concatenate([f[2001:][np.random.default_rng(4).permutation(2096)],
                          f[:2000][np.random.default_rng(5).permutation(2000)]])
    cases.append(("strip_cut_face0_last", v, cut, [dict(), dict(keep_largest=1), dict(min_faces=2050),
                                                   dict(min_area=1000.0, min_faces=2001, keep_largest=2)]))
    v, f = isolated_triangles(2)
    v[3:] += np.float32(100.0)
    cases.append(("two_far_unit_triangles", v, f,
                  [dict(min_area=0.5), dict(min_area=float(np.nextafter(0.5, 1.0))), dict(keep_largest=1)]))
    # all three criteria together on random fans: component k is a fan of k + 1 faces scaled by a random size
    vs, fs, n = [], [], 0
    for k in range(12):
        m = k + 3
        ring = np.stack([np.cos(np.arange(m) * 0.4), np.sin(np.arange(m) * 0.4), np.zeros(m)], 1) * rng.uniform(0.2, 2.0)
        vs.append(np.concatenate([[[0, 0, 0]], ring]) + [5.0 * k, 0, 0])
        fs.append(np.stack([np.zeros(m - 1, np.int64), np.arange(1, m), np.arange(2, m + 1)], 1) + n)
        n += m + 1
    v, f = np.concatenate(vs).astype(np.float32), np.concatenate(fs)
    f = f[rng.permutation(len(f))]
    cases.append(("fans_all_criteria", v, f, [dict(min_area=0.3, min_faces=5, keep_largest=4), dict(min_faces=7),
                                              dict(keep_largest=3), dict(min_area=100.0)]))
    v, f = sphere_and_strays()
    a = sorted(components(v, f)[2].tolist())
    cases.append(("sphere_and_strays", v, f, [dict(min_area=x) for x in
                                              (a[0], (a[0] + a[1]) / 2, (a[1] + a[2]) / 2, (a[2] + a[3]) / 2, a[3] * 2)]))
    cases.append(("no_faces", tri, np.zeros((0, 3), np.int64), [dict()]))
    cases.append(("empty", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), [dict()]))
    return [(n, np.asarray(v, np.float32), np.asarray(f, np.int64).reshape(-1, 3), k) for n, v, f, k in cases]
