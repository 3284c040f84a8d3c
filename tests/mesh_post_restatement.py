"""numpy restatement of the mesh post-processing specification (include/bnv_fusion.h, "Mesh post-processing"), written
from the specification and not from mesh.post_process_mesh: no KD-tree, no sparse matrices, no connected_components.
tests/test_mesh_post_cpu.py pins it to the host function bit for bit; the GPU tests hold the device to the host."""
import numpy as np


def weld(v):
    """-> (u [n, 3] float64 unique rows in lexicographic order, inv [V] vertex -> row)."""
    u = np.rint(np.asarray(v, dtype=np.float64).reshape(-1, 3) * 1e9) / 1e9 + 0.0     # + 0.0: -0 -> +0
    order = np.lexsort((u[:, 2], u[:, 1], u[:, 0]))
    s = u[order]
    head = np.ones(len(s), dtype=bool)
    head[1:] = (s[1:] != s[:-1]).any(1)
    rank = np.cumsum(head) - 1
    inv = np.empty(len(u), dtype=np.int64)
    inv[order] = rank
    return s[head], inv


def close_pairs(u, eps):
    """Every pair i < j with (dx*dx + dy*dy) + dz*dz <= eps*eps, through a uniform grid of cells a little over eps."""
    n = len(u)
    if eps <= 0 or n < 2:
        return np.zeros((0, 2), dtype=np.int64)
    cell = np.floor(u / (eps * (1 + 2.0 ** -20))).astype(np.int64)
    cell -= cell.min(0) - 1
    span = cell.max(0) + 2
    key = (cell[:, 0] * span[1] + cell[:, 1]) * span[2] + cell[:, 2]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                q = ((cell[:, 0] + dx) * span[1] + cell[:, 1] + dy) * span[2] + cell[:, 2] + dz
                lo, hi = np.searchsorted(sk, q, "left"), np.searchsorted(sk, q, "right")
                cnt = hi - lo
                i = np.repeat(np.arange(n), cnt)
                j = order[np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)]
                keep = j > i
                i, j = i[keep], j[keep]
                d = u[i] - u[j]
                ok = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= eps * eps
                out.append(np.stack([i[ok], j[ok]], 1))
    return np.concatenate(out)


def components(n, pairs):
    """Label of every point = the smallest index of its connected component (min-label propagation)."""
    lab = np.arange(n)
    if len(pairs) == 0:
        return lab
    i, j = pairs[:, 0], pairs[:, 1]
    while True:
        old = lab.copy()
        np.minimum.at(lab, i, lab[j])
        np.minimum.at(lab, j, lab[i])
        lab = lab[lab]
        if np.array_equal(lab, old):
            return lab


def post_process(vertices, faces, eps):
    """-> (vertices [V', 3] float32, faces [T', 3] int64) per the specification."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(v) == 0 or len(f) == 0:
        return v.copy(), f.copy()
    u, inv = weld(v)
    root = components(len(u), close_pairs(u, eps))
    roots = np.unique(root)                                    # ascending smallest members
    cid = np.searchsorted(roots, root)
    mean = np.zeros((len(roots), 3))
    for k in range(len(u)):                                    # one after another, ascending index
        mean[cid[k]] += u[k]
    mean /= np.bincount(cid, minlength=len(roots)).astype(np.float64)[:, None]
    c = cid[inv[f]]
    kept, seen = [], set()
    for t, (a, b, d) in enumerate(c.tolist()):
        if a == b or b == d or a == d:
            continue
        r = min((a, b, d), (b, d, a), (d, a, b))               # smallest label first, cyclic order kept
        if r not in seen:
            seen.add(r)
            kept.append(t)
    c = c[np.array(kept, dtype=np.int64)].reshape(-1, 3)
    used = np.unique(c)
    remap = np.full(len(roots), -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    vm, c = mean[used], remap[c]
    nb = [set() for _ in range(len(vm))]
    for a, b, d in c.tolist():
        nb[a] |= {b, d}
        nb[b] |= {a, d}
        nb[d] |= {a, b}
    out = np.empty_like(vm)
    for i, s in enumerate(nb):
        acc = np.zeros(3)
        for j in sorted(s):                                    # ascending index
            acc = acc + vm[j]
        out[i] = (vm[i] + acc) / (1.0 + len(s))
    return out.astype(np.float32), c


# ---- shared test meshes ---------------------------------------------------------------------------------------------
def soup_sphere(voxel, offset, n_lat=24, n_lon=48, seed=0):
    """A UV sphere of radius 3.3 voxels as a triangle soup (every face its own 3 vertices, like meshes whose voxels
    repeat the vertices on common edges), some copies nudged by far less than a voxel."""
    rng = np.random.default_rng(seed)
    th = np.linspace(0, np.pi, n_lat + 1)
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    p = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)),
                  np.outer(np.cos(th), np.ones_like(ph))], -1).reshape(-1, 3)
    idx = np.arange(len(p)).reshape(n_lat + 1, n_lon)
    a, b = idx[:-1], np.roll(idx[:-1], -1, axis=1)
    c, d = idx[1:], np.roll(idx[1:], -1, axis=1)
    f = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    v = (p[f.reshape(-1)] * 3.3 * voxel).astype(np.float32)
    nudge = rng.random(len(v)) < 0.2
    v[nudge] += (rng.normal(size=(int(nudge.sum()), 3)) * 0.02 * voxel).astype(np.float32)
    v = (v + np.asarray(offset, dtype=np.float32)).astype(np.float32)
    return v, np.arange(len(v), dtype=np.int64).reshape(-1, 3)


def adversarial_cases():
    """[(name, vertices f32 [V, 3], faces i64 [T, 3], eps)]"""
    rng = np.random.default_rng(7)
    cases = []
    # exact duplicates and offsets below 1e-9 (near 0 float32 resolves them; the weld must not)
    base = rng.uniform(-1e-8, 1e-8, size=(40, 3)).astype(np.float32)
    v = np.concatenate([base, base, base + np.float32(3e-10), -base[:10], np.zeros((3, 3), np.float32),
                        -np.zeros((3, 3), np.float32)]).astype(np.float32)
    f = rng.integers(0, len(v), size=(120, 3))
    cases.append(("duplicates_subnano", v, f, 2e-9))
    # chains: each point within eps of the next, the chain spanning many eps
    t = np.arange(12, dtype=np.float64) * 0.9
    chain = np.stack([t, np.zeros_like(t), np.zeros_like(t)], 1)
    v = np.concatenate([chain, chain + [0, 5.0, 0], chain[::3] + [0, 0, 5.0]]).astype(np.float32)
    f = np.concatenate([rng.integers(0, len(v), size=(60, 3)), [[0, 12, 24], [11, 23, 27], [1, 13, 25]]])
    cases.append(("chains", v, f, 1.0))
    # a dyadic grid: neighbours at exactly eps join, diagonals do not
    g = np.stack(np.meshgrid(*[np.arange(5) * 0.25] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    v = np.concatenate([g, g[::7] + np.float32(0.125)]).astype(np.float32)
    f = rng.integers(0, len(v), size=(200, 3))
    cases.append(("dyadic_exact_eps", v, f, 0.25))
    # degenerate faces, duplicates under rotation (removed) and reversal (kept), unreferenced and isolated vertices
    v = rng.uniform(-1, 1, size=(30, 3)).astype(np.float32)
    v[20] = v[3] + np.float32(1e-4)
    f = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [3, 4, 5], [20, 4, 5], [5, 20, 4], [6, 6, 7],
                  [8, 9, 8], [10, 11, 12], [12, 11, 10], [3, 20, 13], [14, 15, 16], [0, 1, 2]])
    cases.append(("faces_rot_rev_degenerate", v, f, 1e-3))
    # random clustered points, random faces
    centres = rng.uniform(-2, 2, size=(50, 3))
    v = (centres[rng.integers(0, 50, size=600)] + rng.normal(scale=0.01, size=(600, 3))).astype(np.float32)
    f = rng.integers(0, 600, size=(1500, 3))
    cases.append(("random_clusters", v, f, 0.02))
    # every face collapses
    v = rng.uniform(0, 0.1, size=(30, 3)).astype(np.float32)
    cases.append(("all_degenerate", v, rng.integers(0, 30, size=(40, 3)), 1.0))
    # no faces (the host returns the mesh unchanged) and nothing at all
    cases.append(("no_faces", rng.uniform(size=(9, 3)).astype(np.float32), np.zeros((0, 3), np.int64), 0.1))
    cases.append(("empty", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), 0.1))
    # eps = 0: the exact weld alone
    v, f = soup_sphere(0.5, [0.3, -0.2, 0.001], n_lat=8, n_lon=12)
    cases.append(("eps_zero", v, f, 0.0))
    return [(n, np.asarray(v, np.float32), np.asarray(f, np.int64).reshape(-1, 3), float(e)) for n, v, f, e in cases]
