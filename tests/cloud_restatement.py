"""Point-cloud normals restated in numpy: include/bnv_fusion.h, "Point-cloud normals", operation by operation in the
order written there.  This file is the specification csrc/cloud.hip is held to bit for bit (tests/test_gpu_cloud.py);
tests/test_cloud_cpu.py pins it against a brute-force sort, numpy.linalg.eigh and the depth front end's normals.

Every float operation is one numpy ufunc call on arrays of the stated dtype (one rounding each, no fused multiply-add):
fp32 for the distances, float64 for the fit.  The neighbour search is exhaustive; it is written for clarity and for test
sizes (tens of thousands of points), not for speed."""
import numpy as np

MIN_K, MAX_K = 8, 32           # BNV_CLOUD_MIN_K, BNV_CLOUD_MAX_K
JACOBI_SWEEPS = 6              # BNV_CLOUD_JACOBI_SWEEPS
PLANE_RATIO = 1e-6             # a plane needs lambda_1 > PLANE_RATIO * lambda_2
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))   # (p, q, r): the cyclic order of a sweep


def radius2(max_radius):
    """r2: the fp32 product max_radius * max_radius, +inf without a radius (None or 0)."""
    if max_radius is None or float(max_radius) == 0.0:
        return np.float32(np.inf)
    r = np.float32(max_radius)
    with np.errstate(over="ignore"):
        return np.float32(r * r)


def d2_rows(q, ref):
    """fp32 (dx*dx + dy*dy) + dz*dz of every query row against every reference row -> [len(q), len(ref)]."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = q[:, None, 0] - ref[None, :, 0]
        dy = q[:, None, 1] - ref[None, :, 1]
        dz = q[:, None, 2] - ref[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def neighbors(points, k, max_radius=None, chunk=512):
    """-> (idx int64 [N, k]: the neighbours of every row in (d2, index) order, -1 beyond the m found; m int32 [N]).
    Non-finite rows have m = 0 and are nobody's neighbour."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    N = len(pts)
    r2 = radius2(max_radius)
    finite = np.flatnonzero(np.isfinite(pts).all(1))      # ascending: positions in it order like the indices
    ref = pts[finite]
    idx = np.full((N, k), -1, dtype=np.int64)
    m = np.zeros(N, dtype=np.int32)
    kk = min(k, len(ref))
    for s in range(0, len(ref), chunk):
        d2 = d2_rows(ref[s:s + chunk], ref)
        # the kk-th smallest d2 of every row: everything up to it, ties included, is a candidate
        kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
        for row in range(d2.shape[0]):
            cand = np.flatnonzero(d2[row] <= kth[row])                   # ascending index
            cand = cand[np.argsort(d2[row, cand], kind="stable")][:kk]   # (d2, index) lexicographic
            cand = cand[d2[row, cand] <= r2]
            i = finite[s + row]
            m[i] = len(cand)
            idx[i, :len(cand)] = finite[cand]
    return idx, m


def brute_force_neighbors(points, k, max_radius=None):
    """The definition, row by row: a lexicographic sort of every (d2, index) pair."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    r2 = radius2(max_radius)
    ok = np.isfinite(pts).all(1)
    out = []
    for i in range(len(pts)):
        if not ok[i]:
            out.append([])
            continue
        d2 = d2_rows(pts[i:i + 1], pts)[0]
        order = [j for j in np.lexsort((np.arange(len(pts)), d2)) if ok[j]][:k]
        out.append([int(j) for j in order if d2[j] <= r2])
    return out


def covariance(points, idx, m):
    """Float64 mean [N, 3] and the moments a [N, 3, 3] (symmetric) of every row's first m neighbours, as ordered sums
    divided by m.  Rows with m = 0 come out NaN."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    N, k = idx.shape
    dm = m.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.zeros((N, 3))
        for j in range(k):
            use = (j < m)[:, None]
            s = np.where(use, s + pts[np.maximum(idx[:, j], 0)], s)
        mean = s / dm[:, None]
        a = np.zeros((N, 3, 3))
        for j in range(k):
            use = j < m
            d = pts[np.maximum(idx[:, j], 0)] - mean
            for u in range(3):
                for v in range(u, 3):
                    a[:, u, v] = np.where(use, a[:, u, v] + d[:, u] * d[:, v], a[:, u, v])
        for u in range(3):
            for v in range(u, 3):
                a[:, u, v] = a[:, u, v] / dm
                a[:, v, u] = a[:, u, v]
    return mean, a


def jacobi(a, sweeps=JACOBI_SWEEPS):
    """Cyclic Jacobi on a batch of symmetric 3x3 matrices -> (diagonal [N, 3], V [N, 3, 3], columns = eigenvectors)."""
    a = a.copy()
    N = len(a)
    V = np.zeros((N, 3, 3))
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for _ in range(sweeps):
            for p, q, r in PAIRS:
                apq = a[:, p, q].copy()
                go = apq != 0.0
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * apq
                a[:, p, p] = np.where(go, a[:, p, p] - h, a[:, p, p])
                a[:, q, q] = np.where(go, a[:, q, q] + h, a[:, q, q])
                a[:, p, q] = a[:, q, p] = np.where(go, 0.0, apq)
                rp, rq = a[:, r, p].copy(), a[:, r, q].copy()
                a[:, r, p] = a[:, p, r] = np.where(go, c * rp - s * rq, rp)
                a[:, r, q] = a[:, q, r] = np.where(go, s * rp + c * rq, rq)
                for i in range(3):
                    vp, vq = V[:, i, p].copy(), V[:, i, q].copy()
                    V[:, i, p] = np.where(go, c * vp - s * vq, vp)
                    V[:, i, q] = np.where(go, s * vp + c * vq, vq)
    return np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1), V


def order_eigen(lam):
    """-> (i0, i1, i2): the smallest (first index among equals), the middle, the largest (last index among equals)."""
    rows = np.arange(len(lam))
    i0 = np.zeros(len(lam), dtype=np.int64)
    i0 = np.where(lam[:, 1] < lam[rows, i0], 1, i0)
    i0 = np.where(lam[:, 2] < lam[rows, i0], 2, i0)
    i2 = np.full(len(lam), 2, dtype=np.int64)
    i2 = np.where(lam[:, 1] > lam[rows, i2], 1, i2)
    i2 = np.where(lam[:, 0] > lam[rows, i2], 0, i2)
    return i0, 3 - i0 - i2, i2


def estimate_normals(points, origins, origin_index=None, k=16, max_radius=None, min_neighbors=6, nbrs=None):
    """-> dict(input_pts fp32 [N, 6], variation fp32 [N], n_neighbors int32 [N], status int32 [4], normal64 float64
    [N, 3] (the oriented normal before its rounding to fp32), lam float64 [N, 3] ascending).  ``nbrs``: a precomputed
    ``neighbors(points, k, max_radius)`` to share between calls."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    org = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    N = len(pts)
    assert MIN_K <= k <= MAX_K and 3 <= min_neighbors <= k and N > 0 and len(org) > 0
    idx, m = neighbors(pts, k, max_radius) if nbrs is None else nbrs
    oi = np.zeros(N, dtype=np.int64) if origin_index is None else np.asarray(origin_index, dtype=np.int64).reshape(N)
    bad = (oi < 0) | (oi >= len(org))
    finite = np.isfinite(pts).all(1)
    _, a = covariance(pts, idx, m)
    lam, V = jacobi(a)
    i0, i1, i2 = order_eigen(lam)
    rows = np.arange(N)
    l0, l1, l2 = lam[rows, i0], lam[rows, i1], lam[rows, i2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        plane = l1 > PLANE_RATIO * l2
        rejected = ~finite | (m < min_neighbors) | bad | ~plane
        n = V[rows, :, i0]
        p64 = pts.astype(np.float64)
        o64 = org[np.where(bad, 0, oi)].astype(np.float64)
        dot = (n[:, 0] * (p64[:, 0] - o64[:, 0]) + n[:, 1] * (p64[:, 1] - o64[:, 1])) + n[:, 2] * (p64[:, 2] - o64[:, 2])
        n = np.where((dot < 0.0)[:, None], -n, n)
        var = np.where(l0 < 0.0, 0.0, l0) / ((l0 + l1) + l2)
        out = np.concatenate([pts, n.astype(np.float32)], axis=1)
        var = var.astype(np.float32)
    out[rejected] = np.float32(np.nan)
    var[rejected] = np.float32(np.nan)
    n64 = np.where(rejected[:, None], np.nan, n)
    status = np.array([int(rejected.sum()), int(bad.sum()), 0, 0], dtype=np.int32)
    return {"input_pts": out, "variation": var, "n_neighbors": m.astype(np.int32), "status": status, "normal64": n64,
            "lam": np.stack([l0, l1, l2], axis=1), "cov": a}
