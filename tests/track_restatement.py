"""Frame-to-model ICP restated in float64 numpy: include/bnv_fusion.h, "Tracking", operation by operation in the order
written there (elementwise numpy arithmetic is one IEEE rounding per operation; no ``@`` on the decision path).  The
sums are taken with numpy's own summation: the order of a float64 sum is what the tests' summation bound covers.

    accumulate(...)   -> (A [6, 6], b [6], sum r^2, pairs, abs [29]: sum of |terms| of every sum, the kernel's order)
    solve_update(...) -> (T_next, status, stats [5], xi [6])
    align(...)        -> (T, status, stats [n_iter, 5], poses [n_iter + 1, 4, 4])
"""
import math

import numpy as np

OK, LOST, DEGENERATE, JUMP = 0, 1, 2, 3
DEFAULT_LEVELS = ((4, 4), (2, 5), (1, 10))
MAX_ROTATION, MAX_TRANSLATION = 0.1, 0.2


def depth_f64(depth):
    """uint16 millimetres or float32 metres -> float64 metres, the kernel's conversion."""
    d = np.asarray(depth)
    if d.dtype == np.uint16:
        return d.astype(np.float64) / 1000.0
    if d.dtype == np.float32:
        return d.astype(np.float64)
    raise TypeError(f"depth dtype {d.dtype}: uint16 or float32")


def _rigid(T, p0, p1, p2):
    return [((T[a, 0] * p0 + T[a, 1] * p1) + T[a, 2] * p2) + T[a, 3] for a in range(3)]


def pairs_of(depth, K, max_depth, model_depth, model_normals, model_K, model_T, model_T_inv, T, stride, dist):
    """The pairs of one iteration: (J [n, 6], r [n]) in sampled-pixel order."""
    d = depth_f64(depth)
    H, W = d.shape
    K, Km = np.asarray(K, dtype=np.float64), np.asarray(model_K, dtype=np.float64)
    Tm, Tmi, T = (np.asarray(m, dtype=np.float64).reshape(4, 4) for m in (model_T, model_T_inv, T))
    Dm = np.asarray(model_depth, dtype=np.float32)
    Nm = np.asarray(model_normals, dtype=np.float32)
    Hm, Wm = Dm.shape
    v, u = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    d = d[v, u]
    with np.errstate(all="ignore"):
        keep = (d > 0.0) & (d <= max_depth)
        u, v, d = u[keep], v[keep], d[keep]
        x = (u.astype(np.float64) - K[0, 2]) / K[0, 0]
        y = (v.astype(np.float64) - K[1, 2]) / K[1, 1]
        pw = _rigid(T, x * d, y * d, d)
        pm = _rigid(Tmi, *pw)
        um = np.rint(Km[0, 0] * pm[0] / pm[2] + Km[0, 2])
        vm = np.rint(Km[1, 1] * pm[1] / pm[2] + Km[1, 2])
        keep = (pm[2] > 0.0) & (um >= 0.0) & (um <= Wm - 1.0) & (vm >= 0.0) & (vm <= Hm - 1.0)
        pw = [p[keep] for p in pw]
        um, vm = um[keep], vm[keep]
        ui, vi = um.astype(np.int64), vm.astype(np.int64)
        dm = Dm[vi, ui].astype(np.float64)
        n = [Nm[vi, ui, a].astype(np.float64) for a in range(3)]
        xm = (um - Km[0, 2]) / Km[0, 0]
        ym = (vm - Km[1, 2]) / Km[1, 1]
        q = _rigid(Tm, xm * dm, ym * dm, dm)
        e = [q[a] - pw[a] for a in range(3)]
        tq = [T[a, 3] - q[a] for a in range(3)]
        r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
        keep = (dm > 0.0) & np.isfinite(dm) & ((n[0] != 0.0) | (n[1] != 0.0) | (n[2] != 0.0))
        keep &= (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= dist * dist
        keep &= (n[0] * tq[0] + n[1] * tq[1]) + n[2] * tq[2] > 0.0
        keep &= np.isfinite(r)
        J = [pw[1] * n[2] - pw[2] * n[1], pw[2] * n[0] - pw[0] * n[2], pw[0] * n[1] - pw[1] * n[0], n[0], n[1], n[2]]
    return np.stack([j[keep] for j in J], 1), r[keep]


def accumulate(depth, K, max_depth, model_depth, model_normals, model_K, model_T, model_T_inv, T, stride, dist=0.1):
    J, r = pairs_of(depth, K, max_depth, model_depth, model_normals, model_K, model_T, model_T_inv, T, stride, dist)
    A, b, absum = np.zeros((6, 6)), np.zeros(6), []
    for i in range(6):
        for j in range(i, 6):
            t = J[:, i] * J[:, j]
            A[i, j] = A[j, i] = t.sum()
            absum.append(np.abs(t).sum())
    for i in range(6):
        t = J[:, i] * r
        b[i] = t.sum()
        absum.append(np.abs(t).sum())
    rr = float((r * r).sum())
    pairs = float(len(r))
    return A, b, rr, pairs, np.array(absum + [rr, pairs])


def sums_vector(A, b, rr, pairs):
    """The 29 sums in the kernel's order."""
    return np.array([A[i, j] for i in range(6) for j in range(i, 6)] + list(b) + [rr, pairs])


def from_sums(s):
    A, k = np.zeros((6, 6)), 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = s[k]
            k += 1
    return A, np.array(s[21:27], dtype=np.float64), float(s[27]), float(s[28])


def min_eig3(M):
    M = [[float(M[i][j]) for j in range(3)] for i in range(3)]
    for _ in range(6):
        for p in range(2):
            for q in range(p + 1, 3):
                apq = M[p][q]
                if apq == 0.0:
                    continue
                theta = (M[q][q] - M[p][p]) / (2.0 * apq)
                tt = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                t = -tt if theta < 0.0 else tt
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(3):
                    mkp, mkq = M[k][p], M[k][q]
                    M[k][p] = c * mkp - s * mkq
                    M[k][q] = s * mkp + c * mkq
                for k in range(3):
                    mpk, mqk = M[p][k], M[q][k]
                    M[p][k] = c * mpk - s * mqk
                    M[q][k] = s * mpk + c * mqk
    return min(M[0][0], M[1][1], M[2][2])


def ldlt_solve(A, b):
    """xi of A xi = b by LDL^T without pivoting, or None when a pivot is <= 0."""
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        dj = float(A[j][j])
        for k in range(j):
            dj = dj - (L[j][k] * L[j][k]) * D[k]
        if not dj > 0.0:
            return None
        D[j] = dj
        for i in range(j + 1, 6):
            l = float(A[i][j])
            for k in range(j):
                l = l - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = l / dj
    z = [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for k in range(i):
            s = s - L[i][k] * z[k]
        z[i] = s
    z = [z[i] / D[i] for i in range(6)]
    xi = [0.0] * 6
    for i in range(5, -1, -1):
        s = z[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * xi[k]
        xi[i] = s
    return xi


def exp_apply(xi, T):
    """exp(xi^) T."""
    T = np.asarray(T, dtype=np.float64)
    th2 = (xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]
    th = math.sqrt(th2)
    if th < 1e-8:
        ca, cb, cc = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        sn, cs = math.sin(th), math.cos(th)
        ca, cb, cc = sn / th, (1.0 - cs) / th2, (th - sn) / (th2 * th)
    K = [[0.0, -xi[2], xi[1]], [xi[2], 0.0, -xi[0]], [-xi[1], xi[0], 0.0]]
    K2 = [[(K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j] for j in range(3)] for i in range(3)]
    E = [[((1.0 if i == j else 0.0) + ca * K[i][j]) + cb * K2[i][j] for j in range(3)] for i in range(3)]
    V = [[((1.0 if i == j else 0.0) + cb * K[i][j]) + cc * K2[i][j] for j in range(3)] for i in range(3)]
    out = np.eye(4)
    for i in range(3):
        for j in range(3):
            out[i, j] = (E[i][0] * T[0, j] + E[i][1] * T[1, j]) + E[i][2] * T[2, j]
        tv = (V[i][0] * xi[3] + V[i][1] * xi[4]) + V[i][2] * xi[5]
        out[i, 3] = ((E[i][0] * T[0, 3] + E[i][1] * T[1, 3]) + E[i][2] * T[2, 3]) + tv
    return out


def solve_update(A, b, rr, pairs, T, n_samples, min_pair_share=0.05, min_spread=1e-3):
    """-> (T_next (``T`` itself unless OK), status, stats [5] = pairs, rmse, |w|, |v|, spread, xi [6])."""
    rmse = math.sqrt(rr / pairs) if pairs > 0.0 else 0.0
    stats = [pairs, rmse, 0.0, 0.0, 0.0]
    zero = [0.0] * 6
    if not pairs > 0.0 or pairs < min_pair_share * float(n_samples):
        return T, LOST, np.array(stats), zero
    stats[4] = spread = min_eig3([[A[3 + i][3 + j] / pairs for j in range(3)] for i in range(3)])
    if not spread >= min_spread:
        return T, DEGENERATE, np.array(stats), zero
    xi = ldlt_solve(A, b)
    if xi is None:
        return T, DEGENERATE, np.array(stats), zero
    stats[2] = wn = math.sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2])
    stats[3] = vn = math.sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5])
    if not (wn <= MAX_ROTATION and vn <= MAX_TRANSLATION):
        return T, JUMP, np.array(stats), xi
    return exp_apply(xi, T), OK, np.array(stats), xi


def n_samples(H, W, stride):
    return ((H + stride - 1) // stride) * ((W + stride - 1) // stride)


def rigid_inverse(T):
    T = np.asarray(T, dtype=np.float64)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def align(depth, K, model_depth, model_normals, model_K, model_T, T_guess, levels=DEFAULT_LEVELS, dist=0.1,
          max_depth=3.0, min_pair_share=0.05, min_spread=1e-3):
    H, W = np.asarray(depth).shape
    n_iter = sum(k for _, k in levels)
    T0 = np.array(T_guess, dtype=np.float64)
    T, Tmi = T0.copy(), rigid_inverse(model_T)
    stats, poses = np.zeros((n_iter, 5)), np.tile(T0, (n_iter + 1, 1, 1))
    it = 0
    for stride, iters in levels:
        for _ in range(iters):
            poses[it] = T
            A, b, rr, pairs, _ = accumulate(depth, K, max_depth, model_depth, model_normals, model_K, model_T, Tmi, T,
                                            stride, dist)
            T, status, stats[it], _ = solve_update(A, b, rr, pairs, T, n_samples(H, W, stride), min_pair_share,
                                                   min_spread)
            if status != OK:
                return T0, status, stats, poses
            it += 1
    poses[n_iter] = T
    return T, OK, stats, poses


# ---- model views without a GPU -----------------------------------------------------------------------------------

def se3_exp(xi):
    return exp_apply([float(x) for x in xi], np.eye(4))


def pose_error(T, T_true):
    """(translation error in metres, rotation error in radians)."""
    T, T_true = np.asarray(T), np.asarray(T_true)
    dR = T[:3, :3].T @ T_true[:3, :3]
    return (float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])),
            float(math.acos(min(1.0, max(-1.0, (np.trace(dR) - 1.0) / 2.0)))))


def analytic_view(T, K, H, W, scale, max_depth=None):
    """(depth f32 [H, W], world normals f32 [H, W, 3]) of the analytic room from pose ``T``: the scene's surfaces are
    axis-aligned box faces, so the normal of a pixel is the axis along which its hit point lies on a face, turned
    towards the camera."""
    from bnv_fusion_amd import sequence
    z = sequence.render_depth(T, K, H, W, scale).numpy()
    T = np.asarray(T, dtype=np.float64)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y = (u - K[0][2]) / K[0][0], (v - K[1][2]) / K[1][1]
    dirs = np.stack([x, y, np.ones_like(x)], -1) @ T[:3, :3].T
    pts = T[:3, 3] + z[..., None] * dirs
    boxes = [([-scale * h for h in sequence.ROOM_HALF], [scale * h for h in sequence.ROOM_HALF])]
    for c, h in sequence.FURNITURE:
        boxes.append(([scale * (c[a] - h[a]) for a in range(3)], [scale * (c[a] + h[a]) for a in range(3)]))
    best = np.full((H, W), np.inf)
    axis = np.zeros((H, W), dtype=np.int64)
    for lo, hi in boxes:
        inside = np.ones((H, W), dtype=bool)
        for a in range(3):
            inside &= (pts[..., a] >= lo[a] - 1e-6) & (pts[..., a] <= hi[a] + 1e-6)
        for a in range(3):
            for plane in (lo[a], hi[a]):
                dist = np.abs(pts[..., a] - plane)
                better = inside & (dist < best)
                best = np.where(better, dist, best)
                axis = np.where(better, a, axis)
    n = np.zeros((H, W, 3))
    for a in range(3):
        n[..., a] = np.where(axis == a, -np.sign(dirs[..., a]), 0.0)
    ok = np.isfinite(z) & (z > 0) & (best < 1e-5)
    if max_depth is not None:
        ok &= z < max_depth
    depth = np.where(ok, z, 0.0).astype(np.float32)
    return depth, np.where(ok[..., None], n, 0.0).astype(np.float32)
