"""Point-to-mesh registration restated in float64 numpy: include/bnv_fusion.h, "Registration", operation by operation
in the order written there (elementwise numpy arithmetic is one IEEE rounding per operation).  The closest points come
from the brute force of tests/mesh_sdf_restatement.py in float32 (``mesh_sdf(dtype=np.float32)``: the precision the
kernel's search works in); the sums are taken in the tracker's manner (tests/track_restatement.py: numpy's own
summation, whose order the tests' summation bound covers); the solve is the tracker's with the clamp.

    transform(T, P)          -> q float32 [n, 3]: the sampled points at the estimate T
    rows(q, c, feature, ...) -> (J [m, 6], r [m], pairs): the rows of the kept pairs and their number
    accumulate(...)          -> (A, b, sum r^2, pairs, abs [29]) of one iteration
    solve_update(...)        -> (T_next, status, stats [5], xi [6], scale)
    register(...)            -> (T, status, stats [n_iter, 5], poses [n_iter + 1, 4, 4])

Not a test module (no ``test_`` prefix): tests/test_register_cpu.py and tests/test_gpu_register.py import it.
"""
import math

import numpy as np

import mesh_sdf_restatement as R
import track_restatement as tr

OK, LOST, DEGENERATE, JUMP = tr.OK, tr.LOST, tr.DEGENERATE, tr.JUMP
DEFAULT_LEVELS = ((4, 10, 0.2), (2, 6, 0.05), (1, 4, 0.02))


def n_samples(n_points, stride):
    return (n_points + stride - 1) // stride


def transform(T, P):
    """float32 points [n, 3] at the estimate ``T`` -> float32 [n, 3]: float64 in the header's order, rounded once."""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    p = np.asarray(P, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        q = [((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)]
        return np.stack(q, 1).astype(np.float32)


def rows(q, closest, feature, dist, reject_boundary=True):
    """The rows of one iteration from every sampled point's fp32 ``q``, closest point (NaN: none) and feature byte ->
    (J [m, 6], r [m], pairs).  A point on the mesh (d == 0) counts in ``pairs`` and has no row."""
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    c = np.asarray(closest).astype(np.float64)
    feature = np.asarray(feature)
    with np.errstate(all="ignore"):
        u = [q[:, a] - c[:, a] for a in range(3)]
        d2 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
        d = np.sqrt(d2)
        keep = np.isfinite(q).all(1) & np.isfinite(c).all(1) & (d2 <= dist * dist)
        if reject_boundary:
            keep &= (feature & R.BOUNDARY) == 0
        pairs = float(keep.sum())
        keep &= d != 0.0
        n = [u[a] / d for a in range(3)]
        e = [-u[a] for a in range(3)]
        r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
        J = [q[:, 1] * n[2] - q[:, 2] * n[1], q[:, 2] * n[0] - q[:, 0] * n[2], q[:, 0] * n[1] - q[:, 1] * n[0],
             n[0], n[1], n[2]]
    return np.stack([j[keep] for j in J], 1), r[keep], pairs


def sums_of(J, r, pairs):
    """-> (A, b, rr, pairs, abs [29]) of the rows, as track_restatement.accumulate makes them."""
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
    return A, b, rr, pairs, np.array(absum + [rr, pairs])


def closest_points(q, V, F, topology=None):
    """The float32 brute force -> (closest [n, 3] (NaN for a non-finite q), feature uint8 [n], face [n])."""
    out = R.mesh_sdf(q, V, F, dtype=np.float32, topology=topology)
    return out["closest"], out["feature"], out["face"]


def accumulate(P, V, F, T, stride, dist, reject_boundary=True, topology=None):
    q = transform(T, np.asarray(P, dtype=np.float32)[::stride])
    c, feature, _ = closest_points(q, V, F, topology)
    return sums_of(*rows(q, c, feature, dist, reject_boundary))


def solve_update(A, b, rr, pairs, T, n_s, min_pair_share=0.05, min_spread=1e-3, max_rotation=0.1, max_translation=0.2):
    """track_restatement.solve_update with the clamp: a step beyond the limits is scaled onto them ->
    (T_next (``T`` itself unless OK), status, stats [5] = pairs, rmse, applied |w|, applied |v|, spread, applied xi
    [6], the scale s)."""
    rmse = math.sqrt(rr / pairs) if pairs > 0.0 else 0.0
    stats = [pairs, rmse, 0.0, 0.0, 0.0]
    zero = [0.0] * 6
    if not pairs > 0.0 or pairs < min_pair_share * float(n_s):
        return T, LOST, np.array(stats), zero, 1.0
    stats[4] = spread = tr.min_eig3([[A[3 + i][3 + j] / pairs for j in range(3)] for i in range(3)])
    if not spread >= min_spread:
        return T, DEGENERATE, np.array(stats), zero, 1.0
    xi = tr.ldlt_solve(A, b)
    if xi is None:
        return T, DEGENERATE, np.array(stats), zero, 1.0

    def norms(x):
        return (math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]),
                math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]))

    wn, vn = norms(xi)
    if not (math.isfinite(wn) and math.isfinite(vn)):
        stats[2], stats[3] = wn, vn
        return T, JUMP, np.array(stats), xi, 1.0
    s = min(1.0, max_rotation / wn if wn > 0.0 else math.inf, max_translation / vn if vn > 0.0 else math.inf)
    if s < 1.0:
        xi = [x * s for x in xi]
        wn, vn = norms(xi)
    stats[2], stats[3] = wn, vn
    return tr.exp_apply(xi, T), OK, np.array(stats), xi, s


def register(P, V, F, T_guess, levels=DEFAULT_LEVELS, reject_boundary=True, min_pair_share=0.05, min_spread=1e-3,
             max_rotation=0.1, max_translation=0.2):
    """The loop -> (T, status, stats [n_iter, 5], poses [n_iter + 1, 4, 4], scales [n_iter])."""
    P = np.asarray(P, dtype=np.float32)
    top = R.Topology(V, F)
    n_iter = sum(k for _, k, _ in levels)
    T0 = np.array(T_guess, dtype=np.float64).reshape(4, 4)
    T = T0.copy()
    stats, poses, scales = np.zeros((n_iter, 5)), np.tile(T0, (n_iter + 1, 1, 1)), np.ones(n_iter)
    it = 0
    for stride, iters, dist in levels:
        for _ in range(iters):
            poses[it] = T
            A, b, rr, pairs, _ = accumulate(P, V, F, T, stride, dist, reject_boundary, top)
            T, status, stats[it], _, scales[it] = solve_update(A, b, rr, pairs, T, n_samples(len(P), stride),
                                                               min_pair_share, min_spread, max_rotation,
                                                               max_translation)
            if status != OK:
                return T0, status, stats, poses, scales
            it += 1
    poses[n_iter] = T
    return T, OK, stats, poses, scales


# ---- the cases the tests share -------------------------------------------------------------------------------------

XI_NEAR = (0.08, -0.06, 0.07, 0.04, -0.03, 0.05)       # 6.99 degrees
XI_FAR = (0.25, -0.2, 0.2, 0.08, -0.06, 0.1)           # 21.6 degrees: the first steps are clamped
T_TRUE_XI = (0.3, -0.2, 0.25, 0.05, -0.04, 0.03)       # the transform the tests hide: source -> mesh
BOX_LEVELS = ((1, 10, 0.2), (1, 6, 0.05), (1, 4, 0.02))


def box():
    V, F, _ = R.box_mesh((1.0, -0.5, 2.0), R.rotation(3), (0.31, 0.22, 0.17), n=6)
    return V, F


def surface_samples(V, F, n, seed):
    """``n`` area-weighted samples of the mesh's surface, float64 [n, 3] (numpy, seeded)."""
    rng = np.random.default_rng(seed)
    P = np.asarray(V, np.float64)[np.asarray(F, np.int64)]
    area = 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
    f = rng.choice(len(P), size=n, p=area / area.sum())
    a, b = rng.random(n), rng.random(n)
    flip = a + b > 1.0
    a, b = np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)
    return P[f, 0] + a[:, None] * (P[f, 1] - P[f, 0]) + b[:, None] * (P[f, 2] - P[f, 0])


def moved(samples, T_true, noise=0.0, seed=0):
    """Mesh-frame samples -> float32 source points: (optional Gaussian noise, then) inv(T_true), so that ``T_true`` is
    the registration's answer."""
    s = np.asarray(samples, np.float64)
    if noise:
        s = s + np.random.default_rng(seed).normal(scale=noise, size=s.shape)
    Ti = tr.rigid_inverse(T_true)
    return (s @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)


def box_case(name, n=1500):
    """-> (V, F, source points f32 [n, 3], T_true, T_start) of the three recovery cases "near", "far", "noise"."""
    V, F = box()
    T_true = tr.se3_exp(T_TRUE_XI)
    pts = moved(surface_samples(V, F, n, seed=7), T_true, noise=0.002 if name == "noise" else 0.0, seed=8)
    xi = XI_FAR if name == "far" else XI_NEAR
    return V, F, pts, T_true, tr.se3_exp(xi) @ T_true
