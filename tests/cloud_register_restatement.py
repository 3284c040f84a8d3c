"""Cloud-to-cloud registration restated in float64 numpy: include/bnv_fusion.h, "Cloud registration", operation by
operation in the order written there (elementwise numpy arithmetic is one IEEE rounding per operation).  The nearest
neighbour is a brute force in float32 in ``nn_d2``'s operation order (``cloud_restatement.d2_rows``) with the lowest
index on ties; the sums are taken in the tracker's manner (``register_restatement.sums_of``: numpy's own summation,
whose order the tests' summation bound covers); the solve is ``register_restatement.solve_update``.

    index_rows(input_pts)        -> (pos f32 [n, 3], nrm f32 [n, 3]): what the index keeps, rejected rows all NaN
    nearest(q, pos)              -> (d2 f32 [m], idx int64 [m]): (+inf, -1) without an answer
    candidates(q, pos, dist)     -> idx int64 [m]: the nearest kept row with d2 <= float32(dist * dist), else -1
    rows(q, idx, pos, nrm, ...)  -> (J [k, 6], r [k], pairs)
    accumulate(...)              -> (A, b, sum r^2, pairs, abs [29])
    register(...)                -> (T, status, stats [n_iter, 5], poses [n_iter + 1, 4, 4], scales [n_iter])

Not a test module (no ``test_`` prefix): tests/test_cloud_register_cpu.py and tests/test_gpu_cloud_register.py import
it.
"""
import numpy as np

import cloud_restatement as cr
import register_restatement as rr
import track_restatement as tr

OK, LOST, DEGENERATE, JUMP = rr.OK, rr.LOST, rr.DEGENERATE, rr.JUMP
MIN_NORMAL = 1e-12
BOX_LEVELS = rr.BOX_LEVELS


def index_rows(input_pts):
    """fp32 [n, 6] rows -> the position copy and the unit normals of the index; a row with a non-finite component or a
    normal shorter than 1e-12 is all NaN in both."""
    x = np.ascontiguousarray(input_pts, dtype=np.float32).reshape(-1, 6)
    n = x[:, 3:].astype(np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = np.isfinite(x[:, :3]).all(1) & np.isfinite(length) & (length >= MIN_NORMAL)
        nrm = (n / length[:, None]).astype(np.float32)
    pos = x[:, :3].copy()
    pos[~ok] = np.nan
    nrm[~ok] = np.nan
    return pos, nrm


def nearest(q, pos, chunk=256):
    """The fp32 brute force: for every query the least d2 over the finite rows of ``pos`` and the lowest index
    attaining it; (+inf, -1) for a non-finite query or when no row is finite."""
    q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    d2 = np.full(len(q), np.inf, dtype=np.float32)
    idx = np.full(len(q), -1, dtype=np.int64)
    dead = ~np.isfinite(pos).all(1)
    ask = np.flatnonzero(np.isfinite(q).all(1))
    if dead.all():
        return d2, idx
    for s in range(0, len(ask), chunk):
        rows_ = ask[s:s + chunk]
        d = cr.d2_rows(q[rows_], pos)
        d[:, dead] = np.inf
        d[np.isnan(d)] = np.inf                            # (an overflow: inf - inf)
        best = np.argmin(d, axis=1)                        # the first occurrence: the lowest index
        d2[rows_] = d[np.arange(len(rows_)), best]
        idx[rows_] = np.where(np.isinf(d2[rows_]), -1, best)   # (a d2 of +inf does not beat the initial (+inf, -1))
    return d2, idx


def gate2(dist):
    """float32 of the float64 product."""
    return np.float32(np.float64(dist) * np.float64(dist))


def candidates(q, pos, dist):
    d2, idx = nearest(q, pos)
    return np.where((idx >= 0) & (d2 <= gate2(dist)), idx, -1)


def rows(q, idx, pos, nrm, T=None, normals=None, min_normal_cos=None, oriented=False):
    """The rows of one iteration from every sampled point's fp32 ``q`` and candidate ``idx`` (-1: none) ->
    (J [k, 6], r [k], pairs).  ``normals``: the sampled points' source normals, gated at ``min_normal_cos`` under the
    rotation of ``T``."""
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    keep = np.asarray(idx) >= 0
    j = np.where(keep, idx, 0)
    c = np.asarray(pos, dtype=np.float32)[j].astype(np.float64)
    n = np.asarray(nrm, dtype=np.float32)[j].astype(np.float64)
    with np.errstate(all="ignore"):
        if normals is not None and min_normal_cos is not None:
            R = np.asarray(T, dtype=np.float64).reshape(4, 4)
            s32 = np.asarray(normals, dtype=np.float32)
            s = s32.astype(np.float64)
            m = [(R[a, 0] * s[:, 0] + R[a, 1] * s[:, 1]) + R[a, 2] * s[:, 2] for a in range(3)]
            cs = (m[0] * n[:, 0] + m[1] * n[:, 1]) + m[2] * n[:, 2]
            keep &= np.isfinite(s32).all(1) & ((cs if oriented else np.abs(cs)) >= min_normal_cos)
        e = [c[:, a] - q[:, a] for a in range(3)]
        r = (n[:, 0] * e[0] + n[:, 1] * e[1]) + n[:, 2] * e[2]
        J = [q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1], q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2],
             q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]]
    return np.stack([x[keep] for x in J], 1), r[keep], float(keep.sum())


def accumulate(P, pos, nrm, T, stride, dist, normals=None, min_normal_cos=None, oriented=False):
    """-> (A, b, rr, pairs, abs [29]), and the dumps (q f32 [n_s, 3], idx int64 [n_s])."""
    q = rr.transform(T, np.asarray(P, dtype=np.float32)[::stride])
    idx = candidates(q, pos, dist)
    ns = None if normals is None else np.asarray(normals, dtype=np.float32)[::stride]
    return rr.sums_of(*rows(q, idx, pos, nrm, T, ns, min_normal_cos, oriented)), (q, idx)


def register(P, input_pts, T_guess, levels=rr.DEFAULT_LEVELS, normals=None, min_normal_cos=None, oriented=False,
             min_pair_share=0.05, min_spread=1e-3, max_rotation=0.1, max_translation=0.2):
    """The loop -> (T, status, stats [n_iter, 5], poses [n_iter + 1, 4, 4], scales [n_iter])."""
    P = np.asarray(P, dtype=np.float32)
    pos, nrm = index_rows(input_pts)
    n_iter = sum(k for _, k, _ in levels)
    T0 = np.array(T_guess, dtype=np.float64).reshape(4, 4)
    T = T0.copy()
    stats, poses, scales = np.zeros((n_iter, 5)), np.tile(T0, (n_iter + 1, 1, 1)), np.ones(n_iter)
    it = 0
    for stride, iters, dist in levels:
        for _ in range(iters):
            poses[it] = T
            (A, b, rsum, pairs, _), _ = accumulate(P, pos, nrm, T, stride, dist, normals, min_normal_cos, oriented)
            T, status, stats[it], _, scales[it] = rr.solve_update(A, b, rsum, pairs, T, rr.n_samples(len(P), stride),
                                                                  min_pair_share, min_spread, max_rotation,
                                                                  max_translation)
            if status != OK:
                return T0, status, stats, poses, scales
            it += 1
    poses[n_iter] = T
    return T, OK, stats, poses, scales


# ---- the cases the tests share -------------------------------------------------------------------------------------

def sampled_cloud(V, F, n, seed):
    """``n`` area-weighted samples of the mesh with their unit face normals -> fp32 [n, 6] (numpy, seeded)."""
    rng = np.random.default_rng(seed)
    P = np.asarray(V, np.float64)[np.asarray(F, np.int64)]
    cross = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    area = 0.5 * np.linalg.norm(cross, axis=1)
    f = rng.choice(len(P), size=n, p=area / area.sum())
    a, b = rng.random(n), rng.random(n)
    flip = a + b > 1.0
    a, b = np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)
    pts = P[f, 0] + a[:, None] * (P[f, 1] - P[f, 0]) + b[:, None] * (P[f, 2] - P[f, 0])
    return np.concatenate([pts, cross[f] / (2.0 * area[f])[:, None]], 1).astype(np.float32)


def box_target(n=3000, seed=21):
    """The target of the shared cases: ``n`` samples of ``register_restatement.box()`` with their face normals."""
    return sampled_cloud(*rr.box(), n, seed)


def flipped(input_pts, seed=5):
    """The same rows with a seeded half of the normals negated."""
    out = np.array(input_pts, dtype=np.float32)
    out[np.random.default_rng(seed).random(len(out)) < 0.5, 3:] *= -1.0
    return out


def source_normals(n=1500):
    """The face normals of ``box_case``'s source samples, in the source frame: ``sampled_cloud`` draws what
    ``register_restatement.surface_samples`` draws from the same seed, so row k is the normal of sample k."""
    R = tr.se3_exp(rr.T_TRUE_XI)[:3, :3]
    return (sampled_cloud(*rr.box(), n, seed=7)[:, 3:].astype(np.float64) @ R).astype(np.float32)


def cloud_case(name, n=1500, n_target=3000):
    """-> (target fp32 [n_target, 6], source points f32 [n, 3], T_true, T_start) of "near", "far" and "noise"."""
    _, _, pts, T_true, T0 = rr.box_case(name, n)
    return box_target(n_target), pts, T_true, T0
