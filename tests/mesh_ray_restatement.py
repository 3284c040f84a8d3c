"""Restatements the ray caster and the depth sensor (csrc/meshray.hip, bnv_fusion_amd/scan.py) are pinned to.

``brute_force``: float64 Moeller-Trumbore over ALL valid triangles, no grid -> nearest t > 0, its face, barycentrics and
the nearest t of any other face.  ``woop``: the kernel's formulas (Woop, Benthin & Wald 2013) in a numpy dtype, one
rounding per operation -- in float32 it measures what fp32 costs (tests/test_mesh_ray_cpu.py), it is not a reference.
``camera_rays``: the kernel's ray of a pixel in a numpy dtype.  ``sure``: which pixels have a stable float64 answer.
``aimed_directions`` / ``legitimate_hit``: rays through vertices and edges, and what may be answered on them.
``philox4x32_10`` / ``sensor``: the sensor model in float64 with Philox in integer arithmetic.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import mesh_sdf_restatement as S

ULP32 = 2.0 ** -23
SHIFT = 2.0 ** -10          # pixels: the shifts under which a sure pixel's answer is stable
SLOPE_MAX = 16.0            # a sure pixel's surface is no steeper than this against the image plane (see ``sure``)
PAIRS_PER_CHUNK = 1_000_000
RAYS_PER_BLOCK, THREADS = 20_000, 8


def camera_rays(K, T_wc, H, W, dtype=np.float64, du=0.0, dv=0.0):
    """The kernel's rays: x = (u - cx) / fx, y = (v - cy) / fy, d = (R[a][0] x + R[a][1] y) + R[a][2], o = T[:3, 3], every
    operation one rounding in ``dtype`` -> (o [3], d [H * W, 3]) as float64 VALUES of that arithmetic.  (du, dv): a
    sub-pixel shift (float64 only)."""
    K, T = np.asarray(K, dtype), np.asarray(T_wc, dtype)
    u = np.arange(W).astype(dtype) + dtype(du)
    v = np.arange(H).astype(dtype) + dtype(dv)
    x = ((u - K[0, 2]) / K[0, 0])[None, :].repeat(H, 0).reshape(-1)
    y = ((v - K[1, 2]) / K[1, 1])[:, None].repeat(W, 1).reshape(-1)
    d = np.stack([(T[a, 0] * x + T[a, 1] * y) + T[a, 2] for a in range(3)], -1)
    return T[:3, 3].astype(np.float64), d.astype(np.float64)


def _valid_triangles(V, F):
    ok = S.valid_faces(V, F)
    ids = np.nonzero(ok)[0]
    P = np.asarray(V, np.float64)[np.asarray(F)[ids]]
    return ids, P


def brute_force(o, d, V, F, t_min=0.0, t_max=np.inf, margin=0.0):
    """Rays o [3] or [N, 3], d [N, 3] against every valid face, float64 Moeller-Trumbore, two-sided -> dict(t [N] (inf:
    no hit), face [N] (-1; the lowest index among exactly equal t), second [N] (the nearest t of any OTHER face, inf),
    u, v [N] (hit = (1 - u - v) v0 + u v1 + v v2)).  A hit needs t > t_min (nearest t > 0) and t <= t_max.
    ``margin``: every barycentric coordinate must be >= margin -- positive shrinks the triangles to the hits no
    arithmetic can lose, negative grows them to every hit an arithmetic may find; 0 is the test itself."""
    o = np.broadcast_to(np.asarray(o, np.float64), np.asarray(d).shape)
    d = np.asarray(d, np.float64)
    n = len(d)
    if n > RAYS_PER_BLOCK:                                  # rays are independent: blocks of them on a few threads
        blocks = [slice(s, s + RAYS_PER_BLOCK) for s in range(0, n, RAYS_PER_BLOCK)]
        with ThreadPoolExecutor(max_workers=THREADS) as pool:
            parts = list(pool.map(lambda b: brute_force(o[b], d[b], V, F, t_min, t_max, margin), blocks))
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    ids, P = _valid_triangles(V, F)
    best = np.full(n, np.inf)
    second = np.full(n, np.inf)
    face = np.full(n, -1, np.int64)
    bu, bv = np.full(n, np.nan), np.full(n, np.nan)
    chunk = max(1, PAIRS_PER_CHUNK // max(n, 1))
    for s in range(0, len(ids), chunk):
        A, B, C = (P[s:s + chunk, k][None] for k in range(3))          # [1, c, 3]
        e1, e2 = B - A, C - A
        dd, oo = d[:, None, :], o[:, None, :]
        pv = np.cross(dd, e2)
        det = (e1 * pv).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = oo - A
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, e1)
            v = (dd * qv).sum(-1) * inv
            t = (e2 * qv).sum(-1) * inv
        hit = (det != 0) & (u >= margin) & (v >= margin) & (u + v <= 1 - margin) & (t > t_min) & (t <= t_max)
        t = np.where(hit, t, np.inf)
        k = np.argmin(t, axis=1)                                       # first = lowest face index of the chunk
        r = np.arange(n)
        tk = t[r, k]
        t[r, k] = np.inf
        t2 = t.min(axis=1)
        better = tk < best
        second = np.where(better, np.minimum(best, t2), np.minimum(second, tk))
        face = np.where(better, ids[s:s + chunk][k], face)
        bu, bv = np.where(better, u[r, k], bu), np.where(better, v[r, k], bv)
        best = np.where(better, tk, best)
    return {"t": best, "face": face, "second": second, "u": bu, "v": bv}


def woop(o, d, V, F, dtype=np.float32, t_min=0.0, t_max=np.inf, return_face=False):
    """The kernel's ray / triangle test in ``dtype`` over all valid faces (o, d: values of that dtype) -> nearest t
    [N] as float64 (inf: no hit)[, its face: the lowest index among equal t, -1].  Common origin or one per ray."""
    f = dtype
    d = np.asarray(d).astype(f)
    o = np.broadcast_to(np.asarray(o).astype(f), d.shape)
    n = len(d)
    ids, P = _valid_triangles(V, F)
    P = P.astype(f)
    kz = np.argmax(np.abs(d) >= np.abs(d).max(1, keepdims=True), axis=1)      # the first of the largest: x, then y
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    r = np.arange(n)
    neg = d[r, kz] < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    dz = d[r, kz]
    Sx, Sy, Sz = (d[r, kx] / dz)[:, None], (d[r, ky] / dz)[:, None], (f(1) / dz)[:, None]
    best = np.full(n, np.inf)
    face = np.full(n, -1, np.int64)
    chunk = max(1, PAIRS_PER_CHUNK // max(n, 1))
    for s in range(0, len(ids), chunk):
        sh = []
        for k in range(3):
            Q = P[s:s + chunk, k][None] - o[:, None, :]                       # [n, c, 3]
            qx = np.take_along_axis(Q, kx[:, None, None], 2)[..., 0]
            qy = np.take_along_axis(Q, ky[:, None, None], 2)[..., 0]
            qz = np.take_along_axis(Q, kz[:, None, None], 2)[..., 0]
            sh.append((qx - Sx * qz, qy - Sy * qz, Sz * qz))
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = sh
        U, Vv, Ww = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        z = (U == 0) | (Vv == 0) | (Ww == 0)
        if z.any():
            g = np.float64
            U = np.where(z, (Cx.astype(g) * By - Cy.astype(g) * Bx).astype(f), U)
            Vv = np.where(z, (Ax.astype(g) * Cy - Ay.astype(g) * Cx).astype(f), Vv)
            Ww = np.where(z, (Bx.astype(g) * Ay - By.astype(g) * Ax).astype(f), Ww)
        miss = ((U < 0) | (Vv < 0) | (Ww < 0)) & ((U > 0) | (Vv > 0) | (Ww > 0))
        det = (U + Vv) + Ww
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((U * Az + Vv * Bz) + Ww * Cz) / det
        ok = ~miss & (det != 0) & (t >= f(t_min)) & (t <= f(t_max))
        t = np.where(ok, t, np.inf).astype(np.float64)
        k = np.argmin(t, axis=1)                                       # first = lowest face index of the chunk
        tk = t[r, k]
        face = np.where(tk < best, ids[s:s + chunk][k], face)
        best = np.minimum(best, tk)
    return (best, face) if return_face else best


def aimed_directions(V, F, o):
    """Float32 directions from ``o`` exactly at every vertex and every edge midpoint, and within 2^-20 of them."""
    V = np.asarray(V, np.float32)
    tri = V[np.asarray(F)]
    mid = ((tri.astype(np.float64) + tri[:, [1, 2, 0]]) / 2).reshape(-1, 3).astype(np.float32)
    targets = np.concatenate([V, mid])
    d = targets - np.asarray(o, np.float32)
    jitter = np.random.default_rng(3).uniform(-1, 1, d.shape).astype(np.float32) * np.float32(2.0 ** -20)
    return np.concatenate([d, d + jitter * np.abs(d).max()])


def legitimate_hit(o, d, V, F, t, face, tol, margin):
    """Is the hit (t, face) of each ray one a correct ray caster may report, wherever the ray runs -- through an edge, a
    vertex or along a silhouette, where ``brute_force`` itself is only one of the legitimate answers (it loses rays
    aimed exactly at an edge, and then reports the far side of a closed surface)?  All in float64; distances in metres
    (t times |d|), ``margin`` in barycentric coordinates.  Three conditions:
      - the point o + t d lies within ``tol`` of the plane of ``face`` and, projected into it, inside the triangle
        grown by ``margin``: it is a point of the surface;
      - no nearer than the nearest hit of the triangles grown by ``margin``: nothing was hit that is not there;
      - no further than the nearest hit of the triangles shrunk by ``margin``: nothing was passed that no arithmetic
        can lose.
    -> bool [N]"""
    o = np.broadcast_to(np.asarray(o, np.float64), np.asarray(d).shape)
    d, t, face = np.asarray(d, np.float64), np.asarray(t, np.float64), np.asarray(face)
    dn = np.linalg.norm(d, axis=1)
    P = np.asarray(V, np.float64)[np.asarray(F)[face]]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    w = o + t[:, None] * d - P[:, 0]
    off = (w * n).sum(-1)
    w = w - off[:, None] * n
    a, b, c = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    p, q = (w * e1).sum(-1), (w * e2).sum(-1)
    u, v = (c * p - b * q) / (a * c - b * b), (a * q - b * p) / (a * c - b * b)
    on_face = (np.abs(off) <= tol) & (u >= -margin) & (v >= -margin) & (u + v <= 1 + margin)
    grown = brute_force(o, d, V, F, margin=-margin)["t"]
    shrunk = brute_force(o, d, V, F, margin=margin)["t"]
    return (face >= 0) & on_face & ((t - grown) * dn >= -tol) & ((t - shrunk) * dn <= tol)


def sure(K, T_wc, H, W, V, F, center=None):
    """Which pixels have a float64 answer a kernel can be held to: the same hit / miss under shifts of +-2^-10 pixel in u
    and in v, and a depth that moves by no more than depth * 2^-10 / f * SLOPE_MAX -- what a surface SLOPE_MAX times
    steeper than the image plane gives; beyond it lie silhouettes (a jump) and grazing surfaces, where one fp32
    rounding of the ray moves the depth by many of its own ulp.  -> (sure bool [H * W], the centre's brute force)."""
    o, d = camera_rays(K, T_wc, H, W)
    c = center if center is not None else brute_force(o, d, V, F)
    ok = np.ones(H * W, bool)
    fmin = min(abs(float(K[0][0])), abs(float(K[1][1])))
    for du, dv in ((SHIFT, 0.0), (-SHIFT, 0.0), (0.0, SHIFT), (0.0, -SHIFT)):
        o2, d2 = camera_rays(K, T_wc, H, W, du=du, dv=dv)
        s = brute_force(o2, d2, V, F)
        hit_c, hit_s = np.isfinite(c["t"]), np.isfinite(s["t"])
        ok &= hit_c == hit_s
        both = hit_c & hit_s
        ok[both] &= np.abs(s["t"][both] - c["t"][both]) <= c["t"][both] * SHIFT / fmin * SLOPE_MAX
    return ok, c


# --------------------------------------------------------------------------- #
# the depth sensor
# --------------------------------------------------------------------------- #
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011) in integer arithmetic: counter uint32 [..., 4], key uint32 [..., 2] (or
    broadcastable) -> uint32 [..., 4]."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0 = np.asarray(key)[..., 0].astype(np.uint64)
    k1 = np.asarray(key)[..., 1].astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, -1).astype(np.uint32)


def sensor_draws(H, W, seed, frame, dtype=np.float64):
    """The three standard normals of every pixel, as bnv_depth_sensor draws them: key (seed low, seed high), counter
    (r W + c, frame, 0, 0), uniforms ((w >> 9) + 0.5) 2^-23, Box-Muller in ``dtype`` -> [H, W, 3] of that dtype."""
    ctr = np.zeros((H * W, 4), np.uint32)
    ctr[:, 0] = np.arange(H * W, dtype=np.uint32)
    ctr[:, 1] = np.uint32(frame)
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32))
    f = dtype
    u = ((w >> np.uint32(9)).astype(f) + f(0.5)) * f(2.0 ** -23)
    two_pi = f(np.float32(2 * np.pi))                        # the kernel's constant: fp32(2 pi)
    ra, rb = np.sqrt(f(-2) * np.log(u[:, 0])), np.sqrt(f(-2) * np.log(u[:, 2]))
    pa, pb = two_pi * u[:, 1], two_pi * u[:, 3]
    return np.stack([ra * np.cos(pa), ra * np.sin(pa), rb * np.cos(pb)], -1).reshape(H, W, 3)


def sensor(clean, seed=0, frame=0, draws=None, table=None, bf=35.130, sigma_d=0.027778, sigma_px=0.25):
    """Simulator.simulate (the reference's src/utils/geometry.py:42-72) in float64, vectorised.  ``clean`` [H, W]
    metres; ``draws`` [H, W, 3] standard normals (default: ``sensor_draws(H, W, seed, frame)``); ``table`` [80, 80, 5]
    or None (factor 1).  -> dict(depth float64 [H, W] metres, mm uint16 = trunc(depth * 1000), q [H, W, 3]: the three
    quantities before rounding -- q[..., 2] is nan where the sampled depth is 0)."""
    clean = np.asarray(clean, np.float64)
    H, W = clean.shape
    n = np.asarray(draws if draws is not None else sensor_draws(H, W, seed, frame), np.float64)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    qx, qy = c + sigma_px * n[..., 0], r + sigma_px * n[..., 1]
    x = np.clip(np.rint(qx), 0, W - 1).astype(np.int64)
    y = np.clip(np.rint(qy), 0, H - 1).astype(np.int64)
    d = clean[y - y % 2, x - x % 2]
    if table is not None:
        m = np.asarray(table, np.float64)
        i2 = ((d + 1) / 2).astype(np.int64)                  # int(): towards zero; d >= 0
        i1 = i2 - 1
        a = (d - (i1 * 2 + 1)) / 2
        tx, ty = np.minimum(x * 80 // W, 79), np.minimum(y * 80 // H, 79)
        f = (1 - a) * m[ty, tx, np.clip(i1, 0, 4)] + a * m[ty, tx, np.clip(i2, 0, 4)]
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(f == 0, 0.0, d / f)
    with np.errstate(divide="ignore", invalid="ignore"):
        qd = np.where(d > 0, (bf / d + sigma_d * n[..., 2]) * 8, np.nan)
        k = np.rint(qd)
        out = np.where((d > 0) & (k != 0), bf * 8 / k, 0.0)
    mm = np.clip(np.trunc(out * 1000.0), 0, 65535).astype(np.uint16)
    return {"depth": out, "mm": mm, "q": np.stack([qx, qy, qd], -1)}
