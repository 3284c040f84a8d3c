"""Frame-to-frame RGB-D odometry restated in float64 numpy: include/bnv_fusion.h, "Odometry", operation by operation in
the order written there (elementwise numpy arithmetic is one IEEE rounding per operation; no ``@`` on the decision
path).  Sums over pairs are taken with numpy's own summation: the order of a float64 sum is what the tests' summation
bound covers.  The solve is the tracker's (track_restatement.solve_update): the kernels share it too.

    intensity(rgb, H, W, K, K_rgb)     -> f32 [H, W]
    prepare(depth, rgb, K, ...)        -> [level] of {"D", "I", "Ix", "Iy", "Dx", "Dy", "valid", "K"}
    pairs_of(ref_l, cur_l, T, ...)     -> (J [n, 2, 6], r [n, 2]): the intensity and the depth row of every pair
    accumulate(...)                    -> (A [6, 6], b [6], sum r^2, pairs, abs [29])
    align(ref, cur, T_guess, ...)      -> (T, status, stats [n_iter, 5], poses [n_iter + 1, 4, 4])
"""
import math

import numpy as np

from track_restatement import (DEGENERATE, JUMP, LOST, OK, exp_apply, from_sums, pose_error, rigid_inverse,  # noqa: F401
                               se3_exp, solve_update, sums_vector)

DEFAULT_SCHEDULE = ((2, 6), (1, 6), (0, 8))      # (pyramid level, iterations), coarse to fine
LAMBDA_DEPTH, DIST, DEPTH_JUMP, MAX_DEPTH = 0.968, 0.07, 0.05, 3.0


def scaled_intrinsics(K, s):
    """tracking.scaled_intrinsics: fx / s and cx' = (cx + 0.5) / s - 0.5."""
    K = np.array(np.asarray(K, dtype=np.float64)[:3, :3])
    K[0, 0], K[0, 2] = K[0, 0] / s, (K[0, 2] + 0.5) / s - 0.5
    K[1, 1], K[1, 2] = K[1, 1] / s, (K[1, 2] + 0.5) / s - 0.5
    return K


def _footprint(n, f, c, fc, cc, nc):
    """Per depth pixel 0..n-1 along one axis: first and one-past-last colour pixel whose centre lies in the footprint
    [p - 0.5, p + 0.5), clamped to the colour image, and the centre's colour coordinate."""
    p = np.arange(n, dtype=np.float64)
    lo = fc * (((p - 0.5) - c) / f) + cc
    hi = fc * (((p + 0.5) - c) / f) + cc
    mid = fc * ((p - c) / f) + cc
    first = np.minimum(np.maximum(np.ceil(lo), 0.0), float(nc))
    last = np.minimum(np.ceil(hi), float(nc))
    return first.astype(np.int64), np.maximum(last, first).astype(np.int64), mid


def _bilinear_axis(mid, nc):
    """Clamped sample position along one axis -> (i0, i1, weight of i1)."""
    x = np.minimum(np.maximum(mid, 0.0), float(nc - 1))
    i0 = np.minimum(np.floor(x), float(max(nc - 2, 0)))
    a = x - i0
    i0 = i0.astype(np.int64)
    return i0, np.minimum(i0 + 1, nc - 1), a


def intensity(rgb, H, W, K, K_rgb=None):
    """Y = ((0.299 R + 0.587 G) + 0.114 B) per colour pixel in float64; a depth pixel takes the mean (sum in row-major
    order / count) of the colour pixels whose centres fall in its footprint, or the bilinear sample at its centre when
    there is none; / 255, rounded to float32.  ``rgb`` None -> zeros."""
    if rgb is None:
        return np.zeros((H, W), dtype=np.float32)
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    Hc, Wc = rgb.shape[:2]
    K = np.asarray(K, dtype=np.float64)
    Kc = K if K_rgb is None else np.asarray(K_rgb, dtype=np.float64)
    c = rgb.astype(np.float64)
    Y = (0.299 * c[..., 0] + 0.587 * c[..., 1]) + 0.114 * c[..., 2]
    j0, j1, xm = _footprint(W, K[0, 0], K[0, 2], Kc[0, 0], Kc[0, 2], Wc)
    i0, i1, ym = _footprint(H, K[1, 1], K[1, 2], Kc[1, 1], Kc[1, 2], Hc)
    acc = np.zeros((H, W))
    for dy in range(int((i1 - i0).max(initial=0))):
        for dx in range(int((j1 - j0).max(initial=0))):
            rows, cols = i0 + dy, j0 + dx
            inside = (rows < i1)[:, None] & (cols < j1)[None, :]
            vals = Y[np.minimum(rows, Hc - 1)[:, None], np.minimum(cols, Wc - 1)[None, :]]
            acc = acc + np.where(inside, vals, 0.0)
    count = ((i1 - i0)[:, None] * (j1 - j0)[None, :]).astype(np.float64)
    with np.errstate(all="ignore"):
        mean = acc / count
    bx0, bx1, ax = _bilinear_axis(xm, Wc)
    by0, by1, ay = _bilinear_axis(ym, Hc)
    ax, ay = ax[None, :], ay[:, None]
    y00, y01 = Y[by0[:, None], bx0[None, :]], Y[by0[:, None], bx1[None, :]]
    y10, y11 = Y[by1[:, None], bx0[None, :]], Y[by1[:, None], bx1[None, :]]
    top = y00 + ax * (y01 - y00)
    bot = y10 + ax * (y11 - y10)
    bil = top + ay * (bot - top)
    return (np.where(count > 0.0, mean, bil) / 255.0).astype(np.float32)


def level0_depth(depth, max_depth=MAX_DEPTH):
    """uint16 millimetres (d = mm / 1000.0) or float32 metres -> float32 metres, 0 unless 0 < d <= max_depth, finite."""
    d = np.asarray(depth)
    if d.dtype == np.uint16:
        d = d.astype(np.float64) / 1000.0
    elif d.dtype == np.float32:
        d = d.astype(np.float64)
    else:
        raise TypeError(f"depth dtype {d.dtype}: uint16 or float32")
    with np.errstate(all="ignore"):
        ok = (d > 0.0) & (d <= max_depth) & np.isfinite(d)
    return np.where(ok, d, 0.0).astype(np.float32)


def downsample(D, I, depth_jump=DEPTH_JUMP):
    """One pyramid level from the one above: every 2 x 2 block (an odd last row / column is dropped) keeps its valid
    depths within ``depth_jump`` of its smallest valid one; mean depth and mean intensity of the kept pixels (float64,
    row-major order) rounded to float32, 0 when none is kept."""
    H, W = D.shape
    Hn, Wn = H // 2, W // 2
    d = [D[dy:2 * Hn:2, dx:2 * Wn:2].astype(np.float64) for dy in (0, 1) for dx in (0, 1)]
    i = [I[dy:2 * Hn:2, dx:2 * Wn:2].astype(np.float64) for dy in (0, 1) for dx in (0, 1)]
    dmin = np.full((Hn, Wn), np.inf)
    for k in range(4):
        dmin = np.where((d[k] > 0.0) & (d[k] < dmin), d[k], dmin)
    sd, si, n = np.zeros((Hn, Wn)), np.zeros((Hn, Wn)), np.zeros((Hn, Wn))
    for k in range(4):
        keep = (d[k] > 0.0) & (d[k] - dmin <= depth_jump)
        sd = sd + np.where(keep, d[k], 0.0)
        si = si + np.where(keep, i[k], 0.0)
        n = n + np.where(keep, 1.0, 0.0)
    with np.errstate(all="ignore"):
        Dn = np.where(n > 0.0, sd / n, 0.0).astype(np.float32)
        In = np.where(n > 0.0, si / n, 0.0).astype(np.float32)
    return Dn, In


def gradients(D, I, depth_jump=DEPTH_JUMP):
    """Central differences (a[+1] - a[-1]) / 2 in float64, rounded to float32 -> (Ix, Iy, Dx, Dy, valid).  A pixel is
    gradient-valid iff it and its four neighbours are valid and every neighbour's depth lies within ``depth_jump`` of
    its own; the gradients of any other pixel are 0."""
    H, W = D.shape
    d, i = D.astype(np.float64), I.astype(np.float64)
    valid = np.zeros((H, W), dtype=bool)
    out = [np.zeros((H, W), dtype=np.float32) for _ in range(4)]
    if H >= 3 and W >= 3:
        c = d[1:-1, 1:-1]
        nb = [d[1:-1, :-2], d[1:-1, 2:], d[:-2, 1:-1], d[2:, 1:-1]]       # left, right, up, down
        ok = c > 0.0
        for n in nb:
            ok &= (n > 0.0) & (np.abs(n - c) <= depth_jump)
        valid[1:-1, 1:-1] = ok
        g = [(i[1:-1, 2:] - i[1:-1, :-2]) / 2.0, (i[2:, 1:-1] - i[:-2, 1:-1]) / 2.0,
             (d[1:-1, 2:] - d[1:-1, :-2]) / 2.0, (d[2:, 1:-1] - d[:-2, 1:-1]) / 2.0]
        for o, gk in zip(out, g):
            o[1:-1, 1:-1] = np.where(ok, gk, 0.0).astype(np.float32)
    return out[0], out[1], out[2], out[3], valid


def prepare(depth, rgb, K, levels=3, max_depth=MAX_DEPTH, depth_jump=DEPTH_JUMP, K_rgb=None):
    """A frame's pyramid: level l at intrinsics scaled_intrinsics(K, 2**l).  ``depth_jump`` is the depth step between
    neighbouring pixels of level 0 that counts as an edge; the pixels of level l are 2**l as wide and the same surface
    slope steps 2**l as far between them, so level l uses jump_l = 2**l depth_jump: in its 2 x 2 blocks (taken from
    level l - 1), in its gradients and in its pairs."""
    D = level0_depth(depth, max_depth)
    I = intensity(rgb, D.shape[0], D.shape[1], K, K_rgb)
    out = []
    for l in range(levels):
        jump = depth_jump * 2.0 ** l
        if l:
            D, I = downsample(D, I, jump)
        Ix, Iy, Dx, Dy, valid = gradients(D, I, jump)
        out.append({"D": D, "I": I, "Ix": Ix, "Iy": Iy, "Dx": Dx, "Dy": Dy, "valid": valid,
                    "K": scaled_intrinsics(K, 2 ** l), "jump": jump})
    return out


def _rigid(T, p0, p1, p2):
    return [((T[a, 0] * p0 + T[a, 1] * p1) + T[a, 2] * p2) + T[a, 3] for a in range(3)]


def _row(a, b, c, r, s, fx, fy, Q):
    """The scaled row of image gradient (a, b), z-term c and residual r: (J [6 x n], s r)."""
    a, b, c = s * a, s * b, s * c
    gx = (a * fx) / Q[2]
    gy = (b * fy) / Q[2]
    gz = (0.0 - (gx * Q[0] + gy * Q[1]) / Q[2]) - c
    J = [Q[1] * gz - Q[2] * gy, Q[2] * gx - Q[0] * gz, Q[0] * gy - Q[1] * gx, gx, gy, gz]
    return J, s * r


def pairs_of(ref, cur, T, lambda_depth=LAMBDA_DEPTH, dist=DIST, return_pixels=False):
    """The pairs of one iteration at pose ``T`` (current <- reference) between one level of two prepared frames, in
    reference-pixel order: J [n, 2, 6] and r [n, 2] (row 0: intensity, scaled sqrt(1 - lambda); row 1: depth, scaled
    sqrt(lambda))."""
    K = ref["K"]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    H, W = ref["D"].shape
    Hc, Wc = cur["D"].shape
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    z = ref["D"].astype(np.float64).reshape(-1)
    i0 = ref["I"].astype(np.float64).reshape(-1)
    keep = z > 0.0
    u, v, z, i0 = u[keep], v[keep], z[keep], i0[keep]
    with np.errstate(all="ignore"):
        x = (u.astype(np.float64) - cx) / fx
        y = (v.astype(np.float64) - cy) / fy
        Q = _rigid(T, x * z, y * z, z)
        xq = fx * Q[0] / Q[2] + cx
        yq = fy * Q[1] / Q[2] + cy
        x0, y0 = np.floor(xq), np.floor(yq)
        keep = (Q[2] > 0.0) & (x0 >= 0.0) & (x0 <= Wc - 2.0) & (y0 >= 0.0) & (y0 <= Hc - 2.0)
    u, v, i0, xq, yq, x0, y0 = (a[keep] for a in (u, v, i0, xq, yq, x0, y0))
    Q = [q[keep] for q in Q]
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    ax, ay = xq - x0, yq - y0
    corners = [(yi, xi), (yi, xi + 1), (yi + 1, xi), (yi + 1, xi + 1)]
    ok = np.ones(len(xi), dtype=bool)
    for c in corners:
        ok &= cur["valid"][c]
    dc = [cur["D"][c].astype(np.float64) for c in corners]
    dmax = np.maximum(np.maximum(dc[0], dc[1]), np.maximum(dc[2], dc[3]))
    dmin = np.minimum(np.minimum(dc[0], dc[1]), np.minimum(dc[2], dc[3]))
    ok &= dmax - dmin <= cur["jump"]

    def sample(name):
        c = [cur[name][k].astype(np.float64) for k in corners]
        top = c[0] + ax * (c[1] - c[0])
        bot = c[2] + ax * (c[3] - c[2])
        return top + ay * (bot - top)

    I1, D1, Ix, Iy, Dx, Dy = (sample(k) for k in ("I", "D", "Ix", "Iy", "Dx", "Dy"))
    rd = Q[2] - D1
    ok &= np.abs(rd) <= dist
    sI, sD = math.sqrt(1.0 - lambda_depth), math.sqrt(lambda_depth)
    with np.errstate(all="ignore"):
        JI, rI = _row(Ix, Iy, 0.0, i0 - I1, sI, fx, fy, Q)
        JD, rD = _row(Dx, Dy, 1.0, rd, sD, fx, fy, Q)
    J = np.stack([np.stack([j[ok] for j in JI], 1), np.stack([j[ok] for j in JD], 1)], 1)
    r = np.stack([rI[ok], rD[ok]], 1)
    if return_pixels:
        return J, r, u[ok], v[ok]
    return J, r


def accumulate(ref, cur, T, lambda_depth=LAMBDA_DEPTH, dist=DIST):
    """-> (A, b, sum r^2, pairs, abs [29]): both rows of every pair enter the sums, a pair counts once."""
    J, r = pairs_of(ref, cur, T, lambda_depth, dist)
    pairs = float(len(r))
    J, r = J.reshape(-1, 6), r.reshape(-1)
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


def align(ref, cur, T_guess=None, schedule=DEFAULT_SCHEDULE, lambda_depth=LAMBDA_DEPTH, dist=DIST,
          min_pair_share=0.05, min_spread=1e-3):
    """``ref``, ``cur``: prepared frames -> (T current <- reference, status, stats, poses); a refused pair returns the
    guess."""
    n_iter = sum(k for _, k in schedule)
    T0 = np.eye(4) if T_guess is None else np.array(T_guess, dtype=np.float64)
    T = T0.copy()
    stats, poses = np.zeros((n_iter, 5)), np.tile(T0, (n_iter + 1, 1, 1))
    it = 0
    for level, iters in schedule:
        for _ in range(iters):
            poses[it] = T
            A, b, rr, pairs, _ = accumulate(ref[level], cur[level], T, lambda_depth, dist)
            T, status, stats[it], _ = solve_update(A, b, rr, pairs, T, ref[level]["D"].size, min_pair_share, min_spread)
            if status != OK:
                return T0, status, stats, poses
            it += 1
    poses[n_iter] = T
    return T, OK, stats, poses


# ---- test scenes ------------------------------------------------------------------------------------------------

SCALE = 0.5


def colour_of(depth, K, T_wc):
    """uint8 [H, W, 3]: synthetic.surface_color of the back-projected world points, rounded; 0 where depth is 0."""
    from bnv_fusion_amd import synthetic
    d = np.asarray(depth, dtype=np.float64)
    H, W = d.shape
    T_wc = np.asarray(T_wc, dtype=np.float64)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    P = np.stack([(u - K[0][2]) / K[0][0] * d, (v - K[1][2]) / K[1][1] * d, d], -1) @ T_wc[:3, :3].T + T_wc[:3, 3]
    return np.where((d > 0)[..., None], np.rint(synthetic.surface_color(P)), 0.0).astype(np.uint8)


def room_frame(t, H=120, W=160, dtype="f32"):
    """Sweep frame t of the half-size analytic room, clean: (depth float32 metres or uint16 millimetres, depth beyond
    3 m set to 0; rgb; K; T_wc)."""
    from bnv_fusion_amd import sequence
    K, T = sequence.intrinsics(H, W), sequence.sweep_pose(t, SCALE)
    d = sequence.render_depth(T, K, H, W, SCALE).numpy()
    d = np.where(np.isfinite(d) & (d <= MAX_DEPTH), d, 0.0)
    rgb = colour_of(d, K, T)
    if dtype == "u16":
        return np.rint(d * 1000.0).astype(np.uint16), rgb, K, T
    return d.astype(np.float32), rgb, K, T


def plane_pair(H=48, W=64, shift=(0.020, -0.010, 0.0), grey=None, z=1.5):
    """A fronto-parallel plane at ``z`` metres seen from the origin and from ``shift``: ((depth, rgb), (depth, rgb), K,
    T current <- reference).  ``grey``: a constant colour instead of the procedural texture."""
    from bnv_fusion_amd import sequence
    K = sequence.intrinsics(H, W)
    d = np.full((H, W), z, dtype=np.float32)
    frames = []
    for c in ((0.0, 0.0, 0.0), shift):
        T = np.eye(4)
        T[:3, 3] = c
        rgb = colour_of(d, K, T) if grey is None else np.full((H, W, 3), grey, dtype=np.uint8)
        frames.append((d, rgb))
    T_rel = np.eye(4)
    T_rel[:3, 3] = [-s for s in shift]
    return frames[0], frames[1], K, T_rel
