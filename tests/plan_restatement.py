"""Volume planning restated in numpy: the definition that bnv_fusion_amd/plan.py and csrc/plan.hip are held to, bit for
bit (tests/test_gpu_plan.py), and that tests/test_plan_cpu.py pins to the reference through the oracle.

Two passes over depth frames (``depth`` uint16 millimetres or float metres, ``intr_mat`` 3x3, ``T_wc`` 4x4, optionally
``conf`` / ``conf_level``):

* pass 1 (``extent_hist`` -> ``bounds``): per valid pixel the front end's float32 world point p (``points``), per
  direction d the bin of t = (d0 p0 + d1 p1) + d2 p2 in float64; the (trimmed) extent along d from the histogram; with
  ``align_yaw`` the yaw about ``up`` whose footprint is smallest (``yaw_dirs`` / ``choose_yaw``);
* pass 2 (``count``): per candidate voxel size the encoder's bounds mask and 8-corner voxelisation -> points in bounds,
  touched voxels and the histogram of (point, corner) pairs per voxel, by ``np.unique``.

``stats`` is SparseVolume.track_n_pts / print_statistic on the per-frame float32 ``n_avg_pts``; ``plan`` strings it all
together.  No torch, no package import: numpy only.
"""
import math

import numpy as np

HIST_CAP = 64
AXES = {"x": 0, "y": 1, "z": 2}


def frame_depth_metres(depth):
    d = np.asarray(depth)
    if d.dtype in (np.uint16, np.int16):
        return d.astype(np.uint16).astype(np.float64) / 1000.0
    return d.astype(np.float64)


def valid_mask(depth, max_depth, conf=None, conf_level=0):
    d = frame_depth_metres(depth)
    with np.errstate(invalid="ignore"):
        m = (d > 0) & (d < max_depth)
    if conf is not None:
        m &= np.asarray(conf).astype(np.int64) >= int(conf_level)
    return d, m


def points(depth, K, T, max_depth=3.0, conf=None, conf_level=0):
    """float32 [N, 3]: the world points of the valid pixels in row-major order (frontend.hpp: world_point)."""
    d, m = valid_mask(depth, max_depth, conf, conf_level)
    d = np.where(m, d, 0.0)
    H, W = d.shape
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = np.float32(K[0, 0]), np.float32(K[1, 1]), np.float32(K[0, 2]), np.float32(K[1, 2])
    ur = ((np.arange(W, dtype=np.float32) - cx) / fx).astype(np.float64)
    vr = ((np.arange(H, dtype=np.float32) - cy) / fy).astype(np.float64)
    pc = [ur[None, :] * d, vr[:, None] * d, d]
    T = np.asarray(T, np.float64)
    with np.errstate(over="ignore"):
        pw = [(((T[i, 0] * pc[0] + T[i, 1] * pc[1]) + T[i, 2] * pc[2]) + T[i, 3]).astype(np.float32) for i in range(3)]
    return np.stack(pw, -1).reshape(-1, 3)[m.reshape(-1)]


def extent_hist(p, dirs, bin_size, n_bins):
    """int64 [n_dirs, n_bins] of float32 points p [N, 3]."""
    P = np.asarray(p, np.float32).astype(np.float64)
    out = np.zeros((len(dirs), n_bins), np.int64)
    for j, d in enumerate(np.asarray(dirs, np.float64)):
        with np.errstate(invalid="ignore", over="ignore"):
            t = (d[0] * P[:, 0] + d[1] * P[:, 1]) + d[2] * P[:, 2]
            q = np.floor(t / bin_size)
        q = np.where(q >= -n_bins, q, -float(n_bins))       # (NaN too)
        q = np.where(q <= n_bins, q, float(n_bins))
        b = np.clip(q.astype(np.int64) + n_bins // 2, 0, n_bins - 1)
        np.add.at(out[j], b, 1)
    return out


def bounds_bins(h, trim):
    h = np.asarray(h, np.int64)
    N = int(h.sum())
    k = int(math.floor(trim * N))
    n = len(h)
    lo = int(np.argmax(np.cumsum(h) > k))
    hi = n - 1 - int(np.argmax(np.cumsum(h[::-1]) > k))
    return lo, hi


def bounds(h, trim, bin_size):
    """(lo, hi) in metres of one direction's histogram; ValueError when they touch an overflow bin or nothing counted."""
    n = len(h)
    if int(np.asarray(h).sum()) == 0:
        raise ValueError("no valid point")
    lo, hi = bounds_bins(h, trim)
    if lo == 0 or hi == n - 1:
        raise ValueError("bounds touch an overflow bin")
    return (lo - n // 2) * bin_size, (hi + 1 - n // 2) * bin_size


def plane_axes(up):
    u = AXES[up]
    return (u + 1) % 3, (u + 2) % 3


def yaw_dirs(K, up):
    """The 2 K vectors a_0, b_0, a_1, b_1, ... appended to the three axis directions."""
    i1, i2 = plane_axes(up)
    e1, e2 = np.eye(3)[i1], np.eye(3)[i2]
    out = []
    for j in range(K):
        th = j * (np.pi / 2) / K
        c, s = np.cos(th), np.sin(th)
        out += [c * e1 + s * e2, -s * e1 + c * e2]
    return out


def directions(align_yaw=None, up="y"):
    return [np.array(e, np.float64) for e in np.eye(3)] + (yaw_dirs(int(align_yaw), up) if align_yaw else [])


def choose_yaw(hist, K, trim, bin_size):
    best, area_best = 0, None
    for j in range(K):
        la, ha = bounds(hist[3 + 2 * j], trim, bin_size)
        lb, hb = bounds(hist[4 + 2 * j], trim, bin_size)
        area = (ha - la) * (hb - lb)
        if area_best is None or area < area_best:
            best, area_best = j, area
    return best


def alignment(hist, bin_size, trim=0.0, margin=0.05, align_yaw=None, up="y"):
    """-> dict(center, dimensions, axis_align_mat, yaw_deg, bounds [3, 2] in the aligned frame, R)."""
    R = np.eye(3)
    b = [bounds(hist[a], trim, bin_size) for a in range(3)]
    yaw_deg = 0.0
    if align_yaw:
        K = int(align_yaw)
        j = choose_yaw(hist, K, trim, bin_size)
        i1, i2 = plane_axes(up)
        dirs = yaw_dirs(K, up)
        R = np.zeros((3, 3))
        R[i1], R[i2], R[AXES[up]] = dirs[2 * j], dirs[2 * j + 1], np.eye(3)[AXES[up]]
        b[i1] = bounds(hist[3 + 2 * j], trim, bin_size)
        b[i2] = bounds(hist[4 + 2 * j], trim, bin_size)
        yaw_deg = j * 90.0 / K
    b = np.asarray(b, np.float64)
    center = (b[:, 0] + b[:, 1]) / 2
    A = np.eye(4)
    A[:3, :3] = R
    Tm = np.eye(4)
    Tm[:3, 3] = -center
    return {"center": center, "dimensions": (b[:, 1] - b[:, 0]) + 2 * margin, "axis_align_mat": Tm @ A,
            "yaw_deg": yaw_deg, "bounds": b, "R": R}


def get_world_range(dimensions, voxel_size):
    dimensions = np.asarray(dimensions, dtype=np.float64)
    min_ = -dimensions / 2 - voxel_size
    max_ = dimensions / 2 + voxel_size
    n_xyz = np.ceil((max_ - min_) / voxel_size).astype(int).tolist()
    return min_, min_ + voxel_size * np.asarray(n_xyz), n_xyz


def grid(dimensions, voxel_size):
    """The float32 numbers the encoder compares against: (bound_min, bound_lo, bound_hi, voxel, n_xyz)."""
    mn, mx, n_xyz = get_world_range(dimensions, voxel_size)
    bmin, bmax, v = mn.astype(np.float32), mx.astype(np.float32), np.float32(voxel_size)
    return bmin, bmin + v, bmax - v, v, [int(n) for n in n_xyz]


def n_voxels(dimensions, voxel_size):
    n = get_world_range(dimensions, voxel_size)[2]
    return int(n[0]) * int(n[1]) * int(n[2])


def voxel_counts(p, dimensions, voxel_size):
    """-> (nv, unique flat ids, their (point, corner) pair counts) of float32 points p."""
    bmin, lo, hi, v, n_xyz = grid(dimensions, voxel_size)
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore"):
        inb = np.all((p < hi) & (p > lo), axis=1)
    q = p[inb]
    if len(q) == 0:
        return 0, np.zeros(0, np.int64), np.zeros(0, np.int64)
    xn = (q - bmin) / v                                   # two float32 roundings
    f, c = np.floor(xn).astype(np.int64), np.ceil(xn).astype(np.int64)
    ids = []
    for k in range(8):
        g = [c[:, a] if (k >> a) & 1 else f[:, a] for a in range(3)]
        ids.append((g[0] * n_xyz[1] + g[1]) * n_xyz[2] + g[2])
    u, cnt = np.unique(np.concatenate(ids), return_counts=True)
    return len(q), u, cnt


def count(p, dimensions, voxel_size):
    """-> (nv, U, hist int64 [HIST_CAP + 1]: hist[c] voxels with exactly c pairs, hist[HIST_CAP] with that many or more)."""
    nv, u, cnt = voxel_counts(p, dimensions, voxel_size)
    return nv, len(u), np.bincount(np.minimum(cnt, HIST_CAP), minlength=HIST_CAP + 1).astype(np.int64)


def n_avg_pts(nv, U):
    return np.float32(8 * nv) / np.float32(U)


def live(hist, min_pts):
    return int(np.asarray(hist)[int(min_pts):].sum())


def stats(n_list):
    """SparseVolume.track_n_pts / print_statistic on the frames' n_avg_pts (python floats of float32 values)."""
    avg, n, mn, mx, lst = 0, 0, 1000, 0, []
    for v in n_list:
        v = float(v)
        lst.append(v)
        avg = (avg * n + v) / (n + 1)
        n += 1
        mn, mx = min(mn, v), max(mx, v)
    p = np.percentile(lst, [25, 50, 75]) if lst else [0, 0, 0]
    return {"mean": avg, "min": mn, "max": mx, "p25": p[0], "p50": p[1], "p75": p[2]}


def recommend(cands):
    """The smallest candidate with fits, min > 4 and mean >= 8 (the reference README's rule), or None."""
    ok = [c["voxel_size"] for c in cands if c["ok"]]
    return min(ok) if ok else None


def frame_points(f, T, max_depth):
    return points(f["depth"], f["intr_mat"], T, max_depth, f.get("conf"), f.get("conf_level", 0))


def candidates(frames, dimensions, axis_align_mat, voxel_sizes, max_depth=3.0, min_pts_in_grid=8):
    out = []
    frames = [f for f in frames if np.isfinite(np.asarray(f["T_wc"], np.float64)).all()]
    for v in voxel_sizes:
        nvox = n_voxels(dimensions, v)
        c = {"voxel_size": v, "n_xyz": get_world_range(dimensions, v)[2], "n_voxels": nvox, "fits": nvox < 2 ** 31,
             "rows": [], "n_avg_pts": [], "live": 0, "unique": 0}
        if c["fits"]:
            for f in frames:
                p = frame_points(f, np.asarray(axis_align_mat, np.float64) @ np.asarray(f["T_wc"], np.float64), max_depth)
                nv, U, h = count(p, dimensions, v)
                c["rows"].append((nv, U, h))
                if nv == 0:
                    continue
                c["n_avg_pts"].append(n_avg_pts(nv, U))
                c["live"] += live(h, min_pts_in_grid)
                c["unique"] += U
        c.update(stats(c["n_avg_pts"]))
        c["n_avg_pts"] = np.asarray(c["n_avg_pts"], np.float32)
        c["live_fraction"] = c["live"] / c["unique"] if c["unique"] else 0.0
        c["ok"] = bool(c["fits"] and len(c["n_avg_pts"]) and c["min"] > 4 and c["mean"] >= 8)
        out.append(c)
    return out


def plan(frames, voxel_sizes=(0.005, 0.01, 0.02, 0.04), max_depth=3.0, bin_size=0.01, n_bins=32768, trim=0.0,
         margin=0.05, align_yaw=None, up="y", min_pts_in_grid=8):
    if margin < bin_size:
        raise ValueError("margin must be at least one bin")
    dirs = directions(align_yaw, up)
    hist = np.zeros((len(dirs), n_bins), np.int64)
    n_points = n_frames = n_skipped = 0
    for f in frames:
        T = np.asarray(f["T_wc"], np.float64)
        if not np.isfinite(T).all():
            n_skipped += 1
            continue
        p = frame_points(f, T, max_depth)
        n_points += len(p)
        n_frames += 1
        hist += extent_hist(p, dirs, bin_size, n_bins)
    out = alignment(hist, bin_size, trim, margin, align_yaw, up)
    out.update(hist=hist, n_points=n_points, n_frames=n_frames, n_skipped=n_skipped)
    out["candidates"] = candidates(frames, out["dimensions"], out["axis_align_mat"], voxel_sizes, max_depth,
                                   min_pts_in_grid)
    out["voxel_size"] = recommend(out["candidates"])
    return out


def apply_points(axis_align_mat, xyz):
    A = np.asarray(axis_align_mat, np.float64)
    x = np.asarray(xyz, np.float64)
    return x @ A[:3, :3].T + A[:3, 3]
