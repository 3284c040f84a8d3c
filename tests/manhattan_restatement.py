"""The Manhattan frame of a scene restated in numpy: the definition that pass 0 of the volume planner
(csrc/plan.hip: k_plan_normals; bnv_fusion_amd/plan.py: ManhattanFrame) is held to -- the histogram bit for bit
(tests/test_gpu_manhattan.py), the estimate to 1e-9.

* ``pixel_normals``: per pixel with four valid neighbours ``step`` pixels away a float64 normal, every operation one
  numpy ufunc call (one rounding), in the order include/bnv_fusion.h writes them;
* ``bins`` / ``histogram``: the cube-map bin of a unit normal, and per bin the count and the sum of the normals in
  2^-20 fixed point -- integers, so any order of accumulation gives the same histogram;
* ``estimate``: the three dominant orthogonal directions of the histogram (coarse search over the 16 fullest bins and
  45 angles, five rounds of count-weighted cone means projected to the nearest rotation) and which of them is down.

No torch, no package import: numpy only.
"""
import math

import numpy as np

SCALE = 1048576.0            # 2^20
N_FIRST = 16                 # bins tried as the first axis
N_ANGLES = 45                # angles in [0, 90) degrees about it
N_ROUNDS = 5


class Refused(ValueError):
    """No Manhattan frame is defined for these normals."""


# ---- the histogram ---------------------------------------------------------------------------------------------------

def depth_metres(depth, max_depth, conf=None, conf_level=0):
    """float64 [H, W] and the validity mask: finite, 0 < z <= max_depth, conf >= conf_level."""
    d = np.asarray(depth)
    z = d.astype(np.float64) / 1000.0 if d.dtype == np.uint16 else d.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(z) & (z > 0.0) & (z <= max_depth)
    if conf is not None:
        ok &= np.asarray(conf).astype(np.int64) >= int(conf_level)
    return np.where(ok, z, 0.0), ok


def camera_points(z, K):
    H, W = z.shape
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x = ((np.arange(W, dtype=np.float64) - cx) / fx)[None, :] * z
    y = ((np.arange(H, dtype=np.float64) - cy) / fy)[:, None] * z
    return x, y, z


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def pixel_normals(depth, K, T_wc, max_depth=3.0, conf=None, conf_level=0, step=1, jump=0.1):
    """float64 [N, 3]: the world normals of the pixels that count, in row-major order."""
    z, ok = depth_metres(depth, max_depth, conf, conf_level)
    H, W = z.shape
    s = int(step)
    if H <= 2 * s or W <= 2 * s:
        return np.zeros((0, 3))
    P = camera_points(z, K)
    c = (slice(s, H - s), slice(s, W - s))
    l, r = (slice(s, H - s), slice(0, W - 2 * s)), (slice(s, H - s), slice(2 * s, W))
    u, d = (slice(0, H - 2 * s), slice(s, W - s)), (slice(2 * s, H), slice(s, W - s))
    keep = ok[c] & ok[l] & ok[r] & ok[u] & ok[d]
    gate = jump * z[c]
    for q in (l, r, u, d):
        keep &= np.abs(z[q] - z[c]) <= gate
    e = [P[i][r] - P[i][l] for i in range(3)]
    f = [P[i][d] - P[i][u] for i in range(3)]
    n = [e[1] * f[2] - e[2] * f[1], e[2] * f[0] - e[0] * f[2], e[0] * f[1] - e[1] * f[0]]
    away = dot3(n, [P[i][c] for i in range(3)]) > 0.0
    n = [np.where(away, -v, v) for v in n]
    R = np.asarray(T_wc, np.float64)[:3, :3]
    w = [(R[i, 0] * n[0] + R[i, 1] * n[1]) + R[i, 2] * n[2] for i in range(3)]
    with np.errstate(invalid="ignore", divide="ignore"):
        length = np.sqrt(dot3(w, w))
        keep &= np.isfinite(length) & (length > 0.0)
        w = [v / length for v in w]
    return np.stack(w, -1)[keep]


def bins(w, n_side):
    """int64 [N]: the cube-map bin of unit normals w [N, 3]."""
    w = np.asarray(w, np.float64).reshape(-1, 3)
    a = np.abs(w)
    m = np.zeros(len(w), np.int64)
    m[a[:, 1] > a[:, 0]] = 1
    m[a[:, 2] > a[np.arange(len(w)), m]] = 2
    i = np.arange(len(w))
    wm = w[i, m]
    face = 2 * m + (wm < 0.0)
    out = []
    for k in (1, 2):
        q = w[i, (m + k) % 3] / np.abs(wm)
        out.append(np.clip(np.floor(((q + 1.0) * 0.5) * float(n_side)), 0, n_side - 1).astype(np.int64))
    return (face * n_side + out[0]) * n_side + out[1]


def histogram(normals, n_side):
    """int64 [6 n_side^2, 4]: count and the fixed-point sums of the normals' three components."""
    hist = np.zeros((6 * n_side * n_side, 4), np.int64)
    w = np.asarray(normals, np.float64).reshape(-1, 3)
    if len(w):
        b = bins(w, n_side)
        np.add.at(hist[:, 0], b, 1)
        fixed = np.rint(w * SCALE).astype(np.int64)
        for k in range(3):
            np.add.at(hist[:, 1 + k], b, fixed[:, k])
    return hist


def frame_normals(f, max_depth=3.0, step=1, jump=0.1):
    return pixel_normals(f["depth"], f["intr_mat"], f["T_wc"], max_depth, f.get("conf"),
                         f.get("conf_level", 0) if f.get("conf") is not None else 0, step, jump)


def frames_histogram(frames, n_side=32, max_depth=3.0, step=1, jump=0.1):
    hist = np.zeros((6 * n_side * n_side, 4), np.int64)
    for f in frames:
        hist += histogram(frame_normals(f, max_depth, step, jump), n_side)
    return hist


# ---- the frame -------------------------------------------------------------------------------------------------------

def bin_centres(n_side):
    """float64 [6 n_side^2, 3]: the unit vector through the middle of every bin."""
    out = np.zeros((6, n_side, n_side, 3))
    q = (np.arange(n_side) + 0.5) * 2.0 / n_side - 1.0
    for face in range(6):
        m = face // 2
        out[face, :, :, m] = -1.0 if face & 1 else 1.0
        out[face, :, :, (m + 1) % 3] = q[:, None]
        out[face, :, :, (m + 2) % 3] = q[None, :]
    out = out.reshape(-1, 3)
    return out / np.sqrt(dot3(out.T, out.T))[:, None]


def cone_dots(centres, axis):
    return (centres[:, 0] * axis[0] + centres[:, 1] * axis[1]) + centres[:, 2] * axis[2]


def nearest_rotation(M):
    U, _, Vt = np.linalg.svd(M)
    D = np.diag([1.0, 1.0, np.linalg.det(U @ Vt)])
    return U @ D @ Vt


def coarse(hist, centres, cos_cone):
    count = hist[:, 0]
    first = [int(b) for b in np.argsort(-count, kind="stable")[:N_FIRST] if count[b] > 0]
    best, best_score = None, -1
    for b in first:
        a = centres[b]
        e = np.zeros(3)
        e[int(np.argmin(np.abs(a)))] = 1.0
        p = np.cross(a, e)
        p = p / np.sqrt(dot3(p, p))
        q = np.cross(a, p)
        for j in range(N_ANGLES):
            th = j * (math.pi / 2) / N_ANGLES
            s = math.cos(th) * p + math.sin(th) * q
            axes = np.stack([a, s, np.cross(a, s)])
            inside = np.zeros(len(count), bool)
            for ax in axes:
                inside |= np.abs(cone_dots(centres, ax)) >= cos_cone
            score = int(count[inside].sum())
            if score > best_score:
                best, best_score = axes, score
    return best


def refine(hist, centres, axes, cos_cone):
    sums = hist[:, 1:].astype(np.float64)
    for _ in range(N_ROUNDS):
        new = []
        for ax in axes:
            d = cone_dots(centres, ax)
            inside = np.abs(d) >= cos_cone
            v = (np.where(d[inside] < 0.0, -1.0, 1.0)[:, None] * sums[inside]).sum(axis=0)
            length = math.sqrt(float(dot3(v, v)))
            # each axis weighs what its cone counts: an axis a few stray normals define must not turn the other two
            new.append(float(hist[inside, 0].sum()) * (v / length if length > 0.0 else ax))
        axes = nearest_rotation(np.stack(new))
    return axes


def estimate(hist, n_side, cone=10.0, min_confidence=0.3, down=(0.0, 1.0, 0.0), view=(0.0, 0.0, 1.0)):
    """-> dict(R [3, 3] with rows x, y (down), z; confidence; axis_mass [3] in the order of R's rows; n_normals).
    ``down``: the mean camera down in the world; ``view``: the first frame's viewing direction."""
    hist = np.asarray(hist, np.int64)
    total = int(hist[:, 0].sum())
    if total == 0:
        raise Refused("no normal counted")
    centres, cos_cone = bin_centres(n_side), math.cos(math.radians(cone))
    axes = refine(hist, centres, coarse(hist, centres, cos_cone), cos_cone)
    mass = np.array([int(hist[np.abs(cone_dots(centres, ax)) >= cos_cone, 0].sum()) for ax in axes]) / total
    confidence = float(mass.sum())
    if int((mass > 0).sum()) < 2:
        raise Refused(f"only {int((mass > 0).sum())} axis carries normals")
    if confidence < min_confidence:
        raise Refused(f"confidence {confidence:.3f} < {min_confidence}")
    signed = [(i, s) for i in range(3) for s in (1.0, -1.0)]

    def closest(v, among):
        best, best_dot = None, None
        for i, s in among:
            d = float(dot3(s * axes[i], np.asarray(v, np.float64)))
            if best_dot is None or d > best_dot:
                best, best_dot = (i, s), d
        return best

    iy, sy = closest(down, signed)
    iz, sz = closest(view, [c for c in signed if c[0] != iy])
    y, z = sy * axes[iy], sz * axes[iz]
    x = np.cross(y, z)
    ix = 3 - iy - iz
    return {"R": np.stack([x, y, z]), "confidence": confidence, "axis_mass": mass[[ix, iy, iz]], "n_normals": total}


def estimate_frames(frames, n_side=32, max_depth=3.0, step=1, jump=0.1, cone=10.0, min_confidence=0.3, down_hint=None):
    """The frame of depth frames with finite poses: down is the sum of the cameras' down axes (or ``down_hint``), +z the
    horizontal axis closest to the first frame's viewing direction."""
    frames = [f for f in frames if np.isfinite(np.asarray(f["T_wc"], np.float64)).all()]
    hist = frames_histogram(frames, n_side, max_depth, step, jump)
    down = np.sum([np.asarray(f["T_wc"], np.float64)[:3, 1] for f in frames], axis=0) if down_hint is None else down_hint
    out = estimate(hist, n_side, cone, min_confidence, down, np.asarray(frames[0]["T_wc"], np.float64)[:3, 2])
    out["hist"] = hist
    out["n_frames"] = len(frames)
    return out


def axis_errors_deg(R, G):
    """Per row of R the angle to the room's axis of the same name in a world rotated by G (its columns), sign folded."""
    G = np.asarray(G, np.float64)
    return [math.degrees(math.acos(min(1.0, abs(float(dot3(R[i], G[:, i])))))) for i in range(3)]


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(degrees)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def issue_rotation():
    """G of the issue: 37 degrees about (0.3, -0.8, 0.5) times -21 degrees about x."""
    return rotation((0.3, -0.8, 0.5), 37.0) @ rotation((1.0, 0.0, 0.0), -21.0)


def premultiplied(frames, G, shift=(0.0, 0.0, 0.0)):
    G4 = np.eye(4)
    G4[:3, :3] = G
    G4[:3, 3] = shift
    return [dict(f, T_wc=G4 @ np.asarray(f["T_wc"], np.float64)) for f in frames]
