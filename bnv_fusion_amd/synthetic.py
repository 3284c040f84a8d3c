"""Synthetic benchmark frames (SURVEY.md section 8d / BASELINE.md section 3).

Deviation from the letter of BASELINE.md section 3, in the direction of its stated intent ("frames overlap
as in real sequences", "decode masks are live"): there the depth pattern was a function of the pixel
only, i.e. glued to the rotating camera, so the observed "scene" moved >1 voxel per frame, no voxel ever
accumulated weight 8 and 93 % of the decode degenerated to the masked constant.  Here the SAME analytic
surface is a static scene and the camera pans over it.

Host-side data generation only (numpy, float64 like the reference's dataset code): depth image ->
camera points + Sobel normals -> world frame -> ``input_pts [1, N, 6]``.  The arithmetic follows
FusionInferenceAbstractDataset.__getitem__ (fusion_inference_dataset.py:40-90) with the kornia
0.6.2 normals it calls restated as in geometry.py:515-527.
"""
import math

import numpy as np

INTRINSICS = np.array([[525.0, 0.0, 319.5], [0.0, 525.0, 239.5], [0.0, 0.0, 1.0]])
# volume dimensions giving exactly 128^3 (v=0.02) / 256^3 (v=0.01) / 512^3 (v=0.01) grids
GRID_DIMS = {128: (2.52, 0.02), 256: (2.54, 0.01), 512: (5.10, 0.01), 64: (1.24, 0.02)}


YAW_STEP_DEG = 0.5      # camera yaw change per frame
YAW_AMPLITUDE_DEG = 4.0  # the camera pans back and forth inside +-4 degrees


def yaw_deg(t):
    """Triangle-wave pan: 0 -> +4 -> -4 -> ... in 0.5 degree steps (the scene stays inside the
    volume and is re-observed, so voxel weights accumulate as in a real scan)."""
    period = int(round(4 * YAW_AMPLITUDE_DEG / YAW_STEP_DEG))
    k = t % period
    q = period // 4
    if k <= q:
        return YAW_STEP_DEG * k
    if k <= 3 * q:
        return YAW_STEP_DEG * (2 * q - k)
    return YAW_STEP_DEG * (k - 4 * q)


def pose(t):
    """T_wc(t) = translate(0, 0, -1.5) . R_y(yaw(t))."""
    a = math.radians(yaw_deg(t))
    T = np.eye(4)
    T[:3, :3] = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    T[:3, 3] = [0.0, 0.0, -1.5]
    return T


def scene_depth0(u, v):
    """The static scene, given as the depth map camera 0 sees (defined for all real pixel
    coordinates of the 640x480 reference camera): 1.5 + 0.2 sin(u/40) cos(v/30) metres."""
    return 1.5 + 0.2 * np.sin(u / 40.0) * np.cos(v / 30.0)


_CLEAN = {}


def _clean_depth(t, H, W):
    """Noise-free depth (float64 metres) of the static scene from pose(t).  It depends on the yaw only, and the pan
    visits 17 yaw values, so it is computed once per (yaw, size) -- a 390-frame multi-GPU bench run builds its
    frames in seconds instead of a minute."""
    key = (yaw_deg(t), H, W)
    if key not in _CLEAN:
        sx, sy = 640.0 / W, 480.0 / H
        fx, fy, cx, cy = INTRINSICS[0, 0], INTRINSICS[1, 1], INTRINSICS[0, 2], INTRINSICS[1, 2]
        v, u = np.meshgrid(np.arange(H, dtype=np.float64) * sy, np.arange(W, dtype=np.float64) * sx, indexing="ij")
        R = pose(t)[:3, :3]
        ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=0).reshape(3, -1)
        r = (R @ ray).reshape(3, H, W)
        u0 = fx * r[0] / r[2] + cx
        v0 = fy * r[1] / r[2] + cy
        _CLEAN[key] = scene_depth0(u0, v0) / r[2]
    return _CLEAN[key]


def depth_image(t, H=480, W=640, seed=0):
    """Depth image of the static scene from pose(t), + N(0, 0.002) m sensor noise, stored as
    uint16 millimetres like the datasets (common.py:93).  All cameras share one optical centre, so
    the view from camera t is an exact homography of camera 0's: ray r = R_t K^-1 [u, v, 1] meets
    the scene at camera-0 pixel (u', v') = K r / r_z, and its depth in camera t is d0(u', v') / r_z."""
    rng = np.random.default_rng(seed + 1000 * t)
    d = _clean_depth(t, H, W) + rng.normal(0.0, 0.002, size=(H, W))
    return np.round(d * 1000.0).astype(np.uint16).astype(np.float64) / 1000.0


def depth_to_input_pts(depth, intr, T_wc, max_depth=10.0):
    """Host (numpy float64) version of the front end; same operation order as csrc/frontend.hip."""
    depth = np.asarray(depth, dtype=np.float64)
    mask = (depth > 0) & (depth < max_depth)
    depth = depth * mask
    H, W = depth.shape
    fx, fy, cx, cy = intr[0, 0], intr[1, 1], intr[0, 2], intr[1, 2]
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xyz = np.stack([(u - cx) / fx * depth, (v - cy) / fy * depth, depth], axis=0)
    p = np.pad(xyz, ((0, 0), (1, 1), (1, 1)), mode="edge")
    gx = (((((p[:, :-2, 2:] + 2 * p[:, 1:-1, 2:]) + p[:, 2:, 2:]) - p[:, :-2, :-2]) - 2 * p[:, 1:-1, :-2])
          - p[:, 2:, :-2]) / 8.0
    gy = (((((p[:, 2:, :-2] + 2 * p[:, 2:, 1:-1]) + p[:, 2:, 2:]) - p[:, :-2, :-2]) - 2 * p[:, :-2, 1:-1])
          - p[:, :-2, 2:]) / 8.0
    n = np.stack([gx[1] * gy[2] - gx[2] * gy[1], gx[2] * gy[0] - gx[0] * gy[2], gx[0] * gy[1] - gx[1] * gy[0]])
    norm = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    n = n / np.maximum(norm, 1e-12)
    ur = ((np.arange(W, dtype=np.float32) - np.float32(cx)) / np.float32(fx)).astype(np.float64)
    vr = ((np.arange(H, dtype=np.float32) - np.float32(cy)) / np.float32(fy)).astype(np.float64)
    pc = np.stack([ur[None, :] * depth, vr[:, None] * depth, depth], axis=0)
    T = np.asarray(T_wc, dtype=np.float64)
    pw = [((T[i, 0] * pc[0] + T[i, 1] * pc[1]) + T[i, 2] * pc[2]) + T[i, 3] for i in range(3)]
    nw = [(T[i, 0] * n[0] + T[i, 1] * n[1]) + T[i, 2] * n[2] for i in range(3)]
    return np.stack(pw + nw, axis=-1).reshape(-1, 6)[mask.reshape(-1)]


def depth_u16(t, H=480, W=640, seed=0):
    """The frame's depth image as the dataset stores it: uint16 millimetres."""
    return np.round(depth_image(t, H, W, seed) * 1000.0).astype(np.uint16)


def intrinsics(H=480, W=640):
    intr = INTRINSICS.copy()
    if (H, W) != (480, 640):
        intr[0] *= W / 640.0
        intr[1] *= H / 480.0
    return intr


def frame(t, H=480, W=640, seed=0):
    """-> numpy float32 [1, N, 6] (the float64 -> .float() cast of run_e2e.py:249)."""
    intr = INTRINSICS.copy()
    if (H, W) != (480, 640):
        intr[0] *= W / 640.0
        intr[1] *= H / 480.0
    pts = depth_to_input_pts(depth_image(t, H, W, seed), intr, pose(t))
    return pts.astype(np.float32)[None]


def _visible_in(R, u0, v0, W=640, H=480):
    """Which camera-0 pixel coordinates (u0, v0) the camera of rotation R (the same optical centre) sees inside its
    W x H image (pixel centres 0 .. W-1, 0 .. H-1)."""
    fx, fy, cx, cy = INTRINSICS[0, 0], INTRINSICS[1, 1], INTRINSICS[0, 2], INTRINSICS[1, 2]
    d = np.stack([(u0 - cx) / fx, (v0 - cy) / fy, np.ones_like(u0)], axis=0).reshape(3, -1)
    dt = (R.T @ d).reshape((3,) + u0.shape)           # the world direction in camera t's frame (pose(0) has R = I)
    with np.errstate(divide="ignore", invalid="ignore"):
        ut = fx * dt[0] / dt[2] + cx
        vt = fy * dt[1] / dt[2] + cy
    return (dt[2] > 0) & (ut >= 0) & (ut <= W - 1) & (vt >= 0) & (vt <= H - 1)


def gt_mesh(region="union", step_px=1.0):
    """Ground-truth mesh of the static scene: ``scene_depth0`` triangulated over camera-0 pixel coordinates (a grid of
    ``step_px``) and lifted to world coordinates with ``pose(0)``, float64 then cast to float32 -> mesh.TriMesh.

    region "union": the part of the surface that ANY yaw of the pan (``yaw_deg`` over a period) sees -- the
    ground truth for precision; "common": the part EVERY yaw sees -- for recall, so that borders only a few frames saw
    do not count as missing.  A triangle is kept when its three vertices are in the region."""
    from .mesh import TriMesh
    if region not in ("union", "common"):
        raise ValueError(f"region {region!r}: 'union' or 'common'")
    step = float(step_px)
    if not step > 0:
        raise ValueError("step_px must be positive")
    yaws = sorted({yaw_deg(t) for t in range(int(round(4 * YAW_AMPLITUDE_DEG / YAW_STEP_DEG)))})
    # camera-0 pixel coordinates wide enough for the extreme yaws (+-4 degrees: ~37 px in u, a few in v)
    u = np.arange(-80.0, 640.0 + 80.0 + step / 2, step)
    v = np.arange(-40.0, 480.0 + 40.0 + step / 2, step)
    v0, u0 = np.meshgrid(v, u, indexing="ij")
    seen = None
    for y in yaws:
        a = math.radians(y)
        R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        m = _visible_in(R, u0, v0)
        seen = m if seen is None else (seen | m if region == "union" else seen & m)
    fx, fy, cx, cy = INTRINSICS[0, 0], INTRINSICS[1, 1], INTRINSICS[0, 2], INTRINSICS[1, 2]
    d = scene_depth0(u0, v0)
    pc = np.stack([(u0 - cx) / fx * d, (v0 - cy) / fy * d, d], axis=-1).reshape(-1, 3)
    T = pose(0)
    pw = pc @ T[:3, :3].T + T[:3, 3]
    rows, cols = u0.shape
    idx = np.arange(rows * cols).reshape(rows, cols)
    a, b, c, e = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    tris = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, e], -1).reshape(-1, 3)])
    s = seen.reshape(-1)
    tris = tris[s[tris].all(axis=1)]
    used, inv = np.unique(tris, return_inverse=True)
    return TriMesh(pw[used].astype(np.float32), inv.reshape(-1, 3))


ARKIT_HW = (192, 256)                      # the LiDAR depth resolution of current iPhones / iPads
ARKIT_CENTER = np.array([0.05, -0.04, 0.1])   # the scene's world box centre: the capture's export.obj is not at 0


def arkit_capture(n_frames, voxel_size=0.01, seed=0):
    """The synthetic scene as an iPhone LiDAR capture would hold it (datasets.write_arkit_capture's arguments): depth at
    256x192 from ``pose(t)``, and wrong depth that the sensor marks as confidence 0.

    * flying pixels: the scene has no occluding edge, so bands of 4 pixels every 48 rows and columns stand in for
      depth edges; each band's depth is pulled 15-25 % towards the camera (one factor per band and frame), as pixels
      that mix a foreground edge with the surface behind it -- a coherent ghost surface, not scattered noise;
    * outliers: 1.5 % of the other pixels, 0.2-0.5 m in front of or behind the surface.

    Corrupted pixels get confidence 0, their clean 4-neighbours 1, every other pixel 2.  The ARKit world is the
    synthetic world; the loader's volume is centred on ``ARKIT_CENTER`` -> dict(depths, confs, intrinsics, poses (in
    the loader's frame), dimensions, center, outliers: per frame the [K, 2] (row, col) pixels of the outliers)."""
    H, W = ARKIT_HW
    rng = np.random.default_rng(seed + 77)
    dims = {0.01: 2.54, 0.02: 2.52}.get(voxel_size, 2.54)
    align = np.eye(4)
    align[:3, 3] = -ARKIT_CENTER
    depths, confs, poses, outliers = [], [], [], []
    for t in range(n_frames):
        d = depth_image(t, H, W, seed)
        bad = np.zeros((H, W), bool)
        band = np.zeros((H, W), bool)
        pull = np.ones((H, W))
        for k in range(24, H, 48):
            band[k:k + 4] = True
            pull[k:k + 4] = rng.uniform(0.75, 0.85)
        for k in range(24, W, 48):
            band[:, k:k + 4] = True
            pull[:, k:k + 4] = rng.uniform(0.75, 0.85)
        d = np.where(band, d * pull, d)
        bad |= band
        sprinkle = (~band) & (rng.random((H, W)) < 0.015)
        off = rng.uniform(0.2, 0.5, size=(H, W)) * np.where(rng.random((H, W)) < 0.5, -1.0, 1.0)
        d = np.where(sprinkle, d + off, d)
        bad |= sprinkle
        near = np.zeros_like(bad)
        near[1:] |= bad[:-1]
        near[:-1] |= bad[1:]
        near[:, 1:] |= bad[:, :-1]
        near[:, :-1] |= bad[:, 1:]
        conf = np.where(bad, 0, np.where(near, 1, 2)).astype(np.uint8)
        depths.append(np.round(d * 1000.0).astype(np.uint16))
        confs.append(conf)
        poses.append(align @ pose(t))
        outliers.append(np.argwhere(sprinkle))
    return {"depths": depths, "confs": confs, "intrinsics": intrinsics(H, W), "poses": poses,
            "dimensions": [dims] * 3, "center": ARKIT_CENTER.copy(), "outliers": outliers}


# --------------------------------------------------------------------------- #
# local surface patches for training the embedding (train.EmbeddingTrainer)
# --------------------------------------------------------------------------- #
PATCH_KINDS = ("plane", "sphere", "cylinder", "box")


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _unit(rng, k=None):
    v = rng.normal(size=(3,) if k is None else (k, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def patch_shape(rng):
    """A random analytic shape whose surface passes through a point q of [-0.3, 0.3]^3, in voxel units: a plane, a
    sphere or a cylinder of radius 0.5 .. 8 voxels, or a box with half extents 0.5 .. 3 voxels, at a random pose."""
    kind = PATCH_KINDS[int(rng.integers(len(PATCH_KINDS)))]
    q = rng.uniform(-0.3, 0.3, 3)
    nrm = _unit(rng)
    if kind == "plane":
        return {"kind": kind, "point": q, "normal": nrm}
    r = float(np.exp(rng.uniform(np.log(0.5), np.log(8.0))))
    if kind == "sphere":
        return {"kind": kind, "center": q - r * nrm, "radius": r}
    if kind == "cylinder":
        a = _unit(rng)
        a = a - np.dot(a, nrm) * nrm
        a /= np.linalg.norm(a)
        return {"kind": kind, "center": q - r * nrm, "axis": a, "radius": r}
    R = _rotation(rng)
    h = rng.uniform(0.5, 3.0, 3)
    local = rng.uniform(-0.8, 0.8, 3) * h      # q on the +z face, off its centre
    local[2] = h[2]
    return {"kind": kind, "center": q - R @ local, "rotation": R, "half": h}


def shape_sdf(s, p):
    """Exact signed distance (negative inside) of ``patch_shape`` s at points p [..., 3]."""
    k = s["kind"]
    if k == "plane":
        return (p - s["point"]) @ s["normal"]
    if k == "sphere":
        return np.linalg.norm(p - s["center"], axis=-1) - s["radius"]
    if k == "cylinder":
        d = p - s["center"]
        d = d - (d @ s["axis"])[..., None] * s["axis"]
        return np.linalg.norm(d, axis=-1) - s["radius"]
    loc = (p - s["center"]) @ s["rotation"]
    d = np.abs(loc) - s["half"]
    return np.linalg.norm(np.maximum(d, 0.0), axis=-1) + np.minimum(d.max(-1), 0.0)


def shape_closest(s, p):
    """Closest surface point and the outward unit normal there, for points p [k, 3]."""
    k = s["kind"]
    if k == "plane":
        n = np.broadcast_to(s["normal"], p.shape)
        return p - shape_sdf(s, p)[:, None] * n, n.copy()
    if k == "sphere":
        d = p - s["center"]
        n = d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-12)
        return s["center"] + s["radius"] * n, n
    if k == "cylinder":
        d = p - s["center"]
        ax = (d @ s["axis"])[:, None] * s["axis"]
        radial = d - ax
        n = radial / np.maximum(np.linalg.norm(radial, axis=-1, keepdims=True), 1e-12)
        return s["center"] + ax + s["radius"] * n, n
    R, h = s["rotation"], s["half"]
    loc = (p - s["center"]) @ R
    inside = np.all(np.abs(loc) <= h, axis=-1)
    c = np.clip(loc, -h, h)
    # interior points move to the nearest face
    gap = h - np.abs(loc)
    axis = np.argmin(gap, axis=-1)
    rows = np.nonzero(inside)[0]
    c[rows, axis[rows]] = np.sign(loc[rows, axis[rows]]) * h[axis[rows]]
    # normal: the face the closest point lies on (the largest |c| / h)
    ratio = np.abs(c) / h - 1.0
    face = np.argmax(ratio, axis=-1)
    n_loc = np.zeros_like(c)
    n_loc[np.arange(len(c)), face] = np.where(c[np.arange(len(c)), face] >= 0, 1.0, -1.0)
    return s["center"] + c @ R.T, n_loc @ R.T


def _surface_samples(s, k, rng):
    """k points on the surface near the cube [-1, 1]^3 and their normals: a box's faces sampled uniformly by area
    (a closest-point map would pile points onto its edges), other shapes: uniform points of the cube mapped to their
    closest surface point."""
    if s["kind"] != "box":
        return shape_closest(s, rng.uniform(-1.0, 1.0, (k, 3)))
    h = s["half"]
    area = np.array([h[1] * h[2], h[0] * h[2], h[0] * h[1]]).repeat(2)
    face = rng.choice(6, size=k, p=area / area.sum())
    axis, sign = face // 2, np.where(face % 2 == 0, -1.0, 1.0)
    loc = rng.uniform(-1.0, 1.0, (k, 3)) * h
    loc[np.arange(k), axis] = sign * h[axis]
    n_loc = np.zeros((k, 3))
    n_loc[np.arange(k), axis] = sign
    return s["center"] + loc @ s["rotation"].T, n_loc @ s["rotation"].T


def local_patches(n, M, seed=0, noise=0.0, n_pts=64, near_fraction=0.5, near_sigma=0.15):
    """``n`` training patches from analytic shapes with exact SDF, in the units of the reference's local shapes: the
    cube [-1, 1]^3 around one lattice vertex, in voxel units, ``gt`` in voxel units as well.

    Returns {"input_pts" [n, 64, 6] f32 (surface points inside the cube + outward unit normals; Gaussian position
    noise of std ``noise`` voxels), "training_pts" [n, M, 3] f32 (a ``near_fraction`` of them a Gaussian step of std
    ``near_sigma`` off surface points, the rest uniform in the cube, all clipped into it), "gt" [n, M] f32 (exact
    SDF), "shapes" (the shape of every patch, see ``patch_shape``)}."""
    rng = np.random.default_rng(seed)
    inp = np.zeros((n, n_pts, 6), np.float32)
    tp = np.zeros((n, M, 3), np.float32)
    gt = np.zeros((n, M), np.float32)
    shapes = []
    for i in range(n):
        while True:
            s = patch_shape(rng)
            cand, nrm = _surface_samples(s, 4 * n_pts, rng)
            keep = np.all(np.abs(cand) <= 1.0, axis=-1)
            if keep.sum() >= 8:
                break
        cand, nrm = cand[keep], nrm[keep]
        idx = rng.permutation(len(cand))[:n_pts] if len(cand) >= n_pts else rng.integers(0, len(cand), n_pts)
        pts = cand[idx] + rng.normal(scale=noise, size=(n_pts, 3)) if noise > 0 else cand[idx]
        inp[i, :, :3] = pts
        inp[i, :, 3:] = nrm[idx]
        n_near = int(round(near_fraction * M))
        base = cand[rng.integers(0, len(cand), n_near)]
        near = base + rng.normal(scale=near_sigma, size=(n_near, 3))
        q = np.clip(np.concatenate([near, rng.uniform(-1.0, 1.0, (M - n_near, 3))]), -1.0, 1.0).astype(np.float32)
        tp[i] = q
        gt[i] = shape_sdf(s, q.astype(np.float64))
        shapes.append(s)
    return {"input_pts": inp, "training_pts": tp, "gt": gt, "shapes": shapes}


# ---- a colour field to test mesh colouring with ---------------------------------------------------------------------
# per channel two triangle waves: (axis, 1 / period in metres, phase in periods).  Periods of a few decimetres, other
# periods and axes in every channel: a channel swap or an axis mix-up changes the field everywhere.
COLOR_WAVES = (((0, 1.0 / 0.30, 0.00), (1, 1.0 / 0.50, 0.25)),
               ((1, 1.0 / 0.40, 0.50), (2, 1.0 / 0.70, 0.00)),
               ((2, 1.0 / 0.35, 0.25), (0, 1.0 / 0.60, 0.50)))


def surface_color(points):
    """A fixed procedural colour field of world position: ``points`` [..., 3] float64 (a numpy array or a torch tensor)
    -> [..., 3] float64 in [0, 255] (red, green, blue; not rounded).  Each channel is the mean of two triangle waves
    tri(s) = |2 (s - floor(s + 0.5))| of s = x[axis] / period + phase, times 255: floor, multiply and add only, one
    rounding per operation and no transcendental function, so numpy and torch give the same bits."""
    is_np = isinstance(points, np.ndarray)
    if is_np:
        points = np.asarray(points, dtype=np.float64)
    channels = []
    for waves in COLOR_WAVES:
        acc = None
        for axis, inv_period, phase in waves:
            t = points[..., axis] * inv_period
            t = t + phase
            u = t + 0.5
            u = np.floor(u) if is_np else u.floor()
            d = t - u
            d = d * 2.0
            d = np.abs(d) if is_np else d.abs()
            acc = d if acc is None else acc + d
        acc = acc * 127.5
        channels.append(acc)
    return np.stack(channels, axis=-1) if is_np else _torch_stack(channels)


def _torch_stack(channels):
    import torch
    return torch.stack(channels, dim=-1)
