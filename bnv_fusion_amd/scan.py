"""Scan a triangle mesh into a depth sequence on the GPU: the first stage of the reference's synthetic pipeline.

The reference's ICL-NUIM data are depth images rendered from a mesh plus a simulated Kinect
(src/scripts/generate_fusion_data_icl_nuim.py repackages frames somebody else rendered; src/utils/geometry.py:
``Simulator`` is the sensor model).  ``MeshScanner`` renders them here: a ray caster over the index of
``evaluate.MeshSDF`` (csrc/meshray.hip; include/bnv_fusion.h: bnv_mesh_ray_cast / bnv_mesh_render_depth), which also
knows which faces the camera saw -- the ground truth for recall.  ``simulate_sensor`` is ``Simulator.simulate`` as one
kernel (bnv_depth_sensor).  GPU only: a CPU device is refused.  Camera convention: the data sets' (+z forward, y down),
``T_wc`` camera-to-world.

    scanner = MeshScanner(mesh)
    for frame in scan_frames(scanner, orbit_poses(center, 2.0, 100), K, 480, 640, noise="kinect"):
        neural_map.fuse_and_decode(frame)
    evaluate.evaluate_meshes(result, mesh, gt_recall=scanner.visible_mesh())
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib, evaluate
from .mesh import TriMesh

MAX_POSES = 8                 # BNV_MESH_RENDER_MAX_POSES
HIT, BACK_FACE = 1, 2         # flags of MeshScanner.cast
SENSOR_BF, SENSOR_SIGMA_D, SENSOR_SIGMA_PX = 35.130, 0.027778, 0.25      # geometry.py:54-69


def _fp32_inf(x):
    return float(np.float32(min(max(float(x), -3.4028234663852886e38), 3.4028234663852886e38)))


class MeshScanner:
    """A depth camera and a ray caster over one mesh.  ``vertices`` fp32 [V, 3] and ``faces`` int [T, 3] device
    tensors, or a TriMesh (uploaded to ``device``, default the current GPU) -- the conventions of ``evaluate.MeshSDF``,
    whose index this owns (``.index``)."""

    def __init__(self, vertices, faces=None, device=None):
        v, f = evaluate._mesh_tensors(vertices, faces, device)
        self.vertices, self.faces = v, f
        self.device = v.device
        self.index = evaluate.MeshSDF(v, f)
        self.n_faces = self.index.n_faces
        self.seen = torch.zeros(self.n_faces, dtype=torch.int32, device=self.device)

    def reset_seen(self):
        self.seen.zero_()

    def cast(self, origins, dirs, t_min=0.0, t_max=math.inf):
        """Rays ``origins + t dirs`` (fp32 [..., 3] on the mesh's device; ``dirs`` need not be unit) -> (t fp32 [...],
        face int32 [...], uv fp32 [..., 2], flags uint8 [...]) of the nearest hit with t in [t_min, t_max]: the hit point
        is (1 - u - v) v0 + u v1 + v v2 of ``face``; flags = ``HIT`` | ``BACK_FACE``.  No hit, a non-finite ray or a
        zero direction: (nan, -1, nan, 0)."""
        o = evaluate._on_gpu(origins, "origins", torch.float32)
        d = evaluate._on_gpu(dirs, "dirs", torch.float32)
        if o.shape != d.shape or o.dim() < 1 or o.shape[-1] != 3 or o.numel() == 0:
            raise ValueError(f"origins / dirs: expected equal non-empty [..., 3] tensors, got {tuple(o.shape)} and "
                             f"{tuple(d.shape)}")
        if o.device != self.device or d.device != self.device:
            raise ValueError(f"rays on {o.device} / {d.device}, mesh on {self.device}")
        if not float(t_min) <= float(t_max):
            raise ValueError(f"t_min {t_min} > t_max {t_max}")
        lead = tuple(o.shape[:-1])
        o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        n = int(o.shape[0])
        lib = _lib.load()
        with torch.cuda.device(self.device):
            t = torch.empty(n, dtype=torch.float32, device=self.device)
            face = torch.empty(n, dtype=torch.int32, device=self.device)
            uv = torch.empty((n, 2), dtype=torch.float32, device=self.device)
            flags = torch.empty(n, dtype=torch.uint8, device=self.device)
            _lib.check(lib.bnv_mesh_ray_cast(_lib.ptr(self.index._ws), self.index._ws_bytes, _lib.ptr(o), _lib.ptr(d), n,
                                             _fp32_inf(t_min), _fp32_inf(t_max) if math.isfinite(t_max) else math.inf,
                                             _lib.ptr(t), _lib.ptr(face), _lib.ptr(uv), _lib.ptr(flags),
                                             _lib.stream_ptr()), "bnv_mesh_ray_cast")
        return t.reshape(lead), face.reshape(lead), uv.reshape(lead + (2,)), flags.reshape(lead)

    def render_depth(self, T_wc, K, H, W, near=0.0, max_depth=math.inf, normals=False, count_seen=True):
        """z-depth image(s) of the mesh from camera-to-world pose(s) ``T_wc`` ([4, 4] or [n, 4, 4]; any n: launches of
        up to ``MAX_POSES`` poses) with intrinsics ``K`` [3, 3] -> (depth fp32 [H, W] or [n, H, W] in metres, 0 where
        nothing is hit or the nearest hit lies outside [near, max_depth); face int32, -1 there[; normals fp32
        [..., 3]: unit, world coordinates, turned towards the camera]).  Every pixel with depth adds one to ``.seen`` of
        its face unless ``count_seen=False``."""
        T = np.asarray(T_wc, dtype=np.float64)
        single = T.ndim == 2
        T = T.reshape(-1, 4, 4)
        Kf = np.ascontiguousarray(np.asarray(K, dtype=np.float64)[:3, :3], dtype=np.float32).reshape(-1)
        H, W, n = int(H), int(W), int(T.shape[0])
        if n == 0:
            raise ValueError("render_depth: no pose")
        if not (float(near) <= float(max_depth) and float(max_depth) > 0):
            raise ValueError(f"render_depth: near {near}, max_depth {max_depth}")
        lib = _lib.load()
        with torch.cuda.device(self.device):
            depth = torch.empty((n, H, W), dtype=torch.float32, device=self.device)
            face = torch.empty((n, H, W), dtype=torch.int32, device=self.device)
            nrm = torch.empty((n, H, W, 3), dtype=torch.float32, device=self.device) if normals else None
            for s in range(0, n, MAX_POSES):
                k = min(MAX_POSES, n - s)
                poses = np.ascontiguousarray(T[s:s + k], dtype=np.float32).reshape(-1)
                _lib.check(lib.bnv_mesh_render_depth(
                    _lib.ptr(self.index._ws), self.index._ws_bytes, k, Kf.ctypes.data_as(C.POINTER(C.c_float)),
                    poses.ctypes.data_as(C.POINTER(C.c_float)), H, W, _fp32_inf(near),
                    _fp32_inf(max_depth) if math.isfinite(max_depth) else math.inf, _lib.ptr(depth[s:]),
                    _lib.ptr(face[s:]), _lib.ptr(nrm[s:]) if normals else None,
                    _lib.ptr(self.seen) if count_seen else None, self.n_faces, _lib.stream_ptr()),
                    "bnv_mesh_render_depth")
        out = (depth, face, nrm) if normals else (depth, face)
        return tuple(t[0] for t in out) if single else out

    def track(self, frame, T_guess=None, model_size=None, **icp):
        """Localises a depth frame against the mesh: renders it at ``T_guess`` (default ``frame['T_wc']``; view of
        ``model_size`` = (H, W), default the frame's; ``.seen`` is not counted) and aligns the frame to that view
        (``tracking.icp_align``) -> ``TrackResult``."""
        from . import tracking
        max_depth = icp.pop("max_depth", 3.0)

        def render(T, K, H, W):
            depth, _, nrm = self.render_depth(T, K, H, W, max_depth=max_depth, normals=True, count_seen=False)
            return depth, nrm
        return tracking.track_against(render, frame, T_guess, model_size, max_depth=max_depth, **icp)

    def visible_mesh(self, min_pixels=1):
        """The faces seen by at least ``min_pixels`` pixels since construction or ``reset_seen`` -> TriMesh (host) with
        the vertices they use: the ground truth for recall."""
        keep = (self.seen >= int(min_pixels)).cpu().numpy()
        faces = self.faces.cpu().numpy()[keep].astype(np.int64)
        used, inv = np.unique(faces, return_inverse=True)
        return TriMesh(self.vertices.cpu().numpy()[used], inv.reshape(-1, 3))


def simulate_sensor(depth, seed, frame, table=None, bf=SENSOR_BF, sigma_d=SENSOR_SIGMA_D, sigma_px=SENSOR_SIGMA_PX):
    """The reference's ``Simulator.simulate`` (geometry.py:42-72: pixel shuffle, 2 x 2 block downsample, optional
    distortion ``table`` fp32 [80, 80, 5] in the layout ``Simulator.__init__`` builds, disparity quantisation) on a clean
    depth image fp32 [H, W] in metres on the GPU -> uint16 millimetres (truncated, as
    generate_fusion_data_icl_nuim.py:142 stores them).  Counter-based randomness: the same (seed, frame) gives the same
    bits (include/bnv_fusion.h: bnv_depth_sensor)."""
    d = evaluate._on_gpu(depth, "depth", torch.float32)
    if d.dim() != 2 or d.numel() == 0:
        raise ValueError(f"depth: expected a non-empty [H, W] image, got {tuple(d.shape)}")
    tab = None
    if table is not None:
        tab = evaluate._on_gpu(table, "table", torch.float32)
        if tuple(tab.shape) != (80, 80, 5) or tab.device != d.device:
            raise ValueError(f"table: expected [80, 80, 5] on {d.device}, got {tuple(tab.shape)} on {tab.device}")
    seed, frame = int(seed), int(frame)
    if not (0 <= seed < 2 ** 64 and 0 <= frame < 2 ** 32):
        raise ValueError(f"seed {seed} / frame {frame} out of range")
    lib = _lib.load()
    with torch.cuda.device(d.device):
        out = torch.empty(d.shape, dtype=torch.uint16, device=d.device)
        _lib.check(lib.bnv_depth_sensor(_lib.ptr(d), int(d.shape[0]), int(d.shape[1]), _lib.ptr(tab), seed, frame,
                                        float(bf), float(sigma_d), float(sigma_px), _lib.ptr(out), _lib.stream_ptr()),
                   "bnv_depth_sensor")
    return out


def to_u16(depth, rounding="trunc"):
    """Depth in metres (device tensor) -> uint16 millimetres; "trunc" as the reference's ICL-NUIM script stores them,
    "nearest" (half to even) as ``sequence.depth_u16`` does.  Values outside (0, 65535] become 0."""
    if rounding not in ("trunc", "nearest"):
        raise ValueError(f"rounding {rounding!r}: 'trunc' or 'nearest'")
    mm = evaluate._on_gpu(depth, "depth", torch.float64) * 1000.0
    mm = torch.trunc(mm) if rounding == "trunc" else torch.round(mm)
    mm = torch.where((mm > 0) & (mm <= 65535), mm, torch.zeros_like(mm))
    return mm.to(torch.int32).to(torch.uint16)


def render_color(depth, K, T_wc, color="procedural"):
    """The colour image that goes with a clean depth image (fp32 [H, W] metres on the GPU, 0 = nothing): every pixel's
    hit point, back-projected in float64 -- x = (c - cx) / fx d, y = (r - cy) / fy d, z = d (integer pixel coordinates
    are pixel centres), then ((R0 x + R1 y) + R2 z) + t per world axis -- and coloured by ``color``: "procedural"
    (``synthetic.surface_color``) or a callable of world points float64 [H, W, 3] -> [H, W, 3] in [0, 255].  -> uint8
    [H, W, 3] (rounded half to even), 0 where nothing is hit.  Torch elementwise code: it makes a test asset."""
    from . import synthetic
    fn = synthetic.surface_color if isinstance(color, str) and color == "procedural" else color
    if not callable(fn):
        raise ValueError(f"color {color!r}: None, 'procedural' or a callable")
    d = evaluate._on_gpu(depth, "depth", torch.float64)
    H, W = int(d.shape[0]), int(d.shape[1])
    K, T = np.asarray(K, dtype=np.float64), np.asarray(T_wc, dtype=np.float64)
    c = torch.arange(W, dtype=torch.float64, device=d.device)[None, :]
    r = torch.arange(H, dtype=torch.float64, device=d.device)[:, None]
    x = (c - float(K[0, 2])) / float(K[0, 0]) * d
    y = (r - float(K[1, 2])) / float(K[1, 1]) * d
    world = torch.stack([((x * float(T[a, 0]) + y * float(T[a, 1])) + d * float(T[a, 2])) + float(T[a, 3])
                         for a in range(3)], dim=-1)
    rgb = torch.round(torch.as_tensor(fn(world), dtype=torch.float64, device=d.device)).clamp(0.0, 255.0)
    return torch.where((d > 0)[..., None], rgb, torch.zeros_like(rgb)).to(torch.uint8)


def scan_frames(scanner, poses, K, H, W, noise=None, seed=0, max_depth=math.inf, near=0.0, table=None,
                rounding="trunc", color=None):
    """The frame dicts ``NeuralMap`` takes (``sequence.sweep_frames``' keys: ``frame_id``, ``depth`` uint16 millimetres
    on the scanner's device, ``intr_mat``, ``T_wc``) of the mesh seen from ``poses`` ([n, 4, 4]).  noise None: the
    clean depth through ``to_u16(rounding=rounding)``; "kinect": ``simulate_sensor`` with ``seed`` and the frame's number.
    ``color``: None (the keys above only), or "procedural" / a callable -- every frame then also carries ``rgb`` uint8
    [H, W, 3] on the scanner's device (``render_color`` of the CLEAN depth)."""
    if noise not in (None, "kinect"):
        raise ValueError(f"noise {noise!r}: None or 'kinect'")
    if color is not None and not (callable(color) or (isinstance(color, str) and color == "procedural")):
        raise ValueError(f"color {color!r}: None, 'procedural' or a callable")
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    K = np.asarray(K, dtype=np.float64)
    for s in range(0, len(poses), MAX_POSES):
        depth, _ = scanner.render_depth(poses[s:s + MAX_POSES], K, H, W, near=near, max_depth=max_depth)
        for j in range(depth.shape[0]):
            i = s + j
            d = simulate_sensor(depth[j], seed, i, table=table) if noise == "kinect" else to_u16(depth[j], rounding)
            frame = {"frame_id": i, "depth": d, "intr_mat": K.copy(), "T_wc": poses[i].copy()}
            if color is not None:
                frame["rgb"] = render_color(depth[j], K, poses[i], color)
            yield frame


def scan_cloud(scanner, poses, K, H, W, max_depth=math.inf, near=0.0):
    """A multi-station point cloud of the mesh: the valid pixels of the clean depth images rendered from ``poses``
    ([n, 4, 4] camera-to-world), back-projected in float64 as ``render_color`` does and concatenated in pose order,
    row-major inside a view -> (points fp32 [N, 3] on the scanner's device, origins float64 [n, 3] -- the camera
    centres --, origin_index int32 [N] on the device: the view every point came from).  What
    ``pointcloud.estimate_normals`` / ``NeuralMap.integrate_cloud`` take.  Torch elementwise code: it makes a test and
    demo asset."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    K = np.asarray(K, dtype=np.float64)
    H, W = int(H), int(W)
    pts, idx = [], []
    dev = scanner.device
    c = torch.arange(W, dtype=torch.float64, device=dev)[None, :]
    r = torch.arange(H, dtype=torch.float64, device=dev)[:, None]
    for s in range(0, len(poses), MAX_POSES):
        depth, _ = scanner.render_depth(poses[s:s + MAX_POSES], K, H, W, near=near, max_depth=max_depth)
        for j in range(depth.shape[0]):
            d, T = depth[j].double(), poses[s + j]
            x = (c - float(K[0, 2])) / float(K[0, 0]) * d
            y = (r - float(K[1, 2])) / float(K[1, 1]) * d
            world = torch.stack([((x * float(T[a, 0]) + y * float(T[a, 1])) + d * float(T[a, 2])) + float(T[a, 3])
                                 for a in range(3)], dim=-1)
            keep = d > 0
            pts.append(world[keep].float())
            idx.append(torch.full((int(pts[-1].shape[0]),), s + j, dtype=torch.int32, device=dev))
    return torch.cat(pts).contiguous(), poses[:, :3, 3].copy(), torch.cat(idx).contiguous()


def drift_poses(poses, sigma_t, sigma_r, seed=0):
    """Odometry that drifts: every relative motion ``T_{i-1}^-1 T_i`` of ``poses`` ([n, 4, 4]) is followed by a small
    random motion exp((w, v)) in the camera's frame, w ~ N(0, sigma_r^2) radians and v ~ N(0, sigma_t^2) metres per
    axis, and the perturbed motions are chained from the first pose, which stays exact: a random walk, as a phone's
    odometry drifts.  ``numpy.random.Generator(PCG64(seed))``: the same seed gives the same poses -> float64
    [n, 4, 4]."""
    from .tracking import rigid_inverse, se3_exp
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    out = [poses[0].copy()]
    for i in range(1, len(poses)):
        noise = rng.standard_normal(6) * np.array([sigma_r] * 3 + [sigma_t] * 3, dtype=np.float64)
        out.append(out[-1] @ (rigid_inverse(poses[i - 1]) @ poses[i]) @ se3_exp(noise))
    return np.stack(out)


def look_at_pose(eye, target, down=(0.0, 1.0, 0.0)):
    """Camera-to-world pose at ``eye`` looking at ``target``: +z forward, +y along ``down`` as far as the view allows."""
    eye, target, down = (np.asarray(a, dtype=np.float64) for a in (eye, target, down))
    z = target - eye
    if not np.linalg.norm(z) > 0:
        raise ValueError("look_at_pose: eye and target coincide")
    z = z / np.linalg.norm(z)
    x = np.cross(down, z)
    if np.linalg.norm(x) < 1e-9:                      # looking straight along `down`
        x = np.cross(np.roll(down, 1), z)
    x = x / np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def orbit_poses(center, radius, n, height=0.0, look_at=None):
    """``n`` poses on a circle of ``radius`` around ``center`` in the x-z plane, ``height`` above it (y is down: the
    eye's y is center.y - height), looking at ``look_at`` (default: ``center``) -> float64 [n, 4, 4]."""
    center = np.asarray(center, dtype=np.float64)
    target = center if look_at is None else np.asarray(look_at, dtype=np.float64)
    out = []
    for k in range(int(n)):
        a = 2.0 * math.pi * k / int(n)
        eye = center + np.array([radius * math.sin(a), -float(height), -radius * math.cos(a)])
        out.append(look_at_pose(eye, target))
    return np.stack(out)


def _quat(R):
    w = math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    x = math.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2.0
    y = math.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2.0
    z = math.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2.0
    return np.array([w, math.copysign(x, R[2, 1] - R[1, 2]), math.copysign(y, R[0, 2] - R[2, 0]),
                     math.copysign(z, R[1, 0] - R[0, 1])])


def _rot(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def interpolate_poses(key_poses, n):
    """``n`` poses along the key poses ([k, 4, 4], k >= 2), evenly spaced in key index: rotations by quaternion slerp,
    positions by linear interpolation (the job of the reference's geometry.pose_spline) -> float64 [n, 4, 4]."""
    keys = np.asarray(key_poses, dtype=np.float64).reshape(-1, 4, 4)
    if len(keys) < 2 or int(n) < 1:
        raise ValueError("interpolate_poses: at least two key poses and one output pose")
    quats = [_quat(T[:3, :3]) for T in keys]
    out = []
    for s in (np.linspace(0.0, len(keys) - 1, int(n)) if int(n) > 1 else np.array([0.0])):
        i = min(int(math.floor(s)), len(keys) - 2)
        a = s - i
        q0, q1 = quats[i], quats[i + 1]
        dot = float(np.dot(q0, q1))
        if dot < 0:
            q1, dot = -q1, -dot
        if dot > 1 - 1e-9:
            q = (1 - a) * q0 + a * q1
        else:
            th = math.acos(dot)
            q = (math.sin((1 - a) * th) * q0 + math.sin(a * th) * q1) / math.sin(th)
        T = np.eye(4)
        T[:3, :3] = _rot(q)
        T[:3, 3] = (1 - a) * keys[i][:3, 3] + a * keys[i + 1][:3, 3]
        out.append(T)
    return np.stack(out)


def write_scan(data_dir, scan_id, scanner, poses, K, H, W, noise=None, seed=0, max_depth=math.inf, table=None,
               rounding="trunc"):
    """Scans the mesh from ``poses`` and writes the sequence in the reference's layout (``datasets.write_sequence``),
    recentred as the reference's scripts do (generate_fusion_data_icl_nuim.py:55-60: the mesh's box centre goes to the
    origin, every pose with it), plus ``gt_mesh.ply`` (the whole mesh), ``gt_mesh_visible.ply`` (the faces these
    frames saw) and ``pose/dimensions.txt`` (the mesh's box).  -> the sequence's directory."""
    from . import datasets
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    v = scanner.vertices.cpu().numpy().astype(np.float64)
    v = v[np.isfinite(v).all(1)]
    lo, hi = v.min(0), v.max(0)
    center, dimensions = (lo + hi) / 2.0, hi - lo
    shifted = poses.copy()
    shifted[:, :3, 3] -= center
    scanner.reset_seen()
    frames = scan_frames(scanner, poses, K, H, W, noise=noise, seed=seed, max_depth=max_depth, table=table,
                         rounding=rounding)
    root = datasets.write_sequence(data_dir, scan_id, (f["depth"].cpu().numpy() for f in frames), np.asarray(K),
                                   shifted, dimensions)

    def recentred(m):
        return TriMesh((m.vertices.astype(np.float64) - center).astype(np.float32), m.faces)

    recentred(TriMesh(scanner.vertices.cpu().numpy(), scanner.faces.cpu().numpy())).export(os.path.join(root, "gt_mesh.ply"))
    recentred(scanner.visible_mesh()).export(os.path.join(root, "gt_mesh_visible.ply"))
    return root
