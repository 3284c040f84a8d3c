"""Point clouds without a pixel grid -- a terrestrial or mobile LiDAR scan, the cloud another SLAM system exported, a
PLY of points -- as frames of the map.  The encoder takes ``input_pts [1, N, 6]``, world points plus world normals;
the depth front end gets its normals from a Sobel stencil over the image, which a cloud does not have.
``estimate_normals`` gets them from the k nearest neighbours of every point (csrc/cloud.hip; include/bnv_fusion.h,
"Point-cloud normals": an exact k-NN self-join on the index of ``evaluate.nearest_neighbors``, a float64 plane fit, the
sign from a known sensor position), and ``NeuralMap.integrate_cloud`` fuses the result like any other frame.  GPU only:
a CPU tensor is refused, there is no CPU fallback.  Normals are oriented from sensor positions only: a cloud whose
sensor positions are unknown cannot be oriented here.

    pts, normals = load_cloud("scan.ply")
    nm.integrate_cloud(torch.from_numpy(pts).cuda(), origins=[[0.0, 0.0, 0.0]])
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

MIN_K, MAX_K = 8, 32        # BNV_CLOUD_MIN_K, BNV_CLOUD_MAX_K
# The encoder takes at most 2^27 points in one frame (csrc/encode.hip: bnv_encode_begin refuses n_points > 1 << 27).
# Its workspace and pair buffers grow with the frame (8 (point, voxel) pairs per point), so a cloud goes in in chunks
# of a depth frame's order of size instead: 2^20 points, a little over three 640 x 480 frames.
ENCODER_MAX_POINTS = 1 << 27
CLOUD_CHUNK_POINTS = 1 << 20


def _points(points, what="points"):
    if not isinstance(points, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor on the GPU, got {type(points).__name__}")
    if not points.is_cuda:
        raise ValueError(f"{what}: a CPU tensor; point-cloud normals run on the GPU only (no CPU fallback)")
    p = points.detach()
    if p.dim() == 3 and p.shape[0] == 1:
        p = p[0]
    if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] == 0:
        raise ValueError(f"{what}: expected a non-empty [N, 3] tensor, got {tuple(points.shape)}")
    if p.shape[0] > 2 ** 31 - 3:
        raise ValueError(f"{what}: {p.shape[0]} points; at most 2^31 - 3")
    return p.to(torch.float32).contiguous()


def _origins(origins, dev):
    if isinstance(origins, torch.Tensor):
        o = origins.detach().to(device=dev, dtype=torch.float32)
    else:
        o = torch.from_numpy(np.ascontiguousarray(np.asarray(origins, dtype=np.float32))).to(dev)
    o = o.reshape(-1, 3) if o.numel() % 3 == 0 and o.dim() <= 2 else o
    if o.dim() != 2 or o.shape[1] != 3 or o.shape[0] == 0:
        raise ValueError(f"origins: expected [M, 3] (or one [3]) sensor positions, got {tuple(o.shape)}")
    return o.contiguous()


def estimate_normals(points, origins, origin_index=None, k=16, max_radius=None, min_neighbors=6, return_stats=False):
    """``points`` fp32 [N, 3] on the GPU -> ``input_pts`` fp32 [1, N, 6] on the same device, in the input's row order:
    the points and the normal of the plane through each point's ``k`` nearest neighbours (itself included; 8 <= k <=
    32), turned away from the sensor that saw it -- ``origins`` [M, 3] sensor positions (tensor or array) and
    ``origin_index`` int [N] into them (None: every point was seen from ``origins[0]``).  ``max_radius``: neighbours
    farther than this do not count (None: no limit).  A row is six NaNs, which the encoder drops, when fewer than
    ``min_neighbors`` (>= 3) neighbours were found, when they are not a plane (coincident or collinear), when its origin
    index is out of range, or when the point itself is not finite.

    ``return_stats=True``: -> (input_pts, {"variation": fp32 [N] surface variation lambda_0 / (lambda_0 + lambda_1 +
    lambda_2), "n_neighbors": int32 [N], "status": int32 [4] on the device -- [0] rejected rows, [1] bad origin
    indices}).  Nothing is read back: the call does not synchronise.  Arguments are checked on the host before any
    launch."""
    p = _points(points)
    dev = p.device
    n = int(p.shape[0])
    k, min_neighbors = int(k), int(min_neighbors)
    if not MIN_K <= k <= MAX_K:
        raise ValueError(f"k = {k}: {MIN_K} to {MAX_K}")
    if not 3 <= min_neighbors <= k:
        raise ValueError(f"min_neighbors = {min_neighbors}: 3 to k = {k}")
    radius = 0.0
    if max_radius is not None:
        radius = float(np.float32(max_radius))
        if not (np.isfinite(radius) and radius > 0.0):
            raise ValueError(f"max_radius = {max_radius!r}: a positive finite float32 distance, or None")
    o = _origins(origins, dev)
    oi = None
    if origin_index is not None:
        oi = torch.as_tensor(origin_index)
        if oi.dtype.is_floating_point or oi.dtype == torch.bool or oi.numel() != n:
            raise ValueError(f"origin_index: expected {n} integers, got {tuple(oi.shape)} {oi.dtype}")
        oi = oi.detach().to(device=dev, dtype=torch.int32).reshape(n).contiguous()
    lib = _lib.require_device(dev.index or 0)
    need = C.c_int64()
    _lib.check(lib.bnv_cloud_normals_bytes(n, C.byref(need)), "bnv_cloud_normals_bytes")
    with torch.cuda.device(dev):
        ws = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
        out = torch.empty((n, 6), dtype=torch.float32, device=dev)
        var = torch.empty(n, dtype=torch.float32, device=dev) if return_stats else None
        cnt = torch.empty(n, dtype=torch.int32, device=dev) if return_stats else None
        status = torch.empty(4, dtype=torch.int32, device=dev)
        _lib.check(lib.bnv_cloud_normals(_lib.ptr(p), n, k, radius, min_neighbors, _lib.ptr(o), int(o.shape[0]),
                                         _lib.ptr(oi), _lib.ptr(ws), int(need.value), _lib.ptr(out), _lib.ptr(var),
                                         _lib.ptr(cnt), _lib.ptr(status), _lib.stream_ptr()), "bnv_cloud_normals")
    out = out.unsqueeze(0)
    return (out, {"variation": var, "n_neighbors": cnt, "status": status}) if return_stats else out


class CloudIndex:
    """A point cloud with normals as a registration target and nearest-neighbour reference, indexed once on the GPU
    (csrc/cloud_register.hip; include/bnv_fusion.h, "Cloud registration": bnv_cloud_index_build): the index of
    ``evaluate.nearest_neighbors`` over the positions, kept, next to the unit normals.  ``points`` fp32 [N, 3] with
    ``normals`` fp32 [N, 3], or ``input_pts`` fp32 [N, 6] / [1, N, 6] (what ``estimate_normals`` returns), on the GPU.
    Without normals they are estimated (``estimate_normals`` with ``k``); a target's normals need no orientation, so
    ``origins`` defaults to the cloud's first point.  A row with a non-finite component or a normal shorter than 1e-12
    is in the index but never anyone's neighbour.  Building reads nothing back.

        d2, idx = CloudIndex(scan_a).nearest(scan_b)
        res = register.register_cloud(scan_b, CloudIndex(scan_a), T_guess=T0)
    """

    def __init__(self, points=None, normals=None, *, input_pts=None, k=16, origins=None):
        if input_pts is not None:
            if points is not None or normals is not None:
                raise ValueError("CloudIndex: input_pts carries positions and normals; give it alone")
            rows = _rows6(input_pts, "input_pts")
        else:
            if points is None:
                raise ValueError("CloudIndex: points, or input_pts")
            p = _points(points)
            if normals is None:
                rows = estimate_normals(p, p[:1] if origins is None else origins, k=k)[0]
            else:
                nrm = _points(normals, "normals")
                if nrm.shape != p.shape or nrm.device != p.device:
                    raise ValueError(f"normals: expected {tuple(p.shape)} on {p.device}, got {tuple(nrm.shape)} on "
                                     f"{nrm.device}")
                rows = torch.cat([p, nrm], 1).contiguous()
        self.device = rows.device
        self.n = int(rows.shape[0])
        lib = _lib.require_device(self.device.index or 0)
        need = C.c_int64()
        _lib.check(lib.bnv_cloud_index_bytes(self.n, C.byref(need)), "bnv_cloud_index_bytes")
        self._ws_bytes = int(need.value)
        with torch.cuda.device(self.device):
            self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=self.device)
            _lib.check(lib.bnv_cloud_index_build(_lib.ptr(rows), self.n, _lib.ptr(self._ws), self._ws_bytes,
                                                 _lib.stream_ptr()), "bnv_cloud_index_build")

    def nearest(self, query):
        """``query`` fp32 [M, 3] on the index's device -> (d2 fp32 [M], idx int32 [M]): ``evaluate.nn_d2(query,
        points)`` bit for bit over the rows the index kept, without building the index again."""
        q = _points(query, "query")
        if q.device != self.device:
            raise ValueError(f"query on {q.device}, index on {self.device}")
        m = int(q.shape[0])
        lib = _lib.load()
        with torch.cuda.device(self.device):
            d2 = torch.empty(m, dtype=torch.float32, device=self.device)
            idx = torch.empty(m, dtype=torch.int32, device=self.device)
            _lib.check(lib.bnv_cloud_index_nearest(_lib.ptr(self._ws), self._ws_bytes, _lib.ptr(q), m, _lib.ptr(d2),
                                                   _lib.ptr(idx), _lib.stream_ptr()), "bnv_cloud_index_nearest")
        return d2, idx


def _rows6(input_pts, what):
    if not isinstance(input_pts, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor on the GPU, got {type(input_pts).__name__}")
    if not input_pts.is_cuda:
        raise ValueError(f"{what}: a CPU tensor; cloud registration runs on the GPU only (no CPU fallback)")
    r = input_pts.detach()
    if r.dim() == 3 and r.shape[0] == 1:
        r = r[0]
    if r.dim() != 2 or r.shape[1] != 6 or r.shape[0] == 0 or r.shape[0] > 2 ** 31 - 3:
        raise ValueError(f"{what}: expected a non-empty [N, 6] tensor of at most 2^31 - 3 rows, got "
                         f"{tuple(input_pts.shape)}")
    return r.to(torch.float32).contiguous()


def align_scans(scans, T_guess, origins=None, **kw):
    """Aligns the stations of a multi-station scan to each other before fusion, one after the other: ``scans`` a list
    of fp32 [N_i, 3] device tensors, each in its own station's frame, ``T_guess`` [n, 4, 4] the rough station poses
    (station -> common frame).  Scan 0 keeps its pose; scan i is registered (``register.register_cloud``, whose
    keywords ``kw`` are) to a ``CloudIndex`` over the union of the scans 0 .. i - 1 at their aligned poses ->
    (poses float64 [n, 4, 4], statuses [n]).  A refused scan keeps its guess (and still joins the union there).
    ``origins`` [n, 3]: sensor positions in the stations' own frames for the targets' normals (default: none needed).
    Sequential: an error made early is not revisited (no pose graph)."""
    from . import register
    T_guess = np.asarray(T_guess, dtype=np.float64).reshape(-1, 4, 4)
    if len(scans) == 0 or len(T_guess) != len(scans):
        raise ValueError(f"align_scans: {len(scans)} scans, {len(T_guess)} poses")
    clouds = [_points(s, f"scans[{i}]") for i, s in enumerate(scans)]
    poses, statuses = T_guess.copy(), [register.OK]
    placed = [register.transform_points(poses[0], clouds[0])]
    org = None if origins is None else np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    for i in range(1, len(clouds)):
        world_origin = None
        if org is not None:                                # one origin serves: the sign of a target normal is irrelevant
            world_origin = (poses[0, :3, :3] @ org[0] + poses[0, :3, 3])[None]
        target = CloudIndex(torch.cat(placed), origins=world_origin)
        res = register.register_cloud(clouds[i], target, T_guess=poses[i], **kw)
        statuses.append(res.status)
        if res.status == register.OK:
            poses[i] = res.T
        placed.append(register.transform_points(poses[i], clouds[i]))
    return poses, statuses


def load_cloud(path):
    """The vertices of a PLY file (``mesh.load_ply``: ASCII or binary little-endian; faces, if any, are ignored) ->
    (points float32 [N, 3], normals float32 [N, 3] or None).  With normals in the file (``nx ny nz``) no estimation is
    needed: ``input_pts`` is the two side by side, ``np.concatenate([points, normals], 1)[None]``."""
    from .mesh import load_ply
    m = load_ply(path)
    normals = None if m.vertex_normals is None else np.ascontiguousarray(m.vertex_normals, dtype=np.float32)
    return np.ascontiguousarray(m.vertices, dtype=np.float32), normals


def cloud_chunks(n, chunk=CLOUD_CHUNK_POINTS):
    """Index ranges [(start, stop)] of a cloud of ``n`` points cut in index order into frames of at most ``chunk``."""
    chunk = int(chunk)
    if not 0 < chunk <= ENCODER_MAX_POINTS:
        raise ValueError(f"chunk = {chunk}: 1 to {ENCODER_MAX_POINTS} (the encoder's limit for one frame)")
    return [(s, min(s + chunk, int(n))) for s in range(0, int(n), chunk)]


def integrate_cloud(nm, points, origins, origin_index=None, chunk=CLOUD_CHUNK_POINTS, **kw):
    """``NeuralMap.integrate_cloud``: see there."""
    p = _points(points)
    pts = estimate_normals(p, origins, origin_index, **kw)        # over the whole cloud: chunks share neighbours
    touched = [nm.integrate({"input_pts": pts[:, s:e]}) for s, e in cloud_chunks(p.shape[0], chunk)]
    touched = [t for t in touched if t is not None]
    if not touched:
        return None
    return touched[0] if len(touched) == 1 else torch.unique(torch.cat(touched), dim=0)
