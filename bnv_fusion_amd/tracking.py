"""Frame-to-model tracking on the GPU: correct a camera pose against the map before the frame is fused.

``icp_align`` is projective point-to-plane ICP of a depth frame against a rendered view of the map (z-depth + world
normals, as ``NeuralMap.render``, ``NeuralMap.render_tsdf`` and ``MeshScanner.render_depth`` make them):
csrc/track.hip behind bnv_icp_align (include/bnv_fusion.h, "Tracking").  All iterations run on the device without a
host read in between; the host reads the result once.  ``Tracker`` is the tracked fusion loop: the poses a data set
gives serve as odometry (or, with ``odometry="rgbd"``, the frame-to-frame motion ``odometry.RgbdOdometry`` estimates
from the frames themselves), every frame is aligned to the map built so far and fused with the corrected pose.  GPU
only.

    tracker = Tracker(neural_map, source="tsdf", model_size=(120, 160))
    for frame in frames:                       # frame["T_wc"]: drifting odometry
        tracker.integrate(frame)
    evaluate.trajectory_errors(tracker.poses, ground_truth)
"""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

OK, LOST, DEGENERATE, JUMP = 0, 1, 2, 3                  # BNV_ICP_*
STATUS_NAMES = {OK: "ok", LOST: "lost", DEGENERATE: "degenerate", JUMP: "jump"}
DEFAULT_LEVELS = ((4, 4), (2, 5), (1, 10))               # (stride, iterations), coarse to fine
ICP_BLOCKS, ICP_SUMS, ICP_RECORD = 256, 29, 36           # BNV_ICP_BLOCKS, BNV_ICP_SUMS, BNV_ICP_RECORD_DOUBLES

TrackResult = collections.namedtuple("TrackResult", "T_wc status stats poses records", defaults=(None,))
TrackResult.__doc__ = """T_wc float64 [4, 4]: the aligned camera-to-world pose, or the guess bit for bit when ``status``
is not ``OK``; stats float64 [n_iter, 5] = pairs, rmse, |w|, |v|, spread per iteration; poses float64 [n_iter + 1, 4, 4]:
the estimate before every iteration and the final one; records: float64 [n_iter, 36] (29 sums, xi, pad) on request."""


def se3_exp(xi):
    """exp of the twist ``xi`` = (w, v) -> float64 [4, 4]: Rodrigues' formula, the series below |w| < 1e-8 (the solve
    kernel's form)."""
    xi = np.asarray(xi, dtype=np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    th2 = float(w @ w)
    th = math.sqrt(th2)
    if th < 1e-8:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        a, b, c = math.sin(th) / th, (1.0 - math.cos(th)) / th2, (th - math.sin(th)) / (th2 * th)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    T[:3, 3] = (np.eye(3) + b * K + c * (K @ K)) @ v
    return T


def rigid_inverse(T):
    """[R | t] -> [R^T | -R^T t], float64 [4, 4]."""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def scaled_intrinsics(K, sx, sy=None):
    """Intrinsics of the image downscaled by ``sx`` (``sy``: rows; default the same): pixel centres at integers, so
    fx / s and cx' = (cx + 0.5) / s - 0.5."""
    sy = sx if sy is None else sy
    K = np.array(np.asarray(K, dtype=np.float64)[:3, :3])
    K[0, 0], K[0, 2] = K[0, 0] / sx, (K[0, 2] + 0.5) / sx - 0.5
    K[1, 1], K[1, 2] = K[1, 1] / sy, (K[1, 2] + 0.5) / sy - 0.5
    return K


def _f64(m, n):
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(-1))
    if a.size != n:
        raise ValueError(f"expected {n} matrix entries, got {a.size}")
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def frame_depth_tensor(depth, device):
    """A frame's depth as the kernel reads it: uint16 millimetres or float32 metres, [H, W] on ``device``."""
    d = torch.from_numpy(np.ascontiguousarray(depth)) if isinstance(depth, np.ndarray) else depth
    if d.dtype not in (torch.uint16, torch.float32):
        d = d.to(torch.float32)
    d = d.to(device).contiguous()
    if d.dim() == 3 and d.shape[0] == 1:
        d = d[0]
    if d.dim() != 2 or d.numel() == 0:
        raise ValueError(f"depth: expected a non-empty [H, W] image, got {tuple(d.shape)}")
    return d


def icp_align(depth, K, model_depth, model_normals, model_K, model_T_wc, T_guess, levels=DEFAULT_LEVELS, dist=0.1,
              max_depth=3.0, min_pair_share=0.05, min_spread=1e-3, records=False):
    """Aligns the frame ``depth`` ([H, W] uint16 millimetres or float32 metres, intrinsics ``K``) to the model view
    ``model_depth`` f32 [H_m, W_m] / ``model_normals`` f32 [H_m, W_m, 3] (device tensors, intrinsics ``model_K``,
    camera-to-world ``model_T_wc``) starting from the camera-to-world ``T_guess`` -> ``TrackResult``.  ``levels``:
    (stride, iterations) coarse to fine; ``dist``: the pairing gate in metres; a frame that keeps fewer than
    ``min_pair_share`` of its sampled pixels is ``LOST``, one whose normals spread less than ``min_spread``
    ``DEGENERATE``, a step beyond 0.1 rad / 0.2 m a ``JUMP``: the result is then the guess.  One host read, at the
    end."""
    md = model_depth
    if not (isinstance(md, torch.Tensor) and md.is_cuda and isinstance(model_normals, torch.Tensor)):
        raise ValueError("icp_align: the model view must be device tensors (the renderers' outputs); no CPU fallback")
    dev = md.device
    md = md.detach().to(torch.float32).contiguous()
    mn = model_normals.detach().to(device=dev, dtype=torch.float32).contiguous()
    if md.dim() != 2 or tuple(mn.shape) != tuple(md.shape) + (3,):
        raise ValueError(f"icp_align: model depth {tuple(md.shape)} / normals {tuple(mn.shape)}")
    d = frame_depth_tensor(depth, dev)
    lv = np.ascontiguousarray(np.asarray(levels, dtype=np.int32).reshape(-1, 2))
    lv_p = lv.ctypes.data_as(C.POINTER(C.c_int32))
    lib = _lib.load()
    need = int(lib.bnv_icp_workspace_bytes(len(lv), lv_p))
    if need == 0:
        raise _lib.BnvError(f"icp_align: invalid schedule {levels!r}")
    n_iter = int(lv[:, 1].sum())
    Kh, Kp = _f64(np.asarray(K, dtype=np.float64)[:3, :3], 9)
    Kmh, Kmp = _f64(np.asarray(model_K, dtype=np.float64)[:3, :3], 9)
    Tmh, Tmp = _f64(model_T_wc, 16)
    Tih, Tip = _f64(rigid_inverse(model_T_wc) if np.isfinite(Tmh).all() else Tmh, 16)
    T0h, T0p = _f64(T_guess, 16)
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(1 + 16 + (n_iter + 1) * 16 + n_iter * 5, dtype=torch.float64, device=dev)
        status, pose = out[:1].view(torch.int32), out[1:17]
        poses, stats = out[17:17 + (n_iter + 1) * 16], out[17 + (n_iter + 1) * 16:]
        _lib.check(lib.bnv_icp_align(_lib.ptr(d), 0 if d.dtype == torch.uint16 else 1, int(d.shape[0]),
                                     int(d.shape[1]), Kp, float(max_depth), _lib.ptr(md), _lib.ptr(mn),
                                     int(md.shape[0]), int(md.shape[1]), Kmp, Tmp, Tip, T0p, len(lv), lv_p,
                                     float(dist), float(min_pair_share), float(min_spread), _lib.ptr(ws), need,
                                     _lib.ptr(pose), _lib.ptr(poses), _lib.ptr(stats), _lib.ptr(status),
                                     _lib.stream_ptr()), "bnv_icp_align")
        host = out.cpu()                                   # the one host read
        rec = None
        if records:
            rec = ws.view(torch.float64)[ICP_BLOCKS * ICP_SUMS:].reshape(n_iter, ICP_RECORD).cpu().numpy()
    host_np = host.numpy()
    return TrackResult(host_np[1:17].reshape(4, 4).copy(), int(host[:1].view(torch.int32)[0]),
                       host_np[17 + (n_iter + 1) * 16:].reshape(n_iter, 5).copy(),
                       host_np[17:17 + (n_iter + 1) * 16].reshape(n_iter + 1, 4, 4).copy(), rec)


def track_against(render, frame, T_guess=None, model_size=None, max_depth=3.0, **icp):
    """Renders a model view with ``render(T_wc, K, H, W) -> (depth, normals)`` at the guess and aligns ``frame`` to it
    -> ``TrackResult``.  ``model_size`` (H_m, W_m): the view's size, default the frame's; a smaller view is rendered
    with ``scaled_intrinsics``.  The renderers take float32 poses and intrinsics: the view's own pose and intrinsics
    go to the aligner as the renderer saw them."""
    K = np.asarray(frame["intr_mat"], dtype=np.float64)[:3, :3]
    T0 = np.asarray(frame["T_wc"] if T_guess is None else T_guess, dtype=np.float64).reshape(4, 4)
    H, W = (int(s) for s in frame["depth"].shape[-2:])
    Hm, Wm = (H, W) if model_size is None else (int(model_size[0]), int(model_size[1]))
    Km = scaled_intrinsics(K, W / Wm, H / Hm).astype(np.float32).astype(np.float64)
    Tm = T0.astype(np.float32).astype(np.float64)
    depth, normals = render(Tm, Km, Hm, Wm)
    return icp_align(frame["depth"], K, depth, normals, Km, Tm, T0, max_depth=max_depth, **icp)


class Tracker:
    """The tracked fusion loop over a ``NeuralMap``: ``integrate(frame)`` predicts the frame's pose from the last
    corrected one and the motion between the given poses (``T_pred = T_prev_tracked T_prev_given^-1 T_cur_given``: the
    given poses serve as odometry), renders the map there (``source``: "neural" or "tsdf"; ``model_size``: the view's
    (H, W), default the frame's), aligns the frame and fuses it with the corrected pose.  A frame the aligner refuses
    is fused with ``T_pred`` and counted in ``failures`` (``statuses`` has every frame's code, -1 for the first
    ``warmup`` frames, which are fused with their given pose).  ``poses``: the pose every frame was fused with.
    ``odometry``: None (the given poses, as above), "rgbd" or an ``odometry.RgbdOdometry``: the motion between
    consecutive frames is then estimated from the frames themselves, ``T_pred = T_prev_tracked inv(T_rel)``, and only
    the first frame's ``T_wc`` is read (identity when it has none); a pair the odometry refuses contributes its
    constant-velocity guess (``odometry.failures``).  The map's depth filter runs once, before odometry and tracking."""

    def __init__(self, nm, source="neural", model_size=None, warmup=1, odometry=None, **icp):
        if source not in ("neural", "tsdf"):
            raise ValueError(f"source {source!r}: 'neural' or 'tsdf'")
        if isinstance(odometry, str):
            if odometry != "rgbd":
                raise ValueError(f"odometry {odometry!r}: None, 'rgbd' or an RgbdOdometry")
            from .odometry import RgbdOdometry
            odometry = RgbdOdometry(max_depth=icp.get("max_depth", nm.max_depth))
        self.odometry = odometry
        self.nm, self.source, self.model_size, self.warmup, self.icp = nm, source, model_size, int(warmup), icp
        self.poses, self.statuses, self.failures = [], [], 0
        self.last = None
        self._prev_given = self._prev_tracked = None

    def integrate(self, frame):
        frame = self.nm.prepare_frame(frame)      # the map's depth filter, once: tracking and fusion read one image
        if self.odometry is not None:
            return self._integrate_from_odometry(frame)
        given = np.asarray(frame["T_wc"], dtype=np.float64).reshape(4, 4)
        if len(self.poses) < self.warmup or self._prev_given is None:
            T, status = given, -1
        else:
            T_pred = self._prev_tracked @ rigid_inverse(self._prev_given) @ given
            self.last = self.nm.track(frame, T_guess=T_pred, source=self.source, model_size=self.model_size, **self.icp)
            status = self.last.status
            T = self.last.T_wc if status == OK else T_pred
            self.failures += status != OK
        self._prev_given, self._prev_tracked = given, T
        self.poses.append(T)
        self.statuses.append(status)
        fused = dict(frame)
        fused["T_wc"] = T
        return self.nm.integrate(fused)

    def _integrate_from_odometry(self, frame):
        """``integrate`` when the motion comes from ``self.odometry``: ``frame`` is prepared already."""
        step = self.odometry.step(frame)
        if self._prev_tracked is None:
            T = np.eye(4) if frame.get("T_wc") is None else np.array(frame["T_wc"], dtype=np.float64).reshape(4, 4)
            status = -1
        else:
            T_pred = self._prev_tracked @ rigid_inverse(step.T_wc)
            T, status = T_pred, -1
            if len(self.poses) >= self.warmup:
                self.last = self.nm.track(frame, T_guess=T_pred, source=self.source, model_size=self.model_size,
                                          **self.icp)
                status = self.last.status
                T = self.last.T_wc if status == OK else T_pred
                self.failures += status != OK
        self._prev_tracked = T
        self.poses.append(T)
        self.statuses.append(status)
        fused = dict(frame)
        fused["T_wc"] = T
        return self.nm.integrate(fused)
