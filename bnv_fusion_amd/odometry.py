"""Frame-to-frame RGB-D odometry on the GPU: the camera's motion between two consecutive frames from a joint
photometric and depth alignment (csrc/odometry.hip behind bnv_rgbd_prepare / bnv_rgbd_align; include/bnv_fusion.h,
"Odometry").  It gives the tracker a motion estimate where a stream has no poses, and the colour image constrains the
motion along a flat wall, where point-to-plane ICP is degenerate.  GPU only.

    odo = RgbdOdometry()
    T = first_pose
    for frame in frames:                       # frame["depth"], frame["intr_mat"], optionally frame["rgb"]
        step = odo.step(frame)                 # step.T_wc: current <- previous camera
        T = T @ tracking.rigid_inverse(step.T_wc)

A frame is prepared once (``prepare_frame``: intensity, depth pyramid and gradients in one device buffer) and used in
two alignments.  All iterations of ``rgbd_align`` run on the device without a host read in between.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from .tracking import (DEGENERATE, ICP_BLOCKS, ICP_RECORD, ICP_SUMS, JUMP, LOST, OK, TrackResult, _f64,  # noqa: F401
                       frame_depth_tensor, scaled_intrinsics)

DEFAULT_SCHEDULE = ((2, 6), (1, 6), (0, 8))              # (pyramid level, iterations), coarse to fine
PLANES = ("D", "I", "Ix", "Iy", "Dx", "Dy", "valid")     # the slots of a pixel record (the eighth is a pad)

PreparedFrame = collections.namedtuple("PreparedFrame", "buffer H W levels K has_rgb max_depth depth_jump")
PreparedFrame.__doc__ = """A frame as ``rgbd_align`` reads it: ``buffer`` uint8 on the device (level l: float32
[H >> l, W >> l, 8] records = D, I, Ix, Iy, Dx, Dy, valid, 0, each level on a 256-byte boundary), the depth image's
size, the number of levels, its float64 intrinsics, whether it had a colour image, and the ``max_depth`` and
``depth_jump`` it was prepared with."""


def level_view(prepared, level):
    """Level ``level`` of a prepared frame as a float32 [H_l, W_l, 8] view of its buffer (no copy)."""
    if not 0 <= level < prepared.levels:
        raise ValueError(f"level {level}: 0 .. {prepared.levels - 1}")
    off = 0
    for l in range(level):
        off += ((prepared.H >> l) * (prepared.W >> l) * 32 + 255) // 256 * 256
    h, w = prepared.H >> level, prepared.W >> level
    return prepared.buffer[off:off + h * w * 32].view(torch.float32).reshape(h, w, 8)


def prepare_frame(frame, levels=3, max_depth=3.0, depth_jump=0.05, device=None):
    """``frame``: a frame dict (``depth`` [H, W] uint16 millimetres or float32 metres, ``intr_mat``, optionally ``rgb``
    uint8 [Hc, Wc, 3] and, for a colour image of its own size or intrinsics, ``rgb_intr_mat``; a colour image of
    another size without intrinsics is taken to show the same view) -> ``PreparedFrame`` with ``levels`` pyramid
    levels.  Depth beyond ``max_depth`` is invalid; ``depth_jump`` (metres) is the depth step between neighbouring
    pixels of level 0 that the pyramid, the gradients and the pairs treat as an edge; level l, whose pixels are 2**l as
    wide, uses 2**l times as much (with one jump for all levels an oblique wall keeps no gradient two levels up: a
    61 x 83 frame of the synthetic room has none at level 2).  A frame without ``rgb`` gets zero intensity: align it with ``lambda_depth=1``."""
    depth = frame["depth"]
    if device is None:
        device = depth.device if isinstance(depth, torch.Tensor) and depth.is_cuda else "cuda:0"
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("prepare_frame: GPU only; no CPU fallback")
    d = frame_depth_tensor(depth, dev)
    H, W = int(d.shape[0]), int(d.shape[1])
    K = np.array(np.asarray(frame["intr_mat"], dtype=np.float64)[:3, :3])
    Kh, Kp = _f64(K, 9)
    rgb, Hc, Wc, Kcp = None, 0, 0, None
    if frame.get("rgb") is not None:
        rgb = frame["rgb"]
        rgb = torch.from_numpy(np.ascontiguousarray(rgb)) if isinstance(rgb, np.ndarray) else rgb
        if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3 or rgb.numel() == 0:
            raise ValueError(f"prepare_frame: rgb must be uint8 [H, W, 3] (got {rgb.dtype} {list(rgb.shape)})")
        rgb = rgb.to(dev).contiguous()
        Hc, Wc = int(rgb.shape[0]), int(rgb.shape[1])
        if frame.get("rgb_intr_mat") is not None:
            Kc = np.asarray(frame["rgb_intr_mat"], dtype=np.float64)[:3, :3]
        else:
            Kc = K if (Hc, Wc) == (H, W) else scaled_intrinsics(K, W / Wc, H / Hc)
        Kch, Kcp = _f64(Kc, 9)
    lib = _lib.load()
    need = int(lib.bnv_rgbd_frame_bytes(H, W, int(levels)))
    if need == 0:
        raise _lib.BnvError(f"prepare_frame: no {levels}-level pyramid of a {H} x {W} image")
    with torch.cuda.device(dev):
        buf = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.check(lib.bnv_rgbd_prepare(_lib.ptr(d), 0 if d.dtype == torch.uint16 else 1, H, W, Kp, _lib.ptr(rgb), Hc,
                                        Wc, Kcp, int(levels), float(max_depth), float(depth_jump), _lib.ptr(buf),
                                        need, _lib.stream_ptr()), "bnv_rgbd_prepare")
    return PreparedFrame(buf, H, W, int(levels), K, rgb is not None, float(max_depth), float(depth_jump))


def rgbd_align(ref, cur, T_guess=None, schedule=DEFAULT_SCHEDULE, lambda_depth=0.968, dist=0.07, min_pair_share=0.05,
               min_spread=1e-3, records=False):
    """Aligns two prepared frames -> ``tracking.TrackResult`` whose ``T_wc`` is the relative pose current <- reference
    (it maps reference-camera points to current-camera points), starting from ``T_guess`` (default identity).
    ``schedule``: (pyramid level, iterations) coarse to fine; ``lambda_depth``: the weight of the depth term against
    the photometric one (1 when either frame has no colour image); ``dist``: the gate on the depth residual in metres.
    Statuses as ``tracking.icp_align``: fewer than ``min_pair_share`` of a level's pixels paired is ``LOST``, a
    translation the images do not hold (smallest eigenvalue of the translation block below ``min_spread``)
    ``DEGENERATE``, a step beyond 0.1 rad / 0.2 m a ``JUMP``: the result is then the guess.  One host read, at the
    end.  The defaults are those of the numpy prototype on the synthetic room (0.968 weighs a 5 mm depth residual like
    an intensity residual of 0.0275): tests/test_odometry_cpu.py shows them recover the room's pairs to below 0.2 mm,
    so they stay."""
    if (ref.H, ref.W, ref.levels) != (cur.H, cur.W, cur.levels) or not np.array_equal(ref.K, cur.K):
        raise ValueError("rgbd_align: the two frames differ in size, levels or intrinsics")
    if ref.depth_jump != cur.depth_jump:
        raise ValueError("rgbd_align: the two frames were prepared with different depth_jump")
    dev = ref.buffer.device
    if cur.buffer.device != dev:
        raise ValueError("rgbd_align: the two frames are on different devices")
    if not (ref.has_rgb and cur.has_rgb):
        lambda_depth = 1.0
    sc = np.ascontiguousarray(np.asarray(schedule, dtype=np.int32).reshape(-1, 2))
    sc_p = sc.ctypes.data_as(C.POINTER(C.c_int32))
    lib = _lib.load()
    need = int(lib.bnv_rgbd_align_bytes(len(sc), sc_p))
    if need == 0 or (sc[:, 0] >= ref.levels).any():
        raise _lib.BnvError(f"rgbd_align: invalid schedule {schedule!r} for {ref.levels} levels")
    n_iter = int(sc[:, 1].sum())
    Kh, Kp = _f64(ref.K, 9)
    T0h, T0p = _f64(np.eye(4) if T_guess is None else T_guess, 16)
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(1 + 16 + (n_iter + 1) * 16 + n_iter * 5, dtype=torch.float64, device=dev)
        status, pose = out[:1].view(torch.int32), out[1:17]
        poses, stats = out[17:17 + (n_iter + 1) * 16], out[17 + (n_iter + 1) * 16:]
        _lib.check(lib.bnv_rgbd_align(_lib.ptr(ref.buffer), _lib.ptr(cur.buffer), ref.H, ref.W, ref.levels, Kp, T0p,
                                      len(sc), sc_p, float(lambda_depth), float(dist), float(ref.depth_jump),
                                      float(min_pair_share), float(min_spread), _lib.ptr(ws), need, _lib.ptr(pose),
                                      _lib.ptr(poses), _lib.ptr(stats), _lib.ptr(status), _lib.stream_ptr()),
                   "bnv_rgbd_align")
        host = out.cpu()                                   # the one host read
        rec = None
        if records:
            rec = ws.view(torch.float64)[ICP_BLOCKS * ICP_SUMS:].reshape(n_iter, ICP_RECORD).cpu().numpy()
    host_np = host.numpy()
    return TrackResult(host_np[1:17].reshape(4, 4).copy(), int(host[:1].view(torch.int32)[0]),
                       host_np[17 + (n_iter + 1) * 16:].reshape(n_iter, 5).copy(),
                       host_np[17:17 + (n_iter + 1) * 16].reshape(n_iter + 1, 4, 4).copy(), rec)


class RgbdOdometry:
    """Frame-to-frame odometry over a stream: ``step(frame)`` prepares the frame once, aligns it to the previous one
    (whose pyramid stays on the device) starting from the last motion -- a constant-velocity guess -- and returns a
    ``TrackResult`` whose ``T_wc`` is the relative motion current <- previous and whose ``status`` says whether the
    aligner accepted the pair; a refused pair returns the guess and counts in ``failures``.  The first frame returns
    identity with status -1.  ``levels``, ``max_depth``, ``depth_jump``: ``prepare_frame``'s; everything else goes to
    ``rgbd_align``."""

    def __init__(self, levels=3, max_depth=3.0, depth_jump=0.05, **align):
        self.levels, self.max_depth, self.depth_jump, self.align = int(levels), max_depth, depth_jump, align
        self.reset()

    def reset(self):
        self.previous, self.motion = None, np.eye(4)
        self.statuses, self.failures = [], 0

    def step(self, frame):
        cur = prepare_frame(frame, self.levels, self.max_depth, self.depth_jump)
        if self.previous is None:
            res = TrackResult(np.eye(4), -1, np.zeros((0, 5)), np.eye(4)[None])
        else:
            res = rgbd_align(self.previous, cur, self.motion, **self.align)
            self.failures += res.status != OK
            self.motion = res.T_wc
        self.previous = cur
        self.statuses.append(res.status)
        return res
