"""Register a reconstruction to a mesh on the GPU: point-to-mesh ICP, so that a reconstruction in its own frame (a
tracked sequence, a live capture, a user's mesh) can be scored in the ground truth's frame.

``register_points`` aligns a point cloud to a triangle mesh from a guess: csrc/register.hip behind bnv_mesh_register
(include/bnv_fusion.h, "Registration").  Every point is paired with the exact closest point of the mesh (the search of
``evaluate.MeshSDF``), the sums and the solve are the tracker's, a step beyond the per-iteration limits is scaled onto
them.  All iterations run on the device without a host read in between; the host reads the result once.  GPU only.

``register_cloud`` aligns a point cloud to another point cloud that carries normals (a ``pointcloud.CloudIndex``):
csrc/cloud_register.hip behind bnv_cloud_register (include/bnv_fusion.h, "Cloud registration"): the nearest target
point within the level's gate, a point-to-plane row with the target's normal, the same sums, solve and schedule.

    res = register_mesh(pred_mesh, gt_mesh, T_guess=T0)     # res.T maps pred into gt's frame
    evaluate.evaluate_meshes(pred_mesh, gt_mesh, align={"T_guess": T0})
    res = register_cloud(scan_b, CloudIndex(scan_a), T_guess=T0)

Out of scope: alignment without a guess, scale, robust weights (the per-level gate is the outlier rule, as in the
tracker), a symmetric (two-normal) objective.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from .evaluate import MeshSDF, _on_gpu, sample_surface
from .tracking import ICP_BLOCKS, ICP_RECORD, ICP_SUMS, _f64
from .tracking import DEGENERATE, JUMP, LOST, OK, STATUS_NAMES   # the statuses are the tracker's (BNV_ICP_*)

__all__ = ["register_points", "register_mesh", "register_cloud", "transform_points", "RegisterResult",
           "CloudRegisterResult", "DEFAULT_LEVELS", "OK", "LOST", "DEGENERATE", "JUMP", "STATUS_NAMES"]

DEFAULT_LEVELS = ((4, 10, 0.2), (2, 6, 0.05), (1, 4, 0.02))      # (stride, iterations, gate in metres), coarse to fine

RegisterResult = collections.namedtuple(
    "RegisterResult", "T status stats poses inlier_share rmse records q closest face feature",
    defaults=(None, None, None, None, None))
RegisterResult.__doc__ = """T float64 [4, 4]: source -> target, or the guess bit for bit when ``status`` is not ``OK``;
stats float64 [n_iter, 5] = pairs, rmse, applied |w|, applied |v|, spread per iteration; poses float64
[n_iter + 1, 4, 4]: the estimate before every iteration and the final one; inlier_share / rmse: the pairs of the last
iteration that ran over its sampled points, and its point-to-plane rmse in metres.  With ``records=True`` also records
float64 [n_iter, 36] (29 sums, xi, pad) and the last iteration's dumps per sampled point: q f32 [n_s, 3], closest f32
[n_s, 3], face int32 [n_s], feature uint8 [n_s] (device tensors)."""


def transform_points(T, points):
    """``points`` [..., 3] (a device tensor) under the rigid ``T`` float64 [4, 4] -> float32, computed in float64."""
    T = torch.as_tensor(np.asarray(T, dtype=np.float64).reshape(4, 4), device=points.device)
    return (points.double() @ T[:3, :3].T + T[:3, 3]).float()


CloudRegisterResult = collections.namedtuple(
    "CloudRegisterResult", "T status stats poses inlier_share rmse records q index", defaults=(None, None, None))
CloudRegisterResult.__doc__ = """``RegisterResult``'s fields for a point-cloud target; the dumps of ``records=True``
are q f32 [n_s, 3] and index int32 [n_s]: the target row every sampled point of the last iteration was nearest to
within the gate, -1 where there was none (device tensors)."""


def _source(points):
    p = _on_gpu(points, "points", torch.float32)
    if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] == 0:
        raise ValueError(f"points: expected a non-empty [N, 3] tensor, got {tuple(p.shape)}")
    return p


def _target(target, device):
    if isinstance(target, MeshSDF):
        return target
    if isinstance(target, tuple):
        return MeshSDF(*target)
    return MeshSDF(target, device=device)


def _schedule(levels, what, bytes_entry):
    """(stride, iterations, gate) rows -> (lv int32 [L, 2], gates float64 [L], workspace bytes); the arrays stay alive
    with the caller."""
    lv3 = np.asarray(levels, dtype=np.float64).reshape(-1, 3)
    lv = np.ascontiguousarray(lv3[:, :2].astype(np.int32))
    if not np.array_equal(lv.astype(np.float64), lv3[:, :2]):
        raise ValueError(f"{what}: strides and iterations are integers, got {levels!r}")
    dist = np.ascontiguousarray(lv3[:, 2])
    need = int(bytes_entry(len(lv), lv.ctypes.data_as(C.POINTER(C.c_int32))))
    if need == 0:
        raise _lib.BnvError(f"{what}: invalid schedule {levels!r}")
    return lv, dist, need


def _outputs(n_iter, dev):
    """One float64 buffer for everything the host reads -> (out, status, pose, poses, stats) views of it."""
    out = torch.empty(1 + 16 + (n_iter + 1) * 16 + n_iter * 5, dtype=torch.float64, device=dev)
    return out, out[:1].view(torch.int32), out[1:17], out[17:17 + (n_iter + 1) * 16], out[17 + (n_iter + 1) * 16:]


def _read(out, ws, n, lv, records):
    """The one host read -> (T, status, stats, poses, inlier_share, rmse, records, rows of the dumps that are valid)."""
    n_iter = int(lv[:, 1].sum())
    host = out.cpu()
    rec = None
    if records:
        rec = ws.view(torch.float64)[ICP_BLOCKS * ICP_SUMS:].reshape(n_iter, ICP_RECORD).cpu().numpy()
    host_np = host.numpy()
    st = host_np[17 + (n_iter + 1) * 16:].reshape(n_iter, 5).copy()
    code = int(host[:1].view(torch.int32)[0])
    # the last iteration that ran: its level's sampled points give the inlier share
    per_iter = np.repeat(-(-n // lv[:, 0].astype(np.int64)), lv[:, 1])
    ran = np.nonzero(st.any(1))[0]
    last = int(ran.max()) if len(ran) else 0
    n_last = int(per_iter[last])
    n_dump = int(per_iter[last if code != OK else n_iter - 1])
    return (host_np[1:17].reshape(4, 4).copy(), code, st,
            host_np[17:17 + (n_iter + 1) * 16].reshape(n_iter + 1, 4, 4).copy(), float(st[last, 0]) / n_last,
            float(st[last, 1]), rec, n_dump)


def register_points(points, target, T_guess=None, levels=DEFAULT_LEVELS, reject_boundary=True, min_pair_share=0.05,
                    min_spread=1e-3, max_rotation=0.1, max_translation=0.2, records=False):
    """Aligns ``points`` (fp32 [N, 3] on the GPU, source frame) to ``target`` (a ``MeshSDF``, a ``TriMesh`` or
    (vertices, faces) device tensors) starting from ``T_guess`` (source -> target, default the identity) ->
    ``RegisterResult``.  ``levels``: (stride, iterations, gate in metres) coarse to fine: every ``stride``-th point,
    paired with its closest point of the mesh when that is within the gate.  ``reject_boundary``: a point whose
    closest feature lies on the rim of an open target is not paired.  A level that keeps fewer than
    ``min_pair_share`` of its sampled points is ``LOST``, normals that spread less than ``min_spread`` are
    ``DEGENERATE``: the result is then the guess.  A step beyond ``max_rotation`` radians or ``max_translation``
    metres is scaled onto the limit.  One host read, at the end.  A ``pointcloud.CloudIndex`` as ``target`` goes to
    ``register_cloud`` with the same schedule and thresholds."""
    from .pointcloud import CloudIndex
    if isinstance(target, CloudIndex):                     # (a cloud has no rim: reject_boundary says nothing there)
        return register_cloud(points, target, T_guess, levels, min_pair_share=min_pair_share, min_spread=min_spread,
                              max_rotation=max_rotation, max_translation=max_translation, records=records)
    p = _source(points)
    dev = p.device
    sdf = _target(target, dev)
    if sdf.device != dev:
        raise ValueError(f"points on {dev}, target on {sdf.device}")
    lib = _lib.load()
    lv, dist, need = _schedule(levels, "register_points", lib.bnv_mesh_register_bytes)
    n, n_iter = int(p.shape[0]), int(lv[:, 1].sum())
    T0h, T0p = _f64(np.eye(4) if T_guess is None else T_guess, 16)
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out, status, pose, poses, stats = _outputs(n_iter, dev)
        q = closest = face = feature = None
        if records:
            q = torch.empty((n, 3), dtype=torch.float32, device=dev)
            closest = torch.empty((n, 3), dtype=torch.float32, device=dev)
            face = torch.empty(n, dtype=torch.int32, device=dev)
            feature = torch.empty(n, dtype=torch.uint8, device=dev)
        _lib.check(lib.bnv_mesh_register(_lib.ptr(sdf._ws), sdf._ws_bytes, _lib.ptr(p), n, T0p, len(lv),
                                         lv.ctypes.data_as(C.POINTER(C.c_int32)),
                                         dist.ctypes.data_as(C.POINTER(C.c_double)), int(bool(reject_boundary)),
                                         float(min_pair_share), float(min_spread), float(max_rotation),
                                         float(max_translation), _lib.ptr(ws), need, _lib.ptr(pose), _lib.ptr(poses),
                                         _lib.ptr(stats), _lib.ptr(status), _lib.ptr(q), _lib.ptr(closest),
                                         _lib.ptr(face), _lib.ptr(feature), _lib.stream_ptr()), "bnv_mesh_register")
        *res, n_dump = _read(out, ws, n, lv, records)      # the one host read
    dumps = (q[:n_dump], closest[:n_dump], face[:n_dump], feature[:n_dump]) if records else (None,) * 4
    return RegisterResult(*res, *dumps)


def register_cloud(points, target, T_guess=None, levels=DEFAULT_LEVELS, normals=None, min_normal_cos=None,
                   oriented=False, min_pair_share=0.05, min_spread=1e-3, max_rotation=0.1, max_translation=0.2,
                   records=False):
    """Aligns ``points`` (fp32 [N, 3] on the GPU, source frame) to a point cloud with normals starting from
    ``T_guess`` (source -> target, default the identity) -> ``CloudRegisterResult``: csrc/cloud_register.hip behind
    bnv_cloud_register (include/bnv_fusion.h, "Cloud registration").  ``target``: a ``pointcloud.CloudIndex`` (built
    once, used any number of times) or an ``[N, 6]`` device tensor of positions and normals, indexed for this call.
    The target's normals need no orientation: the sign of a normal changes no bit of the result.  ``levels``,
    ``min_pair_share``, ``min_spread``, ``max_rotation``, ``max_translation`` and the statuses are ``register_points``'s;
    a sampled point is paired with the nearest target point within the level's gate (the lowest index among equals),
    the row is point-to-plane with the target's normal.  ``min_normal_cos`` with ``normals`` (the source's, fp32
    [N, 3]): a pair is kept only when the turned source normal and the target's agree, ``|cos| >= min_normal_cos``
    or, with ``oriented``, ``cos >= min_normal_cos``.  One host read, at the end.  GPU only."""
    from .pointcloud import CloudIndex
    p = _source(points)
    dev = p.device
    index = target if isinstance(target, CloudIndex) else CloudIndex(input_pts=target)
    if index.device != dev:
        raise ValueError(f"points on {dev}, target on {index.device}")
    nrm = None
    if min_normal_cos is not None:
        if normals is None:
            raise ValueError("register_cloud: min_normal_cos needs the source's normals")
        nrm = _on_gpu(normals, "normals", torch.float32)
        if nrm.shape != p.shape or nrm.device != dev:
            raise ValueError(f"normals: expected {tuple(p.shape)} on {dev}, got {tuple(nrm.shape)} on {nrm.device}")
        if not -1.0 <= float(min_normal_cos) <= 1.0:
            raise ValueError(f"min_normal_cos = {min_normal_cos!r}: a cosine")
    lib = _lib.load()
    lv, dist, need = _schedule(levels, "register_cloud", lib.bnv_cloud_register_bytes)
    n, n_iter = int(p.shape[0]), int(lv[:, 1].sum())
    T0h, T0p = _f64(np.eye(4) if T_guess is None else T_guess, 16)
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out, status, pose, poses, stats = _outputs(n_iter, dev)
        q = torch.empty((n, 3), dtype=torch.float32, device=dev) if records else None
        idx = torch.empty(n, dtype=torch.int32, device=dev) if records else None
        _lib.check(lib.bnv_cloud_register(_lib.ptr(index._ws), index._ws_bytes, _lib.ptr(p), n, _lib.ptr(nrm), T0p,
                                          len(lv), lv.ctypes.data_as(C.POINTER(C.c_int32)),
                                          dist.ctypes.data_as(C.POINTER(C.c_double)),
                                          0.0 if nrm is None else float(min_normal_cos), int(bool(oriented)),
                                          float(min_pair_share), float(min_spread), float(max_rotation),
                                          float(max_translation), _lib.ptr(ws), need, _lib.ptr(pose), _lib.ptr(poses),
                                          _lib.ptr(stats), _lib.ptr(status), _lib.ptr(q), _lib.ptr(idx),
                                          _lib.stream_ptr()), "bnv_cloud_register")
        *res, n_dump = _read(out, ws, n, lv, records)      # the one host read
    dumps = (q[:n_dump], idx[:n_dump]) if records else (None, None)
    return CloudRegisterResult(*res, *dumps)


def register_mesh(source, target, n_samples=100000, generator=None, **kw):
    """Samples the surface of ``source`` (a ``TriMesh`` or (vertices, faces) device tensors) with
    ``evaluate.sample_surface`` (``n_samples`` points, uniforms from ``generator``) and registers the samples to
    ``target`` -> ``RegisterResult``; the keywords are ``register_points``'s."""
    if isinstance(source, tuple):
        pts = sample_surface(source[0], source[1], n_samples, generator=generator)[0]
    else:
        dev = target.device if isinstance(target, MeshSDF) else (target[0].device if isinstance(target, tuple) else None)
        pts = sample_surface(source, None, n_samples, generator=generator, device=dev)[0]
    return register_points(pts, target, **kw)
