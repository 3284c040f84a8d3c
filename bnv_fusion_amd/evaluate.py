"""Mesh quality against a ground-truth mesh: the reference's end metric (src/scripts/evaluate_bnvf.py:9-31,
src/scripts/compute_chamfer.py:36-75) on the GPU.

The reference samples 100,000 points on each mesh (trimesh ``sample_surface``), finds every point's nearest neighbour on
the other side (sklearn ball tree) and reports the pred -> gt mean distance, precision at 2.5 cm, the gt -> pred mean
distance, recall at 2.5 cm and F1.  Here the sampling and the exact nearest-neighbour search are HIP kernels
(csrc/eval.hip; include/bnv_fusion.h: bnv_mesh_sample_surface, bnv_nn_query), and so is the exact signed distance to a
mesh (``MeshSDF``, csrc/meshsdf.hip); only the reductions that turn
distances into figures (a mean, a count under the threshold) run in torch, in float64.  Inputs live on the GPU: a CPU
tensor is refused, there is no CPU fallback.

    res = evaluate_meshes(pred_mesh, gt_mesh)               # TriMesh or (vertices, faces) device tensors
    print(summary_line(res))                                # "{:.3f}/{:.4f}/{:.3f}/{:.4f}/{:.4f}", as the reference
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .mesh import TriMesh

KEYS = ("pred_gt", "accuracy", "gt_pred", "recall", "F1")


def _device(device):
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise ValueError(f"device {dev}: the mesh evaluation runs on the GPU only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def _on_gpu(t, what, dtype):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor on the GPU, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{what}: a CPU tensor; the mesh evaluation runs on the GPU only (no CPU fallback)")
    return t.detach().to(dtype).contiguous()


def _points(t, what):
    t = _on_gpu(t, what, torch.float32)
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] == 0:
        raise ValueError(f"{what}: expected a non-empty [N, 3] tensor, got {tuple(t.shape)}")
    return t


def _mesh_tensors(mesh, faces=None, device=None):
    """TriMesh (host) -> device tensors; (vertices, faces) device tensors are checked and passed through."""
    if isinstance(mesh, TriMesh):
        if faces is not None:
            raise ValueError("a TriMesh carries its faces: do not pass `faces` with it")
        dev = _device(device)
        return (torch.from_numpy(np.ascontiguousarray(mesh.vertices, dtype=np.float32)).to(dev),
                torch.from_numpy(np.ascontiguousarray(mesh.faces, dtype=np.int32)).to(dev))
    if faces is None:
        raise ValueError("faces are needed with a vertex tensor")
    v = _points(mesh, "vertices")
    f = _on_gpu(faces, "faces", torch.int32)
    if f.device != v.device:
        raise ValueError(f"faces on {f.device}, vertices on {v.device}")
    if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] == 0:
        raise ValueError(f"faces: expected a non-empty [T, 3] tensor, got {tuple(f.shape)}")
    return v, f


def _uniforms(n, generator, dev):
    if generator is not None and generator.device.type != "cuda":
        return torch.rand((n, 3), generator=generator, dtype=torch.float32).to(dev)
    return torch.rand((n, 3), generator=generator, dtype=torch.float32, device=dev)


def sample_surface_uniforms(vertices, faces, uniforms, return_normals=False):
    """trimesh's ``sample_surface`` with the uniforms given: ``uniforms`` fp32 [n, 3] in [0, 1) on the mesh's device ->
    (points fp32 [n, 3], face_ids int64 [n][, unit face normals fp32 [n, 3]]).  Deterministic: the same inputs give the
    same bits (include/bnv_fusion.h: bnv_mesh_sample_surface)."""
    v, f = _mesh_tensors(vertices, faces)
    u = _points(uniforms, "uniforms")
    if u.device != v.device:
        raise ValueError(f"uniforms on {u.device}, mesh on {v.device}")
    lib = _lib.load()
    n = int(u.shape[0])
    ws_bytes = C.c_int64()
    _lib.check(lib.bnv_mesh_sample_surface_workspace(int(f.shape[0]), C.byref(ws_bytes)),
               "bnv_mesh_sample_surface_workspace")
    with torch.cuda.device(v.device):
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=v.device)
        pts = torch.empty((n, 3), dtype=torch.float32, device=v.device)
        ids = torch.empty(n, dtype=torch.int32, device=v.device)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=v.device) if return_normals else None
        _lib.check(lib.bnv_mesh_sample_surface(_lib.ptr(v), int(v.shape[0]), _lib.ptr(f), int(f.shape[0]), _lib.ptr(u),
                                               n, _lib.ptr(ws), int(ws_bytes.value), _lib.ptr(pts), _lib.ptr(ids),
                                               _lib.ptr(nrm), _lib.stream_ptr()),
                   "bnv_mesh_sample_surface (a mesh without area, or a face index out of range?)")
    return (pts, ids.long(), nrm) if return_normals else (pts, ids.long())


def sample_surface(vertices, faces=None, n=100000, generator=None, return_normals=False, device=None):
    """``n`` area-weighted samples on a mesh (trimesh.sample.sample_surface, which the reference calls): ``vertices``
    fp32 [V, 3] and ``faces`` int [T, 3] device tensors, or a TriMesh (uploaded to ``device``, default the current
    GPU).  The uniforms come from ``torch.rand(generator=generator)``.  -> (points [n, 3], face_ids [n][, normals])."""
    v, f = _mesh_tensors(vertices, faces, device)
    return sample_surface_uniforms(v, f, _uniforms(int(n), generator, v.device), return_normals)


def nn_d2(query, ref):
    """Exact nearest neighbour in ``ref`` of every point of ``query`` (fp32 [N, 3] device tensors) -> (d2 fp32 [N], idx
    int32 [N]): d2 is bitwise the minimum over ``ref`` of the fp32 (dx*dx + dy*dy) + dz*dz, idx the lowest reference
    index attaining it.  A reference point with a NaN / Inf coordinate is never returned; such a query gets (+inf, -1)."""
    q = _points(query, "query")
    r = _points(ref, "ref")
    if q.device != r.device:
        raise ValueError(f"query on {q.device}, ref on {r.device}")
    lib = _lib.load()
    ws_bytes = C.c_int64()
    _lib.check(lib.bnv_nn_workspace_bytes(int(r.shape[0]), int(q.shape[0]), C.byref(ws_bytes)), "bnv_nn_workspace_bytes")
    with torch.cuda.device(q.device):
        ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=q.device)
        d2 = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
        idx = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
        _lib.check(lib.bnv_nn_query(_lib.ptr(r), int(r.shape[0]), _lib.ptr(q), int(q.shape[0]), _lib.ptr(ws),
                                    int(ws_bytes.value), _lib.ptr(d2), _lib.ptr(idx), _lib.stream_ptr()), "bnv_nn_query")
    return d2, idx


def nearest_neighbors(query, ref):
    """-> (dist float64 [N] = sqrt(d2) taken in float64, idx int64 [N]); see ``nn_d2``."""
    d2, idx = nn_d2(query, ref)
    return torch.sqrt(d2.double()), idx.long()


FEATURE_FACE, FEATURE_EDGE, FEATURE_VERTEX = 0, 1, 2
FEATURE_CLASS_MASK = 0x0f
FEATURE_BOUNDARY = 0x10        # the closest edge / vertex lies on the mesh boundary: the sign is not trustworthy
FEATURE_NONMANIFOLD = 0x20     # ... has an edge with more than two faces


class MeshSDF:
    """Exact signed distance to a triangle mesh on the GPU (csrc/meshsdf.hip; include/bnv_fusion.h:
    bnv_mesh_sdf_build / bnv_mesh_sdf_query): negative inside for outward-oriented faces, exact everywhere (no
    truncation band), bitwise reproducible.  ``vertices`` fp32 [V, 3] and ``faces`` int [T, 3] device tensors, or a
    TriMesh (uploaded to ``device``, default the current GPU) -- the conventions of ``sample_surface``.  The index is
    built once; ``query`` may be called any number of times.

        sdf, face, closest, feature = MeshSDF(mesh).query(points)
    """

    def __init__(self, vertices, faces=None, device=None):
        v, f = _mesh_tensors(vertices, faces, device)
        self.device = v.device
        self.n_vertices, self.n_faces = int(v.shape[0]), int(f.shape[0])
        lib = _lib.load()
        ws_bytes = C.c_int64()
        _lib.check(lib.bnv_mesh_sdf_workspace_bytes(self.n_vertices, self.n_faces, C.byref(ws_bytes)),
                   "bnv_mesh_sdf_workspace_bytes")
        self._ws_bytes = int(ws_bytes.value)
        with torch.cuda.device(self.device):
            self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=self.device)
            _lib.check(lib.bnv_mesh_sdf_build(_lib.ptr(v), self.n_vertices, _lib.ptr(f), self.n_faces,
                                              _lib.ptr(self._ws), self._ws_bytes, _lib.stream_ptr()),
                       "bnv_mesh_sdf_build")

    def query(self, points):
        """``points`` fp32 [..., 3] on the mesh's device -> (sdf fp32 [...], face int32 [...] -- the closest triangle,
        the lowest index among equals --, closest fp32 [..., 3], feature uint8 [...]: ``FEATURE_FACE`` / ``_EDGE`` /
        ``_VERTEX``, ``| FEATURE_BOUNDARY``, ``| FEATURE_NONMANIFOLD``).  A non-finite point gets (nan, -1, nan, 0)."""
        q = _on_gpu(points, "points", torch.float32)
        if q.dim() < 1 or q.shape[-1] != 3 or q.numel() == 0:
            raise ValueError(f"points: expected a non-empty [..., 3] tensor, got {tuple(q.shape)}")
        if q.device != self.device:
            raise ValueError(f"points on {q.device}, mesh on {self.device}")
        lead = tuple(q.shape[:-1])
        q = q.reshape(-1, 3)
        n = int(q.shape[0])
        lib = _lib.load()
        with torch.cuda.device(self.device):
            sdf = torch.empty(n, dtype=torch.float32, device=self.device)
            face = torch.empty(n, dtype=torch.int32, device=self.device)
            closest = torch.empty((n, 3), dtype=torch.float32, device=self.device)
            feature = torch.empty(n, dtype=torch.uint8, device=self.device)
            _lib.check(lib.bnv_mesh_sdf_query(_lib.ptr(self._ws), self._ws_bytes, _lib.ptr(q), n, _lib.ptr(sdf),
                                              _lib.ptr(face), _lib.ptr(closest), _lib.ptr(feature), _lib.stream_ptr()),
                       "bnv_mesh_sdf_query")
        return sdf.reshape(lead), face.reshape(lead), closest.reshape(lead + (3,)), feature.reshape(lead)


def mesh_sdf(points, vertices, faces=None):
    """One-shot ``MeshSDF(vertices, faces).query(points)``; a TriMesh goes to the device of ``points``."""
    dev = points.device if isinstance(points, torch.Tensor) and points.is_cuda else None
    return MeshSDF(vertices, faces, device=dev).query(points)


def metrics_from_distances(d_pred_gt, d_gt_pred, threshold=0.025):
    """The five figures of evaluate_bnvf.py:9-31 from the two distance vectors (float64 on the device): means, strict
    ``<`` counts, F1 = 2PR / (P + R) -- nan when P + R = 0, as the reference's numpy gives."""
    a = d_pred_gt.double()
    b = d_gt_pred.double()
    vals = torch.stack([a.mean(), (a < threshold).double().sum() / a.numel(),
                        b.mean(), (b < threshold).double().sum() / b.numel()]).tolist()
    p, r = vals[1], vals[3]
    f1 = 2 * p * r / (p + r) if (p + r) != 0 else float("nan")
    return dict(zip(KEYS, vals[:4] + [f1]))


def evaluate(pred_points, gt_points, threshold=0.025, align=None):
    """evaluate_bnvf.py:9-31: nearest neighbours both ways -> {"pred_gt", "accuracy", "gt_pred", "recall", "F1"}
    (accuracy = precision = fraction of predicted points closer than ``threshold`` to the ground truth).

    align: None scores the two sets as they are.  True, or a dict of ``register.register_cloud`` keywords (a
    ``T_guess`` among them), first registers the predicted points to the ground-truth points (cloud-to-cloud ICP; the
    ground truth's normals are estimated, unoriented) and scores the transformed points: the result gains
    ``"T_align"``, ``"align_status"`` and the five figures before alignment under ``"unaligned"``, as
    ``evaluate_meshes(align=)`` does.  A refused registration scores unaligned."""

    def score(pts):
        d_pg, _ = nearest_neighbors(pts, gt_points)
        d_gp, _ = nearest_neighbors(gt_points, pts)
        return metrics_from_distances(d_pg, d_gp, threshold)

    if align is None or align is False:
        return score(pred_points)
    from . import register
    from .pointcloud import CloudIndex
    unaligned = score(pred_points)
    reg = register.register_cloud(pred_points, CloudIndex(gt_points), **({} if align is True else dict(align)))
    res = score(register.transform_points(reg.T, pred_points)) if reg.status == register.OK else dict(unaligned)
    res["T_align"], res["align_status"], res["unaligned"] = reg.T, reg.status, unaligned
    return res


def evaluate_meshes(pred, gt, n_samples=100000, threshold=0.025, vertices_only=False, normals=False, generator=None,
                    device=None, gt_recall=None, align=None):
    """compute_chamfer.py:36-75 / evaluate_bnvf.py:56-72: ``n_samples`` surface samples on each mesh (TriMesh or
    (vertices, faces) device tensors), then ``evaluate``.

    vertices_only: the ground truth is a ``torch.randperm`` subset of ``n_samples`` of its vertices
    (compute_chamfer.py:40-41) instead of surface samples.  normals: adds ``normal_consistency`` -- the signed mean of
    gt_normal . pred_normal[idx], idx from the gt -> pred query (compute_chamfer.py:66-75).  gt_recall: optionally a
    second ground truth for the recall side (a region every view saw: synthetic.gt_mesh("common")) -- the precision
    side then uses ``gt`` and the recall side ``gt_recall``.

    align: None scores the two meshes as they are.  True, or a dict of ``register.register_points`` keywords (a
    ``T_guess`` among them), first registers the prediction's samples to the ground-truth mesh (point-to-mesh ICP,
    register.py) and scores the transformed samples (the normals turn with them): the result gains ``"T_align"``
    (float64 [4, 4], prediction -> ground truth), ``"align_status"`` (register.OK, ...) and the five figures before
    alignment under ``"unaligned"``.  A refused registration scores unaligned: ``"T_align"`` is then the guess and
    ``"align_status"`` says why."""
    if normals and vertices_only:
        raise ValueError("normals need surface samples of the ground truth (compute_chamfer.py:73)")
    dev = _device(device if device is not None else (pred[0].device if isinstance(pred, tuple) else None))
    pv, pf = _mesh_tensors(*pred) if isinstance(pred, tuple) else _mesh_tensors(pred, None, dev)

    def gt_side(mesh):
        gv, gf = _mesh_tensors(*mesh) if isinstance(mesh, tuple) else _mesh_tensors(mesh, None, dev)
        if vertices_only:
            perm = torch.randperm(int(gv.shape[0]), generator=generator,
                                  device="cpu" if generator is None or generator.device.type != "cuda" else dev)
            return gv[perm[:n_samples].to(dev)], None
        s = sample_surface(gv, gf, n_samples, generator=generator, return_normals=normals)
        return s[0], (s[2] if normals else None)

    p = sample_surface(pv, pf, n_samples, generator=generator, return_normals=normals)
    pred_pts = p[0]
    pred_nrm = p[2] if normals else None
    gt_pts, gt_nrm = gt_side(gt)
    gt_pts_recall, gt_nrm_recall = gt_side(gt_recall) if gt_recall is not None else (gt_pts, gt_nrm)

    def score(pts, nrm):
        d_pg, _ = nearest_neighbors(pts, gt_pts)
        d_gp, idx = nearest_neighbors(gt_pts_recall, pts)
        res = metrics_from_distances(d_pg, d_gp, threshold)
        if normals:
            dots = (gt_nrm_recall.double() * nrm.double()[idx]).sum(-1)
            res["normal_consistency"] = float(dots.mean())
        return res

    if align is None or align is False:
        return score(pred_pts, pred_nrm)
    from . import register
    unaligned = score(pred_pts, pred_nrm)
    kw = {} if align is True else dict(align)
    target = _mesh_tensors(*gt) if isinstance(gt, tuple) else _mesh_tensors(gt, None, dev)
    reg = register.register_points(pred_pts, target, **kw)
    if reg.status == register.OK:
        moved = register.transform_points(reg.T, pred_pts)
        if normals:
            pred_nrm = (pred_nrm.double() @ torch.as_tensor(reg.T[:3, :3], device=dev).T).float()
        res = score(moved, pred_nrm)
    else:
        res = dict(unaligned)
    res["T_align"], res["align_status"], res["unaligned"] = reg.T, reg.status, unaligned
    return res


def summary_line(res):
    """The reference's one-line summary: pred_gt / accuracy / gt_pred / recall / F1."""
    return "{:.3f}/{:.4f}/{:.3f}/{:.4f}/{:.4f}".format(*[res[k] for k in KEYS])


def depth_errors(pred, gt, threshold=0.025):
    """Rendered depth ``pred`` against observed depth ``gt`` (same shape, metres, 0 = none; any device) -> {"coverage":
    hits among pixels with gt > 0, "median" / "mean" absolute error and "rmse" over pixels where both are > 0,
    "within": the fraction of those with |error| <= threshold}.  The error figures are nan when no pixel has both."""
    p = torch.as_tensor(pred).double()
    g = torch.as_tensor(gt).to(p.device).double()
    if p.shape != g.shape:
        raise ValueError(f"depth_errors: shapes differ ({tuple(p.shape)} vs {tuple(g.shape)})")
    obs = g > 0
    both = obs & (p > 0)
    e = (p - g)[both].abs()
    n_obs = int(obs.sum())
    res = {"coverage": (int(both.sum()) / n_obs) if n_obs else float("nan")}
    if e.numel() == 0:
        return dict(res, median=float("nan"), mean=float("nan"), rmse=float("nan"), within=float("nan"))
    return dict(res, median=float(e.median()), mean=float(e.mean()), rmse=float(torch.sqrt((e * e).mean())),
                within=float((e <= threshold).double().mean()))


def rigid_fit(src, dst):
    """The rigid transform (no scale) that best maps the points ``src`` [n, 3] onto ``dst`` [n, 3] in the least-squares
    sense (Horn 1987 / Kabsch: the SVD of the centred cross-covariance, a reflection turned back) -> float64 [4, 4]."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    dst = np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    cs, cd = src.mean(0), dst.mean(0)
    U, _, Vt = np.linalg.svd((dst - cd).T @ (src - cs))
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) >= 0.0 else -1.0])
    T = np.eye(4)
    T[:3, :3] = U @ D @ Vt
    T[:3, 3] = cd - T[:3, :3] @ cs
    return T


def trajectory_errors(est, gt, align=False):
    """Absolute error of a trajectory against the true one, pose by pose: ``est``, ``gt`` [n, 4, 4] camera-to-world ->
    {"translation_rmse": metres, "rotation_mean_deg": the mean angle of R_est^T R_gt, "translation_max",
    "rotation_max_deg", "n"}.  By default without any alignment of the two; ``align=True`` first applies to ``est`` the
    rigid transform (no scale, ``rigid_fit``) that best maps the estimated positions onto the true ones -- for a
    trajectory in a frame of its own -- and returns it as ``"T_align"``."""
    est = np.asarray(est, dtype=np.float64).reshape(-1, 4, 4)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4, 4)
    if est.shape != gt.shape or len(est) == 0:
        raise ValueError(f"trajectory_errors: {est.shape} against {gt.shape}")
    if align:
        T_align = rigid_fit(est[:, :3, 3], gt[:, :3, 3])
        res = trajectory_errors(T_align @ est, gt)
        res["T_align"] = T_align
        return res
    dt = np.linalg.norm(est[:, :3, 3] - gt[:, :3, 3], axis=1)
    tr = np.einsum("nij,nij->n", est[:, :3, :3], gt[:, :3, :3])
    ang = np.degrees(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0)))
    return {"translation_rmse": float(np.sqrt(np.mean(dt * dt))), "rotation_mean_deg": float(ang.mean()),
            "translation_max": float(dt.max()), "rotation_max_deg": float(ang.max()), "n": int(len(est))}
