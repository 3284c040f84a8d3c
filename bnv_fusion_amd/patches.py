"""Embedding-training patches cut from triangle meshes on the GPU.

The reference trains its embedding on patches cut from ShapeNet chair and lamp meshes
(``<data_dir>/local_shapes/{03001627,03636649}_noise/<seq>/*.pkl``, read by src/datasets/fusion_pointnet_dataset.py);
the program that made them is not part of it.  ``cut_local_patches`` makes such patches from any mesh -- a CAD model, a
scanned room, ``TSDFVolume.get_mesh`` output -- in the units of ``synthetic.local_patches``, which both trainers
consume: a patch is the cube [-1, 1]^3, in voxel units, around one lattice vertex.  The surface samples come from
``evaluate.sample_surface``, the ground truth from ``evaluate.MeshSDF`` (csrc/eval.hip, csrc/meshsdf.hip); the grouping
in between is torch sort / unique on the device and runs once per mesh.  GPU only: a CPU device is refused.

    patches = cut_local_patches(mesh, voxel_size=0.02, n_samples=200000)
    trainer.step(**patches.batch(ids))                   # EmbeddingTrainer or TcnnEmbeddingTrainer
    datasets.write_local_patches(data_dir, "03001627_noise", "my_mesh", patches.to_patch_dicts())
"""
import numpy as np
import torch

from . import evaluate
from .datasets import N_LOCAL_SAMPLES

# corner order of get_relative_xyz / get_neighbors: which axes take ceil instead of floor
_CORNERS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
_KEY_OFFSET = 1 << 20      # lattice coordinates are packed 21 bits per axis


def _draw(shape, generator, dev, normal=False):
    fn = torch.randn if normal else torch.rand
    if generator is not None and generator.device.type != "cuda":
        return fn(shape, generator=generator, dtype=torch.float32).to(dev)
    return fn(shape, generator=generator, dtype=torch.float32, device=dev)


class LocalPatches:
    """Patches on the device in CSR form.  ``offsets`` int64 [P + 1] and ``input_pts`` fp32 [N, 6] (position relative
    to the patch centre in voxel units + unit face normal): the points of patch p are rows offsets[p] .. offsets[p + 1].
    ``centers`` float64 [P, 3] (world), ``training_pts`` fp32 [P, M, 3] (voxel units, inside the cube), ``gt`` fp32
    [P, M] (signed distance in voxel units), ``open`` bool [P] (a training point's closest feature lies on the mesh
    boundary: its sign is not trustworthy; all False unless ``drop_open=False``), ``stats``: samples, pairs,
    vertices_seen, vertices_kept, dropped_open, patches."""

    def __init__(self, offsets, input_pts, centers, training_pts, gt, open_, voxel_size, stats):
        self.offsets, self.input_pts, self.centers = offsets, input_pts, centers
        self.training_pts, self.gt, self.open = training_pts, gt, open_
        self.voxel_size, self.stats = float(voxel_size), dict(stats)
        self.device = input_pts.device

    def __len__(self):
        return int(self.offsets.numel()) - 1

    def counts(self):
        return self.offsets[1:] - self.offsets[:-1]

    def batch(self, ids, n_local=N_LOCAL_SAMPLES, generator=None):
        """Patches ``ids`` -> {"input_pts" [B, n_local, 6], "training_pts" [B, M, 3], "gt" [B, M]} device tensors, as
        the trainers' ``step`` takes them.  ``input_pts`` is resized by ``LocalPatchDataset.resize_input_pts``'s rule:
        a patch of fewer than ``n_local`` points is drawn with replacement up to ``n_local``, one of more gives
        ``n_local`` of a random permutation (the draws come from ``generator``)."""
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).to(self.device)
        if ids.numel() == 0:
            raise ValueError("batch: no patch ids")
        if int(ids.min()) < 0 or int(ids.max()) >= len(self):
            raise IndexError(f"batch: patch ids outside [0, {len(self)})")
        n_local = int(n_local)
        start, cnt = self.offsets[ids], self.counts()[ids]
        B, width = int(ids.numel()), max(int(cnt.max()), n_local)
        u = _draw((B, width), generator, self.device)
        # fewer points than n_local: n_local independent draws (any order of independent draws is a permutation of them)
        repl = (u[:, :n_local].double() * cnt[:, None].double()).long().minimum(cnt[:, None] - 1)
        # otherwise: the first n_local of a random permutation = the n_local smallest of one random key per point
        keys = torch.where(torch.arange(width, device=self.device)[None, :] < cnt[:, None], u, torch.full_like(u, 2.0))
        perm = torch.argsort(keys, dim=1, stable=True)[:, :n_local]
        local = torch.where((cnt < n_local)[:, None], repl, perm)
        return {"input_pts": self.input_pts[start[:, None] + local],
                "training_pts": self.training_pts[ids], "gt": self.gt[ids]}

    def to_patch_dicts(self):
        """The list ``datasets.write_local_patches`` writes (host arrays): per patch {"input_pts" [k, 6], "center"
        [1, 3], "training_pts" [M, 3], "gt_sdf" [M]} -- the layout the reference's fusion_pointnet_dataset reads."""
        off = self.offsets.cpu().numpy()
        inp, ctr = self.input_pts.cpu().numpy(), self.centers.cpu().numpy().astype(np.float32)
        tp, gt = self.training_pts.cpu().numpy(), self.gt.cpu().numpy()
        return [{"input_pts": inp[off[p]:off[p + 1]].copy(), "center": ctr[p:p + 1].copy(),
                 "training_pts": tp[p].copy(), "gt_sdf": gt[p].copy()} for p in range(len(self))]


def cut_local_patches(mesh, voxel_size, n_samples, M=256, noise=0.0, min_pts=16, max_pts=128, near_fraction=0.5,
                      near_sigma=0.15, origin=None, generator=None, device=None, faces=None, drop_open=True):
    """Cuts training patches from ``mesh`` (a TriMesh, or vertices with ``faces`` as device tensors) -> LocalPatches.

    1. ``n_samples`` area-weighted surface samples with unit face normals (``evaluate.sample_surface``), plus Gaussian
       position noise of std ``noise`` voxels (the reference's "_noise" data).
    2. Every sample pairs with its 8 neighbouring vertices of the lattice ``origin + voxel_size * Z^3`` (floor / ceil
       per axis, in the corner order of ``get_relative_xyz``).  A sample at an integer coordinate pairs 2, 4 or 8 times
       with the same vertex: it counts that often in the vertex's sample count and appears once among its samples.
    3. Vertices with at least ``min_pts`` samples become patches; each keeps at most ``max_pts`` samples, a random
       subset drawn from ``generator``.
    4. Per patch ``M`` training points in the cube: ``round(near_fraction * M)`` a Gaussian step of std ``near_sigma``
       voxels off the patch's own samples, the rest uniform, all clipped into the cube;
       ``gt = MeshSDF.query(centre + q * voxel_size) / voxel_size``.
    5. A patch with a training point whose closest feature lies on the mesh boundary (an open mesh: no trustworthy
       sign) is dropped (``drop_open``, counted in ``stats["dropped_open"]``) or kept and flagged in ``.open``.
    The same ``generator`` state gives the same bits."""
    v, f = evaluate._mesh_tensors(mesh, faces, device)          # refuses a CPU device / CPU tensors
    voxel_size, n_samples, M = float(voxel_size), int(n_samples), int(M)
    min_pts, max_pts = int(min_pts), int(max_pts)
    if not voxel_size > 0 or n_samples < 1 or M < 1:
        raise ValueError("voxel_size must be positive, n_samples and M at least 1")
    if min_pts < 1 or max_pts < min_pts:
        raise ValueError(f"min_pts={min_pts}, max_pts={max_pts}: need 1 <= min_pts <= max_pts")
    if not 0.0 <= near_fraction <= 1.0 or noise < 0 or near_sigma < 0:
        raise ValueError("near_fraction must be in [0, 1], noise and near_sigma non-negative")
    dev = v.device
    org = torch.zeros(3, dtype=torch.float64, device=dev) if origin is None else \
        torch.as_tensor(np.asarray(origin, dtype=np.float64).reshape(3)).to(dev)

    # 1. samples
    pts, _, nrm = evaluate.sample_surface(v, f, n_samples, generator=generator, return_normals=True)
    if noise > 0:
        pts = pts + _draw((n_samples, 3), generator, dev, normal=True) * (noise * voxel_size)
    # 2. pairs (sample, lattice vertex), lattice arithmetic in float64
    xn = (pts.double() - org) / voxel_size
    lo, hi = torch.floor(xn), torch.ceil(xn)
    pick = torch.tensor(_CORNERS, dtype=torch.bool, device=dev)                  # [8, 3]
    vert = torch.where(pick[None], hi[:, None, :], lo[:, None, :]).long()         # [n, 8, 3]
    if int(vert.abs().max()) >= _KEY_OFFSET:
        raise ValueError("the mesh spans more than 2^20 voxels from the origin: choose a larger voxel_size or an origin")
    k = vert + _KEY_OFFSET
    key = ((k[..., 0] << 42) | (k[..., 1] << 21) | k[..., 2]).reshape(-1)        # [8 n]
    sample = torch.arange(n_samples, device=dev)[:, None].expand(n_samples, 8).reshape(-1)
    ukey, vid = torch.unique(key, return_inverse=True)
    n_seen = int(ukey.numel())
    seen_count = torch.bincount(vid, minlength=n_seen)                           # with the 2/4/8-fold multiplicity
    pair = torch.unique(vid * n_samples + sample)                                # sorted by (vertex, sample), once each
    pv, ps = pair // n_samples, pair % n_samples
    # 3. vertices kept, at most max_pts samples each: rank of a random key inside the vertex's group
    keep_v = seen_count >= min_pts
    sel = keep_v[pv]
    pv, ps = pv[sel], ps[sel]
    stats = {"samples": n_samples, "pairs": int(key.numel()), "vertices_seen": n_seen,
             "vertices_kept": int(keep_v.sum()), "dropped_open": 0, "patches": 0}
    if pv.numel() == 0:
        raise ValueError(f"no lattice vertex has {min_pts} samples: more samples or a larger voxel_size")
    order = torch.argsort(_draw((int(pv.numel()),), generator, dev), stable=True)
    order = order[torch.argsort(pv[order], stable=True)]                         # by vertex, random inside a vertex
    pv, ps = pv[order], ps[order]
    pid = torch.unique_consecutive(pv, return_inverse=True)[1]                   # patch number 0 .. P-1
    group = torch.bincount(pid)
    first = torch.cumsum(group, 0) - group
    sel = torch.arange(int(pv.numel()), device=dev) - first[pid] < max_pts
    pv, ps, pid = pv[sel], ps[sel], pid[sel]
    cnt = torch.bincount(pid, minlength=int(group.numel()))
    P = int(cnt.numel())
    offsets = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(cnt, 0)
    # 4. input points: position relative to the centre, in voxels, and the normal
    kept_key = ukey[keep_v]                                                      # sorted like the patch numbers
    lattice = torch.stack([(kept_key >> 42) & 0x1fffff, (kept_key >> 21) & 0x1fffff, kept_key & 0x1fffff], 1) - _KEY_OFFSET
    centers = org + lattice.double() * voxel_size                                # [P, 3]
    rel = (xn[ps] - lattice[pid].double()).float()
    input_pts = torch.cat([rel, nrm[ps]], dim=1).contiguous()
    # training points
    n_near = int(round(near_fraction * M))
    parts = []
    if n_near:
        j = (_draw((P, n_near), generator, dev).double() * cnt[:, None].double()).long().minimum(cnt[:, None] - 1)
        base = input_pts[offsets[:-1, None] + j, :3]
        parts.append(base + _draw((P, n_near, 3), generator, dev, normal=True) * near_sigma)
    if M - n_near:
        parts.append(_draw((P, M - n_near, 3), generator, dev) * 2.0 - 1.0)
    q = torch.cat(parts, dim=1).clamp_(-1.0, 1.0).contiguous()
    world = (centers[:, None, :] + q.double() * voxel_size).float()
    sdf, _, _, feature = evaluate.MeshSDF(v, f).query(world)
    gt = sdf / voxel_size
    # 5. open meshes
    open_ = ((feature & evaluate.FEATURE_BOUNDARY) != 0).any(dim=1)
    if drop_open and bool(open_.any()):
        keep_p = ~open_
        stats["dropped_open"] = int(open_.sum())
        rows = keep_p[pid]
        input_pts = input_pts[rows].contiguous()
        cnt = cnt[keep_p]
        P = int(cnt.numel())
        offsets = torch.zeros(P + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(cnt, 0)
        centers, q, gt, open_ = centers[keep_p], q[keep_p].contiguous(), gt[keep_p].contiguous(), open_[keep_p]
    stats["patches"] = P
    return LocalPatches(offsets, input_pts, centers, q, gt, open_, voxel_size, stats)
