"""Mesh extraction from decoded SDF lattices: per-voxel marching cubes on the GPU (csrc/mesh.hip), the
last stage of SparseVolume.meshlize (src/models/sparse_volume.py:740-766).

``marching_cubes_lattice_indexed`` produces what the reference's loop produces: per voxel a vertex list without
duplicates and faces indexing it, concatenated with ``faces + last_face_id`` / ``last_face_id += max(faces) + 1``
(:748-751).  ``marching_cubes_lattice`` is the older triangle-soup form (3 vertices per face).

``TriMesh`` stands in for the ``trimesh.Trimesh(vertices, faces, process=False)`` the reference returns:
``.vertices`` [V, 3] float32, ``.faces`` [T, 3] int64 (numpy, like trimesh), ``.export(path)`` (binary PLY).
"""
import ctypes as C
import struct

import numpy as np
import torch

from . import _lib
from .mc_tables import TRI_TABLE

_TABLES = {}


def _table(device):
    key = str(device)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(np.ascontiguousarray(TRI_TABLE)).to(device)
    return _TABLES[key]


def to_host(*tensors):
    """Device tensors -> numpy arrays through PINNED host memory, all copies in flight at once, one synchronisation.  A
    whole-volume mesh is ~100 MB (12 B per vertex, 24 B per triangle); ``tensor.cpu()`` stages pageable copies at a
    quarter of the link's rate, and they were two thirds of an ``extract_mesh`` call.  The arrays own their pinned
    blocks (torch's host allocator takes them back when the mesh is dropped and hands them to the next call)."""
    hosts = []
    for t in tensors:
        t = t.detach()
        if not t.is_cuda or t.numel() == 0:
            hosts.append(t.cpu())
            continue
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t.contiguous(), non_blocking=True)
        hosts.append(h)
    if any(t.is_cuda for t in tensors):
        torch.cuda.current_stream(next(t.device for t in tensors if t.is_cuda)).synchronize()
    return [h.numpy() for h in hosts]


class TriMesh:
    """``vertices`` [V, 3] float32, ``faces`` [T, 3] int64.  Optional per-vertex attributes, None unless set:
    ``vertex_normals`` [V, 3] float32 and ``vertex_colors`` [V, 3] uint8 (red, green, blue), computed on the final mesh
    (``vertex_normals`` / ``color_vertices``; ``extract_mesh(normals=..., color=...)``) and written by ``export``."""

    def __init__(self, vertices, faces):
        self.vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        self.vertex_normals = None
        self.vertex_colors = None

    def export(self, path):
        """Binary little-endian PLY (what trimesh writes for a ``.ply`` path); with attributes set, the vertex element
        also carries ``float nx ny nz`` and / or ``uchar red green blue``."""
        v, f = self.vertices, self.faces
        props, fields = "property float x\nproperty float y\nproperty float z\n", [("p", "<f4", 3)]
        if self.vertex_normals is not None:
            props += "property float nx\nproperty float ny\nproperty float nz\n"
            fields.append(("n", "<f4", 3))
        if self.vertex_colors is not None:
            props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            fields.append(("c", "u1", 3))
        header = ("ply\nformat binary_little_endian 1.0\n"
                  f"element vertex {len(v)}\n{props}"
                  f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        vrec = np.empty(len(v), dtype=fields)          # (a packed record: x y z [nx ny nz] [red green blue])
        vrec["p"] = v.astype("<f4")
        for key, name, attr, dt in (("n", "vertex_normals", self.vertex_normals, np.float32),
                                    ("c", "vertex_colors", self.vertex_colors, np.uint8)):
            if attr is not None:
                a = np.asarray(attr)
                if a.shape != (len(v), 3):
                    raise ValueError(f"TriMesh.export: {name} must be [{len(v)}, 3] (got {list(a.shape)})")
                vrec[key] = a.astype(dt)
        rec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", 3)])
        rec["n"] = 3
        rec["i"] = f.astype(np.int32)
        with open(path, "wb") as fh:
            fh.write(header.encode("ascii"))
            fh.write(vrec.tobytes())
            fh.write(rec.tobytes())
        return path

    def merge_vertices(self):
        """Weld coincident vertices (trimesh's ``merge_vertices``): meshlize shares vertices inside a voxel only,
        neighbouring voxels repeat the vertices on their common lattice edges.  A mesh that carries vertex attributes
        is refused: they are computed on the final mesh and are not carried through welding."""
        if self.vertex_normals is not None or self.vertex_colors is not None:
            raise ValueError("TriMesh.merge_vertices: the mesh carries vertex_normals / vertex_colors; weld first and "
                             "compute the attributes on the final mesh")
        u, inv = np.unique(np.ascontiguousarray(self.vertices).view([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]).reshape(-1),
                           return_inverse=True)
        self.vertices = u.view(np.float32).reshape(-1, 3).copy()
        self.faces = inv.reshape(-1)[self.faces].astype(np.int64)
        return self


def marching_cubes_lattice(sdf, origins, voxel_size, min_coords, level=0.0, n_dev=None):
    """sdf [n, 27] (or [n, 3, 3, 3]) float32 on the GPU: the lattice {-.5, 0, .5}^3 of every voxel;
    origins [n, 3] int64 voxel coordinates.  -> (vertices [3T, 3] f32 world coordinates, faces [T, 3] i64)
    on the device, as a triangle soup (faces = arange)."""
    lib = _lib.load()
    sdf = sdf.detach().reshape(-1, 27).float().contiguous()
    origins = origins.detach().reshape(-1, 3).long().contiguous()
    n = int(sdf.shape[0])
    dev = sdf.device
    assert origins.shape[0] == n
    if n == 0:
        return torch.zeros((0, 3), device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev)
    table = _table(dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(lib.bnv_mc_count(_lib.ptr(sdf), n, _lib.ptr(n_dev), float(level), _lib.ptr(table), _lib.ptr(counts),
                                _lib.stream_ptr()), "bnv_mc_count")
    ends = torch.cumsum(counts.long(), 0)
    total = int(ends[-1])                       # the one host read: the mesh has to be allocated
    offsets = (ends - counts.long()).contiguous()
    verts = torch.empty((3 * total, 3), dtype=torch.float32, device=dev)
    if total:
        mn = (C.c_float * 3)(*[float(x) for x in torch.as_tensor(min_coords).reshape(-1)[:3].tolist()])
        _lib.check(lib.bnv_mc_emit(_lib.ptr(sdf), _lib.ptr(origins), n, _lib.ptr(n_dev), float(level),
                                   float(voxel_size), mn, _lib.ptr(table), _lib.ptr(offsets), _lib.ptr(verts),
                                   _lib.stream_ptr()), "bnv_mc_emit")
    faces = torch.arange(3 * total, dtype=torch.int64, device=dev).reshape(-1, 3)
    return verts, faces


def marching_cubes_lattice_indexed(sdf, origins, voxel_size, min_coords, level=0.0, n_dev=None):
    """sdf [n, 27] (or [n, 3, 3, 3]) float32 on the GPU; origins [n, 3] int64.  -> (vertices [V, 3] f32 world
    coordinates, faces [T, 3] i64, n_verts [n] i32, n_tris [n] i32) on the device: the concatenation
    SparseVolume.meshlize builds (sparse_volume.py:740-756) -- voxels that fail the gate contribute nothing, a voxel's
    faces index its own vertices offset by the vertex counts of the voxels before it."""
    lib = _lib.load()
    sdf = sdf.detach().reshape(-1, 27).float().contiguous()
    origins = origins.detach().reshape(-1, 3).long().contiguous()
    n = int(sdf.shape[0])
    dev = sdf.device
    assert origins.shape[0] == n
    if n == 0:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return torch.zeros((0, 3), device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev), z, z
    table = _table(dev)
    nv = torch.empty(n, dtype=torch.int32, device=dev)
    nt = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(lib.bnv_mc_count_indexed(_lib.ptr(sdf), n, _lib.ptr(n_dev), float(level), _lib.ptr(table),
                                        _lib.ptr(nv), _lib.ptr(nt), _lib.stream_ptr()), "bnv_mc_count_indexed")
    ve, te = torch.cumsum(nv.long(), 0), torch.cumsum(nt.long(), 0)
    totals = torch.stack([ve[-1], te[-1]]).tolist()         # the one host read: the mesh has to be allocated
    V, T = int(totals[0]), int(totals[1])
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((T, 3), dtype=torch.int64, device=dev)
    if T:
        mn = (C.c_float * 3)(*[float(x) for x in torch.as_tensor(min_coords).reshape(-1)[:3].tolist()])
        voff, toff = (ve - nv.long()).contiguous(), (te - nt.long()).contiguous()
        _lib.check(lib.bnv_mc_emit_indexed(_lib.ptr(sdf), _lib.ptr(origins), n, _lib.ptr(n_dev), float(level),
                                           float(voxel_size), mn, _lib.ptr(table), _lib.ptr(voff), _lib.ptr(toff),
                                           _lib.ptr(verts), _lib.ptr(faces), _lib.stream_ptr()), "bnv_mc_emit_indexed")
    return verts, faces, nv, nt


def post_process_mesh(mesh, vertex_threshold=0.005, surface_threshold=None):
    """``o3d_helper.post_process_mesh`` (src/utils/o3d_helper.py:220-241; called at run_e2e.py:278, 293 with
    ``vertex_threshold = voxel_size / 4``): merge close vertices, drop degenerate and duplicated triangles and
    unreferenced / duplicated vertices, one pass of simple Laplacian smoothing.  A one-off at the end of a run, on the
    host like the reference's (Open3D on the CPU there; numpy + scipy here).

    PARITY UNPINNED: Open3D is not in the image.  Restated from its documented behaviour [from memory of Open3D 0.14]:
    ``merge_close_vertices(eps)`` replaces every cluster of vertices closer than ``eps`` by its mean -- here a cluster
    is a connected component of the "closer than eps" graph, Open3D grows clusters greedily in vertex order, which
    differs where chains of near vertices exist; ``filter_smooth_simple(1)``: v <- (v + sum of its edge neighbours) /
    (1 + their number).  Unreferenced vertices: the reference's Open3D chain does NOT drop them (its
    ``remove_unreferenced_vertices`` call is commented out, o3d_helper.py:230) but hands the result to
    ``trimesh.Trimesh(vertices, faces)`` with the default ``process=True``, whose vertex merge keeps referenced vertices
    only [from memory of trimesh 3.x] -- so they are dropped here; against Open3D's intermediate mesh the vertex count and
    the face indices can therefore differ (same surface).

    ``surface_threshold``: None, or an area -- connected components whose surface is below it are then removed after
    the smoothing pass, and the vertices only they reference go with them (the reference's commented block,
    o3d_helper.py:232-236).  Areas are taken on this function's own float32 output: the call equals
    ``remove_small_components(post_process_mesh(mesh, eps), min_area=surface_threshold)`` bit for bit.  The default is
    None because the reference's live code does not filter, and its 0.1 m^2 was never validated by anyone.
    -> a new TriMesh."""
    if surface_threshold is not None:
        _check_filter_args("post_process_mesh", surface_threshold, 0, None)
        return remove_small_components(post_process_mesh(mesh, vertex_threshold), min_area=surface_threshold)
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    v = np.asarray(mesh.vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(mesh.faces, dtype=np.int64).reshape(-1, 3)
    if len(v) == 0 or len(f) == 0:
        return TriMesh(v, f)
    # exact duplicates first (neighbouring voxels repeat the vertices on their common lattice edges): far fewer points
    u, inv = np.unique(v.round(9), axis=0, return_inverse=True)
    pairs = cKDTree(u).query_pairs(float(vertex_threshold), output_type="ndarray")
    n = len(u)
    g = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    n_c, lab = connected_components(g, directed=False)
    cnt = np.bincount(lab, minlength=n_c).astype(np.float64)
    vm = np.stack([np.bincount(lab, weights=u[:, a], minlength=n_c) / cnt for a in range(3)], 1)
    f = lab[inv.reshape(-1)][f]
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]               # degenerate triangles
    if len(f):                                                                               # duplicated triangles:
        lo = np.argmin(f, axis=1)                                                            # the same cyclic order
        rot = np.take_along_axis(f, (lo[:, None] + np.arange(3)[None]) % 3, axis=1)
        _, first = np.unique(rot, axis=0, return_index=True)
        f = f[np.sort(first)]
    used = np.unique(f)
    remap = np.full(n_c, -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    vm, f = vm[used], remap[f]
    # one pass of filter_smooth_simple: neighbours along triangle edges, every neighbour once
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.unique(np.sort(e, axis=1), axis=0)
    m = len(vm)
    adj = coo_matrix((np.ones(2 * len(e)), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))),
                     shape=(m, m)).tocsr()
    deg = np.asarray(adj.sum(1)).reshape(-1)
    vs = (vm + adj @ vm) / (1.0 + deg)[:, None]
    return TriMesh(vs.astype(np.float32), f)


_POST_EXTENT_LIMIT = 2.0 ** 29   # |x| / eps below it: the device neighbour grid is exact (bnv_fusion.h: 2^30 on u)


def _upload(mesh, device):
    """A TriMesh -> (vertices [V, 3] float32, faces [T, 3] int64) on ``device``."""
    return (torch.from_numpy(np.ascontiguousarray(mesh.vertices, dtype=np.float32)).to(device),
            torch.from_numpy(np.ascontiguousarray(mesh.faces, dtype=np.int64)).to(device))


def _workspace(query, dev, *sizes):
    """The workspace a ``bnv_*_workspace_bytes`` entry asks for at ``sizes`` -> (uint8 tensor on ``dev``, its bytes)."""
    need = C.c_int64()
    _lib.check(getattr(_lib.load(), query)(*sizes, C.byref(need)), query)
    return torch.empty(int(need.value), dtype=torch.uint8, device=dev), int(need.value)


def post_process_mesh_tensors(vertices, faces, vertex_threshold=0.005, surface_threshold=None):
    """``post_process_mesh`` on the device (csrc/meshpost.hip; include/bnv_fusion.h, "Mesh post-processing"):
    vertices [V, 3] float32 and faces [T, 3] int64 on the GPU -> (vertices [V', 3] float32, faces [T', 3] int64) on the
    same device, bit for bit what the host function returns.  The only host reads: one for the input checks, one for
    the two output counts (with ``surface_threshold`` a third: the filter's two counts; its input is this function's
    own output, whose size the kernels need on the host).  Raises ValueError on CPU tensors, wrong shapes or dtypes, face indices outside [0, V),
    non-finite vertices, a negative or non-finite threshold, or coordinates beyond 2^29 thresholds.
    ``surface_threshold``: None (the default: the reference's live code does not filter, and its 0.1 m^2 was never
    validated by anyone), or the area below which connected components of the result are removed
    (the device filter of remove_small_components_tensors on this function's own output)."""
    who = "post_process_mesh_tensors"
    if surface_threshold is not None:
        min_area, _, _ = _check_filter_args(who, surface_threshold, 0, None)
        v_out, f_out = post_process_mesh_tensors(vertices, faces, vertex_threshold)
        return _filter_components(who, v_out, f_out, min_area, 0, 0)
    vertices, faces, V, T = _check_mesh_tensors(who, vertices, faces, "post_process_mesh")
    eps = float(vertex_threshold)
    if not (np.isfinite(eps) and eps >= 0.0):
        raise ValueError(f"post_process_mesh_tensors: vertex_threshold must be finite and >= 0 (got {eps})")
    dev = vertices.device
    if V == 0 and T == 0:
        return vertices.clone(), faces.clone()
    # one host read for every check: finite, face index range, extent against the neighbour grid
    checks = [torch.isfinite(vertices).all().to(torch.float64)]
    if V:
        checks.append(vertices.abs().max().to(torch.float64))
    if T:
        checks += [faces.min().to(torch.float64), faces.max().to(torch.float64)]
    got = torch.stack(checks).tolist()
    if not got[0]:
        raise ValueError("post_process_mesh_tensors: vertices must be finite")
    if T and (V == 0 or got[-2] < 0 or got[-1] >= V):
        raise ValueError(f"post_process_mesh_tensors: a face indexes a vertex outside [0, {V})")
    if V and eps > 0.0 and got[1] >= _POST_EXTENT_LIMIT * eps:
        raise ValueError(f"post_process_mesh_tensors: coordinates up to {got[1]:g} are beyond 2^29 vertex thresholds "
                         f"({eps:g}): the device neighbour grid would not be exact")
    lib = _lib.load()
    ws, need = _workspace("bnv_mesh_post_workspace_bytes", dev, V, T)
    with torch.cuda.device(dev):
        v_out = torch.empty((V, 3), dtype=torch.float32, device=dev)
        f_out = torch.empty((T, 3), dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(lib.bnv_mesh_post_process(_lib.ptr(vertices), V, _lib.ptr(faces), T, C.c_double(eps), _lib.ptr(ws),
                                             need, _lib.ptr(v_out), _lib.ptr(f_out), _lib.ptr(counts),
                                             _lib.stream_ptr()), "bnv_mesh_post_process")
        nv, nf = counts.tolist()                   # the one host read of the result: the mesh's size
    if nv < 0:
        raise _lib.BnvError("bnv_mesh_post_process rejected input that passed the host-side checks")
    return v_out[:nv], f_out[:nf]


def post_process_mesh_gpu(mesh, vertex_threshold=0.005, device="cuda:0", surface_threshold=None):
    """``post_process_mesh`` of a TriMesh on the GPU: the same TriMesh, bit for bit, through one upload and
    ``to_host``.  Same errors as post_process_mesh_tensors."""
    vs, fs = post_process_mesh_tensors(*_upload(mesh, device), vertex_threshold, surface_threshold=surface_threshold)
    return TriMesh(*to_host(vs, fs))


# ---- connected components (include/bnv_fusion.h, "Mesh components") -------------------------------------------------
_AREA_SCALE = 2.0 ** 50          # areas are summed as integers in units of 2^-50
_AREA_LIMIT = 2.0 ** 12          # total area below it: the integer sums stay below 2^62


def _check_filter_args(who, min_area, min_faces, keep_largest):
    a = float(min_area)
    if not (np.isfinite(a) and a >= 0.0):
        raise ValueError(f"{who}: the area threshold must be finite and >= 0 (got {a})")
    if int(min_faces) != min_faces or int(min_faces) < 0:
        raise ValueError(f"{who}: min_faces must be an integer >= 0 (got {min_faces})")
    if keep_largest is not None and (int(keep_largest) != keep_largest or int(keep_largest) < 1):
        raise ValueError(f"{who}: keep_largest must be None or an integer >= 1 (got {keep_largest})")
    return a, int(min_faces), 0 if keep_largest is None else int(keep_largest)


def _host_mesh(who, mesh):
    """A TriMesh's arrays with the checks the host functions share -> (v [V, 3] float32, f [T, 3] int64)."""
    v = np.asarray(mesh.vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(mesh.faces, dtype=np.int64).reshape(-1, 3)
    if not np.isfinite(v).all():
        raise ValueError(f"{who}: vertices must be finite")
    if len(f) and (len(v) == 0 or f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"{who}: a face indexes a vertex outside [0, {len(v)})")
    return v, f


def _face_cross64(v, f):
    """(b - a) x (c - a) per face -> (cx, cy, cz) [T] float64 from the float32 coordinates, one rounding per operation."""
    p = v.astype(np.float64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    e1, e2 = b - a, c - a
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return cx, cy, cz


def _face_area_units(v, f, who="connected_components", cross=None):
    """q [T] int64 = rint(area * 2^50) per face, one rounding per operation (``cross``: the caller's ``_face_cross64``)."""
    cx, cy, cz = cross if cross is not None else _face_cross64(v, f)
    area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    q = None if (area >= _AREA_LIMIT).any() else np.rint(area * _AREA_SCALE).astype(np.int64)
    if q is None or int((q >> 31).sum()) * 2 ** 31 + int((q & (2 ** 31 - 1)).sum()) >= 2 ** 62:
        raise ValueError(f"{who}: the mesh's total area reaches 2^12 square units")
    return q


def connected_components(mesh):
    """Connected components of a mesh's faces over shared edges (two faces are adjacent when they have an edge with the
    same two vertex indices), the block the reference keeps commented out in o3d_helper.post_process_mesh
    (src/utils/o3d_helper.py:232-236, ``cluster_connected_triangles``).  -> (labels [T] int32, numbered in ascending
    order of every component's smallest face; n_faces [C] int64; areas [C] float64: per-face areas in units of 2^-50
    summed as integers, so any order gives the same bits).  On the host, with numpy + scipy.

    PARITY UNPINNED: Open3D is not in the image; its clustering rule is restated from memory [Open3D 0.14].  Raises
    ValueError on a non-finite vertex, a face index outside [0, V), or a total area of 2^12 square units or more."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components as cc
    v, f = _host_mesh("connected_components", mesh)
    T = len(f)
    if T == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.float64)
    q = _face_area_units(v, f)
    ends = np.stack([f, np.roll(f, -1, axis=1)], -1).reshape(-1, 2)                  # [3T, 2]: (f0,f1), (f1,f2), (f2,f0)
    face = np.repeat(np.arange(T), 3)
    real = ends[:, 0] != ends[:, 1]
    key = (ends.min(1) << 32 | ends.max(1))[real]
    face = face[real]
    order = np.argsort(key, kind="stable")
    key, face = key[order], face[order]
    same = key[1:] == key[:-1]
    i, j = face[:-1][same], face[1:][same]
    g = coo_matrix((np.ones(len(i), dtype=np.int8), (i, j)), shape=(T, T))
    n_c, lab = cc(g, directed=False)
    first = np.full(n_c, T, dtype=np.int64)                                          # scipy numbers components in order
    np.minimum.at(first, lab, np.arange(T))                                          # of their smallest member already;
    lab = np.argsort(np.argsort(first, kind="stable"), kind="stable")[lab]           # make it hold whatever it does
    by = np.argsort(lab, kind="stable")
    starts = np.searchsorted(lab[by], np.arange(n_c))
    sums = np.add.reduceat(q[by], starts)
    return lab.astype(np.int32), np.bincount(lab, minlength=n_c).astype(np.int64), sums.astype(np.float64) / _AREA_SCALE


def _kept_components(n_faces, areas, min_area, min_faces, keep_largest):
    keep = (areas >= min_area) & (n_faces >= min_faces)
    if keep_largest:
        order = np.lexsort((np.arange(len(areas)), -areas))                          # area descending, label ascending
        top = np.zeros(len(areas), dtype=bool)
        top[order[:keep_largest]] = True
        keep &= top
    return keep


def remove_small_components(mesh, min_area=0.0, min_faces=0, keep_largest=None):
    """Drops the connected components (``connected_components``) that fail any of: area >= ``min_area`` (equality
    keeps; the reference's block removes ``component_surfaces < surface_threshold``), face count >= ``min_faces``,
    among the ``keep_largest`` largest by area over all components (None: no such test; ties go to the smaller label).
    Kept faces and the vertices they reference keep their order and their bits; every other vertex is dropped and the
    faces are renumbered.  Nothing kept, or no faces, gives an empty mesh.  -> a new TriMesh.  Host function; the device
    versions are remove_small_components_tensors / remove_small_components_gpu."""
    min_area, min_faces, k = _check_filter_args("remove_small_components", min_area, min_faces, keep_largest)
    labels, n_faces, areas = connected_components(mesh)
    v = np.asarray(mesh.vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(mesh.faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return TriMesh(v[:0], f)
    f = f[_kept_components(n_faces, areas, min_area, min_faces, k)[labels]]
    used = np.unique(f)
    remap = np.full(len(v), -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    return TriMesh(v[used], remap[f])


def _check_mesh_tensors(who, vertices, faces, host_name):
    """The checks the device mesh functions share -> (vertices, faces, V, T) contiguous and detached."""
    for name, t, dt in (("vertices", vertices, torch.float32), ("faces", faces, torch.int64)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{who}: {name} must be a GPU tensor (there is no CPU path; the host function is "
                             f"mesh.{host_name})")
        if t.dim() != 2 or t.shape[1] != 3 or t.dtype != dt:
            raise ValueError(f"{who}: {name} must be [N, 3] {dt} (got {list(t.shape)} {t.dtype})")
    if vertices.device != faces.device:
        raise ValueError(f"{who}: vertices and faces are on different devices")
    V, T = int(vertices.shape[0]), int(faces.shape[0])
    if V >= 2 ** 31 - 1 or T >= 2 ** 31 - 1:
        raise ValueError(f"{who}: {V} vertices / {T} faces: indices are int32 on the device")
    return vertices.detach().contiguous(), faces.detach().contiguous(), V, T


def _refused_component_input(who, vertices, faces, V, T):
    """The device refused the input (a count of -1): the ValueError that names why.  The kernels check finite vertices,
    the face index range and the total area themselves and report one word, so valid input pays for no check here."""
    got = [torch.isfinite(vertices).all()] + ([faces.min() < 0, faces.max() >= V] if T else [])
    got = torch.stack(got).tolist()
    if not got[0]:
        return ValueError(f"{who}: vertices must be finite")
    if T and (V == 0 or got[1] or got[2]):
        return ValueError(f"{who}: a face indexes a vertex outside [0, {V})")
    return ValueError(f"{who}: the mesh's total area reaches 2^12 square units")      # the one check left


def connected_components_tensors(vertices, faces):
    """``connected_components`` on the device (csrc/meshcomp.hip; include/bnv_fusion.h, "Mesh components"): vertices
    [V, 3] float32 and faces [T, 3] int64 on the GPU -> (labels [T] int32, n_faces [C] int64, areas [C] float64) on the
    same device, bit for bit what the host function returns.  One host read: C, which is -1 when the device's input
    checks refuse the mesh (a second read then finds which check to name).  Raises ValueError on CPU tensors, wrong shapes or dtypes, non-finite vertices, face indices outside [0, V), or a
    total area of 2^12 square units or more."""
    who = "connected_components_tensors"
    vertices, faces, V, T = _check_mesh_tensors(who, vertices, faces, "connected_components")
    dev = vertices.device
    lib = _lib.load()
    ws, need = _workspace("bnv_mesh_components_workspace_bytes", dev, V, T)
    with torch.cuda.device(dev):
        labels = torch.empty(T, dtype=torch.int32, device=dev)
        n_faces = torch.empty(T, dtype=torch.int64, device=dev)
        areas = torch.empty(T, dtype=torch.float64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(lib.bnv_mesh_components(_lib.ptr(vertices), V, _lib.ptr(faces), T, _lib.ptr(ws), need,
                                           _lib.ptr(labels), _lib.ptr(n_faces), _lib.ptr(areas), _lib.ptr(count),
                                           _lib.stream_ptr()), "bnv_mesh_components")
        n_c = int(count.item())                    # the one host read of the result: the number of components
    if n_c < 0:
        raise _refused_component_input(who, vertices, faces, V, T)
    return labels, n_faces[:n_c], areas[:n_c]


def _filter_components(who, vertices, faces, min_area, min_faces, k):
    """bnv_mesh_filter_components on checked tensors (_check_mesh_tensors) and arguments (_check_filter_args)."""
    V, T = int(vertices.shape[0]), int(faces.shape[0])
    dev = vertices.device
    lib = _lib.load()
    ws, need = _workspace("bnv_mesh_components_workspace_bytes", dev, V, T)
    with torch.cuda.device(dev):
        v_out = torch.empty((V, 3), dtype=torch.float32, device=dev)
        f_out = torch.empty((T, 3), dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(lib.bnv_mesh_filter_components(_lib.ptr(vertices), V, _lib.ptr(faces), T, C.c_double(min_area),
                                                  min_faces, k, _lib.ptr(ws), need, _lib.ptr(v_out), _lib.ptr(f_out),
                                                  _lib.ptr(counts), _lib.stream_ptr()), "bnv_mesh_filter_components")
        nv, nf = counts.tolist()                   # the one host read of the result: the mesh's size
    if nv < 0:
        raise _refused_component_input(who, vertices, faces, V, T)
    return v_out[:nv], f_out[:nf]


def remove_small_components_tensors(vertices, faces, min_area=0.0, min_faces=0, keep_largest=None):
    """``remove_small_components`` on the device: vertices [V, 3] float32 and faces [T, 3] int64 on the GPU ->
    (vertices [V', 3] float32, faces [T', 3] int64) on the same device, bit for bit what the host function returns.
    One host read: the two output counts, which are -1 when the device's input checks refuse the mesh (a second read
    then finds which check to name).  Raises ValueError like connected_components_tensors, and on a negative or
    non-finite ``min_area``, a negative ``min_faces`` or a ``keep_largest`` below 1."""
    who = "remove_small_components_tensors"
    min_area, min_faces, k = _check_filter_args(who, min_area, min_faces, keep_largest)
    vertices, faces, _, _ = _check_mesh_tensors(who, vertices, faces, "remove_small_components")
    return _filter_components(who, vertices, faces, min_area, min_faces, k)


def remove_small_components_gpu(mesh, min_area=0.0, min_faces=0, keep_largest=None, device="cuda:0"):
    """``remove_small_components`` of a TriMesh on the GPU: the same TriMesh, bit for bit, through one upload and
    ``to_host``.  Same errors as remove_small_components_tensors."""
    vs, fs = remove_small_components_tensors(*_upload(mesh, device), min_area, min_faces, keep_largest)
    return TriMesh(*to_host(vs, fs))


# ---- simplification (include/bnv_fusion.h, "Mesh simplification"; csrc/meshsimplify.hip) ----------------------------
_SIMPLIFY_EXTENT = 2.0 ** 20     # |x| / cell below it: every axis index fits 21 bits of the cell key
_SIMPLIFY_MAX_FACES = 2 ** 30    # corner ids 3 t + k fit 32 bits
_PLACEMENTS = {"quadric": 0, "mean": 1}     # BNV_SIMPLIFY_QUADRIC, BNV_SIMPLIFY_MEAN
_TARGET_RUNS = 16                # device runs of the bisection of simplify_mesh_gpu(target_faces=...)


def _check_simplify_args(who, cell, placement, min_det):
    if placement not in _PLACEMENTS:
        raise ValueError(f"{who}: placement must be 'quadric' or 'mean' (got {placement!r})")
    h, md = float(cell), float(min_det)
    if not (np.isfinite(h) and h > 0.0):
        raise ValueError(f"{who}: cell must be finite and > 0 (got {h})")
    if not (np.isfinite(md) and md >= 0.0):
        raise ValueError(f"{who}: min_det must be finite and >= 0 (got {md})")
    return h, md


def _ordered_sums(group, n_groups, values):
    """values [n, k] float64 summed per group one after another in the order given -> [n_groups, k].  Round r adds
    every group's r-th member at once: a group occurs once per round, so the sums keep their order."""
    order = np.argsort(group, kind="stable")
    g = group[order]
    rank = np.arange(len(g)) - np.searchsorted(g, g, "left")
    acc = np.zeros((n_groups, values.shape[1]))
    by_rank = np.argsort(rank, kind="stable")
    ends = np.searchsorted(rank[by_rank], np.arange(int(rank.max()) + 2 if len(rank) else 1))
    for r in range(len(ends) - 1):
        sel = by_rank[ends[r]:ends[r + 1]]
        acc[g[sel]] = acc[g[sel]] + values[order[sel]]
    return acc


def simplify_mesh(mesh, cell, placement="quadric", min_det=1e-3):
    """Simplifies a mesh by vertex clustering on a uniform grid of edge ``cell``: all vertices of a grid cell become
    one vertex, faces that collapse are dropped.  ``placement="quadric"`` puts the vertex where the planes of the
    faces around the cluster meet (the minimum of their area-weighted quadric, solved relative to the cell centre),
    which keeps edges and corners sharp; the position is taken only when the quadric is well conditioned --
    |det A| >= ``min_det`` (trace A / 3)^3, 1 for three orthogonal equal planes and 0 for a plane or a straight edge --
    and within the cell dilated to twice its size; otherwise, and always with ``placement="mean"``, the vertex is the
    mean of the cluster's vertices (on a plane or an edge the mean is on the surface already).  Faces: the face step
    of ``post_process_mesh`` (two equal clusters drop a face; of faces with the same cyclic triple the first stays;
    input order kept); vertices: the referenced clusters in ascending cell order; no smoothing.  A mesh without faces
    gives an empty mesh.  Host function in numpy: the path the device functions are held to bit for bit; the
    specification is include/bnv_fusion.h, "Mesh simplification".  Raises ValueError on non-finite vertices, a face
    index outside [0, V), a coordinate 2^20 cells or more from the origin, a non-finite or non-positive ``cell`` or a
    non-finite or negative ``min_det``.  -> a new TriMesh."""
    who = "simplify_mesh"
    h, min_det = _check_simplify_args(who, cell, placement, min_det)
    v, f = _host_mesh(who, mesh)
    V, T = len(v), len(f)
    if V >= 2 ** 31 - 1 or T > _SIMPLIFY_MAX_FACES:
        raise ValueError(f"{who}: {V} vertices / {T} faces: beyond 2^31 - 2 vertices or 2^30 faces")
    p = v.astype(np.float64)
    q = p / h
    if V and np.abs(q).max() >= _SIMPLIFY_EXTENT:
        raise ValueError(f"{who}: coordinates up to {np.abs(p).max():g} are 2^20 cells ({h:g}) or more from the origin")
    if V == 0 or T == 0:
        return TriMesh(v[:0], f[:0])
    idx = np.floor(q).astype(np.int64)
    key = (idx[:, 0] + 2 ** 20) << 42 | (idx[:, 1] + 2 ** 20) << 21 | (idx[:, 2] + 2 ** 20)
    keys, first, cl = np.unique(key, return_index=True, return_inverse=True)
    cl = cl.reshape(-1)
    n_c = len(keys)
    pos = _ordered_sums(cl, n_c, p) / np.bincount(cl, minlength=n_c).astype(np.float64)[:, None]
    if placement == "quadric":
        centre = (idx[first].astype(np.float64) + 0.5) * h                      # [n_c, 3]
        ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
        corner = np.flatnonzero(np.repeat(ok, 3))                               # ascending corner id 3 t + k
        fc = f[corner // 3]
        c = cl[fc[np.arange(len(corner)), corner % 3]]
        ctr = centre[c]
        p0, p1, p2 = p[fc[:, 0]] - ctr, p[fc[:, 1]] - ctr, p[fc[:, 2]] - ctr
        e1, e2 = p1 - p0, p2 - p0
        n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        L = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        live = L != 0.0
        c, p0, n0, n1, n2, L = c[live], p0[live], n0[live], n1[live], n2[live], L[live]
        u0, u1, u2 = n0 / L, n1 / L, n2 / L
        w = 0.5 * L
        d = -((u0 * p0[:, 0] + u1 * p0[:, 1]) + u2 * p0[:, 2])
        wu0, wu1, wu2, wd = w * u0, w * u1, w * u2, w * d
        Q = _ordered_sums(c, n_c, np.stack([wu0 * u0, wu0 * u1, wu0 * u2, wu1 * u1, wu1 * u2, wu2 * u2,
                                            wd * u0, wd * u1, wd * u2], 1))
        a00, a01, a02, a11, a12, a22, b0, b1, b2 = Q.T
        c00 = a11 * a22 - a12 * a12
        c01 = a02 * a12 - a01 * a22
        c02 = a01 * a12 - a02 * a11
        c11 = a00 * a22 - a02 * a02
        c12 = a01 * a02 - a00 * a12
        c22 = a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        tr = (a00 + a11) + a22
        r0, r1, r2 = -b0, -b1, -b2
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):     # det = 0: x infinite or NaN, refused
            x = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                          ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1)
            m = tr / 3.0
            take = (tr > 0.0) & (np.abs(det) >= min_det * ((m * m) * m)) & (np.abs(x) <= h).all(1)
        pos[take] = centre[take] + x[take]
    fcl = cl[f]
    fcl = fcl[(fcl[:, 0] != fcl[:, 1]) & (fcl[:, 1] != fcl[:, 2]) & (fcl[:, 0] != fcl[:, 2])]
    if len(fcl):
        lo = np.argmin(fcl, axis=1)
        rot = np.take_along_axis(fcl, (lo[:, None] + np.arange(3)[None]) % 3, axis=1)
        _, keep = np.unique(rot, axis=0, return_index=True)
        fcl = fcl[np.sort(keep)]
    used = np.unique(fcl)
    remap = np.full(n_c, -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    return TriMesh(pos[used].astype(np.float32), remap[fcl])


def simplify_mesh_tensors(vertices, faces, cell, placement="quadric", min_det=1e-3):
    """``simplify_mesh`` on the device (csrc/meshsimplify.hip; include/bnv_fusion.h, "Mesh simplification"): vertices
    [V, 3] float32 and faces [T, 3] int64 on the GPU -> (vertices [V', 3] float32, faces [T', 3] int64) on the same
    device, bit for bit what the host function returns.  The only host reads: one for the input checks, one for the
    two output counts.  Raises ValueError on CPU tensors, wrong shapes or dtypes, more than 2^30 faces, and on
    everything ``simplify_mesh`` refuses."""
    who = "simplify_mesh_tensors"
    h, min_det = _check_simplify_args(who, cell, placement, min_det)
    vertices, faces, V, T = _check_mesh_tensors(who, vertices, faces, "simplify_mesh")
    if T > _SIMPLIFY_MAX_FACES:
        raise ValueError(f"{who}: {T} faces: corner ids are 32 bits on the device (2^30 faces at most)")
    dev = vertices.device
    # one host read for every check: finite, face index range, extent against the cell keys
    checks = [torch.isfinite(vertices).all().to(torch.float64)]
    if V:
        checks.append(vertices.abs().max().to(torch.float64))
    if T:
        checks += [faces.min().to(torch.float64), faces.max().to(torch.float64)]
    got = torch.stack(checks).tolist()
    if not got[0]:
        raise ValueError(f"{who}: vertices must be finite")
    if T and (V == 0 or got[-2] < 0 or got[-1] >= V):
        raise ValueError(f"{who}: a face indexes a vertex outside [0, {V})")
    if V and got[1] / h >= _SIMPLIFY_EXTENT:
        raise ValueError(f"{who}: coordinates up to {got[1]:g} are 2^20 cells ({h:g}) or more from the origin")
    lib = _lib.load()
    ws, need = _workspace("bnv_mesh_simplify_bytes", dev, V, T)
    with torch.cuda.device(dev):
        v_out = torch.empty((V, 3), dtype=torch.float32, device=dev)
        f_out = torch.empty((T, 3), dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(lib.bnv_mesh_simplify(_lib.ptr(vertices), V, _lib.ptr(faces), T, C.c_double(h),
                                         _PLACEMENTS[placement], C.c_double(min_det), _lib.ptr(ws), need,
                                         _lib.ptr(v_out), _lib.ptr(f_out), _lib.ptr(counts), _lib.stream_ptr()),
                   "bnv_mesh_simplify")
        nv, nf = counts.tolist()                   # the one host read of the result: the mesh's size
    if nv < 0:
        raise _lib.BnvError("bnv_mesh_simplify rejected input that passed the host-side checks")
    return v_out[:nv], f_out[:nf]


def simplify_mesh_gpu(mesh, cell=None, target_faces=None, placement="quadric", min_det=1e-3, device="cuda:0"):
    """``simplify_mesh`` of a TriMesh on the GPU: the same TriMesh, bit for bit, through one upload and ``to_host``.
    Exactly one of ``cell`` and ``target_faces`` is given.  ``target_faces``: the cell is searched on the host by a
    geometric bisection between extent / 2^19 and extent (extent: the largest |coordinate|), 16 device runs, and the
    run with the most faces not above the target is returned -- AT MOST ``target_faces`` faces, not the closest count:
    the face count is not strictly monotone in the cell, and when even the coarsest run tried is above the target the
    result is the empty mesh a single cell gives.  Same errors as simplify_mesh_tensors."""
    who = "simplify_mesh_gpu"
    if (cell is None) == (target_faces is None):
        raise ValueError(f"{who}: give exactly one of cell and target_faces")
    vt, ft = _upload(mesh, device)
    if cell is not None:
        return TriMesh(*to_host(*simplify_mesh_tensors(vt, ft, cell, placement, min_det)))
    if int(target_faces) != target_faces or int(target_faces) < 0:
        raise ValueError(f"{who}: target_faces must be an integer >= 0 (got {target_faces})")
    _check_simplify_args(who, 1.0, placement, min_det)
    extent = float(vt.abs().max()) if vt.numel() else 0.0
    best = (vt[:0], ft[:0])
    if np.isfinite(extent) and extent > 0.0:
        lo, hi = extent / 2.0 ** 19, extent
        for _ in range(_TARGET_RUNS):
            mid = float(np.sqrt(lo * hi))
            got = simplify_mesh_tensors(vt, ft, mid, placement, min_det)
            if len(got[1]) <= int(target_faces):
                hi = mid
                if len(got[1]) >= len(best[1]):
                    best = got
            else:
                lo = mid
    elif not np.isfinite(extent):
        raise ValueError(f"{who}: vertices must be finite")
    return TriMesh(*to_host(*best))


# ---- vertex normals and colours (include/bnv_fusion.h, "Mesh normals and colours"; csrc/meshcolor.hip) --------------
_NORMAL_SCALE = 2.0 ** 48        # cross products are summed as integers in units of 2^-48
COLOR_MAX_FRAMES = 8             # BNV_MESH_COLOR_MAX_FRAMES
DEFAULT_FILL = (128, 128, 128)


def vertex_normals(mesh):
    """Area-weighted vertex normals of a TriMesh on the host -> float32 [V, 3], unit length, or (0, 0, 0) for a vertex
    no face references, that only degenerate faces touch, or whose faces cancel.  Per face the cross product
    (b - a) x (c - a) in float64 from the float32 coordinates (``_face_cross64``), quantised
    to rint(x * 2^48) and summed per vertex as int64: the order of the faces does not matter.  The same bits as
    ``vertex_normals_tensors``.  Raises ValueError on a non-finite vertex, a face index outside [0, V) or a total area
    of 2^12 square units or more."""
    v, f = _host_mesh("vertex_normals", mesh)
    out = np.zeros((len(v), 3), dtype=np.float32)
    if len(f) == 0:
        return out
    cross = _face_cross64(v, f)
    _face_area_units(v, f, "vertex_normals", cross)
    q = np.rint(np.stack(cross, axis=1) * _NORMAL_SCALE).astype(np.int64)
    sums = np.zeros(out.shape, dtype=np.int64)
    for k in range(3):
        np.add.at(sums, f[:, k], q)
    some = (sums != 0).any(axis=1)
    s = sums[some].astype(np.float64)
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    out[some] = (s / length[:, None]).astype(np.float32)
    return out


def vertex_normals_tensors(vertices, faces):
    """``vertex_normals`` on the device: vertices [V, 3] float32 and faces [T, 3] int64 on the GPU -> normals [V, 3]
    float32 on the same device, bit for bit what the host function returns.  One host read: the status word, -1 when
    the device's input checks refuse the mesh (a second read then finds which check to name).  Raises ValueError like
    connected_components_tensors."""
    who = "vertex_normals_tensors"
    vertices, faces, V, T = _check_mesh_tensors(who, vertices, faces, "vertex_normals")
    dev = vertices.device
    if V == 0:
        if T:
            raise ValueError(f"{who}: a face indexes a vertex outside [0, 0)")
        return torch.zeros((0, 3), dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws, need = _workspace("bnv_mesh_normals_workspace_bytes", dev, V)
    with torch.cuda.device(dev):
        out = torch.empty((V, 3), dtype=torch.float32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(lib.bnv_mesh_vertex_normals(_lib.ptr(vertices), V, _lib.ptr(faces), T, _lib.ptr(ws), need,
                                               _lib.ptr(out), _lib.ptr(status), _lib.stream_ptr()),
                   "bnv_mesh_vertex_normals")
        refused = int(status.item()) < 0           # the one host read of the result
    if refused:
        raise _refused_component_input(who, vertices, faces, V, T)
    return out


def _host_matrix(x, shape, what):
    m = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    m = np.asarray(m, dtype=np.float64)
    if m.size != shape[0] * shape[1]:
        raise ValueError(f"{what} must be {shape[0]}x{shape[1]} (got {list(m.shape)})")
    return m.reshape(shape)


def world_to_camera(T_wc):
    """The world-to-camera matrix of a camera-to-world pose, inverted in float64 on the host -> float64 [4, 4]: what
    ``VertexColorer`` hands to bnv_mesh_color_accumulate (and tests/mesh_color_restatement.py restates with)."""
    return np.linalg.inv(_host_matrix(T_wc, (4, 4), "T_wc"))


class VertexColorer:
    """Colours the vertices of a mesh from RGB-D frames on the device (csrc/meshcolor.hip; include/bnv_fusion.h, "Mesh
    normals and colours"): every vertex is projected into every frame, tested against the frame's own depth image
    (``depth_tol``: background pixels at a silhouette and frames in which the vertex is hidden contribute nothing),
    weighted by ``cos / z^2`` of the view (``cos_min`` drops back-facing and grazing views) and sampled bilinearly from
    the full-resolution colour image.

    ``vertices`` [V, 3] float32 and ``faces`` [T, 3] int64 on the GPU; ``normals`` [V, 3] float32 (default:
    ``vertex_normals_tensors``).  ``add(frames)`` may be called any number of times -- key frames can be streamed from
    disk -- and the result does not depend on how the frames are split over calls."""

    def __init__(self, vertices, faces, normals=None, depth_tol=0.02, cos_min=0.2, near=0.0, max_depth=3.0):
        who = "VertexColorer"
        vertices, faces, V, _ = _check_mesh_tensors(who, vertices, faces, "vertex_normals")
        if V == 0:
            raise ValueError(f"{who}: the mesh has no vertices")
        self.depth_tol, self.cos_min, self.near, self.max_depth = (float(depth_tol), float(cos_min), float(near),
                                                                   float(max_depth))
        if not (np.isfinite(self.depth_tol) and self.depth_tol >= 0.0):
            raise ValueError(f"{who}: depth_tol must be finite and >= 0 (got {depth_tol})")
        if not 0.0 <= self.cos_min < 1.0:
            raise ValueError(f"{who}: cos_min must lie in [0, 1) (got {cos_min})")
        if not (np.isfinite(self.near) and self.near >= 0.0 and np.isfinite(self.max_depth)
                and self.max_depth > self.near):
            raise ValueError(f"{who}: need 0 <= near < max_depth, both finite (got {near}, {max_depth})")
        if normals is None:
            normals = vertex_normals_tensors(vertices, faces)
        elif not (torch.is_tensor(normals) and normals.device == vertices.device and normals.dtype == torch.float32
                  and tuple(normals.shape) == (V, 3)):
            raise ValueError(f"{who}: normals must be [{V}, 3] float32 on {vertices.device}")
        self.vertices, self.faces, self.normals = vertices, faces, normals.detach().contiguous()
        self.device, self.n_vertices, self.n_frames = vertices.device, V, 0
        self._lib = _lib.load()
        self._ws, self._ws_bytes = _workspace("bnv_mesh_color_workspace_bytes", self.device, V)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bnv_mesh_color_begin(_lib.ptr(self._ws), self._ws_bytes, V, _lib.stream_ptr()),
                       "bnv_mesh_color_begin")

    def _image(self, x, what):
        if torch.is_tensor(x):
            return x.detach().to(self.device).contiguous(), what
        x = np.ascontiguousarray(x)
        if x.dtype == np.uint16:                       # (uploaded as int32: from_numpy takes no uint16 everywhere)
            return torch.from_numpy(x.astype(np.int32)).to(self.device).to(torch.uint16), what
        return torch.from_numpy(x).to(self.device), what

    def _frame(self, frame):
        """A frame dict -> (bnv_mesh_color_frame_t, the tensors it points into)."""
        who = f"VertexColorer.add: frame {frame.get('frame_id')!r}"
        if frame.get("rgb") is None:
            raise ValueError(f"{who} has no 'rgb'")
        depth, _ = self._image(frame["depth"], "depth")
        if depth.dtype in (torch.uint16, torch.int16):
            dtype = 0
        elif depth.dtype == torch.float32:
            dtype = 1
        else:
            raise ValueError(f"{who}: depth must be uint16 millimetres or float32 metres (got {depth.dtype})")
        if depth.dim() < 2 or depth.numel() != depth.shape[-2] * depth.shape[-1] or depth.numel() == 0:
            raise ValueError(f"{who}: depth must be one [H, W] image (got {list(depth.shape)})")
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        rgb, _ = self._image(frame["rgb"], "rgb")
        if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3 or rgb.numel() == 0:
            raise ValueError(f"{who}: rgb must be uint8 [H, W, 3] (got {rgb.dtype} {list(rgb.shape)})")
        Hc, Wc = int(rgb.shape[0]), int(rgb.shape[1])
        K = _host_matrix(frame["intr_mat"], (3, 3), "intr_mat")
        if frame.get("rgb_intr_mat") is not None:
            Kc = _host_matrix(frame["rgb_intr_mat"], (3, 3), "rgb_intr_mat")
        elif (Hc, Wc) == (H, W):
            Kc = K
        else:
            raise ValueError(f"{who}: rgb is {Hc}x{Wc}, depth {H}x{W}: a colour image of its own size needs "
                             "'rgb_intr_mat'")
        T_wc = _host_matrix(frame["T_wc"], (4, 4), "T_wc")
        T_cw = world_to_camera(T_wc)
        keep = [depth, rgb]
        conf_ptr, level = None, 0
        if frame.get("conf") is not None:
            conf, _ = self._image(frame["conf"], "conf")
            if conf.dtype != torch.uint8 or conf.numel() != H * W:
                raise ValueError(f"{who}: conf must be uint8 [{H}, {W}] (got {conf.dtype} {list(conf.shape)})")
            keep.append(conf)
            conf_ptr, level = conf.data_ptr(), int(frame.get("conf_level", 0))
        f = _lib.MeshColorFrame()
        f.depth, f.conf, f.rgb = depth.data_ptr(), conf_ptr, rgb.data_ptr()
        f.depth_dtype, f.conf_level = dtype, level
        f.height, f.width, f.color_height, f.color_width = H, W, Hc, Wc
        f.K[:] = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
        f.K_color[:] = [Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]]
        f.T_cw[:] = T_cw[:3].reshape(-1).tolist()
        f.center[:] = T_wc[:3, 3].tolist()
        return f, keep

    def _launch(self, batch):
        frames = (_lib.MeshColorFrame * len(batch))(*[f for f, _ in batch])
        with torch.cuda.device(self.device):
            _lib.check(self._lib.bnv_mesh_color_accumulate(
                _lib.ptr(self.vertices), _lib.ptr(self.normals), self.n_vertices, frames, len(batch), self.depth_tol,
                self.cos_min, self.near, self.max_depth, _lib.ptr(self._ws), self._ws_bytes, _lib.stream_ptr()),
                "bnv_mesh_color_accumulate")
        self.n_frames += len(batch)

    def add(self, frames):
        """Adds frames (an iterable of the dicts ``NeuralMap`` takes -- ``depth`` uint16 millimetres or float32 metres,
        ``intr_mat``, ``T_wc`` -- plus ``rgb`` uint8 [Hc, Wc, 3]; optional ``rgb_intr_mat`` for a colour image of its
        own size, ``conf`` / ``conf_level``), ``COLOR_MAX_FRAMES`` per launch.  A frame without ``rgb`` raises
        ValueError naming its ``frame_id``.  -> self"""
        if isinstance(frames, dict):
            frames = [frames]
        batch = []
        for frame in frames:
            batch.append(self._frame(frame))
            if len(batch) == COLOR_MAX_FRAMES:
                self._launch(batch)
                batch = []
        if batch:
            self._launch(batch)
        return self

    def result(self, fill=DEFAULT_FILL, return_weights=False):
        """-> (colors uint8 [V, 3], observed bool [V][, sum_w float64 [V], count int32 [V]]) on the device: the weighted
        mean of the samples, rounded half to even; vertices no frame contributed to get ``fill``."""
        fill = [int(c) for c in fill]
        if len(fill) != 3 or not all(0 <= c <= 255 for c in fill):
            raise ValueError(f"VertexColorer.result: fill must be three values in [0, 255] (got {fill})")
        V = self.n_vertices
        with torch.cuda.device(self.device):
            colors = torch.empty((V, 3), dtype=torch.uint8, device=self.device)
            observed = torch.empty(V, dtype=torch.uint8, device=self.device)
            sum_w = torch.empty(V, dtype=torch.float64, device=self.device) if return_weights else None
            count = torch.empty(V, dtype=torch.int32, device=self.device) if return_weights else None
            _lib.check(self._lib.bnv_mesh_color_resolve(_lib.ptr(self._ws), self._ws_bytes, V, (C.c_uint8 * 3)(*fill),
                                                        _lib.ptr(colors), _lib.ptr(observed), _lib.ptr(sum_w),
                                                        _lib.ptr(count), _lib.stream_ptr()), "bnv_mesh_color_resolve")
        observed = observed.bool()
        return (colors, observed, sum_w, count) if return_weights else (colors, observed)


def color_vertices(mesh_or_tensors, frames, fill=DEFAULT_FILL, return_weights=False, device="cuda:0", **kw):
    """``VertexColorer`` in one call.  ``mesh_or_tensors``: (vertices, faces) device tensors -> what
    ``VertexColorer.result`` returns; or a TriMesh (uploaded to ``device``) -> the same TriMesh with ``vertex_normals``
    and ``vertex_colors`` set, and ``(mesh, observed[, sum_w, count])`` as host arrays.  ``kw``: ``normals``,
    ``depth_tol``, ``cos_min``, ``near``, ``max_depth``."""
    if isinstance(mesh_or_tensors, TriMesh):
        m = mesh_or_tensors
        colorer = VertexColorer(*_upload(m, device), **kw).add(frames)
        out = colorer.result(fill, return_weights)
        host = to_host(colorer.normals, out[0], out[1].to(torch.uint8), *out[2:])
        m.vertex_normals, m.vertex_colors = host[0], host[1]
        return (m, host[2].astype(bool)) + tuple(host[3:])
    vertices, faces = mesh_or_tensors
    return VertexColorer(vertices, faces, **kw).add(frames).result(fill, return_weights)


_PLY_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
                "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
                "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
_PLY_COUNT_TYPES = ("uchar", "uint8")
_PLY_INDEX_TYPES = ("int", "uint", "int32", "uint32")


def _fan(polys):
    """Polygons (lists of vertex indices) -> triangles, each polygon as a fan around its first vertex."""
    tris = []
    for p in polys:
        if len(p) < 3:
            raise ValueError(f"PLY face with {len(p)} vertices")
        for k in range(1, len(p) - 1):
            tris.append((p[0], p[k], p[k + 1]))
    return tris


def load_ply(path):
    """PLY -> TriMesh: ASCII or binary little-endian, as ``TriMesh.export`` and most ground-truth meshes are written.
    Vertices: ``float`` / ``double`` x, y, z, possibly with further scalar properties, which are read past -- except
    ``nx ny nz`` and ``uchar red green blue``, which become ``vertex_normals`` / ``vertex_colors`` of the result.  Faces: ``property list uchar|uint8 int|uint|int32|uint32 vertex_indices`` (or
    ``vertex_index``); quads and larger polygons are triangulated as fans.  Anything else -- big-endian data, list
    properties on vertices, extra face properties, other elements with data -- fails with a ValueError naming it."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    nl = data.find(b"\n", end)
    body = data[nl + 1:]
    fmt = None
    elements = []                      # [name, count, [(prop name, dtype) | (name, ("list", count dtype, item dtype))]]
    for raw in data[:end].decode("ascii", "replace").splitlines()[1:]:
        tok = raw.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            if tok[1] == "list":
                elements[-1][2].append((tok[4], ("list", tok[2], tok[3])))
            else:
                if tok[1] not in _PLY_SCALARS:
                    raise ValueError(f"{path}: unknown PLY property type {tok[1]!r}")
                elements[-1][2].append((tok[2], tok[1]))
        else:
            raise ValueError(f"{path}: unexpected PLY header line {raw!r}")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii and binary_little_endian are)")
    verts, faces = None, np.zeros((0, 3), dtype=np.int64)
    normals = colors = None
    pos = 0                                           # binary: byte offset into body
    lines = body.decode("ascii").split("\n") if fmt == "ascii" else None
    li = 0                                            # ascii: next line
    for name, count, props in elements:
        if name == "vertex":
            if any(isinstance(t, tuple) for _, t in props):
                raise ValueError(f"{path}: list property on vertices")
            names = [n for n, _ in props]
            if names[:3] != ["x", "y", "z"] or any(t not in ("float", "float32", "double", "float64") for _, t in props[:3]):
                raise ValueError(f"{path}: vertices must start with float or double x, y, z (got {props[:3]})")
            if fmt == "ascii":
                rows = [ln.split() for ln in lines[li:li + count]]
                li += count
                verts = np.array([[float(r[0]), float(r[1]), float(r[2])] for r in rows], dtype=np.float64).reshape(-1, 3)
                cols = {n: np.array([float(r[k]) for r in rows], dtype=np.float64) for k, n in enumerate(names)}
            else:
                dt = np.dtype([(n, "<" + _PLY_SCALARS[t]) for n, t in props])
                rec = np.frombuffer(body, dtype=dt, count=count, offset=pos)
                pos += dt.itemsize * count
                verts = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float64)
                cols = {n: rec[n] for n in names}
            if all(n in names for n in ("nx", "ny", "nz")):
                normals = np.stack([cols["nx"], cols["ny"], cols["nz"]], axis=1).astype(np.float32).reshape(-1, 3)
            if all(n in names and dict(props)[n] in ("uchar", "uint8") for n in ("red", "green", "blue")):
                colors = np.stack([cols["red"], cols["green"], cols["blue"]], axis=1).astype(np.uint8).reshape(-1, 3)
        elif name == "face":
            if len(props) != 1 or not isinstance(props[0][1], tuple) or props[0][0] not in ("vertex_indices",
                                                                                             "vertex_index"):
                raise ValueError(f"{path}: faces must carry exactly one list property vertex_indices (got {props})")
            _, ct, it = props[0][1]
            if ct not in _PLY_COUNT_TYPES or it not in _PLY_INDEX_TYPES:
                raise ValueError(f"{path}: face list 'list {ct} {it}' is not supported (list uchar|uint8 "
                                 "int|uint|int32|uint32)")
            if fmt == "ascii":
                polys = []
                for ln in lines[li:li + count]:
                    r = [int(x) for x in ln.split()]
                    if len(r) < 1 or len(r) != r[0] + 1:
                        raise ValueError(f"{path}: malformed face line {ln!r}")
                    polys.append(r[1:])
                li += count
            else:
                idt = np.dtype("<" + _PLY_SCALARS[it])
                buf = memoryview(body)
                tri = np.dtype([("n", "u1"), ("i", idt, 3)])
                # fast path: every face a triangle
                if count and pos + tri.itemsize * count <= len(body):
                    rec = np.frombuffer(body, dtype=tri, count=count, offset=pos)
                    if np.all(rec["n"] == 3):
                        faces = rec["i"].astype(np.int64)
                        pos += tri.itemsize * count
                        continue
                polys = []
                for _ in range(count):
                    k = buf[pos]
                    pos += 1
                    polys.append(np.frombuffer(body, dtype=idt, count=k, offset=pos).astype(np.int64).tolist())
                    pos += k * idt.itemsize
            faces = np.array(_fan(polys), dtype=np.int64).reshape(-1, 3)
        else:
            if count == 0:
                continue
            raise ValueError(f"{path}: PLY element {name!r} with data is not supported")
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError(f"{path}: a face indexes a vertex that does not exist")
    out = TriMesh(verts.astype(np.float32), faces)
    out.vertex_normals, out.vertex_colors = normals, colors
    return out


def load_obj(path):
    """Wavefront OBJ -> TriMesh (ShapeNet's format): ``v x y z`` and ``f`` records only, everything else (normals,
    texture coordinates, groups, materials) is read past.  Face corners may be ``a``, ``a/b``, ``a//c`` or ``a/b/c``
    (the vertex index is the first field); indices are 1-based, negative ones count back from the vertices read so
    far; quads and larger polygons are triangulated as fans."""
    verts, polys = [], []
    with open(path, "r", errors="replace") as fh:
        for no, raw in enumerate(fh, 1):
            tok = raw.split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError(f"{path}:{no}: vertex with {len(tok) - 1} coordinates")
                verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
            elif tok[0] == "f":
                poly = []
                for corner in tok[1:]:
                    i = int(corner.split("/")[0])
                    i = i - 1 if i > 0 else len(verts) + i
                    if i < 0 or i >= len(verts):
                        raise ValueError(f"{path}:{no}: face corner {corner!r} indexes a vertex that does not exist")
                    poly.append(i)
                if len(poly) < 3:
                    raise ValueError(f"{path}:{no}: face with {len(poly)} vertices")
                polys.append(poly)
    if not verts:
        raise ValueError(f"{path}: no vertices")
    return TriMesh(np.array(verts, dtype=np.float64).reshape(-1, 3).astype(np.float32),
                   np.array(_fan(polys), dtype=np.int64).reshape(-1, 3))
