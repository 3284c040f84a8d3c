"""TSDF mesh extraction without a GPU: the reference's PLY writers (third_parties/fusion.py:366-426), a numpy
restatement of the dense marching cubes of csrc/mesh.hip (k_tm_*) with its topology checked on analytic surfaces, and
the argument checks of the bnv_tsdf_mesh_* C entries (before any HIP call).

``restate_mesh`` is written from the conventions of include/bnv_fusion.h (bnv_tsdf_mesh_*), not from the reference: the
reference calls skimage's marching_cubes_lewiner (fusion.py:327) and then maps the vertices to world coordinates
(fusion.py:330) and reads their colours (fusion.py:331-337).  tests/test_gpu_tsdf_mesh.py holds the kernels to it."""
import ctypes as C

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

F32 = np.float32


def _empty():
    return (np.zeros((0, 3), F32), np.zeros((0, 3), np.int64), np.zeros((0, 3), F32), np.zeros((0, 3), np.uint8))


def restate_mesh(tsdf, weight=None, color=None, origin=(0.0, 0.0, 0.0), voxel=1.0, level=0.0, observed_only=False):
    """-> (vertices f32 [V, 3], faces i64 [T, 3], normals f32 [V, 3], colors u8 [V, 3]) for an [X, Y, Z] volume.

    Cells are based at grid points; corner c = 4 dx + 2 dy + dz; case bit c set when tsdf < level; triangles from
    mc_tables.TRI_TABLE.  The vertices are the edges the emitted triangles use, keyed (linear index of the lower grid
    point, axis) and sorted; faces in (cell linear index, table slot) order."""
    from bnv_fusion_amd.mc_tables import CORNERS, EDGE_CORNERS, N_TRI, TRI_TABLE
    tsdf = np.ascontiguousarray(tsdf, dtype=F32)
    X, Y, Z = tsdf.shape
    if min(X, Y, Z) < 2:
        return _empty()
    lev = F32(level)
    inside = tsdf < lev
    case = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    on = np.ones((X - 1, Y - 1, Z - 1), bool)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        case |= inside[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.int64) << c
        if observed_only:
            on &= np.asarray(weight, F32)[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz] > 0
    ntri = np.where(on, N_TRI[case], 0).reshape(-1)
    cells = np.nonzero(ntri)[0]                       # ascending: the cell grid is ordered like the volume
    if len(cells) == 0:
        return _empty()
    cnt = ntri[cells]
    cell_of = np.repeat(cells, cnt)
    slot = np.arange(len(cell_of)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ci, cj, ck = np.unravel_index(cell_of, (X - 1, Y - 1, Z - 1))
    base = (ci * Y + cj) * Z + ck                     # linear index of the cell's base grid point
    cs = case.reshape(-1)[cell_of]
    edges = np.stack([TRI_TABLE[cs, 3 * slot + q] for q in range(3)], 1).astype(np.int64)     # [T, 3] edge ids
    a, b = EDGE_CORNERS[edges, 0], EDGE_CORNERS[edges, 1]
    axis = np.select([(a ^ b) == 4, (a ^ b) == 2], [0, 1], 2)
    owner = base[:, None] + ((a >> 2) & 1) * (Y * Z) + ((a >> 1) & 1) * Z + (a & 1)
    keys = owner * 3 + axis
    vkeys = np.unique(keys)
    faces = np.searchsorted(vkeys, keys).astype(np.int64)

    lin, ax = vkeys // 3, vkeys % 3
    pa = np.stack(np.unravel_index(lin, (X, Y, Z)), 1)
    pb = pa + np.eye(3, dtype=np.int64)[ax]
    va, vb = tsdf[tuple(pa.T)], tsdf[tuple(pb.T)]
    t = (lev - va) / (vb - va)
    pos = pa.astype(F32)
    rows = np.arange(len(vkeys))
    pos[rows, ax] = pos[rows, ax] + t
    verts = pos * F32(voxel) + np.asarray(origin, F32)

    grad = np.stack(np.gradient(tsdf), -1)           # central inside, one-sided at the border, float32
    ga, gb = grad[tuple(pa.T)], grad[tuple(pb.T)]
    g = ga + t[:, None] * (gb - ga)
    length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    norms = np.zeros_like(g)
    np.divide(g, length[:, None], out=norms, where=length[:, None] > 0)

    if color is None:
        colors = np.zeros((len(vkeys), 3), np.uint8)
    else:
        ri = np.rint(pos).astype(np.int64)           # np.round: half to even
        rgb = np.asarray(color, F32)[tuple(ri.T)]
        cb = np.floor(rgb / F32(65536))
        rest = rgb - cb * F32(65536)
        cg = np.floor(rest / F32(256))
        cr = rest - cg * F32(256)
        colors = np.floor(np.stack([cr, cg, cb], 1)).astype(np.uint8)
    return verts, faces, norms, colors


def euler_characteristic(n_verts, faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    return n_verts - len(np.unique(e, axis=0)) + len(faces)


def is_closed(faces):
    """Every edge is in exactly two faces, traversed in opposite directions."""
    faces = np.asarray(faces, np.int64)
    n = int(faces.max()) + 1 if len(faces) else 1
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    fwd = np.sort(d[:, 0] * n + d[:, 1])
    if len(fwd) and (np.diff(fwd) == 0).any():        # a directed edge twice: more than two faces, or misoriented
        return False
    rev = d[:, 1] * n + d[:, 0]
    at = np.minimum(np.searchsorted(fwd, rev), max(len(fwd) - 1, 0))
    return bool(len(fwd) == 0 or (fwd[at] == rev).all())


def sphere_sdf(shape, center, radius):
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return (np.sqrt((i - center[0]) ** 2 + (j - center[1]) ** 2 + (k - center[2]) ** 2) - radius).astype(F32)


def torus_sdf(shape, center, big_r, small_r):
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    x, y, z = i - center[0], j - center[1], k - center[2]
    return (np.sqrt((np.sqrt(x * x + y * y) - big_r) ** 2 + z * z) - small_r).astype(F32)


# ---- meshwrite / pcwrite --------------------------------------------------------------------------------------------
MESH_HEADER = ["ply", "format ascii 1.0", "element vertex {v}", "property float x", "property float y",
               "property float z", "property float nx", "property float ny", "property float nz",
               "property uchar red", "property uchar green", "property uchar blue", "element face {f}",
               "property list uchar int vertex_index", "end_header"]                          # fusion.py:371-385
PC_HEADER = ["ply", "format ascii 1.0", "element vertex {v}", "property float x", "property float y",
             "property float z", "property uchar red", "property uchar green", "property uchar blue",
             "end_header"]                                                                   # fusion.py:409-418


def _mesh_data(n_v=300, n_f=500, seed=0):
    rng = np.random.default_rng(seed)
    verts = (rng.normal(size=(n_v, 3)) * 3).astype(F32)
    norms = rng.normal(size=(n_v, 3)).astype(F32)
    colors = rng.integers(0, 256, size=(n_v, 3)).astype(np.uint8)
    faces = rng.integers(0, n_v, size=(n_f, 3)).astype(np.int64)
    return verts, faces, norms, colors


def test_meshwrite_header_values_and_faces(tmp_path):
    from bnv_fusion_amd.mesh import load_ply
    from bnv_fusion_amd.tsdf import meshwrite
    verts, faces, norms, colors = _mesh_data()
    p = str(tmp_path / "m.ply")
    meshwrite(p, verts, faces, norms, colors)
    lines = open(p).read().splitlines()
    hdr = [h.format(v=len(verts), f=len(faces)) for h in MESH_HEADER]
    assert lines[:len(hdr)] == hdr
    body = lines[len(hdr):]
    assert len(body) == len(verts) + len(faces)
    vals = np.array([ln.split() for ln in body[:len(verts)]])
    assert vals.shape == (len(verts), 9)
    # %f: six decimals of the float32 value (fusion.py:389-393)
    assert np.array_equal(vals[:, :3].astype(np.float64), np.round(verts.astype(np.float64), 6))
    assert np.array_equal(vals[:, 3:6].astype(np.float64), np.round(norms.astype(np.float64), 6))
    assert all(len(x.split(".")[1]) == 6 for x in vals[:, :6].reshape(-1))
    assert np.array_equal(vals[:, 6:].astype(np.int64), colors)
    assert [ln.split()[0] for ln in body[len(verts):]] == ["3"] * len(faces)
    m = load_ply(p)
    assert np.array_equal(m.faces, faces)
    assert np.allclose(m.vertices, verts, atol=5e-7)


def test_pcwrite_header_and_values(tmp_path):
    from bnv_fusion_amd.tsdf import pcwrite
    verts, _, _, colors = _mesh_data(seed=1)
    xyzrgb = np.hstack([verts, colors])             # float32 [V, 6] as get_point_cloud returns it (fusion.py:320)
    p = str(tmp_path / "pc.ply")
    pcwrite(p, xyzrgb)
    lines = open(p).read().splitlines()
    hdr = [h.format(v=len(verts)) for h in PC_HEADER]
    assert lines[:len(hdr)] == hdr
    vals = np.array([ln.split() for ln in lines[len(hdr):]])
    assert vals.shape == (len(verts), 6)
    assert np.array_equal(vals[:, :3].astype(np.float64), np.round(verts.astype(np.float64), 6))
    assert np.array_equal(vals[:, 3:].astype(np.int64), colors)


def test_writers_take_empty_inputs(tmp_path):
    from bnv_fusion_amd.mesh import load_ply
    from bnv_fusion_amd.tsdf import meshwrite, pcwrite
    e = _empty()
    p = str(tmp_path / "e.ply")
    meshwrite(p, *e)
    assert open(p).read().splitlines() == [h.format(v=0, f=0) for h in MESH_HEADER]
    m = load_ply(p)
    assert m.vertices.shape == (0, 3) and len(m.faces) == 0
    q = str(tmp_path / "e_pc.ply")
    pcwrite(q, np.zeros((0, 6), F32))
    assert open(q).read().splitlines() == [h.format(v=0) for h in PC_HEADER]


# ---- the restatement on analytic surfaces ---------------------------------------------------------------------------
def test_restatement_sphere_is_a_closed_genus_0_surface():
    tsdf = sphere_sdf((40, 36, 44), (19.3, 17.6, 21.1), 12.4)
    v, f, n, c = restate_mesh(tsdf)
    assert len(v) > 1000 and euler_characteristic(len(v), f) == 2
    assert is_closed(f)
    assert np.unique(f).size == len(v)               # welded: every vertex is used
    r = np.linalg.norm(v - np.array([19.3, 17.6, 21.1], F32), axis=1)
    assert np.abs(r - 12.4).max() < 0.03
    radial = (v - np.array([19.3, 17.6, 21.1], F32)) / r[:, None]
    assert (np.sum(n * radial, 1) > 0.99).all()     # normals toward increasing TSDF: outward
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.sum(fn * radial[f[:, 0]], 1) >= 0).mean() > 0.999


def test_restatement_torus_has_euler_characteristic_0():
    tsdf = torus_sdf((48, 48, 24), (23.6, 24.2, 11.7), 13.0, 5.2)
    v, f, _, _ = restate_mesh(tsdf)
    assert euler_characteristic(len(v), f) == 0
    assert is_closed(f)


def test_restatement_observed_only_and_degenerate_volumes():
    tsdf = sphere_sdf((24, 24, 24), (11.5, 12.2, 11.8), 7.3)
    w = np.ones_like(tsdf)
    full = restate_mesh(tsdf, w, observed_only=True)
    ref = restate_mesh(tsdf)
    assert all(np.array_equal(a, b) for a, b in zip(full, ref))    # all observed: the same mesh
    w[12:, :, :] = 0
    half = restate_mesh(tsdf, w, observed_only=True)
    assert 0 < len(half[1]) < len(ref[1]) and not is_closed(half[1])
    for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        out = restate_mesh(np.full(shape, -1.0, F32))
        assert [a.shape for a in out] == [(0, 3)] * 4
    assert len(restate_mesh(np.ones((6, 6, 6), F32))[0]) == 0


# ---- the C entries refuse bad arguments before any HIP call ---------------------------------------------------------
def test_tsdf_mesh_entries_validate_arguments_without_a_gpu():
    from bnv_fusion_amd import _lib
    lib = _lib.load()
    INVALID, SMALL = -1, -2
    P = C.c_void_p(256)
    b = C.c_int64(-7)
    dim = (C.c_int32 * 3)(64, 64, 64)
    org = (C.c_float * 3)(0, 0, 0)
    assert lib.bnv_tsdf_mesh_workspace_bytes(None, C.byref(b)) == INVALID
    assert lib.bnv_tsdf_mesh_workspace_bytes(dim, None) == INVALID
    assert lib.bnv_tsdf_mesh_workspace_bytes((C.c_int32 * 3)(64, 0, 64), C.byref(b)) == INVALID
    assert lib.bnv_tsdf_mesh_workspace_bytes((C.c_int32 * 3)(-3, 4, 4), C.byref(b)) == INVALID
    assert lib.bnv_tsdf_mesh_workspace_bytes(dim, C.byref(b)) == 0
    need = b.value
    assert 0 < need <= 64 ** 3                         # at most 1 B per grid point
    assert lib.bnv_tsdf_mesh_workspace_bytes((C.c_int32 * 3)(512, 512, 512), C.byref(b)) == 0 and b.value <= 512 ** 3
    assert lib.bnv_tsdf_mesh_workspace_bytes((C.c_int32 * 3)(1, 1, 1), C.byref(b)) == 0 and b.value > 0

    def count(tsdf=P, weight=P, d=dim, obs=0, table=P, ws=P, nbytes=need, totals=P):
        return lib.bnv_tsdf_mesh_count(tsdf, weight, d, 0.0, obs, table, ws, nbytes, totals, None)
    assert count(tsdf=None) == INVALID
    assert count(d=None) == INVALID
    assert count(d=(C.c_int32 * 3)(0, 4, 4)) == INVALID
    assert count(table=None) == INVALID
    assert count(ws=None) == INVALID
    assert count(totals=None) == INVALID
    assert count(weight=None, obs=1) == INVALID        # observed_only reads the weights
    assert count(nbytes=need - 1) == SMALL

    def emit(tsdf=P, weight=P, color=P, d=dim, o=org, obs=0, table=P, ws=P, nbytes=need, nv=10, nf=10, verts=P):
        return lib.bnv_tsdf_mesh_emit(tsdf, weight, color, d, o, 0.025, 0.0, obs, table, ws, nbytes, nv, nf, verts,
                                      P, P, P, None)
    assert emit(tsdf=None) == INVALID
    assert emit(d=(C.c_int32 * 3)(4, 4, 0)) == INVALID
    assert emit(o=None) == INVALID
    assert emit(table=None) == INVALID
    assert emit(ws=None) == INVALID
    assert emit(verts=None) == INVALID
    assert emit(weight=None, obs=1) == INVALID
    assert emit(nv=-1) == INVALID
    assert emit(nf=-1) == INVALID
    assert emit(nbytes=need - 1) == SMALL

