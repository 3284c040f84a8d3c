"""Mesh simplification on the GPU (csrc/meshsimplify.hip, mesh.simplify_mesh_tensors) against the restatement of the
specification (tests/mesh_simplify_restatement.py), bit for bit: vertex float32 bits, vertex count and order, faces."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
import mesh_simplify_restatement as rs
import register_restatement as reg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLACEMENTS = ("quadric", "mean")


def gpu(v, f, cell, placement="quadric", min_det=1e-3):
    from bnv_fusion_amd import mesh as M
    vt = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEV)
    ft = torch.from_numpy(np.ascontiguousarray(f, np.int64)).to(DEV)
    vs, fs = M.simplify_mesh_tensors(vt, ft, cell, placement, min_det)
    assert vs.is_cuda and fs.is_cuda and vs.dtype == torch.float32 and fs.dtype == torch.int64
    return vs.cpu().numpy(), fs.cpu().numpy()


def assert_same(got, want):
    assert got[0].shape == want[0].shape, (got[0].shape, want[0].shape)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), int((got[0] != want[0]).sum())
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1])


def mc_sphere(voxel=0.05):
    """The per-voxel marching-cubes mesh of a sphere of radius 3.3 voxels, as a triangle soup (marching_cubes_lattice)
    -> numpy (vertices, faces), a few thousand faces around the origin (negative coordinates on every axis)."""
    from bnv_fusion_amd.mesh import marching_cubes_lattice
    c = torch.tensor([6.2, 6.1, 5.9])
    o = torch.stack(torch.meshgrid(*[torch.arange(13)] * 3, indexing="ij"), -1).reshape(-1, 3)
    r = torch.arange(3) * 0.5 - 0.5
    lat = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1)
    s = (((o[:, None, None, None, :] + lat[None] - c).norm(dim=-1) - 3.3) * voxel).float()
    v, f = marching_cubes_lattice(s.to(DEV), o.to(DEV), voxel, torch.tensor([-6.0 * voxel] * 3))
    return v.cpu().numpy(), f.cpu().numpy()


# (name, vertices, faces, cells): every mesh at the identity end (no two distinct vertices in a cell), in the middle,
# and at the coarse end (one cell, where the mesh lies on one side of the origin: everything collapses to an empty mesh)
CASES = [("tetrahedron", *rs.tetrahedron(), (0.05, 0.6, 4.0)),
         ("box432", *reg.box(), (0.01, 0.12, 4.0)),
         ("uv_sphere", *rs.uv_sphere(n_lat=12, n_lon=20), (0.01, 0.11, 1.0)),
         ("strip255", *rs.strip(255), (0.004, 0.05, 8.0)),
         ("strip256", *rs.strip(256), (0.004, 0.05, 8.0)),
         ("strip257", *rs.strip(257), (0.004, 0.05, 8.0)),
         ("fan300", *rs.fan(300), (0.0005, 0.01, 1.0)),
         ("adversarial", *rs.adversarial(0.125), (0.001, 0.03, 0.125, 0.25, 1.0))]


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_equals_the_restatement(case, placement):
    name, v, f, cells = case
    n_out = []
    for h in cells:
        want = rs.simplify(v, f, h, placement)
        assert_same(gpu(v, f, h, placement), want)
        n_out.append(len(want[1]))
        if len(np.unique(np.floor(v.astype(np.float64) / h), axis=0)) == 1:
            assert n_out[-1] == 0                                  # the one-cell end
    assert max(n_out) > 0
    if name in ("tetrahedron", "box432", "strip256", "fan300"):   # (meshes around the origin have no one-cell end)
        assert n_out[-1] == 0


def test_fan_is_one_run_longer_than_a_block():
    """All 300 rim faces' corners at vertex 0 plus the rim's own fall into ONE cluster when the cell covers the fan:
    one thread sums a run of 900 corners; the cells next to it keep the mesh from collapsing entirely."""
    v, f = rs.fan(300)
    far = np.array([[0.35, 0.05, 0.03], [0.05, 0.35, 0.03], [0.35, 0.35, 0.2]], np.float32)
    v2 = np.concatenate([v, far])
    f2 = np.concatenate([f, [[0, 301, 302], [5, 302, 303], [0, 303, 301]]]).astype(np.int64)
    for placement in PLACEMENTS:
        for md in (0.0, 1e-3):
            want = rs.simplify(v2, f2, 0.25, placement, md)
            assert len(want[1]) >= 2
            assert_same(gpu(v2, f2, 0.25, placement, md), want)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_marching_cubes_sphere_equals_the_restatement_and_keeps_the_invariants(placement):
    v, f = mc_sphere()
    assert 1000 < len(f) < 10000 and (v.min(0) < 0).all() and (v.max(0) > 0).all()
    counts = []
    for h in (0.05, 0.1, 0.17):                                    # 1, 2 and 3.4 voxels
        vo, fo, info = rs.simplify(v, f, h, placement, return_info=True)
        assert_same(gpu(v, f, h, placement), (vo, fo))
        assert len(fo) and ((fo[:, 0] != fo[:, 1]) & (fo[:, 1] != fo[:, 2]) & (fo[:, 0] != fo[:, 2])).all()
        lo = np.argmin(fo, axis=1)
        rot = np.take_along_axis(fo, (lo[:, None] + np.arange(3)[None]) % 3, axis=1)
        assert len(np.unique(rot, axis=0)) == len(fo)
        assert np.array_equal(np.unique(fo), np.arange(len(vo)))
        keys = [rs.cell_key(i) for i in info["cells"].tolist()]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        centre = (info["cells"].astype(np.float64) + 0.5) * h
        slack = np.spacing(np.abs(vo).max().astype(np.float32)).astype(np.float64)
        assert (np.abs(vo.astype(np.float64) - centre) <= h + slack).all()
        counts.append(len(fo))
    assert len(f) > counts[0] > counts[1] > counts[2]


def test_min_det_decides_the_same_clusters():
    v, f = reg.box()
    for md in (0.0, 1e-6, 0.5, 1e9):
        assert_same(gpu(v, f, 0.12, "quadric", md), rs.simplify(v, f, 0.12, "quadric", md))


def test_equals_the_host_function_and_trimesh_entry_point():
    from bnv_fusion_amd import mesh as M
    v, f = rs.uv_sphere()
    want = M.simplify_mesh(M.TriMesh(v, f), 0.09)
    got = M.simplify_mesh_gpu(M.TriMesh(v, f), cell=0.09, device=DEV)
    assert_same((got.vertices, got.faces), (want.vertices, want.faces))
    assert 0 < len(want.faces) < len(f)


def test_two_calls_bit_identical():
    from bnv_fusion_amd import mesh as M
    v, f = mc_sphere()
    vt, ft = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    a = M.simplify_mesh_tensors(vt, ft, 0.1)
    b = M.simplify_mesh_tensors(vt, ft, 0.1)
    assert len(a[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_target_faces_returns_at_most_the_asked_number():
    from bnv_fusion_amd import mesh as M
    v, f = rs.uv_sphere()
    m = M.TriMesh(v, f)
    for target in (1500, 400, 60):
        got = M.simplify_mesh_gpu(m, target_faces=target, device=DEV)
        assert 0 < len(got.faces) <= target, (target, len(got.faces))
        assert np.array_equal(np.unique(got.faces), np.arange(len(got.vertices)))
    assert len(M.simplify_mesh_gpu(m, target_faces=0, device=DEV).faces) == 0
    for kw in ({}, {"cell": 0.1, "target_faces": 100}, {"target_faces": -1}, {"target_faces": 10.5}):
        with pytest.raises(ValueError):
            M.simplify_mesh_gpu(m, device=DEV, **kw)


def test_no_faces_and_nothing_give_an_empty_mesh():
    from bnv_fusion_amd import mesh as M
    v = torch.rand((9, 3), device=DEV)
    none = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    for vv in (v, v[:0]):
        vo, fo = M.simplify_mesh_tensors(vv, none, 0.1)
        assert tuple(vo.shape) == (0, 3) and tuple(fo.shape) == (0, 3)


def test_invalid_input_raises():
    from bnv_fusion_amd import mesh as M
    v = torch.rand((10, 3), device=DEV)
    f = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int64, device=DEV)
    bad = [(v.cpu(), f), (v, f.cpu()), (v.double(), f), (v, f.int()), (v[:, :2], f), (v, f[:, :2]),
           (v, f + 8), (v, f - 1)]
    nan = v.clone()
    nan[4, 1] = float("nan")
    inf = v.clone()
    inf[0, 0] = float("inf")
    bad += [(nan, f), (inf, f), (v[:0], f), (nan, f[:0])]
    for vv, ff in bad:
        with pytest.raises(ValueError):
            M.simplify_mesh_tensors(vv, ff, 0.01)
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            M.simplify_mesh_tensors(v, f, cell)
    for md in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            M.simplify_mesh_tensors(v, f, 0.01, "quadric", md)
    with pytest.raises(ValueError):
        M.simplify_mesh_tensors(v, f, 0.01, "median")
    with pytest.raises(ValueError):                               # 2^20 cells or more from the origin
        M.simplify_mesh_tensors(v + 1.0, f, 2.0 ** -20)


def test_device_refuses_what_the_wrapper_checks():
    """The C entry alone, past the Python checks: counts = {-1, -1} for a non-finite vertex, a face index out of range
    and a coordinate 2^20 cells out; nothing is clamped."""
    import ctypes as C
    from bnv_fusion_amd import _lib
    lib = _lib.load()
    v0, f0 = rs.tetrahedron()

    def run(v, f, cell):
        vt, ft = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
        V, T = len(v), len(f)
        need = C.c_int64()
        assert lib.bnv_mesh_simplify_bytes(V, T, C.byref(need)) == 0
        ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
        vo = torch.empty((V, 3), dtype=torch.float32, device=DEV)
        fo = torch.empty((T, 3), dtype=torch.int64, device=DEV)
        counts = torch.empty(2, dtype=torch.int64, device=DEV)
        assert lib.bnv_mesh_simplify(_lib.ptr(vt), V, _lib.ptr(ft), T, C.c_double(cell), 0, C.c_double(1e-3),
                                     _lib.ptr(ws), need.value, _lib.ptr(vo), _lib.ptr(fo), _lib.ptr(counts),
                                     _lib.stream_ptr()) == 0
        return counts.tolist()

    assert run(v0, f0, 0.5) == [4, 4]
    nan = v0.copy()
    nan[1, 2] = np.nan
    assert run(nan, f0, 0.5) == [-1, -1]
    assert run(nan, f0[:0], 0.5) == [-1, -1]
    assert run(v0, f0 + 1, 0.5) == [-1, -1]
    assert run(v0, f0 - 1, 0.5) == [-1, -1]
    assert run(v0, f0, 1.25 / 2 ** 20) == [-1, -1]
    assert run(v0, f0[:0], 0.5) == [0, 0]


def test_extract_mesh_simplify_equals_the_stages_one_after_another():
    import bnv_fusion_amd as bnv
    from bnv_fusion_amd import mesh as M, sequence
    dims, voxel, scale = sequence.DIMS[256]                        # a small map: twelve frames of the room sweep
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)
    nm = bnv.NeuralMap(np.array([dims] * 3), voxel, model, device=DEV)
    for fr in sequence.sweep_frames(range(0, 24, 2), scale=scale, device=DEV):
        nm.integrate(fr)
    eps = voxel / 4
    post = nm.extract_mesh(post_process=eps)
    assert post is not None and len(post.faces) > 1000
    got = nm.extract_mesh(post_process=eps, simplify=2 * voxel, normals=True)
    vt, ft = torch.from_numpy(post.vertices).to(DEV), torch.from_numpy(post.faces).to(DEV)
    want = M.simplify_mesh_tensors(vt, ft, 2 * voxel)
    assert_same((got.vertices, got.faces), (want[0].cpu().numpy(), want[1].cpu().numpy()))
    assert 0 < len(got.faces) < len(post.faces) / 2
    host = M.simplify_mesh(post, 2 * voxel)
    assert_same((got.vertices, got.faces), (host.vertices, host.faces))
    assert got.vertex_normals.shape == got.vertices.shape          # computed on the vertices that are kept
    assert np.array_equal(got.vertex_normals, M.vertex_normals_tensors(*want).cpu().numpy())
