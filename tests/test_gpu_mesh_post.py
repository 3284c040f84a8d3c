"""Mesh post-processing on the GPU (csrc/meshpost.hip, mesh.post_process_mesh_tensors) against the host function
mesh.post_process_mesh, bit for bit: vertex float32 bits, vertex count and order, faces."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
import mesh_post_restatement as rs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gpu_post(v, f, eps):
    from bnv_fusion_amd import mesh as M
    vt = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEV)
    ft = torch.from_numpy(np.ascontiguousarray(f, np.int64)).to(DEV)
    vs, fs = M.post_process_mesh_tensors(vt, ft, eps)
    assert vs.is_cuda and fs.is_cuda and vs.dtype == torch.float32 and fs.dtype == torch.int64
    return vs.cpu().numpy(), fs.cpu().numpy()


def assert_same(got, want):
    gv, gf = got
    assert gv.shape == want.vertices.shape, (gv.shape, want.vertices.shape)
    assert np.array_equal(gv.view(np.uint32), want.vertices.view(np.uint32)), int((gv != want.vertices).sum())
    assert gf.shape == want.faces.shape and np.array_equal(gf, want.faces)


def host_post(v, f, eps):
    from bnv_fusion_amd import mesh as M
    return M.post_process_mesh(M.TriMesh(v, f), eps)


def mc_sphere(voxel, offset):
    """The per-voxel marching-cubes mesh of a sphere of radius 3.3 voxels (SparseVolume.meshlize's concatenation)."""
    from bnv_fusion_amd.mesh import marching_cubes_lattice_indexed
    c = torch.tensor([6.2, 6.1, 5.9])
    o = torch.stack(torch.meshgrid(*[torch.arange(13)] * 3, indexing="ij"), -1).reshape(-1, 3)
    r = torch.arange(3) * 0.5 - 0.5
    lat = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1)
    s = (((o[:, None, None, None, :] + lat[None] - c).norm(dim=-1) - 3.3) * voxel).float()
    mn = torch.tensor(offset, dtype=torch.float32)
    v, f, _, _ = marching_cubes_lattice_indexed(s.to(DEV), o.to(DEV), voxel, mn)
    return v, f


@pytest.mark.parametrize("voxel", [1.0, 0.01])
@pytest.mark.parametrize("frac", [0.25, 0.6])
def test_sphere_equals_host(voxel, frac):
    # min_coords puts lattice planes through the sphere within 1e-2 voxels of 0 (x, y) and at 0 (z)
    v, f = mc_sphere(voxel, [-5.997 * voxel, -6.004 * voxel, -5.5 * voxel])
    vh, fh = v.cpu().numpy(), f.cpu().numpy()
    assert (np.abs(vh) < 1e-2 * voxel).any()
    want = host_post(vh, fh, frac * voxel)
    from bnv_fusion_amd import mesh as M
    vs, fs = M.post_process_mesh_tensors(v, f, frac * voxel)
    assert_same((vs.cpu().numpy(), fs.cpu().numpy()), want)
    if frac == 0.25:
        assert 0 < len(want.vertices) < len(vh) and len(want.faces) > 0
    else:
        assert len(want.vertices) == 0 and len(want.faces) == 0


@pytest.mark.parametrize("case", rs.adversarial_cases(), ids=lambda c: c[0])
def test_adversarial_equals_host(case):
    _, v, f, eps = case
    assert_same(gpu_post(v, f, eps), host_post(v, f, eps))


@pytest.mark.parametrize("voxel,offset", [(1.0, [3.3, 3.295, -3.305]), (0.01, [0.0, 0.033, 0.0])])
def test_soup_sphere_equals_host(voxel, offset):
    v, f = rs.soup_sphere(voxel, offset)
    assert_same(gpu_post(v, f, voxel / 4), host_post(v, f, voxel / 4))


def test_two_calls_bit_identical():
    from bnv_fusion_amd import mesh as M
    v, f = mc_sphere(0.01, [0.0, 0.0, 0.0])
    a = M.post_process_mesh_tensors(v, f, 0.0025)
    b = M.post_process_mesh_tensors(v, f, 0.0025)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_trimesh_entry_point():
    from bnv_fusion_amd import mesh as M
    v, f = rs.soup_sphere(0.5, [0.1, 0.2, 0.3], n_lat=10, n_lon=16)
    got = M.post_process_mesh_gpu(M.TriMesh(v, f), 0.125, device=DEV)
    assert_same((got.vertices, got.faces), host_post(v, f, 0.125))


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
    bad += [(nan, f), (inf, f), (v[:0], f)]
    for vv, ff in bad:
        with pytest.raises(ValueError):
            M.post_process_mesh_tensors(vv, ff, 0.01)
    for eps in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            M.post_process_mesh_tensors(v, f, eps)
    with pytest.raises(ValueError):                       # beyond 2^29 thresholds: the grid would not be exact
        M.post_process_mesh_tensors(v * 1e6, f, 1e-9)


def _sweep_map(grid, frames=range(0, 120, 2)):
    import bnv_fusion_amd as bnv
    from bnv_fusion_amd import sequence
    dims, voxel, scale = sequence.DIMS[grid]
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)
    nm = bnv.NeuralMap(np.array([dims] * 3), voxel, model, device=DEV)
    for fr in sequence.sweep_frames(frames, scale=scale, device=DEV):
        nm.integrate(fr)
    return nm, scale


def test_room_sweep_extract_mesh_post_process():
    from bnv_fusion_amd import evaluate, sequence
    from bnv_fusion_amd import mesh as M
    nm, scale = _sweep_map(256)
    eps = nm.voxel_size / 4
    raw = nm.extract_mesh()
    want = M.post_process_mesh(raw, eps)
    got = nm.extract_mesh(post_process=eps)
    assert_same((got.vertices, got.faces), want)
    assert len(want.vertices) < len(raw.vertices) / 2 and len(want.faces) > len(raw.faces) / 2
    vt = torch.from_numpy(raw.vertices).to(DEV)
    ft = torch.from_numpy(raw.faces).to(DEV)
    dv = M.post_process_mesh_tensors(vt, ft, eps)
    res = evaluate.evaluate_meshes(dv, sequence.gt_mesh(scale), generator=torch.Generator(device=DEV).manual_seed(0))
    print("room sweep, post-processed on the device:", evaluate.summary_line(res))
    assert res["accuracy"] > 0.5, res


def test_room_sweep_512_equals_host():
    from bnv_fusion_amd import mesh as M
    nm, _ = _sweep_map(512, range(600))
    raw = nm.extract_mesh()
    assert len(raw.vertices) > 1_000_000
    eps = nm.voxel_size / 4
    want = M.post_process_mesh(raw, eps)
    got = M.post_process_mesh_gpu(raw, eps, device=DEV)
    print(f"512^3 sweep: {len(raw.vertices)} / {len(raw.faces)} -> {len(want.vertices)} / {len(want.faces)}")
    assert_same((got.vertices, got.faces), want)
