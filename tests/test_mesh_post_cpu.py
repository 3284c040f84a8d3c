"""Mesh post-processing without a GPU: the numpy restatement of the specification (tests/mesh_post_restatement.py)
equals the host function mesh.post_process_mesh bit for bit, which pins the specification the device kernels follow;
the device entry points refuse CPU input (there is no CPU fallback)."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
import mesh_post_restatement as rs
from bnv_fusion_amd import mesh as M


def assert_same(got, want):
    gv, gf = got
    assert gv.dtype == np.float32 and gv.shape == want.vertices.shape
    assert np.array_equal(gv.view(np.uint32), want.vertices.view(np.uint32))
    assert np.array_equal(np.asarray(gf, np.int64), want.faces)


@pytest.mark.parametrize("case", rs.adversarial_cases(), ids=lambda c: c[0])
def test_restatement_equals_host_adversarial(case):
    _, v, f, eps = case
    assert_same(rs.post_process(v, f, eps), M.post_process_mesh(M.TriMesh(v, f), eps))


@pytest.mark.parametrize("voxel,frac,offset", [(1.0, 0.25, [3.3, 3.295, -3.305]), (0.01, 0.25, [0.033, 0.0331, -0.05]),
                                               (1.0, 0.6, [3.3, 3.3, 3.3]), (0.01, 0.6, [0.0, 0.033, 0.0])])
def test_restatement_equals_host_sphere(voxel, frac, offset):
    v, f = rs.soup_sphere(voxel, offset)
    want = M.post_process_mesh(M.TriMesh(v, f), frac * voxel)
    assert_same(rs.post_process(v, f, frac * voxel), want)
    if frac == 0.25:
        assert 0 < len(want.vertices) < len(v) // 3 and len(want.faces) > len(f) // 2


def test_neighbour_sum_order_is_ascending():
    """Vertex 0's neighbours are 1 (a big value) and 2, 3 (small ones): the sum in ascending index order differs in the
    last bit from other orders, and the host adds in that order."""
    v = np.array([[0, 0, 0], [1e8, 0, 0], [1, 1, 0], [-1e8, 1, 0], [0, 2, 1]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4]])
    want = M.post_process_mesh(M.TriMesh(v, f), 1e-6)
    assert_same(rs.post_process(v, f, 1e-6), want)


def test_device_entry_points_refuse_cpu_tensors():
    v = torch.zeros((3, 3), dtype=torch.float32)
    f = torch.tensor([[0, 1, 2]], dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU tensor"):
        M.post_process_mesh_tensors(v, f, 0.01)
    with pytest.raises(ValueError, match="GPU tensor"):
        M.post_process_mesh_tensors(v.numpy(), f.numpy(), 0.01)
    with pytest.raises(ValueError):
        M.post_process_mesh_gpu(M.TriMesh(v.numpy(), f.numpy()), 0.01, device="cpu")
