"""Mesh components without a GPU: the restatement of the specification (tests/mesh_components_restatement.py) equals the
host functions mesh.connected_components / mesh.remove_small_components bit for bit, which pins the specification the
device kernels follow; argument validation; the device entry points refuse CPU input (there is no CPU fallback)."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
import mesh_components_restatement as rs
import mesh_post_restatement as post_rs
from bnv_fusion_amd import mesh as M

CASES = rs.adversarial_cases()


def assert_same_mesh(got, want):
    gv, gf = got
    assert gv.dtype == np.float32 and gv.shape == want.vertices.shape, (gv.shape, want.vertices.shape)
    assert np.array_equal(gv.view(np.uint32), want.vertices.view(np.uint32))
    assert np.array_equal(np.asarray(gf, np.int64), want.faces)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_restatement_equals_host(case):
    _, v, f, filters = case
    want = rs.components(v, f)
    got = M.connected_components(M.TriMesh(v, f))
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[2].dtype == np.float64
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))
    for kw in filters:
        assert_same_mesh(rs.remove_small(v, f, **kw), M.remove_small_components(M.TriMesh(v, f), **kw))


def _case(name):
    return next(c for c in CASES if c[0] == name)


def test_expected_components():
    counts = {"one_face": 1, "edge_same_winding": 1, "edge_opposite_winding": 1, "bow_tie": 2,
              "three_faces_one_edge": 1, "degenerate_beside_neighbour": 2, "duplicate_face": 2,
              "unreferenced_and_trailing": 2, "isolated_255": 255, "isolated_256": 256, "isolated_257": 257,
              "strip_4097_shuffled": 1, "strip_cut_face0_last": 2, "two_far_unit_triangles": 2,
              "fans_all_criteria": 12, "sphere_and_strays": 4, "no_faces": 0, "empty": 0}
    for name, v, f, _ in CASES:
        labels, n_faces, areas = M.connected_components(M.TriMesh(v, f))
        assert len(areas) == counts[name] == len(n_faces), name
        assert int(n_faces.sum()) == len(f)
    _, v, f, _ = _case("strip_4097_shuffled")
    assert M.connected_components(M.TriMesh(v, f))[2].tolist() == [2048.5]
    _, v, f, _ = _case("degenerate_beside_neighbour")
    labels, n_faces, areas = M.connected_components(M.TriMesh(v, f))
    assert labels.tolist() == [0, 0, 1] and n_faces.tolist() == [2, 1] and areas.tolist() == [0.5, 0.5]
    _, v, f, _ = _case("strip_cut_face0_last")
    labels, n_faces, _ = M.connected_components(M.TriMesh(v, f))
    assert labels[0] == 0 and labels[-1] == 1 and sorted(n_faces.tolist()) == [2000, 2096]


def test_equality_keeps_and_ties_go_to_the_smaller_label():
    _, v, f, _ = _case("two_far_unit_triangles")
    m = M.TriMesh(v, f)
    assert M.connected_components(m)[2].tolist() == [0.5, 0.5]
    assert len(M.remove_small_components(m, min_area=0.5).faces) == 2
    out = M.remove_small_components(m, min_area=float(np.nextafter(0.5, 1.0)))
    assert len(out.faces) == 0 and len(out.vertices) == 0
    out = M.remove_small_components(m, keep_largest=1)
    assert np.array_equal(out.vertices, v[:3]) and out.faces.tolist() == [[0, 1, 2]]


def test_thresholds_between_the_strays():
    _, v, f, filters = _case("sphere_and_strays")
    labels, n_faces, areas = M.connected_components(M.TriMesh(v, f))
    assert n_faces.tolist()[1:] == [4, 4, 4] and areas[0] == areas.max()
    for kw, n_left in zip(filters, (4, 3, 2, 1, 0)):
        out = M.remove_small_components(M.TriMesh(v, f), **kw)
        assert len(M.connected_components(out)[2]) == n_left, kw
        assert len(out.faces) == int(n_faces[areas >= kw["min_area"]].sum())
        if n_left:
            assert out.faces.max() == len(out.vertices) - 1 and len(np.unique(out.faces)) == len(out.vertices)


def test_unreferenced_vertices_are_dropped_and_order_kept():
    _, v, f, _ = _case("unreferenced_and_trailing")
    out = M.remove_small_components(M.TriMesh(v, f))
    assert np.array_equal(out.vertices.view(np.uint32), v[[1, 2, 3, 5, 6, 7]].view(np.uint32))
    assert out.faces.tolist() == [[0, 1, 2], [3, 4, 5]]


def test_invalid_input_raises():
    v, f = rs.isolated_triangles(2)
    for kw in (dict(min_area=-1.0), dict(min_area=float("nan")), dict(min_area=float("inf")), dict(min_faces=-1),
               dict(keep_largest=0), dict(keep_largest=-2)):
        with pytest.raises(ValueError):
            M.remove_small_components(M.TriMesh(v, f), **kw)
    bad = v.copy()
    bad[5, 1] = np.nan
    for vv, ff in ((bad, f), (v, f + 1), (v, f - 1), (v[:0], f)):
        with pytest.raises(ValueError):
            M.connected_components(M.TriMesh(vv, ff))
        with pytest.raises(ValueError):
            M.remove_small_components(M.TriMesh(vv, ff))
    with pytest.raises(ValueError):
        M.post_process_mesh(M.TriMesh(v, f), 0.01, surface_threshold=-0.1)


def test_total_area_limit():
    """One right triangle with legs 128 and 64 has area exactly 2^12: refused.  4095 unit-leg strips of area 1 each are
    below it; one more face of area 1 reaches it."""
    big = np.array([[0, 0, 0], [128, 0, 0], [0, 64, 0]], np.float32)
    with pytest.raises(ValueError, match="2\\^12"):
        M.connected_components(M.TriMesh(big, [[0, 1, 2]]))
    with pytest.raises(ValueError, match="2\\^12"):
        rs.components(big, [[0, 1, 2]])
    under = big.copy()
    under[1, 0] = np.nextafter(np.float32(128), np.float32(0))
    assert M.connected_components(M.TriMesh(under, [[0, 1, 2]]))[2][0] < 4096.0
    # many faces whose sum reaches the limit although every face is far below it
    quad = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0]], np.float32)                         # area 1
    f = np.tile(np.array([[0, 1, 2]]), (4096, 1))
    with pytest.raises(ValueError, match="2\\^12"):
        M.connected_components(M.TriMesh(quad, f))
    assert M.connected_components(M.TriMesh(quad, f[:4095]))[2].tolist() == [4095.0]


def test_post_process_surface_threshold_equals_two_steps():
    v, f = rs.sphere_and_strays()
    # unweld: every face its own vertices, as meshes arrive at the post-processing
    vs, fs = v[f.reshape(-1)], np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)
    areas = np.sort(M.connected_components(M.post_process_mesh(M.TriMesh(vs, fs), 0.025))[2])
    assert len(areas) == 4
    for s in (0.0, float(areas[0]), float(areas[1] + areas[2]) / 2, float(areas[3]) * 2):
        one = M.post_process_mesh(M.TriMesh(vs, fs), 0.025, surface_threshold=s)
        two = M.remove_small_components(M.post_process_mesh(M.TriMesh(vs, fs), 0.025), min_area=s)
        assert_same_mesh((one.vertices, one.faces), two)


@pytest.mark.parametrize("case", post_rs.adversarial_cases(), ids=lambda c: c[0])
def test_surface_threshold_none_is_todays_output(case):
    _, v, f, eps = case
    want = post_rs.post_process(v, f, eps)
    got = M.post_process_mesh(M.TriMesh(v, f), eps, surface_threshold=None)
    assert np.array_equal(got.vertices.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got.faces, want[1])


def test_device_entry_points_refuse_cpu_tensors():
    v = torch.zeros((3, 3), dtype=torch.float32)
    f = torch.tensor([[0, 1, 2]], dtype=torch.int64)
    for fn in (M.connected_components_tensors, M.remove_small_components_tensors):
        with pytest.raises(ValueError, match="GPU tensor"):
            fn(v, f)
        with pytest.raises(ValueError, match="GPU tensor"):
            fn(v.numpy(), f.numpy())
    with pytest.raises(ValueError):
        M.remove_small_components_gpu(M.TriMesh(v.numpy(), f.numpy()), device="cpu")
    with pytest.raises(ValueError, match="GPU tensor"):
        M.post_process_mesh_tensors(v, f, 0.01, surface_threshold=0.1)


def test_filter_arguments_are_checked_before_the_tensors():
    v = torch.zeros((3, 3), dtype=torch.float32)
    f = torch.tensor([[0, 1, 2]], dtype=torch.int64)
    for kw in (dict(min_area=-1.0), dict(min_area=float("nan")), dict(min_faces=-3), dict(keep_largest=0)):
        with pytest.raises(ValueError, match="min_faces|keep_largest|area threshold"):
            M.remove_small_components_tensors(v, f, **kw)
