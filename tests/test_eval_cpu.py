"""Mesh evaluation without a GPU: the PLY reader, the ground-truth meshes of the synthetic scenes, argument
validation of the C entries (before any HIP call) and the refusal of CPU tensors."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)


# ---- load_ply ------------------------------------------------------------------------------------------------------
def test_load_ply_round_trips_export(tmp_path):
    from bnv_fusion_amd.mesh import TriMesh, load_ply
    rng = np.random.default_rng(0)
    m = TriMesh(rng.normal(size=(500, 3)).astype(np.float32), rng.integers(0, 500, size=(900, 3)))
    r = load_ply(m.export(str(tmp_path / "m.ply")))
    assert r.vertices.dtype == np.float32 and np.array_equal(r.vertices, m.vertices)
    assert np.array_equal(r.faces, m.faces)


def test_load_ply_ascii_doubles_extra_properties_and_a_quad(tmp_path):
    from bnv_fusion_amd.mesh import load_ply
    p = tmp_path / "a.ply"
    p.write_text("ply\nformat ascii 1.0\ncomment hand written\nelement vertex 5\n"
                 "property double x\nproperty double y\nproperty double z\n"
                 "property float nx\nproperty float ny\nproperty float nz\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                 "element face 2\nproperty list uint8 uint32 vertex_indices\nend_header\n"
                 "0 0 0 0 0 1 255 0 0\n1 0 0 0 0 1 0 255 0\n1 1 0 0 0 1 0 0 255\n0 1 0 0 0 1 1 2 3\n"
                 "0.5 0.5 1.25 0 0 1 4 5 6\n"
                 "4 0 1 2 3\n3 0 1 4\n")
    m = load_ply(str(p))
    assert np.array_equal(m.vertices, np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.25]],
                                               dtype=np.float32))
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4]]    # the quad as a fan


def test_load_ply_binary_doubles_extra_properties_uint8_uint32_lists(tmp_path):
    from bnv_fusion_amd.mesh import load_ply
    p = tmp_path / "b.ply"
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty double x\nproperty double y\n"
           "property double z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red\n"
           "property uchar green\nproperty uchar blue\nproperty uchar alpha\n"
           "element face 2\nproperty list uchar uint vertex_indices\nend_header\n")
    xyz = [(0.1, 0.2, 0.3), (1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1e-9)]
    body = b"".join(struct.pack("<dddfffBBBB", *v, 0, 0, 1, 1, 2, 3, 4) for v in xyz)
    body += struct.pack("<BIII", 3, 0, 1, 2) + struct.pack("<BIIII", 4, 0, 1, 2, 3)
    p.write_bytes(hdr.encode() + body)
    m = load_ply(str(p))
    assert np.array_equal(m.vertices, np.array(xyz, dtype=np.float64).astype(np.float32))
    assert m.faces.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3]]


def test_load_ply_rejects_big_endian_and_unsupported_lists(tmp_path):
    from bnv_fusion_amd.mesh import load_ply
    p = tmp_path / "be.ply"
    p.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\n"
                  b"property float z\nend_header\n" + struct.pack(">fff", 1, 2, 3))
    with pytest.raises(ValueError, match="binary_big_endian"):
        load_ply(str(p))
    q = tmp_path / "short.ply"
    q.write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face 1\nproperty list ushort int vertex_indices\nend_header\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    with pytest.raises(ValueError, match="list ushort int"):
        load_ply(str(q))


# ---- the C entries refuse bad arguments before any HIP call --------------------------------------------------------
def test_eval_entries_validate_arguments_without_a_gpu():
    from bnv_fusion_amd import _lib
    lib = _lib.load()
    INVALID, SMALL = -1, -2
    b = C.c_int64(-7)
    P = C.c_void_p(256)
    assert lib.bnv_mesh_sample_surface_workspace(0, C.byref(b)) == INVALID
    assert lib.bnv_mesh_sample_surface_workspace(10, None) == INVALID
    assert lib.bnv_mesh_sample_surface_workspace(10, C.byref(b)) == 0 and b.value > 10 * 8
    need = b.value
    assert lib.bnv_mesh_sample_surface(None, 3, P, 1, P, 4, P, need, P, P, None, None) == INVALID
    assert lib.bnv_mesh_sample_surface(P, 3, P, 1, P, 0, P, need, P, P, None, None) == INVALID       # n <= 0
    assert lib.bnv_mesh_sample_surface(P, 0, P, 1, P, 4, P, need, P, P, None, None) == INVALID       # no vertices
    assert lib.bnv_mesh_sample_surface(P, 3, P, 1, P, 4, P, need, None, P, None, None) == INVALID    # no output
    assert lib.bnv_mesh_sample_surface(P, 3, P, 10, P, 4, P, need - 1, P, P, None, None) == SMALL
    assert lib.bnv_nn_workspace_bytes(0, 5, C.byref(b)) == INVALID
    assert lib.bnv_nn_workspace_bytes(5, -1, C.byref(b)) == INVALID
    assert lib.bnv_nn_workspace_bytes(5, 5, None) == INVALID
    assert lib.bnv_nn_workspace_bytes(1000, 2000, C.byref(b)) == 0 and b.value >= 16 * 3000
    need = b.value
    assert lib.bnv_nn_workspace_bytes(1000, 2000, C.byref(b)) == 0 and b.value == need        # a function of the counts
    assert lib.bnv_nn_query(None, 1000, P, 2000, P, need, P, P, None) == INVALID
    assert lib.bnv_nn_query(P, 1000, P, 2000, P, need, P, None, None) == INVALID
    assert lib.bnv_nn_query(P, 0, P, 2000, P, need, P, P, None) == INVALID
    assert lib.bnv_nn_query(P, 1000, P, -3, P, need, P, P, None) == INVALID
    assert lib.bnv_nn_query(P, 1000, P, 2000, P, need - 1, P, P, None) == SMALL


def test_eval_refuses_cpu_tensors():
    from bnv_fusion_amd import evaluate
    x = torch.rand(100, 3)
    f = torch.randint(0, 100, (50, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        evaluate.nn_d2(x, x)
    with pytest.raises(ValueError, match="no CPU fallback"):
        evaluate.nearest_neighbors(x, x)
    with pytest.raises(ValueError, match="no CPU fallback"):
        evaluate.evaluate(x, x)
    with pytest.raises(ValueError, match="no CPU fallback"):
        evaluate.sample_surface(x, f, 10)
    with pytest.raises(ValueError, match="no CPU fallback"):
        evaluate.evaluate_meshes((x, f), (x, f))
    with pytest.raises(ValueError, match="no CPU fallback"):
        evaluate.sample_surface_uniforms(x, f, torch.rand(10, 3))


def test_summary_line_and_f1_of_nothing():
    from bnv_fusion_amd import evaluate
    res = evaluate.metrics_from_distances(torch.tensor([0.01, 0.03], dtype=torch.float64),
                                          torch.tensor([0.02, 0.5, 0.001], dtype=torch.float64))
    assert res["accuracy"] == 0.5 and res["recall"] == 2 / 3 and abs(res["F1"] - 2 * 0.5 * (2 / 3) / (0.5 + 2 / 3)) < 1e-15
    assert evaluate.summary_line(res) == "{:.3f}/{:.4f}/{:.3f}/{:.4f}/{:.4f}".format(
        0.02, 0.5, (0.02 + 0.5 + 0.001) / 3, 2 / 3, res["F1"])
    far = torch.tensor([1.0], dtype=torch.float64)
    assert np.isnan(evaluate.metrics_from_distances(far, far)["F1"])          # P + R = 0: nan, as numpy gives


# ---- ground truth of the synthetic scenes ---------------------------------------------------------------------------
def test_synthetic_gt_mesh_lies_on_the_scene():
    from bnv_fusion_amd import synthetic
    union = synthetic.gt_mesh("union", step_px=4.0)
    common = synthetic.gt_mesh("common", step_px=4.0)
    for m in (union, common):
        assert len(m.faces) > 1000 and m.faces.min() >= 0 and m.faces.max() < len(m.vertices)
        p = m.vertices.astype(np.float64) - synthetic.pose(0)[:3, 3]          # camera-0 frame (pose(0): R = I)
        K = synthetic.INTRINSICS
        u = K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2]
        v = K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]
        assert np.abs(p[:, 2] - synthetic.scene_depth0(u, v)).max() < 1e-6
    key = lambda m: {tuple(r) for r in m.vertices.view(np.int32).tolist()}   # noqa: E731
    ku, kc = key(union), key(common)
    assert kc < ku                                                            # common is a proper part of union
    # camera 0 alone sees u in [0, 639]: the union reaches beyond it, the common region stays inside it
    x_cam0 = (np.array([0.0, 639.0]) - 319.5) / 525.0
    xs = lambda m: m.vertices[:, 0] / (m.vertices[:, 2] + 1.5)                # noqa: E731
    assert xs(union).min() < x_cam0[0] and xs(union).max() > x_cam0[1]
    assert xs(common).min() > x_cam0[0] and xs(common).max() < x_cam0[1]
    with pytest.raises(ValueError):
        synthetic.gt_mesh("some")


def test_sequence_gt_mesh_lies_on_room_and_box_faces():
    from bnv_fusion_amd import sequence
    for scale in (1.0, 0.5):
        m = sequence.gt_mesh(scale)
        boxes = [(np.array([-scale * h for h in sequence.ROOM_HALF]), np.array([scale * h for h in sequence.ROOM_HALF]))]
        boxes += [(np.array([scale * (c[a] - h[a]) for a in range(3)]), np.array([scale * (c[a] + h[a]) for a in range(3)]))
                  for c, h in sequence.FURNITURE]
        assert len(m.faces) == 12 * len(boxes)
        v = m.vertices.astype(np.float64)
        tri = v[m.faces]                                  # [T, 3, 3]: every triangle lies in one face of one box

        def on_a_face(t):
            for lo, hi in boxes:
                inside = np.all((t >= lo.astype(np.float32) - 1e-6) & (t <= hi.astype(np.float32) + 1e-6))
                for a in range(3):
                    for plane in (lo[a], hi[a]):
                        if inside and np.all(np.abs(t[:, a] - plane) < 1e-6):
                            return True
            return False
        assert all(on_a_face(t) for t in tri)
        areas = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
        room = 8 * scale ** 2 * (sequence.ROOM_HALF[0] * sequence.ROOM_HALF[1] + sequence.ROOM_HALF[1] *
                                 sequence.ROOM_HALF[2] + sequence.ROOM_HALF[0] * sequence.ROOM_HALF[2])
        assert abs(areas[:12].sum() - room) < 1e-4 * room
