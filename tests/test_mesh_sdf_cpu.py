"""The float64 restatement of the mesh signed distance (tests/mesh_sdf_restatement.py) against analytic shapes, and the
host-side pieces of the patch chain: ``mesh.load_obj``, argument validation of the C entries, the CPU refusal of the
patch cutter.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_sdf_restatement as R


def test_restatement_matches_the_analytic_box():
    """A tessellated, rotated, off-origin box has exactly the analytic box SDF; what remains is the float32 cast of
    the vertices: <= 4 * 2^-23 * L (measured: 1.2e-7 at L = 2.9), no sign disagreement, no boundary flag."""
    from bnv_fusion_amd import synthetic
    V, F, shape = R.box_mesh((1.0, -0.5, 2.0), R.rotation(3), (0.31, 0.22, 0.17), n=6)
    rng = np.random.default_rng(0)
    P = (np.array([1.0, -0.5, 2.0]) + rng.uniform(-0.5, 0.5, (20000, 3))).astype(np.float32)
    ref = R.mesh_sdf(P, V, F)
    exact = synthetic.shape_sdf(shape, P.astype(np.float64))
    L = R.largest_coordinate(V, P)
    err = np.abs(ref["sdf"] - exact).max()
    print(f"box: max |restatement - analytic| = {err:.3e}, bound {4 * R.ULP32 * L:.3e}")
    assert err <= 4 * R.ULP32 * L
    assert not np.any((ref["sdf"] < 0) != (exact < 0))
    assert not np.any(ref["feature"] & (R.BOUNDARY | R.NONMANIFOLD))
    assert (ref["feature"] & 0x0f).max() == 2 and (ref["feature"] & 0x0f).min() == 0   # all three classes occur


def test_restatement_on_a_concave_closed_mesh():
    """A 48 x 24 torus: the mesh lies within the sum of the two sagittas (0.00321) of the analytic torus, so signs must
    agree wherever |analytic| exceeds it, and the distances differ by at most it (measured: 0.00319)."""
    V, F = R.torus_mesh()
    rng = np.random.default_rng(1)
    P = (np.array([0.3, -0.2, 0.4]) + rng.uniform(-0.9, 0.9, (20000, 3)) * np.array([1.0, 1.0, 0.5])).astype(np.float32)
    ref = R.mesh_sdf(P, V, F)
    exact = R.torus_sdf(P)
    sag = R.torus_sagittas()
    assert abs(sag - 0.00321) < 1e-5
    clear = np.abs(exact) > sag
    dev = np.abs(ref["sdf"] - exact).max()
    print(f"torus: max |restatement - analytic| = {dev:.5f}, sagittas {sag:.5f}")
    assert not np.any((ref["sdf"][clear] < 0) != (exact[clear] < 0))
    assert dev <= sag + 1e-6
    assert not np.any(ref["feature"] & (R.BOUNDARY | R.NONMANIFOLD))
    assert (ref["sdf"] < 0).mean() > 0.02                                               # the inside is sampled


def test_restatement_flags_the_rim_of_an_open_mesh():
    """An open height field: exactly the queries whose closest point is on the rim carry the boundary bit."""
    V, F, rim = R.height_field()
    rng = np.random.default_rng(2)
    P = rng.uniform(-1.0, 1.0, (8000, 3)).astype(np.float32) * np.array([0.9, 0.7, 0.4], np.float32)
    ref = R.mesh_sdf(P, V, F)
    flagged = (ref["feature"] & R.BOUNDARY) != 0
    rimmed = R.on_rim(ref["closest"], rim)
    assert flagged.any() and (~flagged).any()
    assert np.array_equal(flagged, rimmed)
    assert not np.any(ref["feature"] & R.NONMANIFOLD)


def test_restatement_skips_degenerate_faces_and_flags_duplicates():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0]], np.float32)
    F = np.array([[0, 1, 3], [0, 1, 2], [0, 0, 2], [0, 1, 7], [0, 1, 4], [0, 1, 2]], np.int64)
    assert R.valid_faces(V, F).tolist() == [False, True, False, False, False, True]
    ref = R.mesh_sdf(np.array([[0.2, 0.2, 0.5], [0.5, -1.0, 0.0], [np.inf, 0, 0]], np.float32), V, F)
    assert ref["face"].tolist() == [1, 1, -1]                       # the lowest index of the two copies
    assert abs(ref["sdf"][0] - 0.5) < 1e-12 and np.isnan(ref["sdf"][2])
    assert ref["feature"][1] == 1                     # an edge; the two copies give it two faces: no flag
    # three faces on one edge: non-manifold
    V = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0], [0.5, 0, 1]], np.float32)
    F = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)
    ref = R.mesh_sdf(np.array([[0.5, 0.0, -0.5]], np.float32), V, F)
    assert ref["feature"][0] == 1 | R.NONMANIFOLD and abs(abs(ref["sdf"][0]) - 0.5) < 1e-12


def test_load_obj_round_trip(tmp_path):
    from bnv_fusion_amd import mesh
    path = tmp_path / "m.obj"
    path.write_text("# comment\nmtllib x.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0 0.5\nvn 0 0 1\nvt 0 0\n"
                    "f 1/1/1 2/1/1 3/1/1 4/1/1\n"          # a quad with a/b/c corners
                    "v 0.5 0.5 1\n"
                    "f -1 1 2\n"                            # a negative index: the vertex just read
                    "f 2//1 3//1 5//1\n"
                    "g group\ns off\nf 3/1 4/1 5/1 1/1 2/1\n")   # a pentagon
    m = mesh.load_obj(str(path))
    assert m.vertices.dtype == np.float32 and m.vertices.shape == (5, 3)
    assert np.array_equal(m.vertices[4], np.array([0.5, 0.5, 1], np.float32))
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [1, 2, 4], [2, 3, 4], [2, 4, 0], [2, 0, 1]]
    # what TriMesh holds survives a write as OBJ and a read back
    out = tmp_path / "o.obj"
    with open(out, "w") as fh:
        for v in m.vertices:
            fh.write("v %r %r %r\n" % tuple(float(x) for x in v))
        for f in m.faces:
            fh.write("f %d %d %d\n" % tuple(int(i) + 1 for i in f))
    back = mesh.load_obj(str(out))
    assert np.array_equal(back.vertices, m.vertices) and np.array_equal(back.faces, m.faces)
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        mesh.load_obj(str(bad))
    bad.write_text("v 0 0 0\nv 1 0 0\nf 1 2\n")
    with pytest.raises(ValueError):
        mesh.load_obj(str(bad))


def test_mesh_sdf_entries_validate_arguments_without_a_gpu():
    """Null pointers, non-positive counts and a short workspace are BNV_ERR_INVALID_ARGUMENT before any HIP call."""
    from bnv_fusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    INVALID = -1
    p = C.c_void_p(256)                                   # never dereferenced: every call below is refused first
    n = C.c_int64()
    assert lib.bnv_mesh_sdf_workspace_bytes(8, 12, C.byref(n)) == 0 and n.value > 0
    need = n.value
    big = C.c_int64()
    assert lib.bnv_mesh_sdf_workspace_bytes(80, 120, C.byref(big)) == 0 and big.value > need
    assert lib.bnv_mesh_sdf_workspace_bytes(8, 12, None) == INVALID
    assert lib.bnv_mesh_sdf_workspace_bytes(0, 12, C.byref(n)) == INVALID
    assert lib.bnv_mesh_sdf_workspace_bytes(8, 0, C.byref(n)) == INVALID
    assert lib.bnv_mesh_sdf_workspace_bytes(8, 1 << 40, C.byref(n)) == INVALID
    assert lib.bnv_mesh_sdf_build(None, 8, p, 12, p, need, None) == INVALID
    assert lib.bnv_mesh_sdf_build(p, 8, None, 12, p, need, None) == INVALID
    assert lib.bnv_mesh_sdf_build(p, 8, p, 12, None, need, None) == INVALID
    assert lib.bnv_mesh_sdf_build(p, 0, p, 12, p, need, None) == INVALID
    assert lib.bnv_mesh_sdf_build(p, 8, p, -1, p, need, None) == INVALID
    assert lib.bnv_mesh_sdf_build(p, 8, p, 12, p, need - 1, None) == INVALID
    assert lib.bnv_mesh_sdf_query(None, need, p, 4, p, p, p, p, None) == INVALID
    assert lib.bnv_mesh_sdf_query(p, need, None, 4, p, p, p, p, None) == INVALID
    assert lib.bnv_mesh_sdf_query(p, need, p, 4, None, p, p, p, None) == INVALID
    assert lib.bnv_mesh_sdf_query(p, need, p, 0, p, p, p, p, None) == INVALID
    assert lib.bnv_mesh_sdf_query(p, 16, p, 4, p, p, p, p, None) == INVALID


def test_patch_cutter_refuses_the_cpu():
    import torch
    from bnv_fusion_amd import evaluate, patches
    V, F, _ = R.box_mesh((0, 0, 0), np.eye(3), (0.1, 0.1, 0.1), n=2)
    from bnv_fusion_amd.mesh import TriMesh
    with pytest.raises(ValueError, match="GPU only"):
        patches.cut_local_patches(TriMesh(V, F), 0.02, 1000, device="cpu")
    with pytest.raises(ValueError, match="CPU tensor"):
        patches.cut_local_patches(torch.from_numpy(V), 0.02, 1000, faces=torch.from_numpy(F))
    with pytest.raises(ValueError, match="GPU only"):
        evaluate.MeshSDF(TriMesh(V, F), device="cpu")
    with pytest.raises(ValueError, match="CPU tensor"):
        evaluate.mesh_sdf(torch.zeros(4, 3), torch.from_numpy(V), torch.from_numpy(F))
