"""The mesh signed-distance kernels (csrc/meshsdf.hip, evaluate.MeshSDF) against the float64 restatement
(tests/mesh_sdf_restatement.py), for every query of every case.

Tolerance: |sdf_gpu - sdf_ref| <= TOL_REL * 2^-23 * L, L the largest absolute coordinate of the case (vertices and
queries).  TOL_REL comes from a plain numpy-float32 evaluation of the same formulas (``mesh_sdf(dtype=np.float32)``:
one rounding per operation) against the float64 brute force on the cases below; its largest |error| / (2^-23 L):

    box 0.723   torus 0.533   height_field 0.522   sequence.gt_mesh 0.212   synthetic.gt_mesh(8) 0.403
    duplicates_and_degenerates 0.621   single_triangle 0.760   far_queries 0.787        (no sign flip in any of them)

The worst is 0.787; a different but legitimate operation order gets a margin of 4x: TOL_REL = 4 * 0.787 = 3.15.
"""
import functools

import numpy as np
import pytest
import torch

import mesh_sdf_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_REL = 3.15
CASES = ("box", "torus", "height_field", "sequence.gt_mesh", "synthetic.gt_mesh(8)", "duplicates_and_degenerates",
         "single_triangle", "far_queries")


@functools.lru_cache(maxsize=None)
def _cases():
    return {name: (V, F, P) for name, V, F, P in R.kernel_cases()}


@functools.lru_cache(maxsize=None)
def _reference(name):
    V, F, P = _cases()[name]
    return R.mesh_sdf(P, V, F)


def _tensors(V, F):
    # a NaN vertex and out-of-range indices are part of one case: device tensors pass them through unchanged
    return torch.from_numpy(np.ascontiguousarray(V, np.float32)).to(DEV), torch.from_numpy(F.astype(np.int32)).to(DEV)


def _gpu(V, F, P):
    from bnv_fusion_amd import evaluate
    v, f = _tensors(V, F)
    out = evaluate.MeshSDF(v, f).query(torch.from_numpy(P).to(DEV))
    return [t.cpu().numpy() for t in out]


def test_cases_are_the_ones_listed():
    assert tuple(_cases()) == CASES


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_float64_restatement(name):
    V, F, P = _cases()[name]
    ref = _reference(name)
    sdf, face, closest, feature = _gpu(V, F, P)
    L = R.largest_coordinate(V, P)
    tol = TOL_REL * R.ULP32 * L
    err = np.abs(sdf.astype(np.float64) - ref["sdf"])
    sure = ref["second"] - np.abs(ref["sdf"]) > tol          # the reference's two best candidates differ by more
    print(f"\n{name}: {len(P)} queries, L = {L:.3f}, max |sdf - ref| = {err.max():.3e} = "
          f"{err.max() / (R.ULP32 * L):.3f} x 2^-23 L (allowed {TOL_REL}), unambiguous {sure.mean():.3f}, "
          f"feature mismatches there {(feature[sure] != ref['feature'][sure]).sum()}, "
          f"face mismatches there {(face[sure] != ref['face'][sure]).sum()}")
    assert sdf.dtype == np.float32 and face.dtype == np.int32 and feature.dtype == np.uint8
    assert np.isfinite(sdf).all()
    assert (err <= tol).all()                                # EVERY query, through the signed value
    # the reported closest point is where the distance is measured to
    d = np.linalg.norm(P.astype(np.float64) - closest.astype(np.float64), axis=1)
    assert (np.abs(d - np.abs(sdf)) <= tol).all()
    assert np.array_equal(face[sure], ref["face"][sure])
    assert np.array_equal(feature[sure] & 0x0f, ref["feature"][sure] & 0x0f)
    assert np.array_equal(feature[sure] & R.BOUNDARY, ref["feature"][sure] & R.BOUNDARY)
    assert ((face >= 0) & (face < len(F))).all() and R.valid_faces(V, F)[face].all()


def test_non_finite_queries_get_nan_and_no_face():
    V, F, P = _cases()["torus"]
    P = P[:64].copy()
    P[3, 0], P[10, 1], P[20, 2], P[33] = np.nan, np.inf, -np.inf, np.nan
    bad = ~np.isfinite(P).all(1)
    sdf, face, closest, feature = _gpu(V, F, P)
    assert np.isnan(sdf[bad]).all() and (face[bad] == -1).all() and np.isnan(closest[bad]).all() and (feature[bad] == 0).all()
    ref = R.mesh_sdf(P, V, F)
    tol = TOL_REL * R.ULP32 * R.largest_coordinate(V, P)
    assert (np.abs(sdf[~bad] - ref["sdf"][~bad]) <= tol).all() and (face[~bad] >= 0).all()


def test_a_mesh_without_a_valid_face_answers_nan():
    V = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    sdf, face, _, _ = _gpu(V, np.array([[0, 1, 2], [0, 0, 1]], np.int64), np.zeros((5, 3), np.float32))
    assert np.isnan(sdf).all() and (face == -1).all()


@pytest.mark.parametrize("name", ["torus", "synthetic.gt_mesh(8)", "duplicates_and_degenerates"])
def test_two_builds_give_the_same_bits(name):
    from bnv_fusion_amd import evaluate
    V, F, P = _cases()[name]
    v, f = _tensors(V, F)
    q = torch.from_numpy(P).to(DEV)
    a = evaluate.MeshSDF(v, f).query(q)
    b = evaluate.MeshSDF(v, f).query(q)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8) if x.dtype == torch.uint8 else x.view(torch.int32),
                           y.view(torch.uint8) if y.dtype == torch.uint8 else y.view(torch.int32))
    # the index is reusable, leading dimensions are kept, the one-shot form agrees
    m = evaluate.MeshSDF(v, f)
    first = m.query(q)
    again = m.query(q.reshape(-1, 4, 3)[:50])
    assert again[0].shape == (50, 4) and again[2].shape == (50, 4, 3)
    assert torch.equal(again[0].reshape(-1).view(torch.int32), first[0][:200].view(torch.int32))
    one = evaluate.mesh_sdf(q, v, f)
    assert torch.equal(one[0].view(torch.int32), first[0].view(torch.int32)) and torch.equal(one[1], first[1])


@pytest.mark.parametrize("name", ["box", "torus", "height_field"])
def test_face_order_does_not_matter(name):
    V, F, P = _cases()[name]
    perm = np.random.default_rng(5).permutation(len(F))
    sdf, face, _, feature = _gpu(V, F, P)
    sdf_p, face_p, _, feature_p = _gpu(V, F[perm], P)
    tol = TOL_REL * R.ULP32 * R.largest_coordinate(V, P)
    assert (np.abs(sdf_p.astype(np.float64) - sdf) <= tol).all()
    ref = _reference(name)
    sure = ref["second"] - np.abs(ref["sdf"]) > tol
    assert np.array_equal(perm[face_p[sure]], face[sure])
    assert np.array_equal(feature_p[sure], feature[sure])


def test_trimesh_input_and_refusals():
    from bnv_fusion_amd import evaluate
    from bnv_fusion_amd.mesh import TriMesh
    V, F, P = _cases()["box"]
    m = evaluate.MeshSDF(TriMesh(V, F), device=DEV)
    sdf = m.query(torch.from_numpy(P[:100]).to(DEV))[0].cpu().numpy()
    assert np.array_equal(sdf, _gpu(V, F, P[:100])[0])
    with pytest.raises(ValueError, match="CPU tensor"):
        m.query(torch.from_numpy(P[:100]))
    with pytest.raises(ValueError):
        m.query(torch.zeros((0, 3), device=DEV))
    with pytest.raises(ValueError):
        m.query(torch.zeros((5, 2), device=DEV))
