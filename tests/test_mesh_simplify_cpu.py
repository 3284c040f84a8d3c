"""Mesh simplification without a GPU: the restatement of the specification (tests/mesh_simplify_restatement.py, the
definition) and the host function mesh.simplify_mesh (the path the device is held to) agree bit for bit; the structural
invariants of the output; the two degenerate ends of the cell size; planes, where both placements are exact or within
a few float32 ulp; cube corners, which the quadric placement recovers and the mean rounds off; and the errors."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401
import mesh_simplify_restatement as rs
import register_restatement as reg

PLACEMENTS = ("quadric", "mean")


def host(v, f, cell, placement="quadric", min_det=1e-3):
    from bnv_fusion_amd import mesh as M
    out = M.simplify_mesh(M.TriMesh(v, f), cell, placement, min_det)
    assert out.vertices.dtype == np.float32 and out.faces.dtype == np.int64
    return out.vertices, out.faces


def assert_same(got, want):
    assert got[0].shape == want[0].shape, (got[0].shape, want[0].shape)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), int((got[0] != want[0]).sum())
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1])


SMALL = [("tetrahedron", *rs.tetrahedron(), (0.05, 0.6, 4.0)),
         ("box432", *reg.box(), (0.01, 0.12, 0.3)),
         ("sphere", *rs.uv_sphere(n_lat=12, n_lon=20), (0.01, 0.11, 0.35)),
         ("strip255", *rs.strip(255), (0.004, 0.05)),
         ("strip256", *rs.strip(256), (0.05,)),
         ("strip257", *rs.strip(257), (0.05, 100.0)),
         ("fan300", *rs.fan(300), (0.01, 1.0)),
         ("adversarial", *rs.adversarial(0.125), (0.03, 0.125, 0.25))]


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c[0])
def test_host_function_equals_the_restatement(case, placement):
    _, v, f, cells = case
    for h in cells:
        assert_same(host(v, f, h, placement), rs.simplify(v, f, h, placement))


def test_host_function_equals_the_restatement_across_min_det():
    v, f = reg.box()
    counts = []
    for md in (0.0, 1e-6, 1e-3, 0.5, 1e9):
        want = rs.simplify(v, f, 0.12, "quadric", md, return_info=True)
        assert_same(host(v, f, 0.12, "quadric", md), want[:2])
        counts.append(int(want[2]["quadric"].sum()))
    assert counts[0] >= counts[2] > counts[-1] == 0 and counts == sorted(counts, reverse=True)
    assert_same(host(v, f, 0.12, "quadric", 1e9), rs.simplify(v, f, 0.12, "mean"))      # every cluster falls back


def check_invariants(v, f, cell, placement):
    (vo, fo, info) = rs.simplify(v, f, cell, placement, return_info=True)
    assert len(fo) > 0
    assert ((fo[:, 0] != fo[:, 1]) & (fo[:, 1] != fo[:, 2]) & (fo[:, 0] != fo[:, 2])).all()
    lo = np.argmin(fo, axis=1)
    rot = np.take_along_axis(fo, (lo[:, None] + np.arange(3)[None]) % 3, axis=1)
    assert len(np.unique(rot, axis=0)) == len(fo)                                      # no cyclic triple twice
    assert np.array_equal(np.unique(fo), np.arange(len(vo)))                           # every vertex referenced
    keys = [rs.cell_key(i) for i in info["cells"].tolist()]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)                        # vertex keys ascend
    centre = (info["cells"].astype(np.float64) + 0.5) * cell
    # within the cell dilated to twice its size (|x| <= h about the centre), up to the float32 rounding of the output
    slack = np.spacing(np.abs(vo).max().astype(np.float32)).astype(np.float64)
    assert (np.abs(vo.astype(np.float64) - centre) <= cell + slack).all()
    if placement == "mean":                                                            # a mean stays in its own cell
        assert (np.abs(vo.astype(np.float64) - centre) <= 0.5 * cell + slack).all()
    return len(vo), len(fo)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("mesh", ["sphere", "box432"])
def test_structural_invariants(mesh, placement):
    v, f = rs.uv_sphere() if mesh == "sphere" else reg.box()
    assert len(f) == (2208 if mesh == "sphere" else 432)
    sizes = [check_invariants(v, f, cell, placement) for cell in (0.05, 0.11, 0.23)]
    assert sizes[0][1] > sizes[1][1] > sizes[2][1]


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_identity_end_keeps_the_mesh(placement):
    """h below the smallest vertex spacing, no two vertices in one cell: the input's faces after the face step, the
    vertices bit-equal to the input's.  (The quadric runs with min_det large enough to force the fallback: a one-vertex
    cluster at a sharp corner may legitimately be moved by its quadric.)"""
    v, f = rs.adversarial(0.125)
    keep = np.unique(v, axis=0, return_index=True)[1]
    v = v[np.sort(keep)]
    f = f[(f < len(v)).all(1)]
    h = 1e-4
    idx = np.floor(v.astype(np.float64) / h).astype(np.int64)
    assert len(np.unique(idx, axis=0)) == len(v)
    vo, fo = rs.simplify(v, f, h, placement, min_det=1e30 if placement == "quadric" else 1e-3)
    kept = f[rs.face_step(f)]
    used = np.unique(kept)
    order = used[np.argsort([rs.cell_key(i) for i in idx[used].tolist()], kind="stable")]
    assert np.array_equal(vo.view(np.uint32), v[order].view(np.uint32))
    remap = np.full(len(v), -1, np.int64)
    remap[order] = np.arange(len(order))
    assert np.array_equal(fo, remap[kept])
    assert_same(host(v, f, h, placement, 1e30 if placement == "quadric" else 1e-3), (vo, fo))


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_one_cell_end_is_an_empty_mesh(placement):
    v, f = rs.uv_sphere(radius=0.4, centre=(0.5, 0.5, 0.5), n_lat=8, n_lon=12)
    assert v.min() > 0
    for fn in (rs.simplify, host):
        vo, fo = fn(v, f, 1.0, placement)[:2]
        assert vo.shape == (0, 3) and fo.shape == (0, 3)


def jittered_grid(n=20, seed=3):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    g = (g + rng.uniform(-0.3, 0.3, size=g.shape)) * 0.05
    i = np.arange(n * n).reshape(n, n)
    a, b, c, d = i[:-1, :-1], i[1:, :-1], i[1:, 1:], i[:-1, 1:]
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return g, f.astype(np.int64)


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_axis_aligned_plane_is_exact(placement):
    g, f = jittered_grid()
    v = np.concatenate([g, np.full((len(g), 1), 0.25)], 1).astype(np.float32)
    for h in (0.11, 0.2):
        vo, fo = rs.simplify(v, f, h, placement)
        assert len(fo) > 8 and (vo[:, 2] == np.float32(0.25)).all()      # k copies summed and divided by k: exact
        assert_same(host(v, f, h, placement), (vo, fo))


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_tilted_plane_within_4_ulp(placement):
    g, f = jittered_grid()
    nrm = np.array([0.3, -0.5, 0.81])
    nrm /= np.linalg.norm(nrm)
    z = (0.4 - g @ nrm[:2]) / nrm[2]
    v = np.concatenate([g, z[:, None]], 1).astype(np.float32)
    # the plane the float32 vertices lie on to their own rounding
    for h in (0.11, 0.2):
        vo, fo = rs.simplify(v, f, h, placement)
        assert len(fo) > 8
        dist = np.abs(vo.astype(np.float64) @ nrm - 0.4)
        ulp = np.spacing(np.float32(np.abs(v).max())).astype(np.float64)
        print(f"tilted plane, {placement}, h = {h}: max distance {dist.max() / ulp:.3f} ulp")
        assert dist.max() <= 4 * ulp


def cube_corner_errors(h=0.25):
    """The eight vertices nearest the true corners of the tessellated axis-aligned cube, under both placements."""
    lo, hi = np.array([-0.31, -0.27, -0.22]), np.array([0.33, 0.29, 0.24])
    v, f = rs.box(n=16, lo=lo, hi=hi)
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    # the cell size puts several vertices of every corner's three sides into the corner's cell
    idx = np.floor(v.astype(np.float64) / h).astype(np.int64)
    for c in corners:
        ci = np.floor(c / h).astype(np.int64)
        assert int((idx == ci).all(1).sum()) >= 7
    err = {}
    for placement in PLACEMENTS:
        vo, _ = rs.simplify(v, f, h, placement)
        d = np.linalg.norm(vo.astype(np.float64)[None] - corners[:, None], axis=2)     # [8, V']
        err[placement] = d.min(1)
        assert len(set(d.argmin(1).tolist())) == 8
    return err


def test_cube_corners_quadric_recovers_them_and_the_mean_does_not():
    err = cube_corner_errors()
    print("cube corners: quadric error", err["quadric"].max(), "m; mean displacement", err["mean"].min(), "m")
    assert err["quadric"].max() <= 1e-6
    assert err["mean"].min() > 0.05                                  # (read off the restatement: 0.098 to 0.122 m)
    assert (err["quadric"] * 100 <= err["mean"]).all()


def test_unreferenced_vertices_count_in_the_mean_only():
    v, f = rs.tetrahedron()
    extra = np.concatenate([v, v[:1] + np.float32(0.01)]).astype(np.float32)          # in vertex 0's cell, no face
    a, b = rs.simplify(v, f, 0.25, "mean"), rs.simplify(extra, f, 0.25, "mean")
    assert np.array_equal(a[1], b[1]) and not np.array_equal(a[0], b[0])
    qa, qb = rs.simplify(v, f, 0.25, "quadric", 0.0), rs.simplify(extra, f, 0.25, "quadric", 0.0)
    assert_same(qa, qb)                                               # every cluster takes its quadric: no mean in it


def test_errors():
    from bnv_fusion_amd import mesh as M
    v, f = rs.tetrahedron()

    def both(vv, ff, *args):
        with pytest.raises(ValueError):
            rs.simplify(vv, ff, *args)
        with pytest.raises(ValueError):
            M.simplify_mesh(M.TriMesh(vv, ff), *args)

    for cell in (0.0, -1.0, float("nan"), float("inf")):
        both(v, f, cell)
    for md in (-1e-9, float("nan"), float("inf")):
        both(v, f, 0.1, "quadric", md)
    both(v, f, 0.1, "median")
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = v.copy()
        w[2, 1] = bad
        both(w, f, 0.1)
    both(v, f + 1, 0.1)
    both(v, f - 1, 0.1)
    both(v[:0], f, 0.1)
    both(v, f, 1.25 / 2 ** 20)                                        # |x| / h >= 2^20 (float32(1.3) > 1.25)
    w = v.copy()
    w[0, 0] = -4.0
    both(w, f, 4.0 / 2 ** 20)                                         # -2^20 cells exactly: refused
    rs.simplify(w, f, 4.0 / 2 ** 20 * (1 + 2.0 ** -20))               # just inside
    M.simplify_mesh(M.TriMesh(w, f), 4.0 / 2 ** 20 * (1 + 2.0 ** -20))
