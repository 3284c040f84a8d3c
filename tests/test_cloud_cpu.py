"""The numpy restatement of the point-cloud normals (tests/cloud_restatement.py; include/bnv_fusion.h, "Point-cloud
normals") pinned on the CPU: its neighbour sets against a brute-force sort, its Jacobi normal against numpy.linalg.eigh,
its normals against the depth front end's, its rejection rules, and the PLY loader.  The GPU kernel is held to the
restatement bit for bit in tests/test_gpu_cloud.py."""
import numpy as np
import pytest

import cloud_cases as cases
import cloud_restatement as R


def _sets(points, k, max_radius=None):
    idx, m = R.neighbors(points, k, max_radius)
    return [[int(j) for j in idx[i, :m[i]]] for i in range(len(points))]


@pytest.mark.parametrize("max_radius", [None, 1.0, 1.5])
def test_neighbour_sets_on_the_tie_lattice(max_radius):
    """5 x 5 x 5 integer points: 6 neighbours at d2 = 1, 12 at 2, 8 at 3 ... -- the k-th place is almost always tied."""
    p = cases.lattice(5)
    for k in (8, 16, 32):
        got, want = _sets(p, k, max_radius), R.brute_force_neighbors(p, k, max_radius)
        assert got == want
        assert all(row[0] == i for i, row in enumerate(got))             # a point is its own first neighbour
    if max_radius == 1.0:
        assert max(len(r) for r in _sets(p, 32, max_radius)) == 7         # d2 <= 1: itself and the 6 axis neighbours


def test_neighbour_sets_of_random_points():
    p = cases.random_cloud(300, 1)
    p[[4, 250]] = np.nan
    for k, radius in ((8, None), (10, None), (16, 0.2), (32, None)):
        got, want = _sets(p, k, radius), R.brute_force_neighbors(p, k, radius)
        assert got == want
    assert got[4] == [] and all(4 not in row and 250 not in row for row in got)


@pytest.fixture(scope="module")
def frames():
    """Per frame size: the points, the front end's normals, and the neighbours for k = 24 -- whose first 8 and 16
    columns are the neighbours for k = 8 and 16 (the list is sorted and there is no radius)."""
    out = {}
    for H, W in ((60, 80), (120, 160)):
        pts = cases.frame_points(H, W)
        out[(H, W)] = (pts, R.neighbors(pts[:, :3], 24))
    return out


def _prefix(nbrs, k):
    idx, m = nbrs
    return idx[:, :k], np.minimum(m, k).astype(np.int32)


@pytest.mark.parametrize("size", [(60, 80), (120, 160)])
def test_normal_against_eigh(frames, size):
    """|n x n_eigh| of the restatement's normal against numpy.linalg.eigh of the same covariance, bar 1e-12: a few eps
    over the smallest relative eigenvalue gap (0.10 on these inputs) is ~2e-14.

    Measured maximum over both frames and k = 8, 16, 24: 1.6e-15 (six sweeps; four already give it, three leave 4e-6);
    smallest relative gap (lambda_1 - lambda_0) / lambda_2: 0.10."""
    pts, nbrs = frames[size]
    worst, gap = 0.0, np.inf
    for k in (8, 16, 24):
        r = R.estimate_normals(pts[:, :3], cases.CAMERA0, k=k, nbrs=_prefix(nbrs, k))
        assert r["status"][0] == 0
        lam, V = np.linalg.eigh(r["cov"])
        cross = np.linalg.norm(np.cross(r["normal64"], V[:, :, 0]), axis=1)
        worst = max(worst, float(cross.max()))
        gap = min(gap, float(((lam[:, 1] - lam[:, 0]) / lam[:, 2]).min()))
        assert np.abs(r["lam"] - lam).max() <= 1e-12 * lam.max()
        assert np.abs(np.linalg.norm(r["normal64"], axis=1) - 1.0).max() < 1e-14
    print(f"{size}: max |n x n_eigh| = {worst:.3g}, smallest relative gap = {gap:.3g}")
    assert worst < 1e-12


def test_agreement_with_the_front_end(frames):
    """The orientation convention and the fit are the ones the encoder was trained on: synthetic.frame(0, 120, 160)
    (19,200 points), origin = the camera centre, k = 16, against the front end's Sobel normals.

    The restatement's own figures: same side 100 %, median angle 2.51 degrees, within 15 degrees 99.61 % (60 x 80:
    100 %, 4.01 degrees, 96.92 %) -- the figures a float64 k-d tree and eigh gave (100 %, 2.5 degrees, 99.6 %; 96.9 %)."""
    figures = {}
    for size in ((60, 80), (120, 160)):
        pts, nbrs = frames[size]
        r = R.estimate_normals(pts[:, :3], cases.CAMERA0, k=16, nbrs=_prefix(nbrs, 16))
        n = r["input_pts"][:, 3:].astype(np.float64)
        assert np.isfinite(n).all() and (r["input_pts"][:, :3] == pts[:, :3]).all()
        cos = (n * pts[:, 3:].astype(np.float64)).sum(1)
        ang = np.degrees(np.arccos(np.clip(np.abs(cos), 0.0, 1.0)))
        figures[size] = ((cos > 0).mean(), float(np.median(ang)), (ang[cos > 0] < 15.0).sum() / len(cos))
        print(f"{size}: same side {figures[size][0]:.4%}, median angle {figures[size][1]:.3f} deg, "
              f"within 15 deg {figures[size][2]:.4%}")
        # away from the sensor
        assert ((n * (pts[:, :3].astype(np.float64) - cases.CAMERA0[0].astype(np.float64))).sum(1) >= 0).all()
    same, _, within = figures[(120, 160)]
    assert same >= 0.999 and within >= 0.98


def test_rejection_and_degenerate_inputs():
    c = cases.degenerate_cases()

    def run(name):
        p, o, oi, kw = c[name]
        return p, R.estimate_normals(p, o, oi, **kw)

    for n in (1, 2, 5):                                   # fewer points than min_neighbors
        p, r = run(f"N={n}")
        assert np.isnan(r["input_pts"]).all() and np.isnan(r["variation"]).all()
        assert (r["n_neighbors"] == n).all() and list(r["status"]) == [n, 0, 0, 0]
    p, r = run("coincident")                              # lambda_2 = 0
    assert np.isnan(r["input_pts"]).all() and (r["n_neighbors"] == 16).all() and r["status"][0] == 40
    p, r = run("collinear")                               # lambda_1 is rounding noise
    assert np.isnan(r["input_pts"]).all() and (r["n_neighbors"] == 16).all() and r["status"][0] == 50
    p, r = run("nan rows")
    bad = ~np.isfinite(p).all(1)
    assert bad.sum() == 7 and np.isnan(r["input_pts"][bad]).all() and (r["n_neighbors"][bad] == 0).all()
    assert np.isfinite(r["input_pts"][~bad]).all() and r["status"][0] == 7
    idx, m = R.neighbors(p, 16)
    assert not np.isin(idx[~bad], np.flatnonzero(bad)).any()       # a non-finite row is nobody's neighbour
    p, r = run("all nan")
    assert np.isnan(r["input_pts"]).all() and list(r["status"]) == [9, 0, 0, 0] and (r["n_neighbors"] == 0).all()
    p, r = run("radius below spacing")                    # everyone is alone
    assert np.isnan(r["input_pts"]).all() and (r["n_neighbors"] == 1).all() and r["status"][0] == len(p)
    p, r = run("radius one spacing")                      # itself + its axis neighbours: 4 (corner) to 7 (inside)
    nn = r["n_neighbors"]
    assert nn.min() == 4 and nn.max() == 7
    # a corner's 4 points span a plane's worth (a tetrahedron: no eigenvalue vanishes) and are accepted
    assert np.isfinite(r["input_pts"]).all()
    p, r = run("bad origin index")
    oi = c["bad origin index"][2]
    bad = (oi < 0) | (oi >= 3)
    assert bad.sum() == 3 and np.isnan(r["input_pts"][bad]).all() and np.isfinite(r["input_pts"][~bad]).all()
    assert list(r["status"]) == [3, 3, 0, 0] and (r["n_neighbors"][bad] == 10).all()
    n64, o64 = r["normal64"][~bad], cases.ORIGINS3[oi[~bad]].astype(np.float64)
    assert ((n64 * (p[~bad].astype(np.float64) - o64)).sum(1) >= 0).all()
    p, r = run("two clusters")                            # the 4 far points find only each other within the radius
    assert (r["n_neighbors"][-4:] == 4).all() and np.isnan(r["input_pts"][-4:]).all()
    assert np.isfinite(r["input_pts"][:-4]).all() and r["status"][0] == 4
    p, r = run("two clusters, no radius")                 # without one they reach into the big cluster: 16 each
    assert (r["n_neighbors"] == 16).all()


def test_orientation_keeps_the_solver_sign_on_an_exact_zero():
    """Points of the plane z = 0 seen from an origin IN that plane: dot(n, p - o) is exactly 0 and nothing is flipped;
    from either side the normal points away from the origin."""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 2)
    p = np.concatenate([g, np.zeros((36, 1))], 1).astype(np.float32)
    nbrs = R.neighbors(p, 9)
    zero = R.estimate_normals(p, [[2.0, 3.0, 0.0]], k=9, nbrs=nbrs)["input_pts"][:, 3:]
    below = R.estimate_normals(p, [[2.0, 3.0, -4.0]], k=9, nbrs=nbrs)["input_pts"][:, 3:]
    above = R.estimate_normals(p, [[2.0, 3.0, 4.0]], k=9, nbrs=nbrs)["input_pts"][:, 3:]
    assert (below == [0.0, 0.0, 1.0]).all() and (above == [0.0, 0.0, -1.0]).all()
    assert (np.abs(zero) == [0.0, 0.0, 1.0]).all() and (zero[:, 2] == 1.0).all()     # V starts as the identity


def test_load_cloud_round_trip(tmp_path):
    from bnv_fusion_amd import load_cloud
    from bnv_fusion_amd.mesh import TriMesh
    pts = cases.random_cloud(57, 8)
    nrm = cases.random_cloud(57, 9)
    m = TriMesh(pts, np.zeros((0, 3), np.int64))
    p1, n1 = load_cloud(m.export(str(tmp_path / "points.ply")))
    assert p1.dtype == np.float32 and p1.tobytes() == pts.tobytes() and n1 is None
    m.vertex_normals = nrm
    p2, n2 = load_cloud(m.export(str(tmp_path / "oriented.ply")))
    assert p2.tobytes() == pts.tobytes() and n2.dtype == np.float32 and n2.tobytes() == nrm.tobytes()
    ascii_ply = tmp_path / "ascii.ply"
    ascii_ply.write_text("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                         "end_header\n0 0.5 1\n-1 2 3.25\n")
    p3, n3 = load_cloud(str(ascii_ply))
    assert p3.tolist() == [[0.0, 0.5, 1.0], [-1.0, 2.0, 3.25]] and n3 is None


def test_size_entry_and_refusals_without_a_gpu():
    """The size entry is pure host code and every bad argument is refused before any HIP call."""
    import ctypes as C
    import os
    from bnv_fusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    INVALID, TOO_SMALL = -1, -2
    n = C.c_int64(-1)
    assert lib.bnv_cloud_normals_bytes(1, C.byref(n)) == 0 and n.value > 0 and n.value % 256 == 0
    small = n.value
    assert lib.bnv_cloud_normals_bytes(100000, C.byref(n)) == 0 and n.value > small and n.value % 256 == 0
    assert n.value < 100 * 100000                               # ~84 B per point
    for bad in (0, -1, 2 ** 31 - 2):
        assert lib.bnv_cloud_normals_bytes(bad, C.byref(n)) == INVALID
    assert lib.bnv_cloud_normals_bytes(10, None) == INVALID
    assert lib.bnv_cloud_normals_bytes(2 ** 31 - 3, C.byref(n)) == 0 and n.value > 2 ** 37
    p8 = C.c_void_p(8)                                          # a non-null pointer no refused call dereferences
    assert lib.bnv_cloud_normals_bytes(100, C.byref(n)) == 0

    def call(points=p8, n_points=100, k=16, radius=0.0, min_nb=6, origins=p8, n_origins=1, ws=p8, ws_bytes=None,
             out=p8, status=p8):
        return lib.bnv_cloud_normals(points, n_points, k, radius, min_nb, origins, n_origins, None, ws,
                                     n.value if ws_bytes is None else ws_bytes, out, None, None, status, None)

    for kw in (dict(points=None), dict(origins=None), dict(ws=None), dict(out=None), dict(status=None),
               dict(n_points=0), dict(n_points=2 ** 31 - 2), dict(n_origins=0), dict(k=7), dict(k=33), dict(min_nb=2),
               dict(min_nb=17), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf"))):
        assert call(**kw) == INVALID, kw
    assert call(ws_bytes=n.value - 1) == TOO_SMALL
    assert call(ws_bytes=0) == TOO_SMALL


def test_python_argument_checks_come_before_the_device():
    import torch
    from bnv_fusion_amd import estimate_normals, pointcloud
    with pytest.raises(ValueError, match="no CPU fallback"):
        estimate_normals(torch.zeros((10, 3)), [[0.0, 0.0, 0.0]])
    with pytest.raises(TypeError):
        estimate_normals(np.zeros((10, 3), np.float32), [[0.0, 0.0, 0.0]])
    assert pointcloud.cloud_chunks(10, 4) == [(0, 4), (4, 8), (8, 10)]
    assert pointcloud.cloud_chunks(5) == [(0, 5)]
    with pytest.raises(ValueError):
        pointcloud.cloud_chunks(5, 0)
    with pytest.raises(ValueError):
        pointcloud.cloud_chunks(5, pointcloud.ENCODER_MAX_POINTS + 1)
