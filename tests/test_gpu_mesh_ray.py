"""The ray caster and the depth sensor kernels (csrc/meshray.hip; scan.MeshScanner, scan.simulate_sensor) against the
float64 restatements of tests/mesh_ray_restatement.py.

Depth tolerance: |t_gpu - t_ref| <= TOL_REL * 2^-23 * L on every sure pixel, L the largest absolute coordinate of the
case (vertices and camera), TOL_REL = 17.08 from the float32 numpy evaluation of the kernel's formulas -- derived and
measured in tests/test_mesh_ray_cpu.py's docstring, as are "sure" pixels (cap: 0.1 % of a frame unsure) and the
sensor's DELTA.  The reference sees the kernel's own rays (``camera_rays(dtype=float32)``: exact float32 values) and
does everything after them in float64.  Faces are compared where the nearest other face is further off than the
tolerance (coplanar duplicates tie legitimately) and the float64 hit lies inside its triangle by more than BARY_MARGIN
in barycentric coordinates: a ray through a shared edge or vertex belongs to either neighbour, and fp32 places a hit
within a few 2^-23 L / (edge length) of its float64 place -- under 1e-4 for every mesh here (edges of L / 500 or more).
"""
import functools

import numpy as np
import pytest
import torch

import mesh_ray_restatement as R
import mesh_sdf_restatement as S
from test_mesh_ray_cpu import (BARY_MARGIN, FRAMES, SENSOR_DELTA, TOL_REL, UNSURE_CAP, legitimate_hits, near_boundary,
                                synthetic_subset)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_SMALL = np.array([[131.25, 0.0, 79.5], [0.0, 131.25, 59.5], [0.0, 0.0, 1.0]])      # 160 x 120


def _look_at(eye, target):
    from bnv_fusion_amd import scan
    return scan.look_at_pose(eye, target)


@functools.lru_cache(maxsize=None)
def _meshes():
    return {name: (V, F) for name, V, F, _ in S.kernel_cases()}


def _views():
    """name -> (V, F, K, T_wc, H, W)"""
    from bnv_fusion_amd import sequence
    m = _meshes()
    room = sequence.gt_mesh()
    views = {
        "box": m["box"] + (K_SMALL, _look_at((1.9, -1.1, 1.1), (1.0, -0.5, 2.0)), 120, 160),
        "box_inside": m["box"] + (K_SMALL, _look_at((1.02, -0.47, 2.03), (1.3, -0.2, 2.4)), 120, 160),
        "torus": m["torus"] + (K_SMALL, _look_at((1.4, -1.0, 1.3), (0.3, -0.2, 0.4)), 120, 160),
        "height_field": m["height_field"] + (K_SMALL, _look_at((0.3, -0.2, 1.2), (0.0, 0.0, 0.0)), 120, 160),
        "duplicates_and_degenerates": m["duplicates_and_degenerates"] +
        (K_SMALL, _look_at((0.2, -1.0, 1.3), (1.0, -0.5, 2.0)), 120, 160),
        "single_triangle": m["single_triangle"] + (K_SMALL, _look_at((0.5, 0.3, -1.5), (0.6, 0.45, 0.1)), 120, 160),
        "far_outside": m["torus"] + (K_SMALL, _look_at((9.0, -7.0, 12.0), (0.3, -0.2, 0.4)), 120, 160),
    }
    for t in FRAMES:
        views[f"room_{t}"] = (room.vertices, room.faces, sequence.intrinsics(), sequence.sweep_pose(t), 480, 640)
    return views


VIEWS = ("box", "box_inside", "torus", "height_field", "duplicates_and_degenerates", "single_triangle", "far_outside") + \
    tuple(f"room_{t}" for t in FRAMES)


@functools.lru_cache(maxsize=None)
def _reference(name):
    V, F, K, T, H, W = _views()[name]
    ok, _ = R.sure(K, T, H, W, V, F)
    o32, d32 = R.camera_rays(K, T, H, W, np.float32)
    return ok, R.brute_force(o32, d32, V, F), o32, d32


def _scanner(V, F):
    from bnv_fusion_amd import scan
    return scan.MeshScanner(torch.from_numpy(np.ascontiguousarray(V, np.float32)).to(DEV),
                            torch.from_numpy(np.asarray(F).astype(np.int32)).to(DEV))


def _inside(ref):
    """The float64 hit lies inside its triangle, away from its edges."""
    with np.errstate(invalid="ignore"):
        return np.minimum(np.minimum(ref["u"], ref["v"]), 1 - ref["u"] - ref["v"]) > BARY_MARGIN


def _tol(V, T):
    V = np.asarray(V, np.float64)
    L = max(float(np.abs(V[np.isfinite(V).all(1)]).max()), float(np.abs(np.asarray(T)[:3, 3]).max()))
    return TOL_REL * R.ULP32 * L


def test_views_are_the_ones_listed():
    assert tuple(_views()) == VIEWS


@pytest.mark.parametrize("name", VIEWS)
def test_render_and_cast_match_the_float64_restatement(name):
    V, F, K, T, H, W = _views()[name]
    ok, ref, o32, d32 = _reference(name)
    sc = _scanner(V, F)
    depth, face, nrm = (x.cpu().numpy() for x in sc.render_depth(T, K, H, W, normals=True))
    depth, face, nrm = depth.reshape(-1).astype(np.float64), face.reshape(-1), nrm.reshape(-1, 3).astype(np.float64)
    tol = _tol(V, T)
    hit_ref, hit = np.isfinite(ref["t"]), depth > 0
    both = ok & hit_ref & hit
    err = np.abs(depth - np.where(hit_ref, ref["t"], 0.0))
    clear = both & (ref["second"] - ref["t"] > tol) & _inside(ref)
    print(f"\n{name}: {H * W} pixels, unsure {100 * (1 - ok.mean()):.4f} %, hits {hit.mean():.3f}, max |t - ref| on sure "
          f"{err[both].max() if both.any() else 0:.3e} m = "
          f"{(err[both].max() if both.any() else 0) / (tol / TOL_REL):.3f} x 2^-23 L (allowed {TOL_REL}), hit / miss "
          f"flips on sure {(hit != hit_ref)[ok].sum()}, face mismatches where unambiguous "
          f"{(face[clear] != ref['face'][clear]).sum()}")
    assert 1 - ok.mean() <= UNSURE_CAP                          # else: a bad test input, not a pass
    assert hit_ref.any()
    assert np.array_equal(hit[ok], hit_ref[ok])
    assert (err[both] <= tol).all()
    assert np.array_equal(face[clear], ref["face"][clear])
    assert (face[~hit] == -1).all() and (nrm[~hit] == 0).all()
    valid = S.valid_faces(V, F)
    assert ((face[hit] >= 0) & (face[hit] < len(F))).all() and valid[face[hit]].all()
    # normals: unit, the face's, towards the camera
    assert np.abs(np.linalg.norm(nrm[hit], axis=1) - 1).max() < 1e-5
    dn = np.linalg.norm(d32[hit], axis=1)
    assert ((nrm[hit] * d32[hit]).sum(-1) <= 1e-6 * dn).all()
    P = np.asarray(V, np.float64)[np.asarray(F)[face[hit]]]
    gn = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    gn /= np.linalg.norm(gn, axis=1, keepdims=True)
    assert np.abs(np.abs((gn * nrm[hit]).sum(-1)) - 1).max() < 1e-5
    # cast() on the same rays: the same bits, and barycentrics that reproduce the hit point
    o = torch.from_numpy(np.broadcast_to(o32.astype(np.float32), d32.shape).copy()).to(DEV)
    t, cf, uv, flags = (x.cpu().numpy() for x in sc.cast(o, torch.from_numpy(d32.astype(np.float32)).to(DEV)))
    assert np.array_equal(t[hit].astype(np.float64), depth[hit]) and np.isnan(t[~hit]).all()
    assert np.array_equal(cf, face) and np.array_equal(flags != 0, hit) and np.isnan(uv[~hit]).all()
    u, v = uv[hit, 0].astype(np.float64), uv[hit, 1].astype(np.float64)
    point = (1 - u - v)[:, None] * P[:, 0] + u[:, None] * P[:, 1] + v[:, None] * P[:, 2]
    along = o32 + depth[hit][:, None] * d32[hit]
    assert (np.linalg.norm(point - along, axis=1) <= 4 * tol * dn)[both[hit]].all()
    assert (u >= -1e-5).all() and (v >= -1e-5).all() and (u + v <= 1 + 1e-5).all()
    cos = (gn * d32[hit]).sum(-1) / dn
    assert np.array_equal(((flags[hit] & 2) != 0)[np.abs(cos) > 1e-4], (cos > 0)[np.abs(cos) > 1e-4])


def test_many_triangles_subset():
    m, K, T, H, W, pix = synthetic_subset()
    o32, d32 = R.camera_rays(K, T, H, W, np.float32)
    ref = R.brute_force(o32, d32[pix], m.vertices, m.faces)
    sc = _scanner(m.vertices, m.faces)
    depth, face = (x.cpu().numpy().reshape(-1)[pix] for x in sc.render_depth(T, K, H, W))
    tol = _tol(m.vertices, T)
    err = np.abs(depth.astype(np.float64) - ref["t"])
    clear = (ref["second"] - ref["t"] > tol) & _inside(ref)
    print(f"\nsynthetic.gt_mesh(step_px=4): {len(m.faces)} faces, max |t - ref| {err.max():.3e} m = "
          f"{err.max() / (tol / TOL_REL):.3f} x 2^-23 L (allowed {TOL_REL}); faces compared at {clear.sum()} of "
          f"{len(pix)} pixels (the camera's pixel grid runs along the mesh's edges), mismatches there "
          f"{(face[clear] != ref['face'][clear]).sum()}, elsewhere {(face[~clear] != ref['face'][~clear]).sum()}")
    assert np.isfinite(ref["t"]).all() and (depth > 0).all()    # a smooth surface seen head-on: every pixel is sure
    assert (err <= tol).all()
    assert np.array_equal(face[clear], ref["face"][clear])


def _sphere(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


_aimed = R.aimed_directions


@pytest.mark.parametrize("name,origin", [("box", (1.02, -0.47, 2.03)), ("torus", (0.8, -0.2, 0.4))])
def test_watertight_from_inside(name, origin):
    """Inside a closed surface every ray hits it, so none may leak out between two faces: random directions, and
    directions aimed exactly at vertices and edge midpoints and within 2^-20 of them.  The float64 Moeller-Trumbore
    reference is not watertight: it loses a few of the rays aimed exactly at an edge, and inside the torus such a ray
    comes back in and the reference reports the far wall.  That is its defect; the kernel must hit on every ray.
    Distances: the reference's, or where they differ a hit that ``legitimate_hits`` (tests/test_mesh_ray_cpu.py)
    admits -- besides the reference's leaks these are rays aimed at the torus's inner equator, which they graze: in
    float64 they pass 1e-6 of a triangle inside the silhouette edge and hit there, in fp32 as far outside it and go
    on to the far wall; the ray stays inside the tube either way."""
    V, F = _meshes()[name]
    d = np.concatenate([_sphere(200000, 1), _aimed(V, F, origin)])
    d = d[np.abs(d).max(1) > 0]
    o = np.broadcast_to(np.asarray(origin, np.float32), d.shape).copy()
    ref = R.brute_force(o[0].astype(np.float64), d.astype(np.float64), V, F)
    has = np.isfinite(ref["t"])
    assert has[:200000].all()                                    # the random directions
    t, face, _, flags = (x.cpu().numpy() for x in _scanner(V, F).cast(torch.from_numpy(o).to(DEV),
                                                                      torch.from_numpy(d).to(DEV)))
    print(f"\n{name} from inside: {len(d)} rays, leaks {(flags == 0).sum()} (the float64 reference leaks {(~has).sum()})")
    assert (flags != 0).all() and np.isfinite(t).all() and (face >= 0).all()
    # outward faces seen from inside are back faces (the random directions: a ray aimed exactly at a vertex on the
    # silhouette may be answered by a neighbour turned just past edge-on)
    assert ((flags[:200000] & 2) != 0).all()
    differs, fine = legitimate_hits(o[0], d, V, F, t, face, ref)
    print(f"{name} from inside: distance differs from the reference's on {differs.sum()} rays "
          f"({differs[:200000].sum()} of the random ones), not legitimate {(~fine).sum()}")
    assert fine.all()


@pytest.mark.parametrize("name,origin", [("box", (1.9, -1.1, 1.1)), ("torus", (1.4, -1.0, 1.3))])
def test_watertight_from_outside(name, origin):
    """From outside: where the float64 reference hits, and still hits when the ray is nudged by 2^-10 of a pixel's
    angle in four directions (not a silhouette), the kernel hits."""
    V, F = _meshes()[name]
    d = _aimed(V, F, origin)
    d = d[np.abs(d).max(1) > 0]
    d64 = d.astype(np.float64)
    o64 = np.asarray(origin, np.float32).astype(np.float64)
    ref = R.brute_force(o64, d64, V, F)
    inner = np.isfinite(ref["t"])
    dn = np.linalg.norm(d64, axis=1, keepdims=True)
    a = np.cross(d64, [0.3, 0.5, 0.8])
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(d64, a) / dn
    for n in (a, -a, b, -b):
        inner &= np.isfinite(R.brute_force(o64, d64 + n * dn * (R.SHIFT / 525.0), V, F)["t"])
    o = np.broadcast_to(np.asarray(origin, np.float32), d.shape).copy()
    flags = _scanner(V, F).cast(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV))[3].cpu().numpy()
    print(f"\n{name} from outside: {len(d)} rays, {inner.sum()} inner hits, missed {(flags[inner] == 0).sum()}")
    assert inner.sum() > len(d) // 8
    assert (flags[inner] != 0).all()


def test_two_runs_and_two_builds_give_the_same_bits():
    V, F, K, T, H, W = _views()["room_37"]
    a, b = _scanner(V, F), _scanner(V, F)
    ra = a.render_depth(T, K, H, W, normals=True)
    for other in (a.render_depth(T, K, H, W, normals=True), b.render_depth(T, K, H, W, normals=True)):
        for x, y in zip(ra, other):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    Vt, Ft = _meshes()["torus"]
    d = torch.from_numpy(_sphere(50000, 2)).to(DEV)
    o = torch.tensor([1.4, -1.0, 1.3], device=DEV).expand_as(d).contiguous()
    ca, cb = _scanner(Vt, Ft).cast(o, d), _scanner(Vt, Ft).cast(o, d)
    for x, y in zip(ca, cb):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


@pytest.mark.parametrize("name", ["box", "torus", "room_390"])
def test_face_order_changes_only_face_ids_and_tie_winners(name):
    V, F, K, T, H, W = _views()[name]
    ok, ref, _, _ = _reference(name)
    perm = np.random.default_rng(5).permutation(len(F))
    depth, face = (x.cpu().numpy().reshape(-1) for x in _scanner(V, F).render_depth(T, K, H, W))
    depth_p, face_p = (x.cpu().numpy().reshape(-1) for x in _scanner(V, np.asarray(F)[perm]).render_depth(T, K, H, W))
    tol = _tol(V, T)
    clear = ok & np.isfinite(ref["t"]) & (ref["second"] - ref["t"] > tol) & _inside(ref)
    assert np.array_equal(depth_p[clear], depth[clear])          # the same triangle, the same arithmetic
    assert np.array_equal(perm[face_p[clear]], face[clear])
    assert np.array_equal((depth_p > 0)[ok], (depth > 0)[ok])
    both = ok & (depth > 0) & (depth_p > 0)
    assert (np.abs(depth_p.astype(np.float64) - depth)[both] <= tol).all()


def test_non_finite_rays_zero_directions_and_a_mesh_without_a_valid_face():
    V, F = _meshes()["torus"]
    sc = _scanner(V, F)
    d = _sphere(256, 4)
    o = np.broadcast_to(np.array([1.4, -1.0, 1.3], np.float32), d.shape).copy()
    d[3, 0], d[10, 1], o[20, 2], d[33] = np.nan, np.inf, -np.inf, 0.0
    bad = ~(np.isfinite(d).all(1) & np.isfinite(o).all(1)) | (d == 0).all(1)
    t, face, uv, flags = (x.cpu().numpy() for x in sc.cast(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)))
    assert np.isnan(t[bad]).all() and (face[bad] == -1).all() and np.isnan(uv[bad]).all() and (flags[bad] == 0).all()
    good = sc.cast(torch.from_numpy(o[~bad]).to(DEV), torch.from_numpy(d[~bad]).to(DEV))[0].cpu().numpy()
    assert np.array_equal(t[~bad].view(np.int32), good.view(np.int32)) and np.isfinite(good).any()
    # axis-parallel rays are ordinary rays: straight down the torus's axis misses, through its tube hits twice
    ax_o = torch.tensor([[0.3, -0.2, 3.0], [0.8, -0.2, 3.0], [0.8, -0.2, 3.0]], device=DEV)
    ax_d = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0]], device=DEV)
    t, face, _, flags = (x.cpu().numpy() for x in sc.cast(ax_o, ax_d))
    assert np.isnan(t[0]) and face[0] == -1 and flags[2] == 0
    assert flags[1] == 1 and abs(t[1] - (3.0 - 0.4 - 0.2)) < 0.01
    Vn = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    none = _scanner(Vn, np.array([[0, 1, 2], [0, 0, 1]], np.int64))
    t, face, _, flags = (x.cpu().numpy() for x in none.cast(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)))
    assert np.isnan(t).all() and (face == -1).all() and (flags == 0).all()
    depth, face = none.render_depth(np.eye(4), K_SMALL, 120, 160)
    assert (depth == 0).all() and (face == -1).all()


def test_batched_poses_equal_single_poses_and_range_limits():
    from bnv_fusion_amd import sequence
    V, F, K, _, H, W = _views()["room_37"]
    sc = _scanner(V, F)
    poses = np.stack([sequence.sweep_pose(t) for t in range(0, 1100, 100)])           # 11: two launches
    depth, face, nrm = sc.render_depth(poses, K, H, W, normals=True)
    assert depth.shape == (11, H, W) and nrm.shape == (11, H, W, 3)
    for i in (0, 7, 8, 10):
        d1, f1, n1 = sc.render_depth(poses[i], K, H, W, normals=True)
        assert torch.equal(d1.view(torch.int32), depth[i].view(torch.int32)) and torch.equal(f1, face[i])
        assert torch.equal(n1.view(torch.int32), nrm[i].view(torch.int32))
    full = depth[3]
    cut, cut_face = sc.render_depth(poses[3], K, H, W, near=1.5, max_depth=3.0)
    keep = (full >= 1.5) & (full < 3.0)
    assert torch.equal(cut, torch.where(keep, full, torch.zeros_like(full)))           # the nearest hit, or nothing
    assert (cut_face[~keep] == -1).all() and keep.any() and (~keep).any()


def test_seen_counts_and_visible_mesh():
    from bnv_fusion_amd import sequence
    room = sequence.gt_mesh()
    sc = _scanner(room.vertices, room.faces)
    K, H, W = sequence.intrinsics(), 480, 640
    hits = 0
    tol = _tol(room.vertices, np.eye(4) * 3.6)
    for t in FRAMES:
        ok, ref, _, _ = _reference(f"room_{t}")
        depth, face = (x.cpu().numpy().reshape(-1) for x in sc.render_depth(sequence.sweep_pose(t), K, H, W))
        hits += int((depth > 0).sum())
        # every counted face is one the restatement reports there, or ties with it
        same = (face == ref["face"]) | (ref["second"] - ref["t"] <= tol) | ~ok
        assert same.all()
    seen = sc.seen.cpu().numpy()
    assert int(seen.sum()) == hits and hits > 0
    V, F = room.vertices, room.faces
    y_floor, z_wall = V[:, 1].max(), np.abs(V[:, 2]).max()
    tri = V[F]
    furniture = np.arange(len(F)) >= 12
    hidden = furniture & ((tri[:, :, 1] == y_floor).all(1) | (np.abs(tri[:, :, 2]) == z_wall).all(1))
    assert hidden.sum() == 2 * 7                                # five box bottoms, two shelf backs
    assert (seen[hidden] == 0).all()
    vis = sc.visible_mesh()
    assert len(vis.faces) == int((seen > 0).sum()) and 0 < len(vis.faces) < len(F)
    assert np.array_equal(np.sort(vis.vertices[vis.faces].reshape(-1, 9), axis=0),
                          np.sort(tri[seen > 0].reshape(-1, 9), axis=0))
    assert len(sc.visible_mesh(min_pixels=10 ** 9).faces) == 0
    sc.reset_seen()
    assert int(sc.seen.sum()) == 0
    sc.render_depth(sequence.sweep_pose(5), K, H, W, count_seen=False)
    assert int(sc.seen.sum()) == 0


@pytest.mark.parametrize("t", [37, 777])
def test_sensor_matches_the_restatement(t):
    """Pixels none of whose three quantities before rounding lies within DELTA of a rounding boundary match exactly;
    the others are at most 0.1 % of the frame (tests/test_mesh_ray_cpu.py measures both for the float32 evaluation)."""
    from bnv_fusion_amd import scan, sequence
    clean = sequence.render_depth(sequence.sweep_pose(t), sequence.intrinsics(), 480, 640).numpy().astype(np.float32)
    clean[100:140, 200:260] = 0.0
    ref = R.sensor(clean, seed=0, frame=t)
    got = scan.simulate_sensor(torch.from_numpy(clean).to(DEV), 0, t)
    assert got.dtype == torch.uint16 and got.shape == (480, 640)
    got = got.cpu().numpy()
    near = near_boundary(ref["q"], SENSOR_DELTA)
    print(f"\nframe {t}: within DELTA of a boundary {100 * near.mean():.5f} %, kernel differs at "
          f"{(got != ref['mm']).sum()} pixels, {(got != ref['mm'])[~near].sum()} of them away from a boundary")
    assert near.mean() <= 1e-3
    assert np.array_equal(got[~near], ref["mm"][~near])
    nz = got > 0
    assert np.array_equal(nz[~near], (ref["mm"] > 0)[~near])
    again = scan.simulate_sensor(torch.from_numpy(clean).to(DEV), 0, t).cpu().numpy()
    assert np.array_equal(again, got)
    other = scan.simulate_sensor(torch.from_numpy(clean).to(DEV), 0, t + 1).cpu().numpy()
    assert (other != got).mean() > 0.2
    # a table of ones is the reference's (1 - a) + a: the same image up to that factor's last bit
    ones = scan.simulate_sensor(torch.from_numpy(clean).to(DEV), 0, t, table=torch.ones((80, 80, 5), device=DEV))
    ref1 = R.sensor(clean, seed=0, frame=t, table=np.ones((80, 80, 5)))
    near1 = near_boundary(ref1["q"], SENSOR_DELTA)
    assert np.array_equal(ones.cpu().numpy()[~near1], ref1["mm"][~near1])


def test_refusals():
    from bnv_fusion_amd import scan
    from bnv_fusion_amd.mesh import TriMesh
    V, F = _meshes()["box"]
    with pytest.raises(ValueError, match="GPU only"):
        scan.MeshScanner(TriMesh(V, F), device="cpu")
    sc = scan.MeshScanner(TriMesh(V, F), device=DEV)
    with pytest.raises(ValueError, match="CPU tensor"):
        sc.cast(torch.zeros((4, 3)), torch.ones((4, 3)))
    with pytest.raises(ValueError):
        sc.cast(torch.zeros((4, 3), device=DEV), torch.ones((5, 3), device=DEV))
    with pytest.raises(ValueError):
        sc.cast(torch.zeros((4, 3), device=DEV), torch.ones((4, 3), device=DEV), t_min=2.0, t_max=1.0)
    with pytest.raises(ValueError):
        sc.render_depth(np.eye(4), K_SMALL, 120, 160, near=3.0, max_depth=1.0)
    with pytest.raises(ValueError, match="CPU tensor"):
        scan.simulate_sensor(torch.zeros((8, 8)), 0, 0)
    with pytest.raises(ValueError):
        scan.to_u16(torch.zeros((8, 8), device=DEV), rounding="floor")
