"""Point-cloud normals on the GPU (csrc/cloud.hip; include/bnv_fusion.h, "Point-cloud normals") against the numpy
restatement of tests/cloud_restatement.py, bit for bit in all three outputs and the status counts; reproducibility,
workspace reuse and refusals; a multi-station cloud; and the path through the product: the same frames fused from
their depth images and, as bare points, through NeuralMap.integrate_cloud."""
import ctypes as C

import numpy as np
import pytest
import torch

import cloud_cases as cases
import cloud_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gpu(points, origins, origin_index=None, **kw):
    from bnv_fusion_amd import estimate_normals
    oi = None if origin_index is None else torch.from_numpy(np.asarray(origin_index, dtype=np.int32)).to(DEV)
    out, st = estimate_normals(torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(DEV), origins, oi,
                               return_stats=True, **kw)
    torch.cuda.synchronize()
    assert out.shape == (1, len(points), 6)
    return {"input_pts": out[0].cpu().numpy(), "variation": st["variation"].cpu().numpy(),
            "n_neighbors": st["n_neighbors"].cpu().numpy(), "status": st["status"].cpu().numpy()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def assert_bit_equal(got, want, what):
    for key in ("n_neighbors", "status"):
        assert (got[key] == want[key]).all(), (what, key, got[key][:8], want[key][:8])
    for key in ("input_pts", "variation"):
        diff = bits(got[key]) != bits(want[key])
        assert not diff.any(), (what, key, int(diff.sum()), got[key][diff][:6], want[key][diff][:6])


@pytest.fixture(scope="module")
def frame60():
    """The 60 x 80 frame's 4,800 points."""
    return cases.frame_points(60, 80)[:, :3]


@pytest.mark.parametrize("n", [1, 2, 7, 63, 64, 65, 257, 1000, 4800])
def test_bit_equal_on_frame_points(frame60, n):
    """The first n points of the frame (row-major: a strip of the surface) for every k, with one origin; with three
    origins and a radius for one k per size."""
    p = frame60[:n]
    nb32 = R.neighbors(p, 32)
    for k in (8, 10, 16, 32):
        nbrs = (nb32[0][:, :k], np.minimum(nb32[1], k).astype(np.int32))
        want = R.estimate_normals(p, cases.CAMERA0, k=k, nbrs=nbrs)
        assert_bit_equal(gpu(p, cases.CAMERA0, k=k), want, (n, k))
    k = (8, 10, 16, 32)[n % 4]
    oi = (np.arange(n) * 7 % 3).astype(np.int32)
    radius = 0.05                                            # ~2 pixel spacings at 60 x 80: ~15 neighbours, cuts k = 16, 32
    want = R.estimate_normals(p, cases.ORIGINS3, oi, k=k, max_radius=radius, min_neighbors=5)
    got = gpu(p, cases.ORIGINS3, oi, k=k, max_radius=radius, min_neighbors=5)
    assert_bit_equal(got, want, (n, k, "radius, 3 origins"))
    if n >= 257 and k >= 16:
        assert want["n_neighbors"].max() < k                   # the radius did cut the lists short


@pytest.mark.parametrize("k", [8, 10, 16, 32])
def test_bit_equal_on_the_tie_lattice(k):
    p = cases.lattice(5)
    for radius in (None, 1.0, 1.5):
        kw = dict(k=k, max_radius=radius, min_neighbors=4)
        assert_bit_equal(gpu(p, cases.ORIGINS3[1:2], **kw), R.estimate_normals(p, cases.ORIGINS3[1:2], **kw), (k, radius))


def test_bit_equal_on_degenerate_inputs():
    for name, (p, o, oi, kw) in cases.degenerate_cases().items():
        assert_bit_equal(gpu(p, o, oi, **kw), R.estimate_normals(p, o, oi, **kw), name)


@pytest.mark.parametrize("k", [8, 16, 32])
def test_bit_equal_when_the_kth_neighbour_is_many_rings_out(k):
    """A tight cluster plus 20 points a hundred cell edges away: with k > 20 those 20 have to reach the cluster, past
    the fine grid's rings and on to the coarse grid; with k = 8 they stop among themselves."""
    p = cases.cluster_and_far()
    want = R.estimate_normals(p, cases.CAMERA0, k=k)
    assert_bit_equal(gpu(p, cases.CAMERA0, k=k), want, k)
    assert (want["n_neighbors"] == k).all()
    far = p[:, 0] > 1.0
    idx, _ = R.neighbors(p, k)
    assert far.sum() == 20 and bool((~far[idx[far]]).any()) == (k > 20)


def test_reproducible_and_workspace_reuse():
    """Two calls give the same bits; a second call through the same workspace with another N is correct; a workspace
    one byte short and bad arguments are refused."""
    from bnv_fusion_amd import _lib, estimate_normals
    lib = _lib.require_device(0)
    a, b = cases.random_cloud(1000, 21), cases.random_cloud(333, 22)
    first, again = gpu(a, cases.CAMERA0, k=16), gpu(a, cases.CAMERA0, k=16)
    assert_bit_equal(first, again, "second call")
    need = C.c_int64()
    assert lib.bnv_cloud_normals_bytes(len(a), C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    org = torch.from_numpy(cases.CAMERA0).to(DEV)

    def run(p, ws_bytes=need.value, k=16):
        t = torch.from_numpy(p).to(DEV)
        out = torch.empty((len(p), 6), dtype=torch.float32, device=DEV)
        var = torch.empty(len(p), dtype=torch.float32, device=DEV)
        cnt = torch.empty(len(p), dtype=torch.int32, device=DEV)
        st = torch.full((4,), -7, dtype=torch.int32, device=DEV)
        rc = lib.bnv_cloud_normals(_lib.ptr(t), len(p), k, 0.0, 6, _lib.ptr(org), 1, None, _lib.ptr(ws), ws_bytes,
                                   _lib.ptr(out), _lib.ptr(var), _lib.ptr(cnt), _lib.ptr(st), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, {"input_pts": out.cpu().numpy(), "variation": var.cpu().numpy(), "n_neighbors": cnt.cpu().numpy(),
                    "status": st.cpu().numpy()}

    rc, got = run(a)
    assert rc == 0
    assert_bit_equal(got, first, "own workspace")
    rc, got = run(b)
    assert rc == 0
    assert_bit_equal(got, R.estimate_normals(b, cases.CAMERA0, k=16), "same workspace, other N")
    rc, got = run(a)
    assert rc == 0
    assert_bit_equal(got, first, "same workspace, first N again")
    assert run(a, ws_bytes=need.value - 1)[0] == -2              # BNV_ERR_WORKSPACE_TOO_SMALL
    assert run(a, k=7)[0] == -1 and run(a, k=33)[0] == -1        # BNV_ERR_INVALID_ARGUMENT
    t = torch.from_numpy(a).to(DEV)
    for kw in (dict(k=7), dict(k=33), dict(min_neighbors=2), dict(min_neighbors=17), dict(max_radius=0.0),
               dict(max_radius=-1.0), dict(max_radius=float("nan")), dict(origin_index=torch.zeros(5, dtype=torch.int32)),
               dict(origin_index=torch.zeros(1000))):
        with pytest.raises(ValueError):
            estimate_normals(t, cases.CAMERA0, **kw)
    with pytest.raises(ValueError):
        estimate_normals(t, np.zeros((0, 3), np.float32))
    with pytest.raises(ValueError):
        estimate_normals(t[:, :2], cases.CAMERA0)
    # without the statistics: the same rows
    assert bits(estimate_normals(t, cases.CAMERA0, k=16)[0].cpu().numpy()).tobytes() == bits(first["input_pts"]).tobytes()


def test_multi_station_cloud():
    """scan.scan_cloud of a box from 4 orbit poses at 40 x 30: every finite normal points away from the station that
    saw its point; rows whose origin index is set out of range are NaN and counted."""
    from bnv_fusion_amd import estimate_normals, mesh, scan, sequence
    v, f = sequence._box_faces([-0.4, -0.3, -0.5], [0.4, 0.3, 0.5])
    scanner = scan.MeshScanner(mesh.TriMesh(v, f), device=DEV)
    poses = scan.orbit_poses([0.0, 0.0, 0.0], 2.0, 4, height=0.7)
    K = np.array([[60.0, 0.0, 19.5], [0.0, 60.0, 14.5], [0.0, 0.0, 1.0]])
    pts, origins, oi = scan.scan_cloud(scanner, poses, K, 30, 40)
    n = int(pts.shape[0])
    assert 400 < n <= 4 * 30 * 40 and origins.shape == (4, 3) and oi.shape == (n,) and oi.dtype == torch.int32
    assert sorted(set(oi.cpu().tolist())) == [0, 1, 2, 3]
    assert np.allclose(origins, poses[:, :3, 3])
    out, st = estimate_normals(pts, origins, oi, k=12, return_stats=True)
    res = out[0].cpu().numpy().astype(np.float64)
    ok = np.isfinite(res).all(1)
    o = origins[oi.cpu().numpy()]
    assert ok.mean() > 0.95
    assert (((res[:, :3] - o) * res[:, 3:])[ok].sum(1) >= 0).all()
    assert (res[ok, :3] == pts.cpu().numpy()[ok].astype(np.float64)).all()
    # the normals of a box are axis directions away from its edges
    assert (np.abs(res[ok, 3:]).max(1) > 0.99).mean() > 0.25
    base = st["status"].cpu().numpy()
    assert base[1] == 0
    bad = oi.clone()
    bad[[0, 5, n - 1]] = torch.tensor([4, -1, 100], dtype=torch.int32, device=DEV)
    out2, st2 = estimate_normals(pts, origins, bad, k=12, return_stats=True)
    res2 = out2[0].cpu().numpy()
    assert np.isnan(res2[[0, 5, n - 1]]).all() and st2["status"].cpu().numpy()[1] == 3
    keep = np.ones(n, bool)
    keep[[0, 5, n - 1]] = False
    assert bits(res2[keep]).tobytes() == bits(out[0].cpu().numpy()[keep]).tobytes()
    assert_bit_equal({"input_pts": res2, "variation": st2["variation"].cpu().numpy(),
                      "n_neighbors": st2["n_neighbors"].cpu().numpy(), "status": st2["status"].cpu().numpy()},
                     R.estimate_normals(pts.cpu().numpy(), origins, bad.cpu().numpy(), k=12), "scan_cloud")


# ---- through the product -----------------------------------------------------------------------------------------------
SCALE, VOXEL, MIN_PTS, MAX_DEPTH = 0.5, 0.02, 2, 3.0
FRAMES = range(96, 141, 4)


def test_cloud_path_against_depth_path():
    """Twelve 160 x 120 room-sweep frames into a 128^3 map at 2 cm with min_pts_in_grid = 2 (tests/test_gpu_mesh_color.py's
    map, without the TSDF side volume, which a cloud cannot feed), once from the depth images and once from the same
    frames' points through integrate_cloud, one call per frame with that frame's camera centre as origin.  Both meshes
    are scored with evaluate_meshes; the depth path measured here is the yardstick: the cloud path's pred -> gt mean
    distance may exceed it by at most half a voxel (1 cm) and its recall may fall by at most a tenth of the depth
    path's.  Both margins are guesses at "the same surface".

    The ground truth is the mesh the frames were rendered from, sequence.gt_mesh(0.5), with the faces the scanner saw
    (MeshScanner.visible_mesh) on the recall side; the same two conditions are also checked against
    synthetic.gt_mesh(), which is another scene (both paths are ~a metre from it and recall nothing of it), so there
    they say little.  Also printed, not asserted: the cloud path with every normal flipped.

    Figures of one MI355X run are in the README row of this feature."""
    import bnv_fusion_amd as bnv
    from bnv_fusion_amd import scan, sequence, synthetic
    scanner = scan.MeshScanner(sequence.gt_mesh(SCALE), device=DEV)
    cams = np.stack([sequence.sweep_pose(t, SCALE) for t in FRAMES])
    K = sequence.intrinsics(120, 160)
    frames = list(scan.scan_frames(scanner, cams, K, 120, 160, max_depth=MAX_DEPTH))
    gt, gt_seen, other = sequence.gt_mesh(SCALE), scanner.visible_mesh(), synthetic.gt_mesh(step_px=4.0)
    model = bnv.load_pretrained(device=DEV, voxel_size=VOXEL, min_pts_in_grid=MIN_PTS)

    def new_map():
        return bnv.NeuralMap(np.array([2.54] * 3), VOXEL, model, min_pts_in_grid=MIN_PTS, device=DEV)

    def score(nm):
        m = nm.extract_mesh(post_process=VOXEL / 4)
        assert m is not None and len(m.faces) > 1000
        gen = torch.Generator(device="cpu").manual_seed(0)
        a = bnv.evaluate_meshes(m, gt, gt_recall=gt_seen, generator=gen)
        b = bnv.evaluate_meshes(m, other, generator=gen)
        return a, b, len(m.faces)

    # the depth path; its front-end rows also give the cloud path the very same points
    depth_map, clouds = new_map(), []
    for fr in frames:
        pts = bnv.neural_map.frame_input_pts(fr, MAX_DEPTH)[0]
        clouds.append(pts[torch.isfinite(pts).all(1)][:, :3].contiguous())
        depth_map.integrate(fr)
    results = {"depth": score(depth_map)}
    for name, sign in (("cloud", 1.0), ("cloud, normals flipped", -1.0)):
        nm = new_map()
        for pts, T in zip(clouds, cams):
            if sign > 0:
                nm.integrate_cloud(pts, T[:3, 3][None], k=16)
            else:
                rows = bnv.estimate_normals(pts, T[:3, 3][None], k=16).clone()
                rows[..., 3:] *= -1.0
                nm.integrate({"input_pts": rows})
        results[name] = score(nm)
    for name, (a, b, faces) in results.items():
        print(f"{name}: {faces} faces; room: pred_gt {a['pred_gt']:.5f} recall {a['recall']:.4f} "
              f"({bnv.evaluate.summary_line(a)}); synthetic.gt_mesh: pred_gt {b['pred_gt']:.5f} recall {b['recall']:.4f}")
    for which in (0, 1):
        d, c = results["depth"][which], results["cloud"][which]
        assert c["pred_gt"] <= d["pred_gt"] + VOXEL / 2, (which, c, d)
        assert c["recall"] >= 0.9 * d["recall"], (which, c, d)
