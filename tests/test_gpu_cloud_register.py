"""Cloud-to-cloud registration on the GPU (csrc/cloud_register.hip; include/bnv_fusion.h, "Cloud registration")
against the float64 restatement of tests/cloud_register_restatement.py: the persistent index's nearest neighbour
against bnv_nn_query and the brute force, every iteration's dumps, pairs, sums and clamped step at the kernel's own
poses, more than one round of points per thread, recovery of the displaced box, the sign of the target's normals, the
refusals, determinism, the dispatch from register_points, evaluate(align=) and align_scans end to end."""
import functools

import numpy as np
import pytest
import torch

import cloud_register_restatement as cc
import mesh_sdf_restatement as R
import register_restatement as rr
import track_restatement as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -52
LEVELS = ((4, 3, 0.2), (2, 3, 0.05), (1, 4, 0.02))


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype.itemsize == 1 else np.uint32)


def index_of(input_pts):
    from bnv_fusion_amd import pointcloud
    return pointcloud.CloudIndex(input_pts=dev(input_pts, np.float32))


@functools.lru_cache(maxsize=None)
def restated(name):
    target, pts, T_true, T0 = cc.cloud_case(name)
    return cc.register(pts, target, T0, levels=cc.BOX_LEVELS)


@functools.lru_cache(maxsize=None)
def near_run():
    """The GPU's run of the near case over LEVELS with records, and what it ran on."""
    from bnv_fusion_amd import register
    target, pts, T_true, T0 = cc.cloud_case("near")
    index, p = index_of(target), dev(pts)
    return register.register_cloud(p, index, T0, levels=LEVELS, records=True), index, p, target, pts, T0


# ---- CloudIndex.nearest ------------------------------------------------------------------------------------------------

def nearest_case(n):
    """-> (target positions f32 [n, 3], queries f32 [m, 3])."""
    rng = np.random.default_rng(100 + n)
    if n == 4800:                                          # the tie lattice: an integer grid, queries at cell centres
        g = np.stack(np.meshgrid(np.arange(16.0), np.arange(15.0), np.arange(20.0), indexing="ij"), -1)
        pos = g.reshape(-1, 3)[rng.permutation(4800)].astype(np.float32)
        centres = pos[(pos[:, 0] < 15) & (pos[:, 1] < 14) & (pos[:, 2] < 19)][:1500] + np.float32(0.5)
        q = [centres, pos[:300], pos[:300] + np.float32(0.25)]
    else:
        pos = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
        if n >= 2:
            pos[n // 2:] = pos[:n - n // 2]                # duplicates: every point twice
        q = [rng.uniform(-1.0, 1.0, (200, 3)).astype(np.float32), pos]
    lo, hi = pos.min(0), pos.max(0)
    outside = (rng.uniform(-1.0, 2.0, (200, 3)) * (hi - lo + 1.0) * 3.0 + lo).astype(np.float32)
    bad = np.array([[np.nan, 0.0, 0.0]], np.float32)       # one non-finite query
    return pos, np.concatenate(q + [outside, bad])


def check_nearest(pos, q):
    from bnv_fusion_amd import evaluate, pointcloud
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (len(pos), 1))
    index = pointcloud.CloudIndex(dev(pos), dev(nrm))
    assert index.n == len(pos) and index.device == torch.device(DEV)
    d2, idx = index.nearest(dev(q))
    d2_q, idx_q = evaluate.nn_d2(dev(q), dev(pos))
    assert np.array_equal(bits(d2), bits(d2_q)) and np.array_equal(idx.cpu().numpy(), idx_q.cpu().numpy())
    d2_b, idx_b = cc.nearest(q, pos)
    assert np.array_equal(bits(d2), bits(d2_b)) and np.array_equal(idx.cpu().numpy(), idx_b)
    return d2.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4800])
def test_nearest_is_nn_query_and_the_brute_force(n):
    pos, q = nearest_case(n)
    d2, idx = check_nearest(pos, q)
    assert idx[-1] == -1 and np.isinf(d2[-1]) and (idx[:-1] >= 0).all()
    if n == 4800:
        assert (d2[:1500] == np.float32(0.75)).all()       # eight corners tie; the brute force names the lowest


def test_nearest_reaches_the_coarse_grid():
    """A tight cluster and one far point: queries around the far point are not settled by the fine grid's rings."""
    rng = np.random.default_rng(17)
    pos = (rng.normal(scale=0.01, size=(4799, 3))).astype(np.float32)
    pos = np.concatenate([pos, np.array([[5.0, 4.0, 3.0]], np.float32)])
    q = np.concatenate([np.array([5.0, 4.0, 3.0]) + rng.normal(scale=0.5, size=(300, 3)),
                        rng.uniform(0.0, 5.0, (300, 3)), rng.normal(scale=0.02, size=(300, 3))]).astype(np.float32)
    d2, idx = check_nearest(pos, np.concatenate([q, np.array([[0.0, np.inf, 0.0]], np.float32)]))
    assert (idx[:300] == 4799).sum() > 250 and (idx[600:900] < 4799).all()


def test_an_index_keeps_no_rejected_row_and_a_foreign_header_answers_nothing():
    from bnv_fusion_amd import pointcloud, register
    target, pts, T_true, T0 = cc.cloud_case("near")
    broken = target.copy()
    broken[::3, 4] = np.nan
    broken[1::30, 3:] = 0.0
    broken[2::30, 1] = np.inf
    pos, nrm = cc.index_rows(broken)
    index = index_of(broken)
    q = rr.transform(T_true, pts)
    d2, idx = index.nearest(dev(q))
    d2_b, idx_b = cc.nearest(q, pos)
    assert np.array_equal(bits(d2), bits(d2_b)) and np.array_equal(idx.cpu().numpy(), idx_b)
    assert np.isfinite(pos[idx_b]).all() and np.isnan(pos).any(1).sum() >= 1000
    res = register.register_cloud(dev(pts), index, T0, levels=((1, 1, 0.2),), records=True)
    check_dumps_and_sums(res, broken, pts, T0, 1, 0.2)
    # memory that holds no index: every query unanswered, every registration lost
    index._ws.zero_()
    d2, idx = index.nearest(dev(q))
    assert torch.isinf(d2).all() and (idx == -1).all()
    lost = register.register_cloud(dev(pts), index, T0)
    assert check_refused(lost, T0, register.LOST) == 0
    assert isinstance(index, pointcloud.CloudIndex)


# ---- iterations --------------------------------------------------------------------------------------------------------

def check_dumps_and_sums(res, target, pts, T, stride, dist, normals=None, min_normal_cos=None, oriented=False):
    """One iteration's dumps against the restated transform and the brute force, its pair count and sums against the
    rows restated from the dumps -> (q, index) on the host."""
    q, index = res.q.cpu().numpy(), res.index.cpu().numpy()
    n_s = rr.n_samples(len(pts), stride)
    assert len(q) == len(index) == n_s
    q_ref = rr.transform(T, pts[::stride])
    finite = np.isfinite(q_ref).all(1)                     # (the bits of a NaN are the processor's choice)
    assert np.array_equal(bits(q[finite]), bits(q_ref[finite])) and not np.isfinite(q[~finite]).all(1).any()
    pos, nrm = cc.index_rows(target)
    want = cc.candidates(q_ref, pos, dist)
    assert np.array_equal(index, want), f"{(index != want).sum()} candidates differ"
    ns = None if normals is None else np.asarray(normals, np.float32)[::stride]
    J, r, pairs = cc.rows(q, index, pos, nrm, T, ns, min_normal_cos, oriented)
    A, b, rsum, pairs, absum = rr.sums_of(J, r, pairs)
    ref, got = tr.sums_vector(A, b, rsum, pairs), res.records[0, :29]
    assert got[28] == pairs == res.stats[0, 0], f"pairs {got[28]} against {pairs}"
    ratio = (np.abs(got - ref) / np.maximum(pairs * EPS * absum, 1e-300)).max()
    print(f"stride {stride}, gate {dist}: {pairs:.0f} pairs of {n_s} ({(want >= 0).sum()} candidates), largest "
          f"|sum - restated| / bound {ratio:.3g}")
    assert (np.abs(got - ref) <= pairs * EPS * absum).all()
    return q, index


@pytest.mark.parametrize("level", [0, 1, 2])
def test_one_iteration_at_each_level(level):
    """One iteration from the near run's pose at the start of each level: q bit for bit the restated transform, the
    candidates those of the brute force with -1 exactly where it has none, the pairs equal, the sums within the float64
    summation bound."""
    from bnv_fusion_amd import register
    res, index, p, target, pts, T0 = near_run()
    assert res.status == register.OK
    k = sum(it for _, it, _ in LEVELS[:level])
    stride, _, dist = LEVELS[level]
    one = register.register_cloud(p, index, res.poses[k], levels=((stride, 1, dist),), records=True)
    assert one.status == register.OK
    q, idx = check_dumps_and_sums(one, target, pts, res.poses[k], stride, dist)
    if level == 2:                                         # at the 2 cm gate some points near the edges have no candidate
        assert (idx == -1).any()


def test_one_iteration_with_the_normal_gate():
    from bnv_fusion_amd import register
    res, index, p, target, pts, T0 = near_run()
    ns = cc.source_normals()
    ns[5] = np.nan
    for oriented, tgt in ((False, cc.flipped(target)), (True, target)):
        ix = index_of(tgt)
        one = register.register_cloud(p, ix, T0, levels=((1, 1, 0.2),), normals=dev(ns), min_normal_cos=0.9,
                                      oriented=oriented, records=True)
        check_dumps_and_sums(one, tgt, pts, T0, 1, 0.2, ns, 0.9, oriented)
        assert 0 < one.stats[0, 0] < (one.index >= 0).sum().item()      # the gate dropped candidates


def test_every_iteration_of_the_near_run():
    """A one-iteration call from the kernel's own pose of every iteration reproduces that iteration's record, stats and
    next pose byte for byte; the applied step is the restated clamped solve of the GPU's own sums at
    tests/test_gpu_register.py's tolerance."""
    from bnv_fusion_amd import register
    res, index, p, target, pts, T0 = near_run()
    assert res.status == register.OK
    assert np.array_equal(res.poses[0], T0) and np.array_equal(res.poses[-1], res.T)
    k = 0
    for stride, iters, dist in LEVELS:
        n_s = rr.n_samples(len(pts), stride)
        for _ in range(iters):
            one = register.register_cloud(p, index, res.poses[k], levels=((stride, 1, dist),), records=True)
            assert one.status == register.OK
            assert one.records[0].tobytes() == res.records[k].tobytes()
            assert one.stats[0].tobytes() == res.stats[k].tobytes() and one.T.tobytes() == res.poses[k + 1].tobytes()
            got = res.records[k, :29]
            Ag, bg, rrg, pg = tr.from_sums(got)
            T1, status, stats, xi, s = rr.solve_update(Ag, bg, rrg, pg, res.poses[k], n_s)
            assert status == rr.OK
            xi_gpu = res.records[k, 29:35]
            tol = 100 * np.linalg.cond(Ag) * EPS * np.linalg.norm(xi)
            assert np.abs(xi_gpu - np.array(xi)).max() <= tol, f"iteration {k}: xi off by {np.abs(xi_gpu - xi).max()}"
            assert np.abs(res.poses[k + 1] - tr.exp_apply(list(xi_gpu), res.poses[k])).max() <= 1e-14
            assert np.abs(res.poses[k + 1] - T1).max() <= 1e-14 + 4 * tol
            assert np.allclose(res.stats[k, [1, 4]], stats[[1, 4]], rtol=1e-12, atol=0)       # rmse, spread
            assert np.abs(res.stats[k, 2:4] - stats[2:4]).max() <= tol
            print(f"iteration {k} stride {stride}: pairs {pg:.0f}, scale {s:.3f}, |w| {stats[2]:.4f}, |v| {stats[3]:.4f}")
            k += 1
    assert k == len(res.stats)


@pytest.mark.parametrize("name", ["near", "far", "noise"])
def test_recovers_the_displaced_box(name):
    from bnv_fusion_amd import register
    target, pts, T_true, T0 = cc.cloud_case(name)
    res = register.register_cloud(dev(pts), index_of(target), T0, levels=cc.BOX_LEVELS)
    T_ref, status = restated(name)[:2]
    e0, e_ref, e = tr.pose_error(T0, T_true), tr.pose_error(T_ref, T_true), tr.pose_error(res.T, T_true)
    print(f"{name}: start {e0[0]:.4g} m / {e0[1]:.4g} rad, restatement {e_ref[0]:.4g} / {e_ref[1]:.4g}, "
          f"GPU {e[0]:.4g} / {e[1]:.4g}, inlier share {res.inlier_share:.3f}, rmse {res.rmse:.3g}")
    assert status == cc.OK and res.status == register.OK
    assert e_ref[0] <= e0[0] / 10 and e_ref[1] <= e0[1] / 10
    assert e[0] <= e_ref[0] + 1e-5 and e[1] <= e_ref[1] + 1e-5
    if name == "far":                                      # at least one step scaled onto a limit
        assert ((np.abs(res.stats[:, 2] - 0.1) <= 1e-15) | (np.abs(res.stats[:, 3] - 0.2) <= 1e-15)).any()


def test_more_than_one_round_per_thread():
    """70,000 points at stride 1: more than the grid's 65,536 threads, so some threads take two points."""
    from bnv_fusion_amd import register
    V, F = rr.box()
    T_true = tr.se3_exp(rr.T_TRUE_XI)
    pts = rr.moved(rr.surface_samples(V, F, 70000, seed=9), T_true)
    T0 = tr.se3_exp(rr.XI_NEAR) @ T_true
    target = cc.box_target()
    res = register.register_cloud(dev(pts), index_of(target), T0, levels=((1, 1, 0.2),), records=True)
    assert res.status == register.OK
    check_dumps_and_sums(res, target, pts, T0, 1, 0.2)
    assert res.stats[0, 0] > 65536


def test_the_sign_of_a_target_normal_changes_no_byte():
    from bnv_fusion_amd import register
    res, index, p, target, pts, T0 = near_run()
    turned = register.register_cloud(p, index_of(cc.flipped(target)), T0, levels=LEVELS, records=True)
    assert turned.status == register.OK
    assert turned.T.tobytes() == res.T.tobytes() and turned.records.tobytes() == res.records.tobytes()
    assert turned.poses.tobytes() == res.poses.tobytes() and turned.stats.tobytes() == res.stats.tobytes()


# ---- refusals, determinism, dispatch -----------------------------------------------------------------------------------

def check_refused(res, T0, code):
    assert res.status == code
    assert res.T.tobytes() == np.ascontiguousarray(T0, dtype=np.float64).tobytes()
    assert np.isfinite(res.T).all() and np.isfinite(res.stats).all() and np.isfinite(res.poses).all()
    ran = np.nonzero(res.stats.any(1))[0]
    stop = int(ran.max()) if len(ran) else 0
    assert not res.stats[stop + 1:].any()
    if res.records is not None:
        assert not res.records[stop + 1:].any()
    return stop


def test_refusals_and_determinism():
    from bnv_fusion_amd import register
    res, index, p, target, pts, T0 = near_run()
    # 10 m away: nothing within the gate
    far = register.register_cloud(p + 10.0, index, T0, records=True)
    assert check_refused(far, T0, register.LOST) == 0 and far.inlier_share == 0.0
    assert (far.index.cpu().numpy() == -1).all()
    # a single plane holds no translation along itself; the guess comes back bit for bit
    Vs = np.array([[0.2, 0.1, -0.3], [1.1, 0.3, 0.2], [0.4, 0.9, 0.5]], np.float32)
    Fs = np.array([[0, 1, 2]], np.int64)
    plane = cc.sampled_cloud(Vs, Fs, 800, seed=3)
    above = (plane[:500, :3].astype(np.float64) + 0.01 * plane[:500, 3:].astype(np.float64)).astype(np.float32)
    Tg = tr.se3_exp([0.001, -0.002, 0.001, 0.002, 0.001, -0.001])
    flat = register.register_cloud(dev(above), index_of(plane), Tg, records=True)
    stop = check_refused(flat, Tg, register.DEGENERATE)
    assert flat.stats[stop, 0] > 0 and flat.stats[stop, 4] < 1e-3
    # non-finite points are skipped
    bad = pts.copy()
    bad[3, 0], bad[10, 1], bad[20, 2], bad[33] = np.nan, np.inf, -np.inf, np.nan
    levels = ((1, 1, 0.2),)
    clean = register.register_cloud(p, index, T0, levels=levels, records=True)
    holes = register.register_cloud(dev(bad), index, T0, levels=levels, records=True)
    assert holes.status == register.OK and holes.stats[0, 0] == clean.stats[0, 0] - 4
    check_dumps_and_sums(holes, target, bad, T0, 1, 0.2)
    assert (holes.index.cpu().numpy()[[3, 10, 20, 33]] == -1).all() and np.isfinite(holes.T).all()
    # two calls give identical bytes
    again = register.register_cloud(p, index, T0, levels=LEVELS, records=True)
    assert again.status == res.status == register.OK
    for x, y in ((res.T, again.T), (res.poses, again.poses), (res.stats, again.stats), (res.records, again.records)):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(bits(res.q), bits(again.q)) and np.array_equal(bits(res.index), bits(again.index))


def test_register_points_dispatches_on_a_cloud_index():
    from bnv_fusion_amd import register
    res, index, p, target, pts, T0 = near_run()
    via = register.register_points(p, index, T0, levels=LEVELS, records=True)
    assert isinstance(via, register.CloudRegisterResult)
    assert via.T.tobytes() == res.T.tobytes() and via.records.tobytes() == res.records.tobytes()
    assert np.array_equal(bits(via.index), bits(res.index))
    # an [N, 6] tensor as the target is indexed for the call
    direct = register.register_cloud(p, dev(target), T0, levels=LEVELS)
    assert direct.T.tobytes() == res.T.tobytes()


def test_evaluate_aligns_before_scoring():
    from bnv_fusion_amd import evaluate, register
    V, F = rr.box()
    gt = cc.sampled_cloud(V, F, 6000, seed=31)[:, :3]
    M = tr.se3_exp([0.02, -0.02, 0.02, 0.05, 0.03, -0.06])
    pred = cc.sampled_cloud(V, F, 6000, seed=32)[:, :3].astype(np.float64)
    pred = (pred @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    plain = evaluate.evaluate(dev(pred), dev(gt))
    res = evaluate.evaluate(dev(pred), dev(gt), align=True)
    assert set(plain) == set(evaluate.KEYS) and set(res) == set(plain) | {"T_align", "align_status", "unaligned"}
    assert res["align_status"] == register.OK and res["unaligned"] == plain
    e = tr.pose_error(res["T_align"], tr.rigid_inverse(M))
    print(f"evaluate: F1 unaligned {plain['F1']:.4f}, aligned {res['F1']:.4f}; T_align off by {e[0]:.3g} m / "
          f"{e[1]:.3g} rad")
    assert res["F1"] > plain["F1"]
    lost = evaluate.evaluate(dev(pred), dev(gt), align={"T_guess": tr.se3_exp([0, 0, 0, 10.0, 0, 0])})
    assert lost["align_status"] == register.LOST and lost["F1"] == lost["unaligned"]["F1"] == plain["F1"]


def test_align_scans_end_to_end():
    """Four stations around one corner of the box, 80 x 60 each; stations 1 to 3 start about 2 degrees / 3 cm off."""
    from bnv_fusion_amd import pointcloud, register, scan
    from bnv_fusion_amd.mesh import TriMesh
    V, F = rr.box()
    centre, rot = np.array([1.0, -0.5, 2.0]), R.rotation(3)
    scanner = scan.MeshScanner(TriMesh(V, F), device=DEV)
    dirs = np.array([[1.0, 1.0, 1.0], [1.6, 0.6, 0.8], [0.6, 1.6, 0.8], [0.8, 0.7, 1.7]])
    poses = np.stack([scan.look_at_pose(centre + 1.3 * (rot @ d) / np.linalg.norm(d), centre) for d in dirs])
    K = np.array([[70.0, 0.0, 39.5], [0.0, 70.0, 29.5], [0.0, 0.0, 1.0]])
    points, origins, origin_index = scan.scan_cloud(scanner, poses, K, 60, 80)
    scans = [register.transform_points(tr.rigid_inverse(poses[i]), points[origin_index == i]) for i in range(4)]
    assert all(len(s) > 300 for s in scans)
    rng = np.random.default_rng(4)
    guess = poses.copy()
    for i in range(1, 4):
        xi = np.concatenate([0.035 * unit(rng.normal(size=3)), 0.03 * unit(rng.normal(size=3))])
        guess[i] = poses[i] @ tr.se3_exp(xi)
    got, statuses = pointcloud.align_scans(scans, guess)
    assert statuses == [register.OK] * 4 and got[0].tobytes() == guess[0].tobytes()
    for i in range(1, 4):
        e0, e = tr.pose_error(guess[i], poses[i]), tr.pose_error(got[i], poses[i])
        print(f"station {i} ({len(scans[i])} points): guess {e0[0] * 1e3:.2f} mm / {np.degrees(e0[1]):.3f} deg -> "
              f"{e[0] * 1e3:.2f} mm / {np.degrees(e[1]):.3f} deg")
        assert e[0] < e0[0] and e[1] < e0[1]


def unit(v):
    return v / np.linalg.norm(v)
