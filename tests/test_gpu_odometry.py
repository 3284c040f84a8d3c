"""RGB-D odometry on the GPU (csrc/odometry.hip; include/bnv_fusion.h, "Odometry") against the float64 restatement of
tests/odometry_restatement.py: a prepared frame bit for bit, every iteration's sums and step at the kernel's own poses,
recovery, the statuses, determinism, a chained trajectory and the tracker without given poses."""
import numpy as np
import pytest
import torch

import odometry_restatement as od

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -52
ROOM_PAIRS = [(10, 12), (10, 14), (100, 104), (250, 256), (500, 504)]
SMALL_SCHEDULE = ((1, 6), (0, 8))        # 48 x 64 frames: two levels (tests/test_odometry_cpu.py says why)
FRAMES = range(96, 141, 4)
PLANES = ("D", "I", "Ix", "Iy", "Dx", "Dy")


def as_device(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.astype(np.int32)).to(DEV).to(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def frame_of(depth, rgb, K, K_rgb=None):
    fr = {"depth": as_device(depth), "intr_mat": K}
    if rgb is not None:
        fr["rgb"] = torch.from_numpy(rgb).to(DEV)
    if K_rgb is not None:
        fr["rgb_intr_mat"] = K_rgb
    return fr


def synthetic_frame(H, W, dtype, Hc=None, Wc=None, seed=0):
    """A sloped surface with a 0.4 m depth step, zero holes, a strip beyond max_depth and a random colour image."""
    rng = np.random.default_rng([seed, H, W])
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = 1.0 + 0.004 * u + 0.003 * v + 0.4 * (u > 0.55 * W) + rng.normal(0.0, 0.002, (H, W))
    d[rng.random((H, W)) < 0.08] = 0.0
    d[-max(H // 8, 1):, :W // 3] = 3.4
    depth = np.rint(d * 1000.0).astype(np.uint16) if dtype == "u16" else d.astype(np.float32)
    rgb = rng.integers(0, 256, (Hc or H, Wc or W, 3), dtype=np.uint8)
    K = np.array([[0.9 * W, 0.0, 0.5 * W - 0.3], [0.0, 0.9 * W, 0.5 * H - 0.7], [0.0, 0.0, 1.0]])
    return depth, rgb, K


def check_prepared(prepared, want):
    from bnv_fusion_amd import odometry
    assert prepared.levels == len(want)
    for l, ref in enumerate(want):
        got = odometry.level_view(prepared, l).cpu().numpy()
        assert got.shape == ref["D"].shape + (8,)
        for k, name in enumerate(PLANES):
            assert got[..., k].tobytes() == ref[name].tobytes(), f"level {l} plane {name}"
        assert np.array_equal(got[..., 6], ref["valid"].astype(np.float32)) and not got[..., 7].any()
        assert ref["valid"].any() or min(ref["D"].shape) < 8


@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("size", [(5, 7, 2), (13, 17, 3), (61, 83, 3)])
def test_prepared_frame_is_bit_equal(size, dtype):
    from bnv_fusion_amd import odometry
    H, W, levels = size
    depth, rgb, K = synthetic_frame(H, W, dtype)
    got = odometry.prepare_frame(frame_of(depth, rgb, K), levels=levels)
    check_prepared(got, od.prepare(depth, rgb, K, levels=levels))
    no_rgb = odometry.prepare_frame(frame_of(depth, None, K), levels=levels)
    check_prepared(no_rgb, od.prepare(depth, None, K, levels=levels))
    assert got.has_rgb and not no_rgb.has_rgb


@pytest.mark.parametrize("color_size", [(100, 190), (20, 30), (37, 70)])
def test_colour_image_of_its_own_size_and_intrinsics(color_size):
    """37 x 70 depth against a larger colour image at a non-integer ratio (footprint means), a smaller one (no centre
    in the footprint: the bilinear sample) and one of the same size with shifted intrinsics."""
    from bnv_fusion_amd import odometry
    Hc, Wc = color_size
    depth, rgb, K = synthetic_frame(37, 70, "f32", Hc, Wc)
    Kc = np.array([[K[0, 0] * Wc / 70 * 1.013, 0.0, K[0, 2] * Wc / 70 + 0.37],
                   [0.0, K[1, 1] * Hc / 37 * 0.991, K[1, 2] * Hc / 37 - 0.21], [0.0, 0.0, 1.0]])
    got = odometry.prepare_frame(frame_of(depth, rgb, K, Kc), levels=3)
    check_prepared(got, od.prepare(depth, rgb, K, levels=3, K_rgb=Kc))
    if (Hc, Wc) != (37, 70):       # without intrinsics the colour image shows the same view
        from bnv_fusion_amd import tracking
        got = odometry.prepare_frame(frame_of(depth, rgb, K), levels=3)
        check_prepared(got, od.prepare(depth, rgb, K, levels=3, K_rgb=tracking.scaled_intrinsics(K, 70 / Wc, 37 / Hc)))


@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_every_iteration_matches_restatement(dtype):
    """61 x 83 frames of the room, pair 100 -> 102, levels 2, 1, 0.  At the kernel's own pose of every iteration the
    restatement finds exactly the same number of pairs, every sum within 2 pairs 2^-52 sum|terms| (2 pairs terms per
    sum: two orders of summing n terms differ by at most n 2^-52 sum|terms|), and the step solve_update makes of the
    GPU's own sums within 100 cond(A) 2^-52 |xi|; the pose that follows is exp(xi^) of the previous one to 1e-14."""
    from bnv_fusion_amd import odometry
    a, b = od.room_frame(100, 61, 83, dtype), od.room_frame(102, 61, 83, dtype)
    K = a[2]
    schedule = ((2, 3), (1, 3), (0, 4))
    ref_g = odometry.prepare_frame(frame_of(a[0], a[1], K))
    cur_g = odometry.prepare_frame(frame_of(b[0], b[1], K))
    res = odometry.rgbd_align(ref_g, cur_g, schedule=schedule, records=True)
    assert res.status == odometry.OK
    assert np.array_equal(res.poses[0], np.eye(4)) and np.array_equal(res.poses[-1], res.T_wc)
    ref, cur = od.prepare(a[0], a[1], K), od.prepare(b[0], b[1], K)
    k = 0
    for level, iters in schedule:
        n_pixels = ref[level]["D"].size
        for _ in range(iters):
            A, bb, rr, pairs, absum = od.accumulate(ref[level], cur[level], res.poses[k])
            want, got = od.sums_vector(A, bb, rr, pairs), res.records[k, :29]
            assert got[28] == pairs == res.stats[k, 0], f"iteration {k}: pairs {got[28]} against {pairs}"
            assert pairs >= 0.05 * n_pixels
            bound = 2 * pairs * EPS * absum
            print(f"iteration {k} level {level}: {pairs:.0f} pairs, largest |diff| / bound "
                  f"{(np.abs(got - want) / np.maximum(bound, 1e-300)).max():.3g}")
            assert (np.abs(got - want) <= bound).all(), f"iteration {k}: sums outside the bound"
            Ag, bg, rrg, pg = od.from_sums(got)
            T1, status, stats, xi = od.solve_update(Ag, bg, rrg, pg, res.poses[k], n_pixels)
            assert status == od.OK
            xi_gpu = res.records[k, 29:35]
            tol = 100 * np.linalg.cond(Ag) * EPS * np.linalg.norm(xi)
            assert np.abs(xi_gpu - np.array(xi)).max() <= tol, f"iteration {k}: xi off by {np.abs(xi_gpu - xi).max()}"
            assert np.abs(res.poses[k + 1] - od.exp_apply(list(xi_gpu), res.poses[k])).max() <= 1e-14
            assert np.abs(res.poses[k + 1] - T1).max() <= 1e-14 + 4 * tol
            assert np.allclose(res.stats[k, [1, 4]], stats[[1, 4]], rtol=1e-12, atol=0)       # rmse, spread
            assert np.abs(res.stats[k, 2:4] - stats[2:4]).max() <= tol
            k += 1


def gpu_and_restatement(a, b, K, T_guess=None, levels=3, **kw):
    from bnv_fusion_amd import odometry
    ref_g = odometry.prepare_frame(frame_of(a[0], a[1], K), levels=levels)
    cur_g = odometry.prepare_frame(frame_of(b[0], b[1], K), levels=levels)
    res = odometry.rgbd_align(ref_g, cur_g, T_guess, **kw)
    want = od.align(od.prepare(a[0], a[1], K, levels=levels), od.prepare(b[0], b[1], K, levels=levels), T_guess, **kw)
    return res, want


@pytest.mark.parametrize("case", ["plane48", "plane120"] + ROOM_PAIRS)
def test_recovery_matches_restatement(case):
    """The GPU's errors are at most the restatement's + 1e-5 (m, rad)."""
    from bnv_fusion_amd import odometry
    if case == "plane48":
        a, b, K, T_true = od.plane_pair()
        res, want = gpu_and_restatement(a, b, K, levels=2, schedule=SMALL_SCHEDULE)
    elif case == "plane120":
        a, b, K, T_true = od.plane_pair(120, 160)
        res, want = gpu_and_restatement(a, b, K)
    else:
        fa, fb = od.room_frame(case[0]), od.room_frame(case[1])
        a, b, K, T_true = fa[:2], fb[:2], fa[2], od.rigid_inverse(fb[3]) @ fa[3]
        res, want = gpu_and_restatement(a, b, K)
    e0, e_ref, e = od.pose_error(np.eye(4), T_true), od.pose_error(want[0], T_true), od.pose_error(res.T_wc, T_true)
    print(f"{case}: start {e0[0]:.4g} m / {e0[1]:.4g} rad, restatement {e_ref[0]:.4g} / {e_ref[1]:.4g}, GPU "
          f"{e[0]:.4g} / {e[1]:.4g}, spread min {res.stats[:, 4].min():.3g}")
    assert want[1] == od.OK and res.status == odometry.OK
    assert e_ref[0] <= e0[0] / 10
    assert e[0] <= e_ref[0] + 1e-5 and e[1] <= e_ref[1] + 1e-5


def check_refused(res, T0, code):
    assert res.status == code
    assert res.T_wc.tobytes() == np.ascontiguousarray(T0, dtype=np.float64).tobytes()
    assert np.isfinite(res.T_wc).all() and np.isfinite(res.stats).all() and np.isfinite(res.poses).all()
    assert not res.stats[1:].any()


def test_failure_statuses():
    from bnv_fusion_amd import odometry
    T0 = np.eye(4)
    T0[:3, 3] = [0.003, 0.001, 0.0]
    a, b, K, _ = od.plane_pair(grey=128)
    res, want = gpu_and_restatement(a, b, K, T0)
    check_refused(res, T0, odometry.DEGENERATE)
    assert want[1] == od.DEGENERATE and res.stats[0, 0] == want[2][0, 0] > 0 and res.stats[0, 4] == 0.0
    zero = (np.zeros_like(a[0]), a[1])
    for x, y in ((zero, b), (a, zero)):
        res, want = gpu_and_restatement(x, y, K, T0)
        check_refused(res, T0, odometry.LOST)
        assert want[1] == od.LOST and not res.stats.any()


def test_two_calls_give_identical_bits():
    from bnv_fusion_amd import odometry
    fa, fb = od.room_frame(250, dtype="u16"), od.room_frame(252, dtype="u16")
    out = []
    for _ in range(2):
        ref = odometry.prepare_frame(frame_of(fa[0], fa[1], fa[2]))
        cur = odometry.prepare_frame(frame_of(fb[0], fb[1], fa[2]))
        out.append(odometry.rgbd_align(ref, cur, records=True))
    a, b = out
    assert a.status == b.status == odometry.OK
    for x, y in ((a.T_wc, b.T_wc), (a.poses, b.poses), (a.stats, b.stats), (a.records, b.records)):
        assert x.tobytes() == y.tobytes()
    fr = frame_of(fa[0], fa[1], fa[2])
    p, q = odometry.prepare_frame(fr), odometry.prepare_frame(fr)
    for level in range(3):      # (the pads between the levels are never written)
        assert torch.equal(odometry.level_view(p, level), odometry.level_view(q, level))


def test_the_flat_view_icp_refuses_is_aligned():
    """View 10 looks at a flat wall: test_gpu_track.py pins icp_align of it as DEGENERATE; the colour holds it."""
    from bnv_fusion_amd import odometry
    fa, fb = od.room_frame(10), od.room_frame(12)
    res, _ = gpu_and_restatement(fa[:2], fb[:2], fa[2])
    assert res.status == odometry.OK and res.stats[:, 4].min() >= 1e-3
    depth_only = odometry.rgbd_align(odometry.prepare_frame(frame_of(fa[0], None, fa[2])),
                                     odometry.prepare_frame(frame_of(fb[0], None, fa[2])))
    assert depth_only.status == odometry.DEGENERATE


# ---- trajectories -------------------------------------------------------------------------------------------------

H, W = 120, 160


@pytest.fixture(scope="module")
def sweep():
    """Sweep frames 96 .. 140 step 4 at 120 x 160: the sensor's noisy uint16 depth, the colour of the clean depth."""
    from bnv_fusion_amd import scan, sequence
    K = sequence.intrinsics(H, W)
    frames = []
    for t in FRAMES:
        T = sequence.sweep_pose(t, od.SCALE)
        clean = sequence.render_depth(T, K, H, W, od.SCALE, device=DEV)
        clean = torch.where(torch.isfinite(clean), clean, torch.zeros_like(clean)).to(torch.float32)
        frames.append({"frame_id": int(t), "depth": sequence.depth_u16(t, H, W, od.SCALE, device=DEV), "intr_mat": K,
                       "T_wc": T, "rgb": scan.render_color(clean, K, T)})
    truth = np.stack([fr["T_wc"] for fr in frames])
    return frames, truth, scan.drift_poses(truth, 0.005, 0.003, seed=0)


def new_map():
    import bnv_fusion_amd as bnv
    model = bnv.load_pretrained(device=DEV, voxel_size=0.02)
    return bnv.NeuralMap(np.array([2.54] * 3), 0.02, model, device=DEV, tsdf=True)


def without_poses(frames):
    return [fr if i == 0 else {k: v for k, v in fr.items() if k != "T_wc"} for i, fr in enumerate(frames)]


def test_chained_odometry_beats_drifting_poses(sweep):
    from bnv_fusion_amd import evaluate, odometry, tracking
    frames, truth, drifted = sweep
    odo = odometry.RgbdOdometry()
    poses = []
    for fr in without_poses(frames):
        step = odo.step(fr)
        poses.append(truth[0] if not poses else poses[-1] @ tracking.rigid_inverse(step.T_wc))
    given, chained = evaluate.trajectory_errors(drifted, truth), evaluate.trajectory_errors(poses, truth)
    print(f"chained odometry: {chained['translation_rmse'] * 1e3:.2f} mm / {chained['rotation_mean_deg']:.3f} deg, "
          f"drifting poses {given['translation_rmse'] * 1e3:.2f} mm / {given['rotation_mean_deg']:.3f} deg, statuses "
          f"{odo.statuses}")
    assert odo.statuses == [-1] + [odometry.OK] * (len(frames) - 1) and odo.failures == 0
    assert chained["translation_rmse"] < given["translation_rmse"]


def test_tracker_without_poses(sweep):
    from bnv_fusion_amd import evaluate, odometry, tracking
    frames, truth, drifted = sweep
    tracker = tracking.Tracker(new_map(), source="tsdf", model_size=(H, W), odometry="rgbd")
    for fr in without_poses(frames):
        tracker.integrate(fr)
    torch.cuda.synchronize()
    odo = odometry.RgbdOdometry()
    chain = []
    for fr in frames:
        step = odo.step(fr)
        chain.append(truth[0] if not chain else chain[-1] @ tracking.rigid_inverse(step.T_wc))
    given, tracked = evaluate.trajectory_errors(drifted, truth), evaluate.trajectory_errors(tracker.poses, truth)
    chained = evaluate.trajectory_errors(chain, truth)
    print(f"tracker on odometry: {tracked['translation_rmse'] * 1e3:.2f} mm / {tracked['rotation_mean_deg']:.3f} deg, "
          f"chained odometry alone {chained['translation_rmse'] * 1e3:.2f} mm, drifting poses "
          f"{given['translation_rmse'] * 1e3:.2f} mm, statuses {tracker.statuses}, odometry {tracker.odometry.statuses}")
    assert len(tracker.poses) == len(frames) and tracker.statuses[0] == -1
    assert np.array_equal(tracker.poses[0], truth[0])
    assert tracked["translation_rmse"] < given["translation_rmse"]


def test_tracker_with_given_poses_is_unchanged(sweep):
    """odometry=None is the tracker as it was: the same poses, byte for byte, as without the argument."""
    from bnv_fusion_amd import tracking
    frames, _, drifted = sweep
    runs = []
    for kw in ({}, {"odometry": None}):
        tracker = tracking.Tracker(new_map(), source="tsdf", model_size=(H, W), **kw)
        for fr, T in zip(frames, drifted):
            tracker.integrate(dict(fr, T_wc=T))
        torch.cuda.synchronize()
        runs.append((np.stack(tracker.poses), tracker.statuses))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1] == runs[1][1]
    assert tracker.odometry is None
