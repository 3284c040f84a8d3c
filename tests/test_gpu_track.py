"""Frame-to-model ICP on the GPU (csrc/track.hip; include/bnv_fusion.h, "Tracking") against the float64 restatement
of tests/track_restatement.py: every iteration's sums and step at the kernel's own poses, recovery of a perturbed
pose against mesh renders, the failure statuses, determinism, and tracking against a fused map."""
import numpy as np
import pytest
import torch

import track_restatement as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE, MAX_DEPTH = 0.5, 3.0
XI = np.array([0.02, -0.015, 0.01, 0.03, -0.02, 0.025])      # about 5 cm / 1.54 degrees
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def scanner():
    from bnv_fusion_amd import scan, sequence
    return scan.MeshScanner(sequence.gt_mesh(SCALE), device=DEV)


def f32_pose(T):
    return np.asarray(T, dtype=np.float64).astype(np.float32).astype(np.float64)


def mesh_view(scanner, t, H, W):
    """The mesh render of sweep pose t (the renderer's float32 pose and intrinsics) -> (depth, normals, K, T)."""
    from bnv_fusion_amd import sequence
    K = sequence.intrinsics(H, W).astype(np.float32).astype(np.float64)
    T = f32_pose(sequence.sweep_pose(t, SCALE))
    depth, _, nrm = scanner.render_depth(T, K, H, W, max_depth=MAX_DEPTH, normals=True, count_seen=False)
    return depth, nrm, K, T


def analytic_frame(t, H, W, dtype):
    from bnv_fusion_amd import sequence
    K = sequence.intrinsics(H, W)
    d = sequence.render_depth(sequence.sweep_pose(t, SCALE), K, H, W, SCALE).numpy()
    d = np.where(np.isfinite(d), d, 0.0)
    if dtype == "u16":
        mm = np.rint(d * 1000.0)
        return np.where((mm > 0) & (mm < 60000), mm, 0).astype(np.uint16), K
    return d.astype(np.float32), K


def as_device(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.astype(np.int32)).to(DEV).to(torch.uint16)
    return torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_every_iteration_matches_restatement(scanner, dtype):
    """61 x 83 frame against a 60 x 80 view, strides 4, 2, 1.  At the kernel's own pose of every iteration the
    restatement finds exactly the same number of pairs, every sum within the float64 summation bound n 2^-52 sum|terms|
    (two orders of summing n terms differ by at most that), and the step solve_update makes of the GPU's own sums
    within 100 cond(A) 2^-52 |xi| (LDL^T is backward stable; the two run the same operations).  The pose that follows
    is exp(xi^) applied to the previous one: sin and cos to an ulp or two and three-term products of entries of at
    most a few metres, 1e-14 absolute."""
    from bnv_fusion_amd import sequence, tracking
    Dm, Nm, Km, Tm = mesh_view(scanner, 100, 60, 80)
    frame, K = analytic_frame(102, 61, 83, dtype)
    T0 = tr.se3_exp(XI) @ sequence.sweep_pose(102, SCALE)
    levels = ((4, 3), (2, 3), (1, 4))
    res = tracking.icp_align(as_device(frame), K, Dm, Nm, Km, Tm, T0, levels=levels, max_depth=MAX_DEPTH,
                             records=True)
    assert res.status == tracking.OK
    assert np.array_equal(res.poses[0], T0) and np.array_equal(res.poses[-1], res.T_wc)
    Dm_h, Nm_h, Tmi = Dm.cpu().numpy(), Nm.cpu().numpy(), tracking.rigid_inverse(Tm)
    k = 0
    for stride, iters in levels:
        for _ in range(iters):
            A, b, rr, pairs, absum = tr.accumulate(frame, K, MAX_DEPTH, Dm_h, Nm_h, Km, Tm, Tmi, res.poses[k], stride)
            ref, got = tr.sums_vector(A, b, rr, pairs), res.records[k, :29]
            assert got[28] == pairs == res.stats[k, 0], f"iteration {k}: pairs {got[28]} against {pairs}"
            assert pairs >= 0.05 * tr.n_samples(61, 83, stride)
            excess = np.abs(got - ref) - pairs * EPS * absum
            print(f"iteration {k} stride {stride}: {pairs:.0f} pairs, largest |diff| / bound "
                  f"{(np.abs(got - ref) / np.maximum(pairs * EPS * absum, 1e-300)).max():.3g}")
            assert (excess <= 0).all(), f"iteration {k}: sums {np.nonzero(excess > 0)[0]} outside the bound"
            Ag, bg, rrg, pg = tr.from_sums(got)
            T1, status, stats, xi = tr.solve_update(Ag, bg, rrg, pg, res.poses[k], tr.n_samples(61, 83, stride))
            assert status == tr.OK
            xi_gpu = res.records[k, 29:35]
            tol = 100 * np.linalg.cond(Ag) * EPS * np.linalg.norm(xi)
            assert np.abs(xi_gpu - np.array(xi)).max() <= tol, f"iteration {k}: xi off by {np.abs(xi_gpu - xi).max()}"
            assert np.abs(res.poses[k + 1] - tr.exp_apply(list(xi_gpu), res.poses[k])).max() <= 1e-14
            assert np.abs(res.poses[k + 1] - T1).max() <= 1e-14 + 4 * tol
            assert np.allclose(res.stats[k, [1, 4]], stats[[1, 4]], rtol=1e-12, atol=0)       # rmse, spread
            assert np.abs(res.stats[k, 2:4] - stats[2:4]).max() <= tol
            k += 1


@pytest.mark.parametrize("t", [100, 150, 250, 500])
def test_recovers_perturbed_pose_against_mesh_render(scanner, t):
    from bnv_fusion_amd import sequence, tracking
    H, W = 120, 160
    Dm, Nm, Km, Tm = mesh_view(scanner, t, H, W)
    frame, K = analytic_frame(t + 2, H, W, "f32")
    Tt = sequence.sweep_pose(t + 2, SCALE)
    T0 = tr.se3_exp(XI) @ Tt
    res = tracking.icp_align(as_device(frame), K, Dm, Nm, Km, Tm, T0, max_depth=MAX_DEPTH)
    T_ref, status, stats, _ = tr.align(frame, K, Dm.cpu().numpy(), Nm.cpu().numpy(), Km, Tm, T0, max_depth=MAX_DEPTH)
    e0, e_ref, e = tr.pose_error(T0, Tt), tr.pose_error(T_ref, Tt), tr.pose_error(res.T_wc, Tt)
    print(f"view {t}: start {e0[0]:.4g} m / {e0[1]:.4g} rad, restatement {e_ref[0]:.4g} / {e_ref[1]:.4g}, "
          f"GPU {e[0]:.4g} / {e[1]:.4g}, spread min {res.stats[:, 4].min():.3g}")
    assert status == tr.OK and res.status == tracking.OK
    assert e_ref[0] <= e0[0] / 10 and e_ref[1] <= e0[1] / 10
    assert e[0] <= e_ref[0] + 1e-5 and e[1] <= e_ref[1] + 1e-5


def check_refused(res, T0, code):
    assert res.status == code
    assert res.T_wc.tobytes() == np.ascontiguousarray(T0, dtype=np.float64).tobytes()
    assert np.isfinite(res.T_wc).all() and np.isfinite(res.stats).all() and np.isfinite(res.poses).all()
    ran = np.nonzero(res.stats.any(1))[0]
    stop = int(ran.max()) if len(ran) else 0
    assert not res.stats[stop + 1:].any()
    return stop


def test_failure_statuses(scanner):
    from bnv_fusion_amd import sequence, tracking
    H, W = 120, 160
    Dm, Nm, Km, Tm = mesh_view(scanner, 100, H, W)
    frame, K = analytic_frame(102, H, W, "f32")
    T0 = tr.se3_exp(XI) @ sequence.sweep_pose(102, SCALE)
    zero_frame = tracking.icp_align(as_device(np.zeros_like(frame)), K, Dm, Nm, Km, Tm, T0, max_depth=MAX_DEPTH)
    assert check_refused(zero_frame, T0, tracking.LOST) == 0 and not zero_frame.stats.any()
    zero_model = tracking.icp_align(as_device(frame), K, torch.zeros_like(Dm), torch.zeros_like(Nm), Km, Tm, T0,
                                    max_depth=MAX_DEPTH)
    assert check_refused(zero_model, T0, tracking.LOST) == 0
    Dm, Nm, Km, Tm = mesh_view(scanner, 10, H, W)
    frame, K = analytic_frame(12, H, W, "f32")
    T0 = tr.se3_exp(XI) @ sequence.sweep_pose(12, SCALE)
    flat = tracking.icp_align(as_device(frame), K, Dm, Nm, Km, Tm, T0, max_depth=MAX_DEPTH)
    stop = check_refused(flat, T0, tracking.DEGENERATE)
    assert flat.stats[stop, 0] > 0 and flat.stats[stop, 4] < 1e-3


def test_two_calls_give_identical_bits(scanner):
    from bnv_fusion_amd import sequence, tracking
    Dm, Nm, Km, Tm = mesh_view(scanner, 250, 120, 160)
    frame, K = analytic_frame(252, 120, 160, "u16")
    T0 = tr.se3_exp(XI) @ sequence.sweep_pose(252, SCALE)
    d = as_device(frame)
    a = tracking.icp_align(d, K, Dm, Nm, Km, Tm, T0, max_depth=MAX_DEPTH)
    b = tracking.icp_align(d, K, Dm, Nm, Km, Tm, T0, max_depth=MAX_DEPTH)
    assert a.status == b.status == tracking.OK
    for x, y in ((a.T_wc, b.T_wc), (a.poses, b.poses), (a.stats, b.stats)):
        assert x.tobytes() == y.tobytes()


def test_mesh_scanner_localises_a_frame(scanner):
    """MeshScanner.track: a 120 x 160 uint16 frame against an 60 x 80 render of the known mesh at the guess itself."""
    from bnv_fusion_amd import sequence, tracking
    frame, K = analytic_frame(252, 120, 160, "u16")
    Tt = sequence.sweep_pose(252, SCALE)
    T0 = tr.se3_exp(XI) @ Tt
    seen = scanner.seen.clone()
    res = scanner.track({"depth": as_device(frame), "intr_mat": K, "T_wc": T0}, model_size=(60, 80),
                        max_depth=MAX_DEPTH)
    e0, e = tr.pose_error(T0, Tt), tr.pose_error(res.T_wc, Tt)
    print(f"scanner.track: {e0[0]:.4g} m / {e0[1]:.4g} rad -> {e[0]:.4g} m / {e[1]:.4g} rad")
    assert res.status == tracking.OK and torch.equal(seen, scanner.seen)
    assert e[0] <= e0[0] / 2 and e[1] <= e0[1] / 2


# ---- against a fused map ------------------------------------------------------------------------------------------

FRAMES = range(96, 141, 4)


def new_map():
    import bnv_fusion_amd as bnv
    model = bnv.load_pretrained(device=DEV, voxel_size=0.02)
    return bnv.NeuralMap(np.array([2.54] * 3), 0.02, model, device=DEV, tsdf=True)


@pytest.fixture(scope="module")
def fused_map():
    """A 128^3 map at 2 cm of the half-size room, sweep frames 96 .. 140 step 4 (test_gpu_render.small_map's recipe)."""
    from bnv_fusion_amd import sequence
    nm = new_map()
    for fr in sequence.sweep_frames(FRAMES, scale=SCALE, device=DEV):
        nm.integrate(fr)
    torch.cuda.synchronize()
    return nm


@pytest.mark.parametrize("source", ["neural", "tsdf"])
def test_track_against_the_map(fused_map, source):
    """Frame 118 (not fused) from a guess 4 cm / 2 degrees off, against a 120 x 160 view of the map."""
    from bnv_fusion_amd import sequence, tracking
    fr = next(sequence.sweep_frames([118], scale=SCALE, device=DEV))
    Tt = fr["T_wc"]
    T0 = tracking.se3_exp(np.concatenate([np.radians(2.0) * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0), np.zeros(3)]))
    T0 = T0 @ np.block([[Tt[:3, :3], np.zeros((3, 1))], [np.zeros((1, 3)), np.ones((1, 1))]])
    T0[:3, 3] = Tt[:3, 3] + 0.04 * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    res = fused_map.track(fr, T_guess=T0, source=source, model_size=(120, 160))
    e0, e = tr.pose_error(T0, Tt), tr.pose_error(res.T_wc, Tt)
    print(f"track/{source}: {e0[0] * 1e3:.2f} mm / {np.degrees(e0[1]):.3f} deg -> {e[0] * 1e3:.2f} mm / "
          f"{np.degrees(e[1]):.3f} deg, pairs {res.stats[-1, 0]:.0f}, rmse {res.stats[-1, 1] * 1e3:.2f} mm, "
          f"spread {res.stats[-1, 4]:.3g}")
    assert abs(e0[0] - 0.04) < 1e-9 and abs(np.degrees(e0[1]) - 2.0) < 1e-6
    assert res.status == tracking.OK
    assert e[0] <= e0[0] / 2 and e[1] <= e0[1] / 2


def test_tracker_reduces_drift():
    """The same frames with drifting odometry: the tracked trajectory ends closer to the truth than the odometry."""
    from bnv_fusion_amd import evaluate, scan, sequence, tracking
    frames = list(sequence.sweep_frames(FRAMES, scale=SCALE, device=DEV))
    truth = np.stack([fr["T_wc"] for fr in frames])
    drifted = scan.drift_poses(truth, sigma_t=0.005, sigma_r=0.003, seed=0)
    tracker = tracking.Tracker(new_map(), source="tsdf", model_size=(120, 160))
    for fr, T in zip(frames, drifted):
        tracker.integrate(dict(fr, T_wc=T))
    torch.cuda.synchronize()
    given, tracked = evaluate.trajectory_errors(drifted, truth), evaluate.trajectory_errors(tracker.poses, truth)
    print(f"tracker: odometry {given['translation_rmse'] * 1e3:.2f} mm / {given['rotation_mean_deg']:.3f} deg, tracked "
          f"{tracked['translation_rmse'] * 1e3:.2f} mm / {tracked['rotation_mean_deg']:.3f} deg, statuses "
          f"{tracker.statuses}")
    assert len(tracker.poses) == len(frames) and tracker.statuses[0] == -1
    assert np.array_equal(tracker.poses[0], truth[0])
    assert tracked["translation_rmse"] < given["translation_rmse"]
