"""Point-to-mesh registration without a GPU: the float64 restatement (tests/register_restatement.py) recovers a known
transform of box samples, its clamped solve is the tracker's wherever no limit is hit, the C entry refuses bad
arguments before any HIP call, and evaluate.trajectory_errors(align=True) recovers a rigid transform.

Recovery, measured with this file's cases (box of 432 faces, 1,500 samples, T_true = exp((.3, -.2, .25, .05, -.04,
.03)), stride 1, gates 0.2 / 0.05 / 0.02 m over 10 + 6 + 4 iterations); the figures are printed by the test:

    near    start 70.7 mm / 6.99 deg    -> 1.0e-4 mm / 1.7e-6 deg   (below 1e-3 mm from iteration 6; step 0 clamped)
    far     start 142 mm / 21.6 deg     -> 1.1e-4 mm / 2.7e-6 deg   (steps 0 .. 9 clamped; below 1e-3 mm from iteration 14)
    noise   near with 2 mm noise        -> 1.94 mm / 0.052 deg      (translation measured at the origin, 2.3 m away)
"""
import ctypes as C
import functools

import numpy as np
import pytest

import register_restatement as rr
import track_restatement as tr


@functools.lru_cache(maxsize=None)
def restated(name):
    V, F, pts, T_true, T0 = rr.box_case(name)
    return rr.register(pts, V, F, T0, levels=rr.BOX_LEVELS), T_true, T0


def test_the_box_has_432_faces_and_the_far_start_is_beyond_the_limits():
    V, F = rr.box()
    assert len(F) == 432 and R_valid(V, F)
    assert abs(np.degrees(np.linalg.norm(rr.XI_NEAR[:3])) - 6.99) < 0.01
    assert abs(np.degrees(np.linalg.norm(rr.XI_FAR[:3])) - 21.6) < 0.1


def R_valid(V, F):
    import mesh_sdf_restatement as R
    return bool(R.valid_faces(V, F).all())


@pytest.mark.parametrize("name", ["near", "far", "noise"])
def test_restatement_recovers_the_box(name):
    (T, status, stats, poses, scales), T_true, T0 = restated(name)
    e0, e = tr.pose_error(T0, T_true), tr.pose_error(T, T_true)
    errs = [tr.pose_error(P, T_true)[0] for P in poses]
    print(f"{name}: start {e0[0] * 1e3:.3g} mm / {np.degrees(e0[1]):.3g} deg -> {e[0] * 1e3:.3g} mm / "
          f"{np.degrees(e[1]):.3g} deg; clamped iterations {np.nonzero(scales < 1.0)[0].tolist()}; "
          f"translation error by iteration (mm) {[float(f'{x * 1e3:.3g}') for x in errs]}")
    assert status == rr.OK
    assert np.array_equal(poses[0], T0) and np.array_equal(poses[-1], T)
    assert e[0] <= e0[0] / 10 and e[1] <= e0[1] / 10
    assert (stats[:, 0] >= 0.05 * 1500).all()
    if name == "far":
        assert scales[0] < 1.0                           # the first step is clamped ...
        assert abs(stats[0, 2] - 0.1) <= 1e-15 or abs(stats[0, 3] - 0.2) <= 1e-15
    if name != "noise":
        assert e[0] <= 1e-6                              # noise-free samples of the mesh itself: to fp32 rounding


def test_without_the_clamp_the_far_start_is_a_jump():
    """The tracker's solve refuses the step the clamp scales: its |w| is beyond 0.1 rad."""
    V, F, pts, T_true, T0 = rr.box_case("far")
    A, b, rrs, pairs, _ = rr.accumulate(pts, V, F, T0, 1, 0.2)
    _, status, stats, _ = tr.solve_update(A, b, rrs, pairs, T0, len(pts))
    assert status == tr.JUMP and stats[2] > 0.1
    T1, status_c, stats_c, xi_c, s = rr.solve_update(A, b, rrs, pairs, T0, len(pts))
    assert status_c == rr.OK and s < 1.0 and abs(s - 0.1 / stats[2]) <= 1e-15
    assert max(stats_c[2] - 0.1, stats_c[3] - 0.2) <= 1e-15


def test_clamped_solve_is_the_trackers_where_no_limit_is_hit():
    V, F, pts, T_true, T0 = rr.box_case("near")
    T = T0
    hit = 0
    for k in range(6):
        A, b, rrs, pairs, _ = rr.accumulate(pts, V, F, T, 1, 0.2)
        ref = tr.solve_update(A, b, rrs, pairs, T, len(pts))
        got = rr.solve_update(A, b, rrs, pairs, T, len(pts))
        if ref[1] == tr.OK:
            hit += 1
            assert got[1] == rr.OK and got[4] == 1.0
            assert got[0].tobytes() == ref[0].tobytes() and got[2].tobytes() == ref[2].tobytes()
            assert list(got[3]) == list(ref[3])
        else:
            assert ref[1] == tr.JUMP and got[4] < 1.0
        T = got[0]
    assert hit >= 3
    # the refusals before the solve are the tracker's too
    for args in ((A, b, rrs, 0.0), (A, b, rrs, 10.0), (np.zeros((6, 6)), b, rrs, pairs)):
        ref, got = tr.solve_update(*args, T, len(pts)), rr.solve_update(*args, T, len(pts))
        assert got[1] == ref[1] != rr.OK and got[2].tobytes() == ref[2].tobytes() and got[0] is T


def test_rows_skip_what_the_header_says():
    q = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [np.nan, 0, 0], [0, 0, 5], [1, 2, 3]], np.float32)
    c = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0], [np.nan] * 3], np.float32)
    feature = np.array([0, 0x11, 0, 0, 0, 0], np.uint8)
    J, r, pairs = rr.rows(q, c, feature, 2.0, True)
    assert pairs == 2.0 and len(r) == 1                  # one row, and the point on the mesh counted
    assert np.array_equal(J[0], [0, 0, 0, 0, 0, 1]) and r[0] == -1.0
    J, r, pairs = rr.rows(q, c, feature, 2.0, False)
    assert pairs == 3.0 and len(r) == 2
    assert rr.n_samples(70001, 4) == 17501 and rr.n_samples(8, 4) == 2


def test_register_entry_refuses_bad_arguments():
    """BNV_ERR_INVALID_ARGUMENT before any HIP call: no GPU needed."""
    from bnv_fusion_amd import _lib
    lib = _lib.load()

    def levels(rows):
        a = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))
        return len(a), a.ctypes.data_as(C.POINTER(C.c_int32)), a

    n, p, keep = levels([(4, 10), (2, 6), (1, 4)])
    assert int(lib.bnv_mesh_register_bytes(n, p)) == (256 * 29 + 20 * 36) * 8
    assert int(lib.bnv_mesh_register_bytes(n, None)) == 0
    for bad in ([(1, 1)] * 9, [(0, 3)], [(2, -1)], [(1, 0)]):
        nb, pb, kb = levels(bad)
        assert int(lib.bnv_mesh_register_bytes(nb, pb)) == 0, bad

    eye = np.eye(4).reshape(-1)

    def dp(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a.ctypes.data_as(C.POINTER(C.c_double)), a

    def call(**over):
        a = dict(index=C.c_void_p(8), index_bytes=1 << 30, points=C.c_void_p(8), n=1000, T0=eye,
                 levels=[(4, 10), (2, 6), (1, 4)], dist=[0.2, 0.05, 0.02], boundary=1, share=0.05, spread=1e-3,
                 max_w=0.1, max_v=0.2, ws=C.c_void_p(8), ws_bytes=1 << 20, pose=C.c_void_p(8), poses=None,
                 stats=C.c_void_p(8), status=C.c_void_p(8))
        a.update(over)
        nl, pl, kl = levels(a["levels"])
        T0 = None if a["T0"] is None else dp(a["T0"])
        dist = None if a["dist"] is None else dp(a["dist"])
        return lib.bnv_mesh_register(a["index"], a["index_bytes"], a["points"], a["n"], T0 and T0[0], nl, pl,
                                     dist and dist[0], a["boundary"], a["share"], a["spread"], a["max_w"], a["max_v"],
                                     a["ws"], a["ws_bytes"], a["pose"], a["poses"], a["stats"], a["status"], None, None,
                                     None, None, None)

    nan_T = eye.copy()
    nan_T[3] = np.nan
    for over in (dict(index=None), dict(points=None), dict(T0=None), dict(dist=None), dict(ws=None), dict(pose=None),
                 dict(stats=None), dict(status=None), dict(n=0), dict(n=-5), dict(n=1 << 31), dict(index_bytes=64),
                 dict(index_bytes=0), dict(levels=[(1, 1)] * 9, dist=[0.1] * 9), dict(levels=[(0, 1)], dist=[0.1]),
                 dict(levels=[(1, 0)], dist=[0.1]), dict(T0=nan_T), dict(dist=[0.2, 0.0, 0.02]),
                 dict(dist=[0.2, 0.05, float("inf")]), dict(dist=[float("nan"), 0.05, 0.02]), dict(dist=[0.2, -1.0, 0.02]),
                 dict(share=-0.1), dict(share=float("nan")), dict(spread=float("nan")), dict(spread=-1.0),
                 dict(max_w=0.0), dict(max_v=float("inf")), dict(max_w=float("nan"))):
        assert call(**over) == -1, over
    assert call(ws_bytes=1024) == -2                                   # BNV_ERR_WORKSPACE_TOO_SMALL


def test_trajectory_errors_align_recovers_a_rigid_transform():
    from bnv_fusion_amd import evaluate, sequence
    gt = np.stack([sequence.sweep_pose(t, 0.5) for t in range(96, 144, 4)])
    assert len(gt) == 12
    M = tr.se3_exp([0.4, -0.7, 0.3, 1.5, -0.8, 0.6])
    est = tr.rigid_inverse(M) @ gt                       # the same trajectory in a frame of its own
    plain = evaluate.trajectory_errors(est, gt)
    assert plain["translation_rmse"] > 0.5 and "T_align" not in plain
    res = evaluate.trajectory_errors(est, gt, align=True)
    assert np.abs(res["T_align"] - M).max() <= 1e-12
    assert res["translation_rmse"] <= 1e-12 and res["translation_max"] <= 1e-12 and res["n"] == 12
    assert res["rotation_max_deg"] <= 1e-5               # arccos near 1: sqrt(2 * 1e-16) radians
    # the default output is what it was: the same keys, the same bytes
    again = evaluate.trajectory_errors(est, gt, align=False)
    assert list(again) == ["translation_rmse", "rotation_mean_deg", "translation_max", "rotation_max_deg", "n"]
    dt = np.linalg.norm(est[:, :3, 3] - gt[:, :3, 3], axis=1)
    tra = np.einsum("nij,nij->n", est[:, :3, :3], gt[:, :3, :3])
    ang = np.degrees(np.arccos(np.clip((tra - 1.0) / 2.0, -1.0, 1.0)))
    want = {"translation_rmse": float(np.sqrt(np.mean(dt * dt))), "rotation_mean_deg": float(ang.mean()),
            "translation_max": float(dt.max()), "rotation_max_deg": float(ang.max()), "n": 12}
    assert repr(again) == repr(want) == repr(plain)
    # a mirrored fit is turned back into a rotation
    T = evaluate.rigid_fit(gt[:, :3, 3], gt[:, :3, 3] * np.array([1.0, 1.0, -1.0]))
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) <= 1e-12
