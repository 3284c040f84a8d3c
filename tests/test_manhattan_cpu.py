"""The Manhattan frame without a GPU: the argument validation of bnv_plan_normals, the numpy restatement
(tests/manhattan_restatement.py, which tests/test_gpu_manhattan.py holds the kernel to bit for bit) on the rotated room
sweep and on the scenes it must refuse, and the host side of bnv_fusion_amd.plan (the estimate works on the integer
histogram alone, so it runs here)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import manhattan_restatement as mr

INVALID = -1
H, W, SCALE = 60, 80, 0.5
TIMES = list(range(0, 720, 30))            # 24 frames of the half-scale room sweep, 2 mm noise
# The largest axis error of the restated estimate on the rotated sweep, in degrees, as measured (the issue's float64
# prototype: 0.037).  The bound of this file and of tests/test_gpu_manhattan.py is three times it, and may never pass
# 0.5 degrees: a third of the half-step of the finest yaw search (90 / 30 degrees).
MEASURED_DEG = 0.0207
BOUND_DEG = 3 * MEASURED_DEG
assert BOUND_DEG <= 0.5


@functools.lru_cache(maxsize=None)
def sweep():
    from bnv_fusion_amd import sequence as S
    K = np.asarray(S.intrinsics(H, W), np.float64)
    return tuple({"depth": S.depth_u16(t, H, W, SCALE).numpy(), "intr_mat": K, "T_wc": S.sweep_pose(t, SCALE)}
                 for t in TIMES)


@functools.lru_cache(maxsize=None)
def rotated_estimate():
    return mr.estimate_frames(mr.premultiplied(sweep(), mr.issue_rotation()))


@functools.lru_cache(maxsize=None)
def uniform_normals():
    v = np.random.default_rng(0).standard_normal((200000, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def wall_frame():
    K = np.asarray([[70.0, 0, 39.5], [0, 70.0, 29.5], [0, 0, 1]])
    return {"depth": np.full((H, W), 1500, np.uint16), "intr_mat": K, "T_wc": np.eye(4)}


# ---- the C entry refuses bad arguments before any HIP call -----------------------------------------------------------

def test_argument_validation_without_a_gpu():
    from bnv_fusion_amd import _lib
    lib = _lib.load()
    depth, conf, hist = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 26)
    Kd = (C.c_double * 9)(50.0, 0, 40.0, 0, 50.0, 30.0, 0, 0, 1)
    Td = (C.c_double * 16)(*np.eye(4).reshape(-1))
    nan, inf = float("nan"), float("inf")

    def normals(depth=depth, dtype=0, H=48, W=64, K=Kd, T=Td, max_depth=3.0, conf=None, level=0, step=1, jump=0.1,
                n_side=32, hist=hist):
        return lib.bnv_plan_normals(depth, dtype, H, W, K, T, max_depth, conf, level, step, jump, n_side, hist, None)

    def bad_T(v):
        T = np.eye(4).reshape(-1)
        T[7] = v
        return (C.c_double * 16)(*T)

    assert normals(depth=None) == INVALID
    assert normals(K=None) == INVALID
    assert normals(T=None) == INVALID
    assert normals(hist=None) == INVALID
    for h, w in ((0, 64), (48, 0), (-1, 64), (48, -5), (40000, 64), (32768, 32768)):
        assert normals(H=h, W=w) == INVALID
    for dtype in (-1, 3):
        assert normals(dtype=dtype) == INVALID
    for bad in (0.0, -1.0, nan, inf, -inf):
        assert normals(max_depth=bad) == INVALID
        assert normals(jump=bad) == INVALID
    assert normals(conf=None, level=1) == INVALID                       # a level without a map
    assert normals(conf=conf, level=-1) == INVALID
    assert normals(T=bad_T(nan)) == INVALID
    assert normals(T=bad_T(inf)) == INVALID
    assert normals(K=(C.c_double * 9)(0.0, 0, 40.0, 0, 50.0, 30.0, 0, 0, 1)) == INVALID
    assert normals(K=(C.c_double * 9)(50.0, 0, nan, 0, 50.0, 30.0, 0, 0, 1)) == INVALID
    for step in (0, -1, 65, 1 << 20):
        assert normals(step=step) == INVALID
    for n_side in (0, 3, 65, -32):
        assert normals(n_side=n_side) == INVALID


# ---- the restated estimate -------------------------------------------------------------------------------------------

def test_rotated_sweep_recovers_the_rooms_axes():
    """Every pose pre-multiplied by G: the room's axes in that world are G's columns."""
    est, G = rotated_estimate(), mr.issue_rotation()
    R = est["R"]
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.allclose(R @ R.T, np.eye(3), atol=1e-12)
    err = mr.axis_errors_deg(R, G)
    print("axis errors (degrees):", err, "confidence:", est["confidence"], "axis mass:", est["axis_mass"])
    assert max(err) <= BOUND_DEG
    assert abs(max(err) - MEASURED_DEG) < 5e-4                          # the figure the README row records
    assert est["n_frames"] == 24 and est["n_normals"] == int(est["hist"][:, 0].sum()) > 90000
    assert 0.85 < est["confidence"] <= 1.0 and abs(est["axis_mass"].sum() - est["confidence"]) < 1e-12


def test_rotated_sweep_names_the_true_vertical_as_down():
    R, G = rotated_estimate()["R"], mr.issue_rotation()
    assert float(R[1] @ G[:, 1]) > math.cos(math.radians(BOUND_DEG))    # +y of the frame is the room's +y (down), signed
    # +z: the horizontal axis the first camera looks along (the sweep starts looking along the room's -z)
    first = mr.premultiplied(sweep()[:1], G)[0]["T_wc"][:3, 2]
    assert float(R[2] @ first) > 0.7 and float(R[2] @ G[:, 2]) < -0.99
    assert np.allclose(np.cross(R[1], R[2]), R[0], atol=1e-12)
    # a hint that points the other way turns the frame over
    hist = rotated_estimate()["hist"]
    flipped = mr.estimate(hist, 32, down=-G[:, 1], view=first)["R"]
    assert float(flipped[1] @ G[:, 1]) < -0.999 and abs(np.linalg.det(flipped) - 1.0) < 1e-12


def test_unrotated_sweep_is_nearly_the_identity():
    est = mr.estimate_frames(sweep())
    assert max(mr.axis_errors_deg(est["R"], np.eye(3))) <= BOUND_DEG
    assert float(est["R"][1, 1]) > 0.999


def test_few_frames_with_a_barely_seen_axis():
    """Three frames and one frame: the third axis has a few per cent of the normals (measured 0.074 and 0.082 degrees;
    an unweighted projection let that axis turn the other two by 2.4 degrees).  The bound is the 0.5 degree cap."""
    G = mr.issue_rotation()
    for n in (3, 1):
        est = mr.estimate_frames(mr.premultiplied(sweep()[:n], G))
        err = mr.axis_errors_deg(est["R"], G)
        print(n, "frames: axis errors (degrees):", err, "axis mass:", est["axis_mass"])
        assert max(err) <= 0.5 and float(est["R"][1] @ G[:, 1]) > 0.999


def test_histogram_is_integer_and_order_free():
    frames = mr.premultiplied(sweep()[:6], mr.issue_rotation())
    whole = mr.frames_histogram(frames)
    assert whole.dtype == np.int64 and whole.shape == (6 * 32 * 32, 4)
    assert np.array_equal(mr.frames_histogram(frames[::-1]), whole)
    assert np.array_equal(mr.frames_histogram(frames[:2]) + mr.frames_histogram(frames[2:]), whole)
    # a bin's sums are those of unit vectors: no longer than its count
    n = whole[:, 0] > 0
    assert (np.linalg.norm(whole[n, 1:] / mr.SCALE, axis=1) <= whole[n, 0] + 1e-3).all()


def test_bins_cover_the_cube_map():
    for n_side in (4, 8, 32, 64):
        c = mr.bin_centres(n_side)
        assert np.array_equal(mr.bins(c, n_side), np.arange(6 * n_side * n_side))
    # ties of the largest component go to the lower index; the sign picks the face
    assert mr.bins(np.array([[1.0, 1.0, 0.0]]) / math.sqrt(2), 8)[0] // 64 == 0
    assert mr.bins(np.array([[0.0, -1.0, -1.0]]) / math.sqrt(2), 8)[0] // 64 == 3
    assert mr.bins(np.array([[0.0, 0.0, -1.0]]), 8)[0] // 64 == 5
    # the far edge of a face is clamped into its last bin
    assert mr.bins(np.array([[1.0, 1.0, 1.0]]) / math.sqrt(3), 8)[0] == 63


def test_uniform_normals_are_refused():
    hist = mr.histogram(uniform_normals(), 32)
    with pytest.raises(mr.Refused, match="confidence"):
        mr.estimate(hist, 32)
    conf = mr.estimate(hist, 32, min_confidence=0.0)["confidence"]
    assert conf < 0.1


def test_single_wall_is_refused():
    n = mr.frame_normals(wall_frame())
    assert len(n) == (H - 2) * (W - 2) and np.abs(n - [0.0, 0.0, -1.0]).max() < 1e-9
    with pytest.raises(mr.Refused, match="axis"):
        mr.estimate_frames([wall_frame()])


# ---- the host side of the package ------------------------------------------------------------------------------------

def test_package_estimate_is_the_restatements():
    from bnv_fusion_amd import plan as P
    est, G = rotated_estimate(), mr.issue_rotation()
    frames = mr.premultiplied(sweep(), G)
    down = np.sum([f["T_wc"][:3, 1] for f in frames], axis=0)
    got = P.manhattan_from_histogram(est["hist"], 32, down=down, view=frames[0]["T_wc"][:3, 2], n_frames=24)
    assert np.abs(got.R - est["R"]).max() <= 1e-9
    assert abs(got.confidence - est["confidence"]) < 1e-12 and np.allclose(got.axis_mass, est["axis_mass"], atol=1e-12)
    assert (got.n_normals, got.n_frames) == (est["n_normals"], 24)
    assert np.array_equal(P._bin_centres(8), mr.bin_centres(8))


def test_package_refusals_name_the_figure():
    from bnv_fusion_amd import BnvError
    from bnv_fusion_amd import plan as P
    with pytest.raises(BnvError, match=r"confidence 0\.0\d+ < min_confidence 0\.3.*align_yaw"):
        P.manhattan_from_histogram(mr.histogram(uniform_normals(), 32), 32)
    with pytest.raises(BnvError, match=r"1 axis carries normals.*align_yaw"):
        P.manhattan_from_histogram(mr.histogram(mr.frame_normals(wall_frame()), 32), 32)
    with pytest.raises(BnvError, match="no pixel gave a normal"):
        P.manhattan_from_histogram(np.zeros((6 * 32 * 32, 4), np.int64), 32)


def test_planner_arguments():
    from bnv_fusion_amd import VolumePlanner
    for kw in ({"align": "gravity"}, {"align": "manhattan", "align_yaw": 18}, {"align": "manhattan", "normal_step": 0},
               {"align": "manhattan", "normal_step": 65}, {"jump": 0.0}, {"jump": float("nan")}, {"n_side": 3},
               {"n_side": 65}, {"cone": 0.0}, {"cone": 45.0}, {"min_confidence": 1.5}, {"down_hint": (0.0, 0.0, 0.0)},
               {"down_hint": (1.0, 0.0)}):
        with pytest.raises(ValueError):
            VolumePlanner(**kw)
    p = VolumePlanner(align="manhattan", down_hint=(0.0, 0.0, -1.0))
    assert p.align == "manhattan" and (p.n_side, p.jump, p.cone, p.min_confidence, p.normal_step) == (32, 0.1, 10.0, 0.3, None)
    plain = VolumePlanner()
    assert plain.align is None and len(plain.dirs) == 3
    with pytest.raises(ValueError):
        plain.add_normals({})
    with pytest.raises(ValueError):
        plain.manhattan()


def test_plan_table_prints_the_frame():
    from bnv_fusion_amd.plan import Extent, ManhattanFrame, plan_from
    frame = ManhattanFrame(R=rotated_estimate()["R"], confidence=0.912, axis_mass=np.array([0.278, 0.223, 0.411]),
                           n_normals=102135, n_frames=24)
    A = np.eye(4)
    A[:3, :3] = frame.R
    ext = Extent(center=np.zeros(3), dimensions=np.ones(3), axis_align_mat=A, yaw_deg=0.0, bounds=np.zeros((3, 2)),
                 n_points=1, n_frames=24, n_skipped=0, hist=np.zeros((3, 2), np.int64), manhattan=frame)
    plan = plan_from(ext, [])
    assert plan.manhattan is frame
    text = plan.table()
    assert "manhattan frame: confidence 0.912" in text and "102135 normals in 24 frames" in text
    old = plan_from(Extent(center=np.zeros(3), dimensions=np.ones(3), axis_align_mat=np.eye(4), yaw_deg=0.0,
                           bounds=np.zeros((3, 2)), n_points=1, n_frames=24, n_skipped=0,
                           hist=np.zeros((3, 2), np.int64)), [])
    assert old.manhattan is None and "manhattan" not in old.table()
