"""Pass 0 of the volume planner on the device (csrc/plan.hip: k_plan_normals; bnv_fusion_amd/plan.py): the normal
histogram against the numpy restatement (tests/manhattan_restatement.py) -- counts and all three sums, every comparison
an exact integer equality -- then the Manhattan frame found in it and the volume planned in that frame."""
import functools
import math

import numpy as np
import pytest
import torch

import manhattan_restatement as mr
from test_manhattan_cpu import BOUND_DEG

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W, SCALE = 60, 80, 0.5
TIMES = list(range(0, 720, 30))


@pytest.fixture(scope="module")
def bnv():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    import bnv_fusion_amd
    return bnv_fusion_amd


def to_device(f):
    out = dict(f, depth=torch.from_numpy(np.ascontiguousarray(f["depth"])).to(DEV))
    if f.get("conf") is not None:
        out["conf"] = torch.from_numpy(f["conf"]).to(DEV)
    return out


@functools.lru_cache(maxsize=None)
def sweep():
    from bnv_fusion_amd import sequence as S
    K = np.asarray(S.intrinsics(H, W), np.float64)
    return tuple({"depth": S.depth_u16(t, H, W, SCALE).numpy(), "intr_mat": K, "T_wc": S.sweep_pose(t, SCALE)}
                 for t in TIMES)


@functools.lru_cache(maxsize=None)
def rotated():
    """Every pose pre-multiplied by the issue's G (and moved: a translation changes no normal)."""
    return tuple(mr.premultiplied(sweep(), mr.issue_rotation(), (0.7, -0.2, 1.3)))


@functools.lru_cache(maxsize=None)
def rotated_dev():
    return tuple(to_device(f) for f in rotated())


@functools.lru_cache(maxsize=None)
def rotated_ref():
    return mr.estimate_frames(rotated())


def random_pose(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = rng.uniform(-1.0, 1.0, 3)
    return T


def scene_frame(rng, h, w, dtype, conf=False, rough=False):
    """Two tilted planes that meet in a depth jump at a random column, 1 mm noise, holes, a band beyond max_depth 3
    and, in the float images, NaN, inf and negative pixels.  ``rough``: depth uniform in 0.3 .. 3.4 m instead -- with
    an open jump gate its normals fall all over the cube map."""
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    if rough:
        d = rng.uniform(0.3, 3.4, (h, w))
    else:
        split = rng.integers(w // 3, 2 * w // 3 + 1)
        a, b = rng.uniform(-0.02, 0.02, 2)
        d = np.where(u < split, 1.2 + a * u + b * v, 2.1 - b * u + a * v) + rng.normal(0, 0.001, (h, w))
        d[v == h - 2] = 3.2                                              # beyond max_depth
    d[rng.random((h, w)) < 0.05] = 0.0
    if dtype == np.uint16:
        depth = np.rint(d * 1000).astype(np.uint16)
    else:
        depth = d.astype(dtype)
        bad = rng.random((h, w))
        depth[bad < 0.01] = np.nan
        depth[(bad >= 0.01) & (bad < 0.02)] = np.inf
        depth[(bad >= 0.02) & (bad < 0.03)] = -1.25
    K = np.array([[0.9 * w, 0, w / 2 - 0.3], [0, 0.95 * w, h / 2 + 0.2], [0, 0, 1]], np.float64)
    f = {"depth": depth, "intr_mat": K, "T_wc": random_pose(rng)}
    if conf:
        f["conf"] = (rng.random((h, w)) < 0.9).astype(np.uint8) * 2
        f["conf_level"] = 2
    return f


def device_hist(bnv, frames, **kw):
    planner = bnv.VolumePlanner(device=DEV, align="manhattan", **kw)
    for f in frames:
        assert planner.add_normals(to_device(f))
    got = planner.normal_histogram()
    assert got.dtype == np.int64 and got.shape == (6 * planner.n_side ** 2, 4)
    return got


def restated_hist(frames, n_side=32, step=1, jump=0.1):
    return mr.frames_histogram(frames, n_side, 3.0, step, jump)


# ---- the histogram ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("shape", [(5, 7), (13, 17), (37, 70)])
def test_normal_histogram(bnv, shape, step, dtype):
    """37 x 70 is eleven workgroups, the last one partly outside the image; 5 x 7 with step 3 has no pixel whose four
    neighbours lie in the image."""
    rng = np.random.default_rng([shape[0], shape[1], step, np.dtype(dtype).itemsize])
    for n_side, conf, rough, jump in ((32, False, False, 0.1), (8, True, False, 0.1), (32, True, True, 5.0),
                                      (8, False, True, 5.0)):
        f = scene_frame(rng, shape[0], shape[1], dtype, conf, rough)
        got = device_hist(bnv, [f], normal_step=step, n_side=n_side, jump=jump)
        ref = restated_hist([f], n_side, step, jump)
        assert np.array_equal(got, ref), (n_side, conf, rough)
        if shape == (5, 7) and step == 3:
            assert not ref.any()
        elif shape != (5, 7):
            assert ref[:, 0].sum() > 0
        if rough and shape == (37, 70) and step == 1:
            assert (ref[:, 0].reshape(6, -1).sum(axis=1) > 0).sum() >= 3    # normals on several faces of the cube map


def test_default_step_follows_the_image_width(bnv):
    rng = np.random.default_rng(3)
    f = scene_frame(rng, 24, 170, np.uint16)                              # 170 // 80 = 2
    assert np.array_equal(device_hist(bnv, [f]), restated_hist([f], step=2))
    assert not np.array_equal(restated_hist([f], step=2), restated_hist([f], step=1))
    g = scene_frame(rng, 13, 17, np.uint16)                               # below 80 columns: step 1
    assert np.array_equal(device_hist(bnv, [g]), restated_hist([g], step=1))


def test_gates_leave_out_exactly_their_pixels(bnv):
    """A fronto-parallel wall at 1 m, 13 x 17: 11 x 15 = 165 interior pixels.  A hole, a NaN, a pixel beyond max_depth
    and a pixel 0.2 m behind the wall (jump 0.1: more than 0.1 z either way) each take out themselves and their four
    neighbours -- 145 remain; a confidence gate on one more pixel takes out five more."""
    K = np.array([[20.0, 0, 8.0], [0, 20.0, 6.0], [0, 0, 1]])
    d = np.full((13, 17), 1.0, np.float32)
    d[3, 3], d[3, 10], d[9, 3], d[9, 10] = 0.0, np.nan, 3.5, 1.2
    f = {"depth": d, "intr_mat": K, "T_wc": np.eye(4)}
    ref = restated_hist([f])
    assert ref[:, 0].sum() == 145
    assert np.array_equal(device_hist(bnv, [f]), ref)
    conf = np.full((13, 17), 2, np.uint8)
    conf[6, 6] = 1
    g = dict(f, conf=conf, conf_level=2)
    ref = restated_hist([g])
    assert ref[:, 0].sum() == 140
    assert np.array_equal(device_hist(bnv, [g]), ref)
    # with the gate wide open the pixel behind the wall counts, and so do its neighbours
    ref = restated_hist([f], jump=0.5)
    assert ref[:, 0].sum() == 150 and np.array_equal(device_hist(bnv, [f], jump=0.5), ref)
    # a depth of exactly max_depth is valid, a millimetre more is not
    at = dict(f, depth=np.full((13, 17), 3000, np.uint16))
    assert device_hist(bnv, [at])[:, 0].sum() == restated_hist([at])[:, 0].sum() == 165
    assert not device_hist(bnv, [dict(f, depth=np.full((13, 17), 3001, np.uint16))]).any()


def test_wall_in_one_bin(bnv):
    """Every pixel of three frames in ONE bin (the combining path: a workgroup's 256 normals leave it as four atomics),
    its sums those of 3 x 58 x 78 normals (0, 0, -1)."""
    K = np.array([[70.0, 0, 39.5], [0, 70.0, 29.5], [0, 0, 1]])
    f = {"depth": np.full((60, 80), 1.505, np.float32), "intr_mat": K, "T_wc": np.eye(4)}
    got = device_hist(bnv, [f, f, f])
    n = 3 * 58 * 78
    b = int(mr.bins(np.array([[0.0, 0.0, -1.0]]), 32)[0])
    assert got[b].tolist() == [n, 0, 0, -n * 2 ** 20] and got[:, 0].sum() == n
    assert np.array_equal(got, restated_hist([f, f, f]))


def test_histogram_accumulates_over_frames(bnv):
    rng = np.random.default_rng(9)
    frames = [scene_frame(rng, 37, 70, (np.uint16, np.float32)[i % 2], conf=i % 3 == 1, rough=i % 4 == 3)
              for i in range(9)]
    full = device_hist(bnv, frames, jump=0.3)
    for n in (1, 3, 9):
        got = full if n == 9 else device_hist(bnv, frames[:n], jump=0.3)
        assert np.array_equal(got, restated_hist(frames[:n], jump=0.3))
    a, b = device_hist(bnv, frames[:4], jump=0.3), device_hist(bnv, frames[4:], jump=0.3)
    assert np.array_equal(a + b, full)
    assert np.array_equal(device_hist(bnv, frames[4:] + frames[:4], jump=0.3), full)


def test_non_finite_pose_is_left_out(bnv):
    frames = [to_device(f) for f in rotated()[:3]]
    planner = bnv.VolumePlanner(device=DEV, align="manhattan")
    assert planner.add_normals(frames[0])
    assert not planner.add_normals(dict(frames[1], T_wc=np.full((4, 4), np.nan)))
    assert planner.add_normals(frames[2])
    assert planner.n_normal_frames == 2
    assert np.array_equal(planner.normal_histogram(), restated_hist([rotated()[0], rotated()[2]]))


# ---- the frame and the plan ------------------------------------------------------------------------------------------

def test_manhattan_frame_of_the_rotated_sweep(bnv):
    planner = bnv.VolumePlanner(device=DEV, align="manhattan")
    for f in rotated_dev():
        planner.add_normals(f)
    ref, G = rotated_ref(), mr.issue_rotation()
    assert np.array_equal(planner.normal_histogram(), ref["hist"])
    frame = planner.manhattan()
    assert isinstance(frame, bnv.ManhattanFrame)
    assert np.abs(frame.R - ref["R"]).max() <= 1e-9
    err = mr.axis_errors_deg(frame.R, G)
    print("axis errors (degrees):", err, "confidence:", frame.confidence)
    assert max(err) <= BOUND_DEG
    assert float(frame.R[1] @ G[:, 1]) > 0.999                          # down is the room's down
    assert (frame.n_normals, frame.n_frames) == (ref["n_normals"], 24)
    assert abs(frame.confidence - ref["confidence"]) < 1e-12 and np.allclose(frame.axis_mass, ref["axis_mass"])
    assert all(np.array_equal(d, r) for d, r in zip(planner.dirs, frame.R))


def test_plan_in_the_manhattan_frame(bnv):
    """The rotated frames planned with align="manhattan" against the unrotated frames planned as before.  Per axis the
    dimensions agree within two histogram bins (each end is rounded outward to a bin, in two worlds whose bins do not
    line up) plus the extent that the measured axis error sweeps over the room's half diagonal (the room's, taken from
    the unrotated bounds: the margins are no part of it)."""
    G = mr.issue_rotation()
    plan = bnv.plan_volume(rotated_dev(), voxel_sizes=(0.04,), device=DEV, align="manhattan")
    want = bnv.plan_volume([to_device(f) for f in sweep()], voxel_sizes=(0.04,), device=DEV)
    plain = bnv.plan_volume(rotated_dev(), voxel_sizes=(0.04,), device=DEV)
    assert plain.manhattan is None and want.manhattan is None and plan.manhattan is not None
    R = plan.axis_align_mat[:3, :3]
    assert np.array_equal(R, plan.manhattan.R) and abs(np.linalg.det(R) - 1.0) < 1e-12
    err = max(mr.axis_errors_deg(R, G))
    assert err <= BOUND_DEG
    half_diagonal = float(np.linalg.norm(want.bounds[:, 1] - want.bounds[:, 0])) / 2
    tol = 2 * 0.01 + half_diagonal * math.sin(math.radians(err))
    print("dimensions", plan.dimensions, "unrotated", want.dimensions, "plain", plain.dimensions, "tolerance", tol)
    assert np.abs(plan.dimensions - want.dimensions).max() <= tol
    assert plan.dimensions[0] * plan.dimensions[2] < plain.dimensions[0] * plain.dimensions[2]
    assert plan.candidates[0].n_voxels < plain.candidates[0].n_voxels
    # trim 0: every valid point of every aligned frame lies in the planned volume
    assert plan.n_points == plain.n_points == want.n_points
    assert int(plan.candidates[0].rows[:, 0].sum()) == plan.n_points
    text = plan.table()
    assert "manhattan frame: confidence" in text and "manhattan" not in plain.table()


def test_scenes_without_a_frame_are_refused(bnv):
    K = np.array([[70.0, 0, 39.5], [0, 70.0, 29.5], [0, 0, 1]])
    wall = to_device({"depth": np.full((60, 80), 1.505, np.float32), "intr_mat": K, "T_wc": np.eye(4)})
    with pytest.raises(bnv.BnvError, match="1 axis carries normals"):
        bnv.plan_volume([wall], voxel_sizes=(0.04,), device=DEV, align="manhattan")
    empty = dict(wall, depth=torch.zeros((60, 80), dtype=torch.float32, device=DEV))
    with pytest.raises(bnv.BnvError, match="no pixel gave a normal"):
        bnv.plan_volume([empty], voxel_sizes=(0.04,), device=DEV, align="manhattan")
    planner = bnv.VolumePlanner(device=DEV, align="manhattan")
    with pytest.raises(bnv.BnvError, match="no pixel gave a normal"):
        planner.add(wall)                                               # pass 1 before any pass 0


def test_sequence_planned_in_its_own_axes(bnv, tmp_path):
    from bnv_fusion_amd import datasets
    host = rotated()[:8]
    datasets.write_sequence(str(tmp_path), "seq", [f["depth"] for f in host], host[0]["intr_mat"],
                            [f["T_wc"] for f in host], [9.0, 9.0, 9.0])
    planned = datasets.FusionInferenceDataset(str(tmp_path), "seq", device=DEV, volume="plan",
                                              plan_options={"align": "manhattan"})
    frame = planned.extent.manhattan
    assert frame is not None and frame.n_frames == 8
    assert np.array_equal(planned.axis_align_mat[:3, :3], frame.R)
    # eight frames, poses read back as float32: the frame is the room's to a tenth of a degree
    assert max(mr.axis_errors_deg(frame.R, mr.issue_rotation())) < 0.1
