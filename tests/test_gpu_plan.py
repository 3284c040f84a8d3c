"""Volume planning on the device (csrc/plan.hip, bnv_fusion_amd/plan.py): both passes against the numpy restatement
(tests/plan_restatement.py) -- every comparison an exact integer or bit equality -- and against the product path the
plan predicts: the per-frame n_avg_pts of NeuralMap and the number of voxels each frame's encode returns."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import plan_restatement as pr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W, SCALE = 60, 80, 0.5
TIMES = list(range(0, 720, 30))
SIZES = (0.02, 0.04, 0.08)


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
    """The 24 frames of the half-scale room sweep at 80 x 60 (host arrays: the restatement's input)."""
    from bnv_fusion_amd import sequence as S
    K = np.asarray(S.intrinsics(H, W), np.float64)
    return tuple({"depth": S.depth_u16(t, H, W, SCALE).numpy(), "intr_mat": K, "T_wc": S.sweep_pose(t, SCALE)}
                 for t in TIMES)


@functools.lru_cache(maxsize=None)
def sweep_dev():
    return tuple(to_device(f) for f in sweep())


@functools.lru_cache(maxsize=None)
def sweep_ref():
    return pr.plan(sweep(), voxel_sizes=SIZES)


def rotated(frames):
    yaw = math.radians(30.0)
    Rw = np.eye(4)
    Rw[:3, :3] = [[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]]
    Rw[:3, 3] = [0.7, -0.2, 1.3]
    return [dict(f, T_wc=Rw @ f["T_wc"]) for f in frames]


def random_pose(rng, shift=1.0):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = rng.uniform(-shift, shift, 3)
    return T


def random_frame(rng, h, w, dtype, conf=False):
    """Depth between 0.3 and 3.4 m (some beyond max_depth 3), holes, and in the float images NaN, inf and negatives."""
    d = rng.uniform(0.3, 3.4, (h, w))
    d[rng.random((h, w)) < 0.1] = 0.0
    if dtype == np.uint16:
        depth = np.rint(d * 1000).astype(np.uint16)
    else:
        depth = d.astype(dtype)
        bad = rng.random((h, w))
        depth[bad < 0.03] = np.nan
        depth[(bad >= 0.03) & (bad < 0.06)] = np.inf
        depth[(bad >= 0.06) & (bad < 0.09)] = -1.25
        depth[(bad >= 0.09) & (bad < 0.10)] = -np.inf
    K = np.array([[0.9 * w, 0, w / 2 - 0.3], [0, 0.95 * w, h / 2 + 0.2], [0, 0, 1]], np.float64)
    f = {"depth": depth, "intr_mat": K, "T_wc": random_pose(rng)}
    if conf:
        f["conf"] = rng.integers(0, 3, (h, w)).astype(np.uint8)
        f["conf_level"] = 2
    return f


def restated_hist(frames, dirs, bin_size, n_bins, max_depth=3.0):
    hist = np.zeros((len(dirs), n_bins), np.int64)
    for f in frames:
        hist += pr.extent_hist(pr.frame_points(f, f["T_wc"], max_depth), dirs, bin_size, n_bins)
    return hist


def device_hist(bnv, frames, **kw):
    planner = bnv.VolumePlanner(device=DEV, **kw)
    for f in frames:
        assert planner.add(to_device(f))
    return planner.histograms(), planner


def assert_rows(cand, frames, dims, A, max_depth=3.0):
    """A candidate's per-frame rows against the restatement: nv, U and the whole histogram."""
    assert cand.rows.shape == (len(frames), 2 + 65)
    for i, f in enumerate(frames):
        nv, U, h = pr.count(pr.frame_points(f, A @ f["T_wc"], max_depth), dims, cand.voxel_size)
        assert (int(cand.rows[i, 0]), int(cand.rows[i, 1])) == (nv, U), (i, cand.voxel_size)
        assert np.array_equal(cand.rows[i, 2:], h), (i, cand.voxel_size)
        assert h[0] == 0 and h.sum() == U


# ---- pass 1 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.float64])
@pytest.mark.parametrize("shape", [(5, 7), (13, 17), (37, 70), (60, 80)])
def test_extent_histograms(bnv, shape, dtype):
    rng = np.random.default_rng([shape[0], shape[1], np.dtype(dtype).itemsize])
    for yaw, conf in ((None, False), (18, False), (18, True), (None, True)):
        f = random_frame(rng, shape[0], shape[1], dtype, conf)
        got, planner = device_hist(bnv, [f], align_yaw=yaw, up="y", n_bins=4096)
        assert got.shape == (39 if yaw else 3, 4096)
        assert all(np.array_equal(a, b) for a, b in zip(planner.dirs, pr.directions(yaw, "y")))
        ref = restated_hist([f], planner.dirs, 0.01, 4096)
        assert np.array_equal(got, ref)
        assert ref[0].sum() == len(pr.frame_points(f, f["T_wc"], 3.0)) > 0
        assert planner.extent().n_points == ref[0].sum()


@pytest.mark.parametrize("up", ["x", "z"])
def test_extent_other_up_axes(bnv, up):
    f = random_frame(np.random.default_rng(5), 13, 17, np.float32)
    got, planner = device_hist(bnv, [f], align_yaw=7, up=up, n_bins=2048)
    assert np.array_equal(got, restated_hist([f], pr.directions(7, up), 0.01, 2048))


def test_extent_all_invalid_frame(bnv):
    f = random_frame(np.random.default_rng(6), 13, 17, np.float32)
    for depth in (np.zeros((13, 17), np.uint16), np.full((13, 17), 3.0, np.float32), np.full((13, 17), np.nan, np.float64)):
        got, planner = device_hist(bnv, [dict(f, depth=depth)], n_bins=1024)
        assert not got.any()
        with pytest.raises(bnv.BnvError):
            planner.extent()
    conf = np.ones((13, 17), np.uint8)
    got, _ = device_hist(bnv, [dict(f, conf=conf, conf_level=2)], n_bins=1024)
    assert not got.any()


def test_extent_wall_in_one_bin(bnv):
    """A wall at constant depth facing the camera: every pixel of the frame in ONE bin along z (the combining path:
    one global atomic per workgroup), a few bins along x and y."""
    K = np.array([[70.0, 0, 39.5], [0, 70.0, 29.5], [0, 0, 1]])
    f = {"depth": np.full((60, 80), 1.505, np.float32), "intr_mat": K, "T_wc": np.eye(4)}
    got, planner = device_hist(bnv, [f, f, f])
    assert got[2, 32768 // 2 + 150] == 3 * 4800 and got[2].sum() == 3 * 4800
    assert np.array_equal(got, restated_hist([f, f, f], planner.dirs, 0.01, 32768))


def test_extent_wider_than_the_window(bnv):
    """1 mm bins: the 256 pixels of a workgroup span thousands of bins, far more than the in-workgroup window holds."""
    f = random_frame(np.random.default_rng(7), 37, 70, np.float32)
    got, planner = device_hist(bnv, [f], bin_size=0.001, n_bins=65536, margin=0.05, align_yaw=3)
    ref = restated_hist([f], planner.dirs, 0.001, 65536)
    assert np.array_equal(got, ref)
    lo, hi = pr.bounds_bins(ref[0], 0.0)
    assert hi - lo > 4 * 256


def test_extent_overflow_bins(bnv):
    f = random_frame(np.random.default_rng(8), 13, 17, np.uint16)
    got, planner = device_hist(bnv, [f], n_bins=64)              # +-0.32 m: most points fall outside
    ref = restated_hist([f], planner.dirs, 0.01, 64)
    assert np.array_equal(got, ref)
    assert ref[:, 0].min() > 0 and ref[0, 63] > 0
    with pytest.raises(bnv.BnvError, match="overflow bin"):
        planner.extent()


def test_extent_accumulates_over_frames(bnv):
    rng = np.random.default_rng(9)
    frames = [random_frame(rng, 37, 70, (np.uint16, np.float32, np.float64)[i % 3], conf=i % 2 == 1) for i in range(9)]
    full, planner = device_hist(bnv, frames, n_bins=4096, align_yaw=18)
    for n in (1, 3, 9):
        got = full if n == 9 else device_hist(bnv, frames[:n], n_bins=4096, align_yaw=18)[0]
        assert np.array_equal(got, restated_hist(frames[:n], planner.dirs, 0.01, 4096))
    a, _ = device_hist(bnv, frames[:4], n_bins=4096, align_yaw=18)
    b, _ = device_hist(bnv, frames[4:], n_bins=4096, align_yaw=18)
    assert np.array_equal(a + b, full)


def test_non_finite_poses_are_skipped(bnv):
    frames = [to_device(f) for f in sweep()[:3]]
    bad = dict(frames[1], T_wc=np.full((4, 4), np.nan))
    plan = bnv.plan_volume([frames[0], bad, frames[2]], voxel_sizes=(0.08,), device=DEV)
    ref = pr.plan([sweep()[0], dict(sweep()[1], T_wc=bad["T_wc"]), sweep()[2]], voxel_sizes=(0.08,))
    assert (plan.n_frames, plan.n_skipped, plan.n_points) == (2, 1, ref["n_points"])
    assert plan.candidates[0].n_avg_pts.tobytes() == ref["candidates"][0]["n_avg_pts"].tobytes()
    assert len(plan.candidates[0].rows) == 2


# ---- pass 2 ----------------------------------------------------------------------------------------------------------

def test_count_sizes_together_and_singly(bnv):
    ref = sweep_ref()
    dims, A = ref["dimensions"], ref["axis_align_mat"]
    frames, host = sweep_dev()[:6], sweep()[:6]
    planner = bnv.VolumePlanner(device=DEV)
    together = planner.count(frames, SIZES, dimensions=dims, axis_align_mat=A)
    assert [c.voxel_size for c in together] == list(SIZES)
    for c in together:
        assert_rows(c, host, dims, A)
        assert c.fits and c.n_xyz == pr.get_world_range(dims, c.voxel_size)[2] and c.table_bytes > 0
    for v, c in zip(SIZES, together):
        alone = planner.count(frames, (v,), dimensions=dims, axis_align_mat=A)[0]
        assert np.array_equal(alone.rows, c.rows) and alone.n_avg_pts.tobytes() == c.n_avg_pts.tobytes()
    swapped = planner.count(frames, SIZES[::-1], dimensions=dims, axis_align_mat=A)
    for a, b in zip(swapped[::-1], together):
        assert np.array_equal(a.rows, b.rows)
    # more than BNV_PLAN_MAX_SIZES candidates go in several launches; one that does not fit is not counted
    many = (0.02, 0.03, 0.04, 0.0005, 0.05, 0.06, 0.07, 0.08, 0.09, 0.1)
    out = planner.count(frames[:2], many, dimensions=dims, axis_align_mat=A)
    assert [c.fits for c in out] == [v != 0.0005 for v in many]
    for c in out:
        if c.fits:
            assert_rows(c, host[:2], dims, A)
        else:
            assert c.n_voxels >= 2 ** 31 and len(c.rows) == 0 and not c.ok and len(c.n_avg_pts) == 0


def test_count_live_and_statistics_are_the_restatements(bnv):
    ref = sweep_ref()
    dims, A = ref["dimensions"], ref["axis_align_mat"]
    for min_pts in (5, 8):
        got = bnv.VolumePlanner(device=DEV).count(sweep_dev(), SIZES, min_pts_in_grid=min_pts, dimensions=dims,
                                                  axis_align_mat=A)
        want = pr.candidates(sweep(), dims, A, SIZES, min_pts_in_grid=min_pts)
        for c, r in zip(got, want):
            assert c.n_avg_pts.dtype == np.float32 and c.n_avg_pts.tobytes() == r["n_avg_pts"].tobytes()
            for k in ("min", "max", "mean", "p25", "p50", "p75", "live_fraction", "ok", "n_voxels", "fits"):
                assert getattr(c, k) == r[k], k
            assert c.live(min_pts).tolist() == [pr.live(h, min_pts) for _, _, h in r["rows"]]


def test_count_power_of_two_voxel_duplicates(bnv):
    """Voxel 2^-5, identity pose, depths at multiples of it, the principal point on a pixel: normalised coordinates are
    integers along z for every pixel and along x / y on the principal row and column, where floor == ceil and two, four
    or eight corners name the same voxel -- each counts, as in the encoder."""
    v = 0.03125
    K = np.array([[40.0, 0, 6.0], [0, 40.0, 4.0], [0, 0, 1]])
    depth = (v * np.random.default_rng(10).integers(8, 40, (9, 13))).astype(np.float32)
    f = {"depth": depth, "intr_mat": K, "T_wc": np.eye(4)}
    dims, A = np.array([2.0, 2.0, 4.0]), np.eye(4)
    p = pr.frame_points(f, A, 3.0)
    bmin = pr.grid(dims, v)[0]
    zn = (p[:, 2] - bmin[2]) / np.float32(v)
    assert (zn == np.floor(zn)).all() and ((p[:, 0] - bmin[0]) / np.float32(v) % 1 == 0).any()
    _, _, cnt = pr.voxel_counts(p, dims, v)
    assert cnt.min() >= 2                                          # every pair has its duplicate along z
    for frames in ([f], [f, f]):
        c = bnv.VolumePlanner(device=DEV).count([to_device(g) for g in frames], (v, 0.0625), dimensions=dims,
                                                axis_align_mat=A)
        assert_rows(c[0], frames, dims, A)
        assert_rows(c[1], frames, dims, A)


def test_count_alternating_voxels_and_runs(bnv):
    """Adjacent pixels alternate between two depths half a metre apart (runs of equal voxels have length 1 and must not
    join across the lane between them), then runs of 2, 3 and 5 pixels."""
    K = np.array([[3000.0, 0, 40.0], [0, 3000.0, 4.0], [0, 0, 1]])   # 80 pixels cover 27 mm at 1 m: one voxel wide
    dims, A = np.array([1.0, 1.0, 4.0]), np.eye(4)
    for period in (1, 2, 3, 5):
        cols = (np.arange(80) // period) % 2
        depth = np.where(cols[None, :] == 0, 1.0, 1.5).astype(np.float32).repeat(8, 0)
        f = {"depth": depth, "intr_mat": K, "T_wc": np.eye(4)}
        for c in bnv.VolumePlanner(device=DEV).count([to_device(f)], (0.08, 0.04), dimensions=dims, axis_align_mat=A):
            assert_rows(c, [f], dims, A)
            assert c.rows[0, 0] == 640


def test_count_reaches_the_histogram_cap(bnv):
    """A wall seen through a long lens: whole waves of 64 consecutive pixels in one voxel, pair counts far above 64."""
    K = np.array([[5000.0, 0, 63.5], [0, 5000.0, 7.5], [0, 0, 1]])
    f = {"depth": np.full((16, 128), 1000, np.uint16), "intr_mat": K, "T_wc": np.eye(4)}
    dims, A = np.array([1.0, 1.0, 3.0]), np.eye(4)
    nv, U, h = pr.count(pr.frame_points(f, A, 3.0), dims, 0.08)
    assert nv == 2048 and h[64] > 0 and h[64] == U                 # every touched voxel holds 64 pairs or more
    nv, U, h = pr.count(pr.frame_points(f, A, 3.0), dims, 0.004)
    assert 0 < h[64] < U                                           # and a size at which some voxels stay below the cap
    for c in bnv.VolumePlanner(device=DEV).count([to_device(f)], (0.08, 0.004), dimensions=dims, axis_align_mat=A):
        assert_rows(c, [f], dims, A)


def test_count_partly_and_wholly_out_of_bounds(bnv):
    far = np.eye(4)
    far[:3, 3] = [40.0, 0.0, 0.0]
    host = [sweep()[0], dict(sweep()[0], T_wc=far @ sweep()[0]["T_wc"]), sweep()[3]]
    dims, A = np.array([2.0, 1.36, 2.48]), np.eye(4)
    got = bnv.VolumePlanner(device=DEV).count([to_device(f) for f in host], (0.04, 0.08), dimensions=dims,
                                              axis_align_mat=A)
    for c in got:
        assert_rows(c, host, dims, A)
        n0 = len(pr.frame_points(host[0], host[0]["T_wc"], 3.0))
        assert 0 < c.rows[0, 0] < n0 and c.rows[1, 0] == 0 and c.rows[1, 1] == 0 and not c.rows[1, 2:].any()
        assert len(c.n_avg_pts) == 2                                # the empty frame is skipped, as integrate skips it


def test_count_confidence_gate_and_dtypes(bnv):
    rng = np.random.default_rng(11)
    host = [random_frame(rng, 37, 70, dt, conf) for dt in (np.uint16, np.float32, np.float64) for conf in (False, True)]
    dims, A = np.array([3.0, 3.0, 3.0]), random_pose(rng, 0.2)
    for c in bnv.VolumePlanner(device=DEV).count([to_device(f) for f in host], (0.05, 0.11), dimensions=dims,
                                                 axis_align_mat=A):
        assert_rows(c, host, dims, A)


def test_count_small_table_reports_overload(bnv):
    ref = sweep_ref()
    dims, A = ref["dimensions"], ref["axis_align_mat"]
    frames, host = sweep_dev()[:2], sweep()[:2]
    U = max(pr.count(pr.frame_points(f, A @ f["T_wc"], 3.0), dims, 0.04)[1] for f in host)
    planner = bnv.VolumePlanner(device=DEV)
    for slots in (64, 4096):                                        # full to the last slot; past half load
        assert slots < 2 * U
        planner.table_slots = slots
        with pytest.raises(bnv.BnvError, match="overflowed"):
            planner.count(frames, (0.04,), dimensions=dims, axis_align_mat=A)
    slots = 64
    while slots < 2 * U:
        slots *= 2
    planner.table_slots = slots                                     # at most half load: exact
    c = planner.count(frames, (0.04,), dimensions=dims, axis_align_mat=A)[0]
    assert_rows(c, host, dims, A)
    assert c.table_bytes == 8 * slots + 256
    planner.table_slots = 0                                         # and the table the library sizes itself
    assert np.array_equal(planner.count(frames, (0.04,), dimensions=dims, axis_align_mat=A)[0].rows, c.rows)


def test_count_table_is_clean_after_every_frame(bnv):
    ref = sweep_ref()
    dims, A = ref["dimensions"], ref["axis_align_mat"]
    f = sweep_dev()[5]
    c = bnv.VolumePlanner(device=DEV).count([f, f, sweep_dev()[6], f], SIZES, dimensions=dims, axis_align_mat=A)
    for cand in c:
        assert np.array_equal(cand.rows[0], cand.rows[1]) and np.array_equal(cand.rows[0], cand.rows[3])
        assert not np.array_equal(cand.rows[0], cand.rows[2])


# ---- the plan against the product path it predicts -------------------------------------------------------------------

def test_plan_of_the_room_is_the_restatements(bnv):
    plan = bnv.plan_volume(sweep_dev(), voxel_sizes=SIZES, device=DEV)
    ref = sweep_ref()
    assert (plan.n_points, plan.n_frames, plan.n_skipped) == (111612, 24, 0)
    for k in ("center", "dimensions", "axis_align_mat", "bounds"):
        assert np.array_equal(getattr(plan, k), ref[k]), k
    assert plan.yaw_deg == 0.0 and plan.voxel_size == ref["voxel_size"] == 0.08
    for c, r in zip(plan.candidates, ref["candidates"]):
        assert c.n_avg_pts.tobytes() == r["n_avg_pts"].tobytes() and len(c.n_avg_pts) == 24
        assert (c.min, c.max, c.mean, c.live_fraction, c.ok) == (r["min"], r["max"], r["mean"], r["live_fraction"], r["ok"])
        assert int(c.rows[:, 0].sum()) == plan.n_points             # trim 0: every valid point is in bounds
    text = plan.table()
    assert "recommended voxel size: 0.08" in text and "3.73 x 1.36 x 2.48" in text


@pytest.mark.parametrize("voxel", [0.04, 0.08])
def test_plan_predicts_the_fusion_statistics(bnv, voxel, capsys):
    """Fusing plan.apply(frame) into NeuralMap(plan.dimensions, voxel): n_pts_list is the candidate's n_avg_pts in
    float32 bits, min / max / mean and print_statistic's percentiles are the candidate's, and every frame's encode
    returns live(min_pts_in_grid) voxels -- through integrate and through fuse_and_decode_async (both pipelines)."""
    plan = bnv.plan_volume(sweep_dev(), voxel_sizes=SIZES, device=DEV)
    cand = plan.candidate(voxel)
    live = cand.live(8)
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)
    frames = [plan.apply(f) for f in sweep_dev()]
    for path in ("integrate", "pipe", "streams"):
        nm = bnv.NeuralMap(plan.dimensions, voxel, model, min_pts_in_grid=8, device=DEV)
        if path == "integrate":
            coords = [nm.integrate(f) for f in frames]
        else:
            nm.frame_pipe = path == "pipe"
            handles = [nm.fuse_and_decode_async(f) for f in frames]
            coords = [h.result()[0] for h in handles]
        torch.cuda.synchronize()
        vol = nm.volume
        assert np.asarray(vol.n_pts_list, np.float32).tobytes() == cand.n_avg_pts.tobytes(), path
        assert [float(np.float32(v)) for v in vol.n_pts_list] == list(vol.n_pts_list)
        assert (vol.min_pts, vol.max_pts, vol.avg_n_pts) == (cand.min, cand.max, cand.mean), path
        vol.print_statistic()
        capsys.readouterr()
        assert (vol.per_25, vol.per_50, vol.per_75) == (cand.p25, cand.p50, cand.p75), path
        assert [0 if c is None else len(c) for c in coords] == live.tolist(), path
    assert cand.ok == (cand.min > 4 and cand.mean >= 8)


# ---- alignment -------------------------------------------------------------------------------------------------------

def test_yaw_alignment_of_the_rotated_room(bnv):
    host = rotated(sweep())
    frames = [to_device(f) for f in host]
    plan = bnv.plan_volume(frames, voxel_sizes=(0.04,), device=DEV, align_yaw=18, up="y")
    plain = bnv.plan_volume(frames, voxel_sizes=(0.04,), device=DEV)
    ref = pr.plan(host, voxel_sizes=(0.04,), align_yaw=18, up="y")
    assert plan.yaw_deg == 30.0 and plain.yaw_deg == 0.0
    for k in ("center", "dimensions", "axis_align_mat", "bounds"):
        assert np.array_equal(getattr(plan, k), ref[k]), k
    assert plan.candidates[0].n_avg_pts.tobytes() == ref["candidates"][0]["n_avg_pts"].tobytes()
    assert plan.candidates[0].n_voxels < plain.candidates[0].n_voxels
    R = plan.axis_align_mat[:3, :3]
    assert abs(np.linalg.det(R) - 1.0) < 1e-12
    # every valid point of every aligned frame is in bounds: by the planner's count, and by the product's front end
    assert int(plan.candidates[0].rows[:, 0].sum()) == plan.n_points == plain.n_points
    from bnv_fusion_amd.frontend import depth_to_input_pts
    from bnv_fusion_amd.sparse_volume import get_world_range, make_grid
    mn, mx, n_xyz = get_world_range(plan.dimensions, 0.04)
    g = make_grid(n_xyz, mn, mx, 0.04, 8)
    lo, hi = np.array(list(g.bound_lo), np.float32), np.array(list(g.bound_hi), np.float32)
    n = 0
    for f in frames[::5]:
        a = plan.apply(f)
        p = depth_to_input_pts(a["depth"], a["intr_mat"], a["T_wc"], max_depth=3.0)[0, :, :3].cpu().numpy()
        assert ((p > lo) & (p < hi)).all()
        n += len(p)
    assert n > 0
    model = bnv.load_pretrained(device=DEV, voxel_size=0.04)
    nm = bnv.NeuralMap(plan.dimensions, 0.04, model, device=DEV)
    for f in frames[:4]:
        nm.integrate(plan.apply(f))
    assert np.asarray(nm.volume.n_pts_list, np.float32).tobytes() == plan.candidates[0].n_avg_pts[:4].tobytes()


# ---- datasets --------------------------------------------------------------------------------------------------------

def test_arkit_capture_without_its_mesh(bnv, tmp_path):
    from bnv_fusion_amd import datasets
    from bnv_fusion_amd.frontend import depth_to_input_pts
    ref = sweep_ref()
    host = sweep()[:8]
    center = np.array([0.4, -0.3, 1.1])
    datasets.write_arkit_capture(str(tmp_path), "cap", [f["depth"] for f in host],
                                 [np.full((H, W), 2, np.uint8)] * len(host), host[0]["intr_mat"],
                                 [f["T_wc"] for f in host], ref["dimensions"], center=center)
    on_file = datasets.ARKitDataset(str(tmp_path), "cap", device=DEV)
    os.remove(tmp_path / "cap" / "export.obj")
    with pytest.raises(FileNotFoundError):
        datasets.ARKitDataset(str(tmp_path), "cap", device=DEV)
    with pytest.raises(FileNotFoundError):
        datasets.ARKitDataset(str(tmp_path), "cap", device=DEV, volume="file")
    planned = datasets.ARKitDataset(str(tmp_path), "cap", device=DEV, volume="plan")
    assert planned.extent.n_frames == len(host) and len(planned) == len(on_file)
    # the planned volume holds every point the mesh's volume holds: the points of the capture's frames
    total = 0
    for k in range(len(planned)):
        a, b = planned[k], on_file[k]
        pa = depth_to_input_pts(a["depth"], a["intr_mat"], a["T_wc"], 3.0, conf=a["conf"], conf_level=2)[0, :, :3].cpu().numpy()
        pb = depth_to_input_pts(b["depth"], b["intr_mat"], b["T_wc"], 3.0, conf=b["conf"], conf_level=2)[0, :, :3].cpu().numpy()
        inside_file = (np.abs(pb) <= on_file.dimensions / 2).all(axis=1)
        assert len(pa) == len(pb) and inside_file.all()
        assert (np.abs(pa) <= planned.dimensions / 2).all()
        # the same points, seen from the two volumes' centres
        shift = planned.axis_align_mat[:3, 3] - on_file.axis_align_mat[:3, 3]
        assert np.abs(pa - (pb + shift)).max() < 1e-5
        total += len(pa)
    assert total == planned.extent.n_points
    assert (planned.dimensions <= on_file.dimensions + 0.13).all()   # no larger than the room plus margin and bins
    # and the plan options reach the planner
    yawed = datasets.ARKitDataset(str(tmp_path), "cap", device=DEV, volume="plan", plan_options={"margin": 0.2})
    assert np.allclose(yawed.dimensions, planned.dimensions + 0.3)


def test_sequence_without_its_dimensions_file(bnv, tmp_path):
    from bnv_fusion_amd import datasets
    host = sweep()[:4]
    datasets.write_sequence(str(tmp_path), "seq", [f["depth"] for f in host], host[0]["intr_mat"],
                            [f["T_wc"] for f in host], [9.0, 9.0, 9.0])
    on_file = datasets.FusionInferenceDataset(str(tmp_path), "seq", device=DEV)
    assert on_file.axis_align_mat is None and list(on_file.dimensions) == [9.0, 9.0, 9.0]
    os.remove(tmp_path / "seq" / "pose" / "dimensions.txt")
    with pytest.raises(FileNotFoundError):
        datasets.FusionInferenceDataset(str(tmp_path), "seq", device=DEV)
    planned = datasets.FusionInferenceDataset(str(tmp_path), "seq", device=DEV, volume="plan")
    # the loader reads poses and intrinsics as float32 (read_pose): the plan is that of those frames
    f32 = lambda m: np.asarray(m, np.float32).astype(np.float64)                     # noqa: E731
    ref = pr.plan([dict(f, T_wc=f32(f["T_wc"]), intr_mat=f32(f["intr_mat"])) for f in host], voxel_sizes=(0.08,))
    assert np.array_equal(planned.dimensions, ref["dimensions"])
    assert np.array_equal(planned.axis_align_mat, ref["axis_align_mat"])
    assert np.array_equal(planned[2]["T_wc"], planned.axis_align_mat @ on_file[2]["T_wc"])


# ---- determinism -----------------------------------------------------------------------------------------------------

def test_planning_twice_gives_identical_bytes(bnv):
    frames = [to_device(f) for f in rotated(sweep())[:12]]

    def blob():
        plan = bnv.plan_volume(frames, voxel_sizes=SIZES, device=DEV, align_yaw=18, trim=1e-3)
        parts = [plan.center, plan.dimensions, plan.axis_align_mat, plan.bounds]
        for c in plan.candidates:
            parts += [c.rows, c.n_avg_pts, np.array([c.min, c.max, c.mean, c.p25, c.p50, c.p75, c.live_fraction])]
        return b"".join(np.ascontiguousarray(p).tobytes() for p in parts), plan
    a, plan = blob()
    b, _ = blob()
    assert a == b
    ref = pr.plan(rotated(sweep())[:12], voxel_sizes=SIZES, align_yaw=18, trim=1e-3)
    assert np.array_equal(plan.dimensions, ref["dimensions"]) and plan.yaw_deg == ref["yaw_deg"]
    for c, r in zip(plan.candidates, ref["candidates"]):
        assert c.n_avg_pts.tobytes() == r["n_avg_pts"].tobytes()
