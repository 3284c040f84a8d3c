"""Volume planning without a GPU: the argument validation of the bnv_plan_* entries, the numpy restatement
(tests/plan_restatement.py, which tests/test_gpu_plan.py holds the kernels to bit for bit) pinned to the reference
through the oracle's encode_pointcloud, the restatement's properties, and the host side of bnv_fusion_amd.plan."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import plan_restatement as pr
from conftest import WEIGHTS_FP32

INVALID = -1
H, W, SCALE = 60, 80, 0.5
TIMES = list(range(0, 720, 30))            # 24 frames of the half-scale room sweep


@functools.lru_cache(maxsize=None)
def sweep():
    from bnv_fusion_amd import sequence as S
    K = np.asarray(S.intrinsics(H, W), np.float64)
    return tuple({"depth": S.depth_u16(t, H, W, SCALE).numpy(), "intr_mat": K, "T_wc": S.sweep_pose(t, SCALE)}
                 for t in TIMES)


def rotated(frames):
    yaw = math.radians(30.0)
    Rw = np.eye(4)
    Rw[:3, :3] = [[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]]
    Rw[:3, 3] = [0.7, -0.2, 1.3]
    return [dict(f, T_wc=Rw @ f["T_wc"]) for f in frames]


@functools.lru_cache(maxsize=None)
def sweep_plan():
    return pr.plan(sweep(), voxel_sizes=(0.02, 0.04, 0.08))


# ---- the C entries refuse bad arguments before any HIP call ----------------------------------------------------------

def _grid(dims=(1.0, 1.0, 1.0), v=0.05):
    from bnv_fusion_amd.sparse_volume import get_world_range, make_grid
    mn, mx, n_xyz = get_world_range(np.asarray(dims), v)
    return make_grid(n_xyz, mn, mx, v, 8)


def test_argument_validation_without_a_gpu():
    from bnv_fusion_amd import _lib
    lib = _lib.load()
    depth, conf, hist, ws, rows = (C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 26), C.c_void_p(1 << 28),
                                   C.c_void_p(1 << 30))
    Kd = (C.c_double * 9)(50.0, 0, 40.0, 0, 50.0, 30.0, 0, 0, 1)
    Td = (C.c_double * 16)(*np.eye(4).reshape(-1))
    dirs = (C.c_double * 9)(*np.eye(3).reshape(-1))
    grids = (_lib.Grid * 2)(_grid(), _grid(v=0.1))
    nan, inf = float("nan"), float("inf")

    def extent(depth=depth, dtype=0, H=48, W=64, K=Kd, T=Td, max_depth=3.0, conf=None, level=0, dirs=dirs, n_dirs=3,
               bin_size=0.01, n_bins=4096, hist=hist):
        return lib.bnv_plan_extent(depth, dtype, H, W, K, T, max_depth, conf, level, dirs, n_dirs, bin_size, n_bins,
                                   hist, None)

    def count(depth=depth, dtype=0, H=48, W=64, K=Kd, T=Td, max_depth=3.0, conf=None, level=0, grids=grids, n_sizes=2,
              slots=0, ws=ws, ws_bytes=1 << 30, rows=rows):
        return lib.bnv_plan_count(depth, dtype, H, W, K, T, max_depth, conf, level, grids, n_sizes, slots, ws, ws_bytes,
                                  rows, None)

    def bad_T(v):
        T = np.eye(4).reshape(-1)
        T[7] = v
        return (C.c_double * 16)(*T)

    for call in (extent, count):
        assert call(depth=None) == INVALID
        assert call(K=None) == INVALID
        assert call(T=None) == INVALID
        for h, w in ((0, 64), (48, 0), (-1, 64), (48, -5), (40000, 64), (32768, 32768)):
            assert call(H=h, W=w) == INVALID
        for dtype in (-1, 3):
            assert call(dtype=dtype) == INVALID
        for bad in (0.0, -1.0, nan, inf, -inf):
            assert call(max_depth=bad) == INVALID
        assert call(conf=None, level=1) == INVALID                       # a level without a map
        assert call(conf=conf, level=-1) == INVALID
        assert call(T=bad_T(nan)) == INVALID
        assert call(T=bad_T(inf)) == INVALID
        assert call(K=(C.c_double * 9)(0.0, 0, 40.0, 0, 50.0, 30.0, 0, 0, 1)) == INVALID
    assert extent(dirs=None) == INVALID
    assert extent(hist=None) == INVALID
    for n_dirs in (0, -1, 65):
        assert extent(n_dirs=n_dirs) == INVALID
    for n_bins in (0, 1, 3, 1000, 131072, -4096):
        assert extent(n_bins=n_bins) == INVALID
    for bad in (0.0, -0.01, nan, inf):
        assert extent(bin_size=bad) == INVALID
    assert extent(dirs=(C.c_double * 9)(1, 0, 0, 0, nan, 0, 0, 0, 1)) == INVALID
    assert count(grids=None) == INVALID
    assert count(ws=None) == INVALID
    assert count(rows=None) == INVALID
    for n_sizes in (0, -1, 9):
        assert count(n_sizes=n_sizes) == INVALID
    for slots in (-64, 32, 100, 1 << 31):
        assert count(slots=slots) == INVALID
    assert count(ws_bytes=1024) == -2                                    # BNV_ERR_WORKSPACE_TOO_SMALL
    huge = _grid()
    huge.n_xyz[0] = huge.n_xyz[1] = huge.n_xyz[2] = 1291                 # 1291^3 >= 2^31
    assert count(grids=(_lib.Grid * 1)(huge), n_sizes=1) == INVALID
    broken = _grid()
    broken.voxel_size = 0.0
    assert count(grids=(_lib.Grid * 1)(broken), n_sizes=1) == INVALID
    broken = _grid()
    broken.n_xyz[1] = 0
    assert count(grids=(_lib.Grid * 1)(broken), n_sizes=1) == INVALID
    # the workspace: its size, and its reset's own checks
    assert int(lib.bnv_plan_workspace_bytes(48, 64, grids, 2, 0)) > 0
    assert int(lib.bnv_plan_workspace_bytes(48, 64, grids, 2, 64)) == 2 * (256 + 256 + 256)
    assert int(lib.bnv_plan_workspace_bytes(0, 64, grids, 2, 0)) == 0
    assert int(lib.bnv_plan_workspace_bytes(48, 64, None, 2, 0)) == 0
    assert int(lib.bnv_plan_workspace_bytes(48, 64, grids, 9, 0)) == 0
    assert int(lib.bnv_plan_workspace_bytes(48, 64, grids, 2, 96)) == 0
    assert lib.bnv_plan_workspace_reset(None, 1 << 30, 48, 64, grids, 2, 0, None) == INVALID
    assert lib.bnv_plan_workspace_reset(ws, 1 << 30, 48, 64, grids, 0, 0, None) == INVALID
    assert lib.bnv_plan_workspace_reset(ws, 1024, 48, 64, grids, 2, 0, None) == -2
    # the table of a candidate never passes half load: 2 min(8 H W, voxels) slots, rounded up to a power of two
    for dims, most in (((1.0, 1.0, 1.0), None), ((9.0, 9.0, 9.0), 8 * 48 * 64)):
        g = _grid(dims)
        nvox = g.n_xyz[0] * g.n_xyz[1] * g.n_xyz[2]
        assert (most is None) == (nvox < 8 * 48 * 64)
        slots = 64
        while slots < 2 * (most or nvox):
            slots *= 2
        assert int(lib.bnv_plan_workspace_bytes(48, 64, (_lib.Grid * 1)(g), 1, 0)) == 2 * slots * 4 + 256


def test_restated_grid_is_the_products():
    """The float32 bounds the restatement compares against are those of make_grid (torch CPU ops, as the reference)."""
    for dims, v in (((3.73, 1.36, 2.48), 0.04), ((3.73, 1.36, 2.48), 0.08), ((1.24, 1.24, 1.24), 0.02),
                    ((0.9, 2.13, 1.77), 0.03125)):
        g = _grid(dims, v)
        bmin, lo, hi, vf, n_xyz = pr.grid(dims, v)
        assert list(g.n_xyz) == n_xyz and np.float32(g.voxel_size) == vf
        for a in range(3):
            assert (np.float32(g.bound_min[a]), np.float32(g.bound_lo[a]), np.float32(g.bound_hi[a])) == \
                (bmin[a], lo[a], hi[a])


# ---- the restatement against the oracle ------------------------------------------------------------------------------

@pytest.mark.parametrize("voxel", [0.04, 0.08])
def test_restatement_matches_the_oracle(voxel):
    """On three sweep frames and a frame moved out of the volume: n_avg_pts bit-equal to encode_pointcloud's, the live
    count equal to the number of voxels it returns (min_pts_in_grid 5 and 8), nv = 0 where it returns None."""
    from oracle import bnv_oracle as O
    plan = sweep_plan()
    dims, A = plan["dimensions"], plan["axis_align_mat"]
    sd = O.load_weights(WEIGHTS_FP32)
    mn, mx, n_xyz = pr.get_world_range(dims, voxel)
    far = np.eye(4)
    far[:3, 3] = [40.0, 0.0, 0.0]
    frames = [sweep()[0], sweep()[1], sweep()[2], dict(sweep()[0], T_wc=far @ sweep()[0]["T_wc"])]
    live8 = []
    for i, f in enumerate(frames):
        T = A @ f["T_wc"]
        p = pr.points(f["depth"], f["intr_mat"], T)
        nv, U, h = pr.count(p, dims, voxel)
        ip = torch.from_numpy(O.depth_to_input_pts(f["depth"].astype(np.float64) / 1000.0, f["intr_mat"], T, 3.0))
        ip = ip.float()[None]
        assert np.array_equal(ip[0, :, :3].numpy(), p)                  # the restated points are the front end's
        for min_pts in (5, 8):
            out = O.encode_pointcloud(sd, ip, n_xyz, torch.from_numpy(mn).float(), torch.from_numpy(mx).float(), voxel,
                                      min_pts)
            if i == 3:
                assert nv == 0 and U == 0 and out[0] is None
                continue
            assert nv == len(p)
            assert np.float32(out[4].item()).tobytes() == pr.n_avg_pts(nv, U).tobytes()
            assert out[2].shape[0] == pr.live(h, min_pts)
            # the histogram is that of the voxels' pair counts
            _, _, cnt = pr.voxel_counts(p, dims, voxel)
            assert h.sum() == U == len(cnt) and (h * np.arange(65))[:64].sum() + cnt[cnt >= 64].sum() == 8 * nv
        if i < 3:
            live8.append(pr.live(h, 8))
    if voxel == 0.04:
        assert live8 == [2098, 2574, 1840]                              # the figures of the issue's prototype


# ---- properties of the restatement -----------------------------------------------------------------------------------

def test_room_figures():
    plan = sweep_plan()
    assert plan["n_points"] == 111612 and plan["n_frames"] == 24 and plan["n_skipped"] == 0
    assert np.allclose(plan["bounds"], [[-1.81, 1.82], [-0.63, 0.63], [-1.19, 1.19]], atol=1e-9)
    assert np.allclose(plan["dimensions"], [3.73, 1.36, 2.48], atol=1e-9)
    assert plan["yaw_deg"] == 0.0 and np.array_equal(plan["axis_align_mat"][:3, :3], np.eye(3))
    want = {0.02: (1.32, 2.46, 0.011), 0.04: (3.01, 9.16, 0.351), 0.08: (8.51, 31.19, 0.719)}
    for c in plan["candidates"]:
        mn, mean, lf = want[c["voxel_size"]]
        assert (round(c["min"], 2), round(c["mean"], 2), round(c["live_fraction"], 3)) == (mn, mean, lf)
        # trim 0 and margin >= one bin: every valid point is in bounds at every candidate
        assert sum(r[0] for r in c["rows"]) == plan["n_points"]
        assert len(c["n_avg_pts"]) == 24 and c["n_avg_pts"].dtype == np.float32
    assert plan["voxel_size"] == 0.08
    assert [c["ok"] for c in plan["candidates"]] == [False, False, True]


def test_trim_moves_the_room_bounds_little():
    plan = sweep_plan()
    for a in range(3):
        lo, hi = pr.bounds(plan["hist"][a], 1e-3, 0.01)
        assert 0 <= lo - plan["bounds"][a, 0] <= 0.10 + 1e-9 and 0 <= plan["bounds"][a, 1] - hi <= 0.10 + 1e-9


def test_trimmed_bounds_ignore_planted_outliers():
    rng = np.random.default_rng(1)
    clean = rng.uniform(-1.0, 1.0, (5000, 3)).astype(np.float32)
    dirs = pr.directions()
    ref = pr.extent_hist(clean, dirs, 0.01, 4096)
    for k in (1, 7):
        out = np.concatenate([clean, np.full((k, 3), 9.0, np.float32) + rng.uniform(0, 1, (k, 3)).astype(np.float32),
                              np.full((k, 3), -9.0, np.float32) - rng.uniform(0, 1, (k, 3)).astype(np.float32)])
        h = pr.extent_hist(out, dirs, 0.01, 4096)
        trim = (k + 0.5) / len(out)
        for a in range(3):
            assert pr.bounds(h[a], trim, 0.01) == pr.bounds(ref[a], 0.0, 0.01)
            assert pr.bounds(h[a], 0.0, 0.01) != pr.bounds(ref[a], 0.0, 0.01)
        # one outlier more than the trim allows moves the bound
        assert pr.bounds(h[0], (k - 0.5) / len(out), 0.01) != pr.bounds(ref[0], 0.0, 0.01)


def test_bounds_translate_with_the_scene():
    """Coordinates on a 2^-10 lattice, bins of 2^-6: a shift by 8 bins is exact in float32 and moves every count by 8
    bins, so the bounds move by exactly 0.125."""
    rng = np.random.default_rng(2)
    p = (rng.integers(-1500, 1500, (4000, 3)) / 1024.0).astype(np.float32)
    dirs, b = pr.directions(), 2.0 ** -6
    h0 = pr.extent_hist(p, dirs, b, 1024)
    h1 = pr.extent_hist(p + np.float32(0.125), dirs, b, 1024)
    assert np.array_equal(h1[:, 8:], h0[:, :-8]) and not h1[:, :8].any()
    for a in range(3):
        lo0, hi0 = pr.bounds(h0[a], 0.0, b)
        assert pr.bounds(h1[a], 0.0, b) == (lo0 + 0.125, hi0 + 0.125)
        lo0, hi0 = pr.bounds(h0[a], 0.01, b)
        assert pr.bounds(h1[a], 0.01, b) == (lo0 + 0.125, hi0 + 0.125)


def test_overflow_bins_refuse_a_plan():
    p = np.array([[0.0, 0.0, 0.0], [100.0, 0.0, 0.0]], np.float32)
    h = pr.extent_hist(p, pr.directions(), 0.01, 1024)
    assert h[0, 1023] == 1 and h[0, 512] == 1
    with pytest.raises(ValueError):
        pr.bounds(h[0], 0.0, 0.01)
    assert pr.bounds(h[1], 0.0, 0.01) == (0.0, 0.01)
    # a point that overflowed float32: +-inf goes to the overflow bin of its side, NaN (0 * inf along the other axes) to bin 0
    h = pr.extent_hist(np.array([[np.inf, 0.0, 0.0]], np.float32), pr.directions(), 0.01, 1024)
    assert h[0, 1023] == 1 and h[1, 0] == 1 and h[2, 0] == 1 and h.sum() == 3
    h = pr.extent_hist(np.array([[0.0, -np.inf, np.nan]], np.float32), pr.directions(), 0.01, 1024)
    assert h[:, 0].tolist() == [1, 1, 1] and h.sum() == 3


def test_yaw_of_the_rotated_room():
    frames = rotated(sweep())
    dirs = pr.directions(18, "y")
    assert len(dirs) == 39
    hist = np.zeros((39, 32768), np.int64)
    for f in frames:
        hist += pr.extent_hist(pr.points(f["depth"], f["intr_mat"], f["T_wc"]), dirs, 0.01, 32768)
    assert pr.choose_yaw(hist, 18, 0.0, 0.01) == 6
    al = pr.alignment(hist, 0.01, 0.0, 0.05, 18, "y")
    assert al["yaw_deg"] == 30.0
    R = al["R"]
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.allclose(R @ R.T, np.eye(3), atol=1e-12)

    def area(j):
        (la, ha), (lb, hb) = pr.bounds(hist[3 + 2 * j], 0.0, 0.01), pr.bounds(hist[4 + 2 * j], 0.0, 0.01)
        return (ha - la) * (hb - lb)

    assert abs(area(6) - 8.60) < 0.0051 and abs(area(0) - 16.56) < 0.0051      # (m^2, the prototype's two decimals)
    # the aligned room is the unrotated one up to bins: its dimensions, and fewer voxels than without yaw
    assert np.allclose(al["dimensions"], sweep_plan()["dimensions"], atol=0.021)
    plain = pr.alignment(hist, 0.01, 0.0, 0.05)
    assert pr.n_voxels(al["dimensions"], 0.04) < pr.n_voxels(plain["dimensions"], 0.04)
    # every point of every aligned frame lies inside the aligned bounds
    for f in frames[::6]:
        p = pr.points(f["depth"], f["intr_mat"], al["axis_align_mat"] @ f["T_wc"]).astype(np.float64)
        half = al["dimensions"] / 2 - 0.05 + 1e-6
        assert (np.abs(p) <= half).all()


@pytest.mark.parametrize("up", ["x", "y", "z"])
def test_yaw_directions(up):
    i1, i2 = pr.plane_axes(up)
    assert (i1, i2) == {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[up]
    d = pr.yaw_dirs(4, up)
    assert len(d) == 8 and np.array_equal(d[0], np.eye(3)[i1]) and np.array_equal(d[1], np.eye(3)[i2])
    for a, b in zip(d[::2], d[1::2]):
        assert a[pr.AXES[up]] == 0 and b[pr.AXES[up]] == 0
        R = np.zeros((3, 3))
        R[i1], R[i2], R[pr.AXES[up]] = a, b, np.eye(3)[pr.AXES[up]]
        assert abs(np.linalg.det(R) - 1.0) < 1e-12


def test_recommendation_rule():
    def cand(v, mn, mean, fits=True):
        return {"voxel_size": v, "ok": bool(fits and mn > 4 and mean >= 8)}
    assert pr.recommend([cand(0.02, 1, 2), cand(0.04, 4.5, 9), cand(0.08, 9, 30)]) == 0.04
    assert pr.recommend([cand(0.08, 9, 30), cand(0.04, 4.5, 9)]) == 0.04           # the smallest, not the first
    assert pr.recommend([cand(0.04, 4.0, 9)]) is None                               # min > 4 is strict
    assert pr.recommend([cand(0.04, 4.5, 8.0)]) == 0.04                             # mean >= 8 is not
    assert pr.recommend([cand(0.04, 4.5, 7.99)]) is None
    assert pr.recommend([cand(0.001, 9, 30, fits=False)]) is None
    assert pr.plan(sweep()[:4], voxel_sizes=(0.02,))["voxel_size"] is None


def test_a_grid_of_2_31_voxels_does_not_fit():
    plan = pr.plan(sweep()[:2], voxel_sizes=(0.0005, 0.08))
    big, ok = plan["candidates"]
    assert big["n_voxels"] >= 2 ** 31 and not big["fits"] and not big["ok"] and big["rows"] == []
    assert ok["fits"] and len(ok["rows"]) == 2
    assert plan["voxel_size"] in (None, 0.08)


def test_non_finite_poses_are_skipped():
    frames = list(sweep()[:3])
    bad = dict(frames[1], T_wc=np.full((4, 4), np.nan))
    a = pr.plan([frames[0], bad, frames[2]], voxel_sizes=(0.08,))
    b = pr.plan([frames[0], frames[2]], voxel_sizes=(0.08,))
    assert a["n_skipped"] == 1 and a["n_frames"] == 2 and np.array_equal(a["hist"], b["hist"])
    assert a["candidates"][0]["n_avg_pts"].tobytes() == b["candidates"][0]["n_avg_pts"].tobytes()


def test_confidence_gate():
    f = sweep()[0]
    conf = np.full((H, W), 2, np.uint8)
    conf[:, : W // 2] = 1
    full = pr.points(f["depth"], f["intr_mat"], f["T_wc"])
    half = pr.points(f["depth"], f["intr_mat"], f["T_wc"], conf=conf, conf_level=2)
    assert 0 < len(half) < len(full)
    assert len(pr.points(f["depth"], f["intr_mat"], f["T_wc"], conf=conf, conf_level=1)) == len(full)


# ---- the host side of the package ------------------------------------------------------------------------------------

def test_stats_share_the_volumes_bookkeeping():
    from bnv_fusion_amd import plan as P
    from bnv_fusion_amd import sparse_volume as sv
    rng = np.random.default_rng(3)
    vals = rng.uniform(1, 40, 57).astype(np.float32)
    got, ref = P._stats(vals), pr.stats(vals)
    assert got == {k: ref[k] for k in got}
    # SparseVolume.track_n_pts is the same function, applied per frame
    avg, n, mn, mx = 0, 0, 1000, 0
    for v in vals:
        avg, n, mn, mx = sv.track_n_pts_update(avg, n, mn, mx, float(v))
    assert (avg, mn, mx) == (ref["mean"], ref["min"], ref["max"])
    assert P._stats([]) == {"mean": 0, "min": 1000, "max": 0, "p25": 0, "p50": 0, "p75": 0}


def _host_plan(al):
    from bnv_fusion_amd.plan import VolumePlan
    return VolumePlan(center=al["center"], dimensions=al["dimensions"], axis_align_mat=al["axis_align_mat"],
                      yaw_deg=al["yaw_deg"], bounds=al["bounds"], n_points=0, n_frames=0, n_skipped=0, candidates=[],
                      voxel_size=None)


def test_apply_and_apply_points_agree():
    """An aligned frame's points equal the aligned points of the original frame to float32 rounding: both are one
    float32 rounding (half an ulp of a coordinate below 8 m, 2^-22) away from the same float64 point, the second after
    a rotation that spreads the first's error over the axes: 2 * sqrt(3) * 2^-22 < 1e-6."""
    frames = rotated(sweep())[:3]
    dirs = pr.directions(18, "y")
    hist = sum(pr.extent_hist(pr.points(f["depth"], f["intr_mat"], f["T_wc"]), dirs, 0.01, 32768) for f in frames)
    plan = _host_plan(pr.alignment(hist, 0.01, 0.0, 0.05, 18, "y"))
    assert plan.yaw_deg != 0.0
    for f in frames:
        g = plan.apply(f)
        assert g is not f and g["depth"] is f["depth"] and np.array_equal(g["T_wc"], plan.axis_align_mat @ f["T_wc"])
        a = pr.points(g["depth"], g["intr_mat"], g["T_wc"]).astype(np.float64)
        b = plan.apply_points(pr.points(f["depth"], f["intr_mat"], f["T_wc"]))
        assert np.array_equal(b, pr.apply_points(plan.axis_align_mat, pr.points(f["depth"], f["intr_mat"], f["T_wc"])))
        assert np.abs(a - b).max() < 1e-6
    with pytest.raises(ValueError):
        plan.apply({"input_pts": np.zeros((1, 4, 6), np.float32), "T_wc": np.eye(4)})


def test_planner_and_dataset_arguments():
    from bnv_fusion_amd import VolumePlanner, datasets
    for kw in ({"up": "w"}, {"align_yaw": 0}, {"align_yaw": 31}, {"n_bins": 1000}, {"n_bins": 131072},
               {"bin_size": 0.0}, {"bin_size": float("nan")}, {"trim": -0.1}, {"trim": 0.5},
               {"margin": 0.005}, {"margin": 0.01, "bin_size": 0.02}):
        with pytest.raises(ValueError):
            VolumePlanner(**kw)
    p = VolumePlanner(align_yaw=18, up="y")
    assert len(p.dirs) == 39 and all(np.array_equal(a, b) for a, b in zip(p.dirs, pr.directions(18, "y")))
    with pytest.raises(ValueError):
        datasets.ARKitDataset("/nonexistent", "scan", volume="guess")
    with pytest.raises(ValueError):
        datasets.FusionInferenceDataset("/nonexistent", "scan", volume="guess")
