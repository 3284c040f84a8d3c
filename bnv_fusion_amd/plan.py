"""Planning the fusion volume from the frames themselves: bounds, yaw and voxel size (csrc/plan.hip;
include/bnv_fusion.h, "Volume planning").

``NeuralMap(dimensions, voxel_size, ...)`` needs the scene's extent and a voxel size before the first frame is fused.
The reference takes the extent from a rough mesh of the scene and leaves the voxel size to a full trial run
(``print_statistic``: "min > 4 and mean >= 8 points per voxel").  ``plan_volume`` answers both from the depth frames and
poses alone, in two passes on the GPU and without evaluating any network:

* pass 1 (``VolumePlanner.add`` / ``extent``): histograms of the frames' world points along the axes -- and, with
  ``align_yaw=K``, along 2 K rotated directions -- give the (optionally trimmed) bounds, the centre, and the yaw about
  ``up`` whose footprint is smallest;
* pass 2 (``VolumePlanner.count``): for several candidate voxel sizes at once, the per-frame statistics
  ``SparseVolume.print_statistic`` would print after fusing the aligned frames into a volume of the planned dimensions
  -- the per-frame ``n_avg_pts`` to the bit, and the number of voxels each frame's encode would return.

    plan = plan_volume(frames, voxel_sizes=(0.02, 0.04, 0.08))
    print(plan.table())
    nm = NeuralMap(plan.dimensions, plan.voxel_size, model)
    for f in frames:
        nm.integrate(plan.apply(f))

tests/plan_restatement.py is the definition in numpy.  GPU only: there is no CPU fallback.
"""
import ctypes as C
import dataclasses
import math

import numpy as np
import torch

from . import _lib
from .frontend import DEPTH_DTYPES, conf_arg
from .sparse_volume import get_world_range, make_grid, n_pts_percentiles, track_n_pts_update

MAX_DIRS = 64          # BNV_PLAN_MAX_DIRS
MAX_SIZES = 8          # BNV_PLAN_MAX_SIZES
ROW_WORDS = 72         # BNV_PLAN_ROW_WORDS
HIST_CAP = 64          # BNV_PLAN_HIST_CAP
_AXES = {"x": 0, "y": 1, "z": 2}
_ROWS_PER_BLOCK = 256  # frames whose rows share one device allocation


def _plane_axes(up):
    u = _AXES[up]
    return (u + 1) % 3, (u + 2) % 3      # (e1, e2) = (y, z), (z, x), (x, y) for up = x, y, z


def _yaw_dirs(K, up):
    i1, i2 = _plane_axes(up)
    e1, e2 = np.eye(3)[i1], np.eye(3)[i2]
    out = []
    for j in range(K):
        th = j * (np.pi / 2) / K
        c, s = np.cos(th), np.sin(th)
        out += [c * e1 + s * e2, -s * e1 + c * e2]
    return out


def _bounds(h, trim, bin_size, what):
    """(lo, hi) in metres along one direction: the first / last bin whose inclusive prefix / suffix sum exceeds
    floor(trim * N), rounded outward to bins."""
    n = len(h)
    total = int(h.sum())
    if total == 0:
        raise _lib.BnvError("volume planning: no valid depth pixel in any frame")
    k = int(math.floor(trim * total))
    lo = int(np.argmax(np.cumsum(h) > k))
    hi = n - 1 - int(np.argmax(np.cumsum(h[::-1]) > k))
    if lo == 0 or hi == n - 1:
        raise _lib.BnvError(
            f"volume planning: the bounds along {what} touch an overflow bin of the extent histogram "
            f"(+-{n // 2 * bin_size:g} m around the origin): raise n_bins or bin_size, or trim outliers (trim > 0)")
    return (lo - n // 2) * bin_size, (hi + 1 - n // 2) * bin_size


@dataclasses.dataclass
class Extent:
    """Result of pass 1.  ``bounds`` [3, 2] and ``center`` are in the ALIGNED frame (axis_align_mat's rotation applied,
    its translation not)."""
    center: np.ndarray
    dimensions: np.ndarray
    axis_align_mat: np.ndarray
    yaw_deg: float
    bounds: np.ndarray
    n_points: int
    n_frames: int
    n_skipped: int
    hist: np.ndarray


@dataclasses.dataclass
class Candidate:
    voxel_size: float
    n_xyz: list
    n_voxels: int
    fits: bool                 # fewer than 2^31 voxels: flat voxel ids are int32
    n_avg_pts: np.ndarray      # float32, per frame with at least one point in bounds, in frame order
    min: float
    max: float
    mean: float
    p25: float
    p50: float
    p75: float
    live_fraction: float       # sum of voxels with >= min_pts_in_grid pairs / sum of touched voxels, over the frames
    ok: bool                   # fits, min > 4 and mean >= 8
    rows: np.ndarray           # int64 [n_frames, 2 + HIST_CAP + 1]: nv, U, hist[0 .. HIST_CAP] per counted frame
    table_bytes: int           # device memory of this candidate's hash table

    def live(self, min_pts):
        """Per frame: the voxels its encode returns with ``min_pts_in_grid = min_pts`` (1 .. HIST_CAP)."""
        if not 1 <= int(min_pts) <= HIST_CAP:
            raise ValueError(f"min_pts {min_pts}: 1 .. {HIST_CAP}")
        return self.rows[:, 2 + int(min_pts):].sum(axis=1)


def _stats(n_list):
    """SparseVolume's bookkeeping on a list of per-frame n_avg_pts: the same arithmetic, hence the same roundings."""
    avg, n, mn, mx = 0, 0, 1000, 0
    for v in n_list:
        avg, n, mn, mx = track_n_pts_update(avg, n, mn, mx, float(v))
    p = n_pts_percentiles([float(v) for v in n_list])
    return {"mean": avg, "min": mn, "max": mx, "p25": p[0], "p50": p[1], "p75": p[2]}


@dataclasses.dataclass
class VolumePlan:
    center: np.ndarray
    dimensions: np.ndarray
    axis_align_mat: np.ndarray
    yaw_deg: float
    bounds: np.ndarray
    n_points: int
    n_frames: int
    n_skipped: int
    candidates: list
    voxel_size: object         # the smallest candidate that is ``ok``, or None
    min_pts_in_grid: int = 8

    def apply(self, frame):
        """A shallow copy of the frame with ``T_wc = axis_align_mat @ T_wc`` (float64): the frame as the planned volume
        sees it.  A frame with ``input_pts`` is refused: the plan works from depth."""
        if "input_pts" in frame:
            raise ValueError("VolumePlan.apply: the frame carries input_pts, which are already in some world frame; "
                             "plan and fuse from depth frames")
        out = dict(frame)
        out["T_wc"] = self.axis_align_mat @ np.asarray(frame["T_wc"], dtype=np.float64)
        return out

    def apply_points(self, xyz):
        """World points [N, 3] (a ground-truth mesh's vertices) -> the planned volume's frame, float64."""
        x = np.asarray(xyz, dtype=np.float64)
        return x @ self.axis_align_mat[:3, :3].T + self.axis_align_mat[:3, 3]

    def candidate(self, voxel_size):
        for c in self.candidates:
            if c.voxel_size == voxel_size:
                return c
        raise KeyError(voxel_size)

    def table(self):
        d, b = self.dimensions, self.bounds
        lines = [f"frames {self.n_frames} (skipped {self.n_skipped}), valid points {self.n_points}",
                 "bounds  " + "  ".join(f"{a} [{b[i, 0]:.2f}, {b[i, 1]:.2f}]" for i, a in enumerate("xyz")),
                 f"dimensions {d[0]:.2f} x {d[1]:.2f} x {d[2]:.2f} m, yaw {self.yaw_deg:g} deg",
                 f"{'voxel':>8} {'grid':>18} {'min':>7} {'mean':>7} {'p50':>7} {'max':>7} {'live':>6}  ok"]
        for c in self.candidates:
            grid = "x".join(str(n) for n in c.n_xyz)
            if not c.fits:
                lines.append(f"{c.voxel_size:>8g} {grid:>18}  does not fit: 2^31 voxels or more")
                continue
            lines.append(f"{c.voxel_size:>8g} {grid:>18} {c.min:>7.2f} {c.mean:>7.2f} {c.p50:>7.2f} {c.max:>7.2f} "
                         f"{c.live_fraction:>6.3f}  {'yes' if c.ok else 'no'}")
        lines.append(f"recommended voxel size: {self.voxel_size} (min > 4 and mean >= 8 points per voxel, "
                     f"live = voxels with >= {self.min_pts_in_grid} pairs)")
        return "\n".join(lines)


def _frame_image(frame, what):
    if "depth" not in frame or frame["depth"] is None:
        raise ValueError(f"{what}: the frame has no depth image (the plan works from depth, not from input_pts)")
    depth = frame["depth"]
    if not (torch.is_tensor(depth) and depth.is_cuda):
        raise _lib.BnvError(f"{what} runs on the GPU only: depth must be a device tensor (no CPU fallback)")
    if depth.dtype not in DEPTH_DTYPES:
        raise _lib.BnvError(f"{what}: depth must be uint16 millimetres or float32 / float64 metres, got {depth.dtype}")
    d = depth[0] if depth.dim() == 3 and depth.shape[0] == 1 else depth
    if d.dim() != 2 or d.numel() == 0:
        raise _lib.BnvError(f"{what}: expected a non-empty [H, W] image, got {tuple(depth.shape)}")
    return d.contiguous()


def _pose_ok(frame):
    return bool(np.isfinite(np.asarray(frame["T_wc"], dtype=np.float64)).all())


class VolumePlanner:
    """The two passes, for callers that stream frames or already have bounds.  ``add(frame)`` per frame, then
    ``extent()``; ``count(frames, voxel_sizes)`` for the statistics (with the extent of the added frames, or with
    ``dimensions`` / ``axis_align_mat`` the caller has).  ``trim``: the fraction of points ignored at each end of every
    direction (0: the exact extent, rounded outward to bins); ``margin``: added on every side, at least one bin;
    ``align_yaw=K`` (1..30): also try K yaw angles in [0, 90) degrees about ``up`` and keep the smallest footprint."""

    def __init__(self, device="cuda:0", max_depth=3.0, bin_size=0.01, n_bins=32768, trim=0.0, margin=0.05,
                 align_yaw=None, up="y"):
        if up not in _AXES:
            raise ValueError(f"up {up!r}: 'x', 'y' or 'z'")
        if align_yaw is not None and not 1 <= int(align_yaw) <= 30:
            raise ValueError(f"align_yaw {align_yaw}: None or 1 .. 30")
        if not (math.isfinite(bin_size) and bin_size > 0):
            raise ValueError(f"bin_size {bin_size}: positive and finite")
        if int(n_bins) < 2 or int(n_bins) > 65536 or int(n_bins) & (int(n_bins) - 1):
            raise ValueError(f"n_bins {n_bins}: a power of two up to 65536")
        if not 0.0 <= trim < 0.5:
            raise ValueError(f"trim {trim}: in [0, 0.5)")
        if not margin >= bin_size:
            raise ValueError(f"margin {margin}: at least one bin ({bin_size})")
        self._dev = torch.device(device)
        self.device = device
        self.max_depth, self.bin_size, self.n_bins = float(max_depth), float(bin_size), int(n_bins)
        self.trim, self.margin, self.up = float(trim), float(margin), up
        self.align_yaw = None if align_yaw is None else int(align_yaw)
        self.dirs = [np.array(e, np.float64) for e in np.eye(3)]
        if self.align_yaw:
            self.dirs += _yaw_dirs(self.align_yaw, up)
        self._dirs_c = (C.c_double * (3 * len(self.dirs)))(*np.concatenate(self.dirs))
        self._lib = None
        self._hist = None
        self._extent = None
        self.n_frames = 0
        self.n_skipped = 0
        self.table_slots = 0      # 0: a table that cannot pass half load; a power of two: forced (tests, small devices)

    def _library(self):
        if self._lib is None:
            self._lib = _lib.require_device(self._dev.index or 0)
        return self._lib

    def _frame_args(self, frame, T, what):
        d = _frame_image(frame, what)
        if d.device != self._dev:
            raise _lib.BnvError(f"{what}: depth is on {d.device}, the planner on {self._dev}")
        H, W = int(d.shape[0]), int(d.shape[1])
        c, c_ptr, level = conf_arg(frame.get("conf"), frame.get("conf_level", 0) if frame.get("conf") is not None else 0,
                                   (H, W), d.device, what)
        K = (C.c_double * 9)(*np.asarray(frame["intr_mat"], dtype=np.float64)[:3, :3].reshape(-1))
        Tc = (C.c_double * 16)(*np.asarray(T, dtype=np.float64).reshape(-1))
        return d, c, (_lib.ptr(d), DEPTH_DTYPES[d.dtype], H, W, K, Tc, self.max_depth, c_ptr, level)

    # ---- pass 1 ----------------------------------------------------------------------------------------------------
    def add(self, frame):
        """Adds one frame's points to the extent histograms; False for a frame whose pose is not finite (skipped and
        counted, as the reference's loader skips it)."""
        if not _pose_ok(frame):
            self.n_skipped += 1
            return False
        lib = self._library()
        with torch.cuda.device(self._dev):
            if self._hist is None:
                self._hist = torch.zeros((len(self.dirs), self.n_bins), dtype=torch.int64, device=self._dev)
            d, c, args = self._frame_args(frame, frame["T_wc"], "VolumePlanner.add")
            _lib.check(lib.bnv_plan_extent(*args, self._dirs_c, len(self.dirs), self.bin_size, self.n_bins,
                                           _lib.ptr(self._hist), _lib.stream_ptr()), "bnv_plan_extent")
        self.n_frames += 1
        self._extent = None
        return True

    def histograms(self):
        """int64 [n_dirs, n_bins] on the host (the one read of pass 1)."""
        if self._hist is None:
            return np.zeros((len(self.dirs), self.n_bins), np.int64)
        return self._hist.cpu().numpy()

    def extent(self):
        if self._extent is not None:
            return self._extent
        hist = self.histograms()
        names = ["x", "y", "z"]
        b = [_bounds(hist[a], self.trim, self.bin_size, names[a]) for a in range(3)]
        R, yaw_deg = np.eye(3), 0.0
        if self.align_yaw:
            K, best, area_best, bb = self.align_yaw, 0, None, None
            for j in range(K):
                ba = _bounds(hist[3 + 2 * j], self.trim, self.bin_size, f"yaw direction a_{j}")
                bq = _bounds(hist[4 + 2 * j], self.trim, self.bin_size, f"yaw direction b_{j}")
                area = (ba[1] - ba[0]) * (bq[1] - bq[0])
                if area_best is None or area < area_best:      # ties: the smallest j
                    best, area_best, bb = j, area, (ba, bq)
            i1, i2 = _plane_axes(self.up)
            R = np.zeros((3, 3))
            R[i1], R[i2], R[_AXES[self.up]] = self.dirs[3 + 2 * best], self.dirs[4 + 2 * best], np.eye(3)[_AXES[self.up]]
            b[i1], b[i2] = bb
            yaw_deg = best * 90.0 / K
        b = np.asarray(b, dtype=np.float64)
        center = (b[:, 0] + b[:, 1]) / 2
        rot, shift = np.eye(4), np.eye(4)
        rot[:3, :3] = R
        shift[:3, 3] = -center
        self._extent = Extent(center=center, dimensions=(b[:, 1] - b[:, 0]) + 2 * self.margin,
                              axis_align_mat=shift @ rot, yaw_deg=yaw_deg, bounds=b, n_points=int(hist[0].sum()),
                              n_frames=self.n_frames, n_skipped=self.n_skipped, hist=hist)
        return self._extent

    # ---- pass 2 ----------------------------------------------------------------------------------------------------
    def count(self, frames, voxel_sizes, min_pts_in_grid=8, dimensions=None, axis_align_mat=None):
        """Per candidate voxel size: the per-frame statistics of fusing ``frames`` (aligned by ``axis_align_mat``) into
        a volume of ``dimensions`` -- both default to ``extent()``'s.  -> [Candidate], in the order of ``voxel_sizes``."""
        voxel_sizes = [float(v) for v in voxel_sizes]
        if not voxel_sizes or any(not (math.isfinite(v) and v > 0) for v in voxel_sizes):
            raise ValueError(f"voxel_sizes {voxel_sizes}: positive and finite")
        if not 1 <= int(min_pts_in_grid) <= HIST_CAP:
            raise ValueError(f"min_pts_in_grid {min_pts_in_grid}: 1 .. {HIST_CAP}")
        if dimensions is None or axis_align_mat is None:
            ext = self.extent()
            dimensions = ext.dimensions if dimensions is None else dimensions
            axis_align_mat = ext.axis_align_mat if axis_align_mat is None else axis_align_mat
        dimensions = np.asarray(dimensions, dtype=np.float64)
        A = np.asarray(axis_align_mat, dtype=np.float64)
        info = []
        for v in voxel_sizes:
            mn, mx, n_xyz = get_world_range(dimensions, v)
            nvox = int(n_xyz[0]) * int(n_xyz[1]) * int(n_xyz[2])
            info.append((v, [int(n) for n in n_xyz], nvox, nvox < 2 ** 31,
                         make_grid(n_xyz, mn, mx, v, min_pts_in_grid) if nvox < 2 ** 31 else None))
        fit = [i for i in info if i[3]]
        rows = np.zeros((0, len(fit), ROW_WORDS), np.int64)
        table_bytes = [0] * len(fit)
        for s in range(0, len(fit), MAX_SIZES):
            part, tb = self._count_grids(frames, [i[4] for i in fit[s: s + MAX_SIZES]], A)
            table_bytes[s: s + MAX_SIZES] = tb
            rows = part if s == 0 else np.concatenate([rows, part], axis=1)
        out, k = [], 0
        for v, n_xyz, nvox, fits, _ in info:
            r = rows[:, k] if fits else np.zeros((0, ROW_WORDS), np.int64)
            if fits:
                if (r[:, 2] != 0).any():
                    f = int(np.argmax(r[:, 2] != 0))
                    raise _lib.BnvError(
                        f"bnv_plan_count: the hash table of voxel size {v:g} overflowed at frame {f} (status "
                        f"{int(r[f, 2])}: 1 = past half load, 2 = no free slot): {int(r[f, 1])} voxels in "
                        f"{self.table_slots} slots; use table_slots = 0 or a larger power of two")
                k += 1
            keep = r[r[:, 0] > 0]                       # frames without a point in bounds return before track_n_pts
            navg = (keep[:, 0] * 8).astype(np.float32) / keep[:, 1].astype(np.float32)
            st = _stats(navg)
            live = int(keep[:, 4 + int(min_pts_in_grid): 4 + HIST_CAP + 1].sum())
            total = int(keep[:, 1].sum())
            out.append(Candidate(
                voxel_size=v, n_xyz=n_xyz, n_voxels=nvox, fits=fits, n_avg_pts=navg, live_fraction=live / total if total else 0.0,
                ok=bool(fits and len(navg) and st["min"] > 4 and st["mean"] >= 8),
                rows=np.concatenate([r[:, :2], r[:, 4: 4 + HIST_CAP + 1]], axis=1),
                table_bytes=table_bytes[k - 1] if fits else 0, **st))
        return out

    def _count_grids(self, frames, grids, A):
        """rows int64 [n_frames, len(grids), ROW_WORDS] on the host (read once), frames with a non-finite pose left out."""
        lib = self._library()
        n = len(grids)
        garr = (_lib.Grid * n)(*grids)
        blocks, ws, ws_shape, used, table_bytes = [], None, None, 0, [0] * n
        with torch.cuda.device(self._dev):
            for frame in frames:
                if not _pose_ok(frame):
                    continue
                d, c, args = self._frame_args(frame, A @ np.asarray(frame["T_wc"], dtype=np.float64),
                                              "VolumePlanner.count")
                H, W = args[2], args[3]
                if ws_shape != (H, W):
                    nbytes = int(lib.bnv_plan_workspace_bytes(H, W, garr, n, self.table_slots))
                    if nbytes == 0:
                        raise _lib.BnvError(f"bnv_plan_workspace_bytes refused {H}x{W}, {n} grids, "
                                            f"table_slots {self.table_slots}")
                    ws = torch.empty(nbytes, dtype=torch.uint8, device=self._dev)
                    _lib.check(lib.bnv_plan_workspace_reset(_lib.ptr(ws), nbytes, H, W, garr, n, self.table_slots,
                                                            _lib.stream_ptr()), "bnv_plan_workspace_reset")
                    ws_shape = (H, W)
                    for s in range(n):
                        one = (_lib.Grid * 1)(grids[s])
                        table_bytes[s] = int(lib.bnv_plan_workspace_bytes(H, W, one, 1, self.table_slots))
                if not blocks or used == _ROWS_PER_BLOCK:
                    blocks.append(torch.zeros((_ROWS_PER_BLOCK, n, ROW_WORDS), dtype=torch.int64, device=self._dev))
                    used = 0
                _lib.check(lib.bnv_plan_count(*args, garr, n, self.table_slots, _lib.ptr(ws), ws.numel(),
                                              _lib.ptr(blocks[-1][used]), _lib.stream_ptr()), "bnv_plan_count")
                used += 1
            if not blocks:
                return np.zeros((0, n, ROW_WORDS), np.int64), table_bytes
            rows = torch.cat(blocks[:-1] + [blocks[-1][:used]]).cpu().numpy()
        return rows, table_bytes


def plan_volume(frames, voxel_sizes=(0.005, 0.01, 0.02, 0.04), min_pts_in_grid=8, **kw):
    """Two passes over a re-iterable frame source (a list or a dataset of depth frame dicts) -> ``VolumePlan``.
    Keyword arguments: those of ``VolumePlanner``."""
    planner = VolumePlanner(**kw)
    for f in frames:
        planner.add(f)
    return plan_from(planner.extent(), planner.count(frames, voxel_sizes, min_pts_in_grid=min_pts_in_grid),
                     min_pts_in_grid)


def plan_from(extent, candidates, min_pts_in_grid=8):
    """The ``VolumePlan`` of an ``Extent`` (pass 1; a dataset opened with ``volume="plan"`` carries one) and the
    candidates counted for it (``VolumePlanner.count``): the recommendation is the smallest candidate that is ``ok``."""
    ok = [c.voxel_size for c in candidates if c.ok]
    return VolumePlan(center=extent.center, dimensions=extent.dimensions, axis_align_mat=extent.axis_align_mat,
                      yaw_deg=extent.yaw_deg, bounds=extent.bounds, n_points=extent.n_points,
                      n_frames=extent.n_frames, n_skipped=extent.n_skipped, candidates=list(candidates),
                      voxel_size=min(ok) if ok else None, min_pts_in_grid=int(min_pts_in_grid))
