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

With ``align="manhattan"`` a pass 0 (``VolumePlanner.add_normals`` / ``manhattan``) comes first, for worlds whose axes
are not the room's: a histogram of per-pixel normals on a cube map, from which the host finds the scene's three dominant
orthogonal plane directions and which of them is down (``ManhattanFrame``); ``axis_align_mat``'s rotation is that frame.

    plan = plan_volume(frames, align="manhattan")        # frames in the first camera's frame, say

tests/plan_restatement.py and tests/manhattan_restatement.py are the definition in numpy.  GPU only: there is no CPU
fallback.
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
    manhattan: object = None   # the ManhattanFrame whose rotation axis_align_mat carries (align="manhattan"), or None


@dataclasses.dataclass
class ManhattanFrame:
    """Result of pass 0: the scene's three dominant orthogonal plane directions.  ``R`` [3, 3]: its rows are the frame's
    x, y (down, the datasets' convention) and z axes in the world, so ``R @ p`` is a world point in the frame;
    ``axis_mass`` [3]: the share of all normals within ``cone`` degrees of +-x, +-y, +-z; ``confidence``: their sum."""
    R: np.ndarray
    confidence: float
    axis_mass: np.ndarray
    n_normals: int
    n_frames: int


NORMAL_SCALE = 2.0 ** 20   # fixed point of the normal sums (csrc/plan.hip: kPlanNormalScale)
_N_FIRST, _N_ANGLES, _N_ROUNDS = 16, 45, 5


def _dot(v, a):
    """v [..., 3] against ONE vector a [3], in a fixed order of operations."""
    return (v[..., 0] * a[0] + v[..., 1] * a[1]) + v[..., 2] * a[2]


def _bin_centres(n_side):
    """float64 [6 n_side^2, 3]: the unit vector through the middle of every cube-map bin, in bin order."""
    q = (np.arange(n_side) + 0.5) * 2.0 / n_side - 1.0
    c = np.zeros((6, n_side, n_side, 3))
    for face in range(6):
        m = face // 2
        c[face, ..., m] = -1.0 if face & 1 else 1.0
        c[face, ..., (m + 1) % 3] = q[:, None]
        c[face, ..., (m + 2) % 3] = q[None, :]
    c = c.reshape(-1, 3)
    return c / np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])[:, None]


def _nearest_rotation(M):
    U, _, Vt = np.linalg.svd(M)
    return U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt


def manhattan_from_histogram(hist, n_side, cone=10.0, min_confidence=0.3, down=(0.0, 1.0, 0.0), view=(0.0, 0.0, 1.0),
                             n_frames=0):
    """The ``ManhattanFrame`` of a normal histogram (int64 [6 n_side^2, 4] of bnv_plan_normals), float64 on the
    integers alone.  Coarse: each of the 16 fullest bins as the first axis, 45 angles in [0, 90) degrees about it, scored
    by the count in bins whose centre lies within ``cone`` degrees of a signed axis (the earlier candidate wins a tie).
    Five rounds of refinement: every axis becomes the sign-folded sum of the fixed-point normal sums of its cone's bins
    -- the sums, not the centres: no half-bin bias -- and the three, each weighted by the count in its cone (an axis that
    a few stray normals define must not turn the other two), are projected to the nearest rotation by SVD.  ``down`` (the
    mean camera down) names +y, ``view`` (the first frame's viewing direction) picks +z among the horizontal axes."""
    hist = np.asarray(hist, dtype=np.int64)
    count, sums = hist[:, 0], hist[:, 1:].astype(np.float64)
    total = int(count.sum())
    refuse = ("a Manhattan frame is not defined for this scene: plan it with a known up axis (up=, align_yaw=) "
              "instead of align=\"manhattan\"")
    if total == 0:
        raise _lib.BnvError(f"volume planning: no pixel gave a normal (0 normals in {n_frames} frames); {refuse}")
    centres, cos_cone = _bin_centres(n_side), math.cos(math.radians(cone))
    axes, best = None, -1
    for b in np.argsort(-count, kind="stable")[:_N_FIRST]:
        if count[b] == 0:
            break
        a = centres[b]
        e = np.zeros(3)
        e[int(np.argmin(np.abs(a)))] = 1.0
        p = np.cross(a, e)
        p = p / np.sqrt(_dot(p, p))
        q = np.cross(a, p)
        in_a = np.abs(_dot(centres, a)) >= cos_cone
        for j in range(_N_ANGLES):
            th = j * (math.pi / 2) / _N_ANGLES
            s = math.cos(th) * p + math.sin(th) * q
            t = np.cross(a, s)
            score = int(count[in_a | (np.abs(_dot(centres, s)) >= cos_cone) | (np.abs(_dot(centres, t)) >= cos_cone)].sum())
            if score > best:
                axes, best = np.stack([a, s, t]), score
    for _ in range(_N_ROUNDS):
        rows = []
        for ax in axes:
            d = _dot(centres, ax)
            inside = np.abs(d) >= cos_cone
            v = (np.where(d[inside] < 0.0, -1.0, 1.0)[:, None] * sums[inside]).sum(axis=0)
            n = math.sqrt(float(_dot(v, v)))
            rows.append(float(count[inside].sum()) * (v / n if n > 0.0 else ax))
        axes = _nearest_rotation(np.stack(rows))
    mass = np.array([int(count[np.abs(_dot(centres, ax)) >= cos_cone].sum()) for ax in axes]) / total
    confidence = float(mass.sum())
    if int((mass > 0).sum()) < 2:
        raise _lib.BnvError(f"volume planning: {int((mass > 0).sum())} axis carries normals (axis mass "
                            f"{mass.round(3).tolist()} of {total} normals), two are needed; {refuse}")
    if confidence < min_confidence:
        raise _lib.BnvError(f"volume planning: confidence {confidence:.3f} < min_confidence {min_confidence:g} (the "
                            f"share of {total} normals within {cone:g} degrees of an axis; normals spread evenly "
                            f"give 0.046); {refuse}")

    def closest(v, among):
        v = np.asarray(v, dtype=np.float64)
        dots = [sg * float(_dot(axes[i], v)) for i, sg in among]
        return among[int(np.argmax(dots))]          # (ties: the first)

    signed = [(i, sg) for i in range(3) for sg in (1.0, -1.0)]
    iy, sy = closest(down, signed)
    iz, sz = closest(view, [c for c in signed if c[0] != iy])
    y, z = sy * axes[iy], sz * axes[iz]
    return ManhattanFrame(R=np.stack([np.cross(y, z), y, z]), confidence=confidence,
                          axis_mass=mass[[3 - iy - iz, iy, iz]], n_normals=total, n_frames=int(n_frames))


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
    manhattan: object = None   # the ManhattanFrame of align="manhattan" (axis_align_mat's rotation is its R), or None

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
                 f"dimensions {d[0]:.2f} x {d[1]:.2f} x {d[2]:.2f} m, yaw {self.yaw_deg:g} deg"]
        if self.manhattan is not None:
            m = self.manhattan
            lines.append(f"manhattan frame: confidence {m.confidence:.3f} (x {m.axis_mass[0]:.3f}, y {m.axis_mass[1]:.3f}, "
                         f"z {m.axis_mass[2]:.3f}) of {m.n_normals} normals in {m.n_frames} frames")
            lines += [f"  {a} = ({r[0]:+.6f}, {r[1]:+.6f}, {r[2]:+.6f})" for a, r in zip("xyz", m.R)]
        lines += [f"{'voxel':>8} {'grid':>18} {'min':>7} {'mean':>7} {'p50':>7} {'max':>7} {'live':>6}  ok"]
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
    ``align_yaw=K`` (1..30): also try K yaw angles in [0, 90) degrees about ``up`` and keep the smallest footprint.

    ``align="manhattan"``: for a world whose axes are not the room's (a first camera's frame, a capture's arbitrary
    one).  A pass 0 comes first -- ``add_normals(frame)`` per frame, then ``manhattan()`` -- which finds the scene's
    three dominant orthogonal plane directions and which of them is down, from a histogram of per-pixel normals
    (central differences over ``normal_step`` pixels, None: max(1, W // 80); neighbours further than ``jump`` * z away
    in depth do not count; a cube map of ``n_side`` x ``n_side`` bins a face).  Pass 1 then runs along the frame's three
    axes and ``axis_align_mat``'s rotation is the frame: no ``up``, no yaw search.  A scene with less than
    ``min_confidence`` of its normals within ``cone`` degrees of the axes, or with fewer than two axes, is refused.
    ``down_hint``: a world vector that points roughly down, instead of the mean of the cameras' down axes."""

    def __init__(self, device="cuda:0", max_depth=3.0, bin_size=0.01, n_bins=32768, trim=0.0, margin=0.05,
                 align_yaw=None, up="y", align=None, normal_step=None, jump=0.1, n_side=32, cone=10.0,
                 min_confidence=0.3, down_hint=None):
        if up not in _AXES:
            raise ValueError(f"up {up!r}: 'x', 'y' or 'z'")
        if align_yaw is not None and not 1 <= int(align_yaw) <= 30:
            raise ValueError(f"align_yaw {align_yaw}: None or 1 .. 30")
        if align not in (None, "manhattan"):
            raise ValueError(f"align {align!r}: None or 'manhattan'")
        if align is not None and align_yaw is not None:
            raise ValueError("align='manhattan' finds the whole rotation: it does not go together with align_yaw")
        if normal_step is not None and not 1 <= int(normal_step) <= 64:
            raise ValueError(f"normal_step {normal_step}: None or 1 .. 64")
        if not (math.isfinite(jump) and jump > 0):
            raise ValueError(f"jump {jump}: positive and finite")
        if not 4 <= int(n_side) <= 64:
            raise ValueError(f"n_side {n_side}: 4 .. 64")
        if not 0.0 < cone < 45.0:
            raise ValueError(f"cone {cone}: in (0, 45) degrees")
        if not 0.0 <= min_confidence <= 1.0:
            raise ValueError(f"min_confidence {min_confidence}: in [0, 1]")
        if down_hint is not None:
            down_hint = np.asarray(down_hint, dtype=np.float64)
            if down_hint.shape != (3,) or not np.isfinite(down_hint).all() or not down_hint.any():
                raise ValueError(f"down_hint {down_hint}: a finite non-zero 3-vector")
        self.align, self.normal_step = align, None if normal_step is None else int(normal_step)
        self.jump, self.n_side, self.cone = float(jump), int(n_side), float(cone)
        self.min_confidence, self.down_hint = float(min_confidence), down_hint
        self._normal_hist = None
        self._frame = None
        self._down_sum = np.zeros(3)
        self._view = None
        self.n_normal_frames = 0
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

    # ---- pass 0 ----------------------------------------------------------------------------------------------------
    def add_normals(self, frame):
        """Adds one frame's normals to the normal histogram (``align="manhattan"``); False for a frame whose pose is not
        finite (left out here, skipped and counted by ``add``)."""
        if self.align != "manhattan":
            raise ValueError("add_normals: the planner was made without align='manhattan'")
        if self._hist is not None:
            raise _lib.BnvError("VolumePlanner.add_normals: pass 1 has begun along the frame found so far")
        if not _pose_ok(frame):
            return False
        lib = self._library()
        with torch.cuda.device(self._dev):
            if self._normal_hist is None:
                self._normal_hist = torch.zeros((6 * self.n_side * self.n_side, 4), dtype=torch.int64, device=self._dev)
            d, c, args = self._frame_args(frame, frame["T_wc"], "VolumePlanner.add_normals")
            step = self.normal_step or max(1, int(d.shape[1]) // 80)
            _lib.check(lib.bnv_plan_normals(*args, min(step, 64), self.jump, self.n_side, _lib.ptr(self._normal_hist),
                                            _lib.stream_ptr()), "bnv_plan_normals")
        R = np.asarray(frame["T_wc"], dtype=np.float64)[:3, :3]
        self._down_sum = self._down_sum + R[:, 1]
        if self._view is None:
            self._view = R[:, 2].copy()
        self.n_normal_frames += 1
        self._frame = None
        return True

    def normal_histogram(self):
        """int64 [6 n_side^2, 4] on the host (the one read of pass 0): per cube-map bin the number of normals and the
        sums of their components in 2^-20 fixed point."""
        if self._normal_hist is None:
            return np.zeros((6 * self.n_side * self.n_side, 4), np.int64)
        return self._normal_hist.cpu().numpy()

    def manhattan(self):
        """The ``ManhattanFrame`` of the frames added with ``add_normals``; pass 1 then runs along its axes.  BnvError
        when the scene has none (``manhattan_from_histogram``)."""
        if self.align != "manhattan":
            raise ValueError("manhattan: the planner was made without align='manhattan'")
        if self._frame is None:
            self._frame = manhattan_from_histogram(
                self.normal_histogram(), self.n_side, self.cone, self.min_confidence,
                self._down_sum if self.down_hint is None else self.down_hint,
                (0.0, 0.0, 1.0) if self._view is None else self._view, self.n_normal_frames)
            self.dirs = [np.array(r, np.float64) for r in self._frame.R]
            self._dirs_c = (C.c_double * 9)(*np.concatenate(self.dirs))
        return self._frame

    # ---- pass 1 ----------------------------------------------------------------------------------------------------
    def add(self, frame):
        """Adds one frame's points to the extent histograms; False for a frame whose pose is not finite (skipped and
        counted, as the reference's loader skips it)."""
        if not _pose_ok(frame):
            self.n_skipped += 1
            return False
        if self.align == "manhattan":
            self.manhattan()      # (pass 1 counts along the frame's axes)
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
        if self.align == "manhattan":
            R = self.manhattan().R      # (the three histograms were counted along its rows)
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
                              n_frames=self.n_frames, n_skipped=self.n_skipped, hist=hist, manhattan=self._frame)
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
    Keyword arguments: those of ``VolumePlanner``; with ``align="manhattan"`` a pass 0 over the frames comes first."""
    planner = VolumePlanner(**kw)
    if planner.align == "manhattan":
        for f in frames:
            planner.add_normals(f)
        planner.manhattan()
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
                      voxel_size=min(ok) if ok else None, min_pts_in_grid=int(min_pts_in_grid),
                      manhattan=getattr(extent, "manhattan", None))
