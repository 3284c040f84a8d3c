"""Timings of frame-to-frame RGB-D odometry (csrc/odometry.hip, bnv_fusion_amd/odometry.py) -> one JSON line per case.

    python tools/odometry_bench.py [--frames N] [--json OUT]

``prepare``: ms per ``prepare_frame`` of a 640 x 480 sweep frame with its colour image (three levels).  ``align``: ms
per ``rgbd_align`` of two such frames with the default schedule (20 iterations; includes its one host read), beside
``icp_align`` of the same frame against a 640 x 480 TSDF view in the same run (19 iterations).  ``accumulate``: ms per
level-0 iteration, that is one launch of k_rgbd_accumulate and one of the one-wave k_icp_solve, from an alignment of
200 level-0 iterations less one of 100, so that the call's set-up and host read cancel; k_icp_accumulate at stride 1,
with the same solve, likewise.  ``loop``: frames/s of ``Tracker(odometry="rgbd")`` (TSDF view, 160 x 120) beside the
tracker with given poses over the same frames.  HIP events, median of 5 after 2 warm-up calls.  For the time of each
kernel alone, in a run of its own:
rocprofv3 --kernel-trace --stats -- python tools/odometry_bench.py"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bnv_fusion_amd as bnv  # noqa: E402

bnv.configure_runtime()
from bnv_fusion_amd import odometry, scan, sequence, tracking  # noqa: E402

DEV = "cuda:0"
H, W = 480, 640


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def new_map():
    dims, voxel, _ = sequence.DIMS[256]
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)
    return bnv.NeuralMap(np.array([dims] * 3), voxel, model, device=DEV, tsdf=True)


def with_colour(frame, scale):
    """The sweep frame with the colour image of its clean depth."""
    K, T = frame["intr_mat"], frame["T_wc"]
    clean = sequence.render_depth(T, K, H, W, scale, device=DEV)
    clean = torch.where(torch.isfinite(clean), clean, torch.zeros_like(clean)).to(torch.float32)
    return dict(frame, rgb=scan.render_color(clean, K, T))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--json")
    args = ap.parse_args()
    scale = sequence.DIMS[256][2]
    ts = range(96, 96 + 2 * args.frames, 2)
    frames = [with_colour(fr, scale) for fr in sequence.sweep_frames(ts, scale=scale, device=DEV)]
    out = []
    mid = len(frames) // 2
    fa, fb = frames[mid], frames[mid + 1]
    T_true = tracking.rigid_inverse(fb["T_wc"]) @ fa["T_wc"]
    ref, cur = odometry.prepare_frame(fa), odometry.prepare_frame(fb)
    res = odometry.rgbd_align(ref, cur)
    out.append({"case": "prepare", "frame": [H, W], "levels": 3, "ms": timed(lambda: odometry.prepare_frame(fb))})
    out.append({"case": "align", "what": "rgbd_align", "frame": [H, W], "iterations": 20,
                "ms": timed(lambda: odometry.rgbd_align(ref, cur)), "status": tracking.STATUS_NAMES[res.status],
                "pairs": float(res.stats[-1, 0]),
                "translation_error_mm": 1e3 * float(np.linalg.norm(res.T_wc[:3, 3] - T_true[:3, 3]))})
    nm = new_map()
    for fr in frames:
        nm.integrate(fr)
    torch.cuda.synchronize()
    K = np.asarray(fb["intr_mat"], dtype=np.float64)[:3, :3]
    T0 = tracking.se3_exp([0.01, -0.01, 0.01, 0.02, -0.01, 0.015]) @ fb["T_wc"]
    Km, Tm = K.astype(np.float32).astype(np.float64), T0.astype(np.float32).astype(np.float64)
    view = nm.render_tsdf(Tm, Km, H, W)

    def icp(levels=tracking.DEFAULT_LEVELS):
        return tracking.icp_align(fb["depth"], K, view[0], view[1], Km, Tm, T0, levels=levels, max_depth=nm.max_depth)

    res = icp()
    out.append({"case": "align", "what": "icp_align", "frame": [H, W], "view": [H, W], "iterations": 19, "ms": timed(icp),
                "status": tracking.STATUS_NAMES[res.status], "pairs": float(res.stats[-1, 0])})
    for what, run in (("k_rgbd_accumulate + solve", lambda n: odometry.rgbd_align(ref, cur, schedule=((0, n),))),
                      ("k_icp_accumulate + solve", lambda n: icp(((1, n),)))):
        status = run(200).status                       # (a refused call stops early: its time would mean nothing)
        ms = (timed(lambda: run(200)) - timed(lambda: run(100))) / 100.0 if status == tracking.OK else None
        out.append({"case": "accumulate", "what": what, "pixels": H * W, "status": tracking.STATUS_NAMES[status],
                    "ms_per_iteration": ms})
    for name, kw in (("tracker, given poses", {}), ("tracker, rgbd odometry", {"odometry": "rgbd"})):
        tracker = tracking.Tracker(new_map(), source="tsdf", model_size=(120, 160), **kw)
        tracker.integrate(frames[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in frames[1:]:
            tracker.integrate(f)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out.append({"case": "loop", "what": name, "frames": len(frames) - 1, "frames_per_s": (len(frames) - 1) / dt,
                    "ms_per_frame": 1e3 * dt / (len(frames) - 1), "refused": int(tracker.failures)})
    for row in out:
        print(json.dumps(row))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
