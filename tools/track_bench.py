"""Timings of frame-to-model tracking (csrc/track.hip, bnv_fusion_amd/tracking.py) -> one JSON line per case.

    python tools/track_bench.py [--frames N] [--json OUT]

``align``: ms per ``icp_align`` of a 640 x 480 sweep frame (default schedule: 19 iterations) against a 640 x 480 and a
160 x 120 view of a 256^3 map of the half-size room, for the neural and the TSDF render, each figure split into the
render of the view and the alignment (the alignment includes its one host read).  ``loop``: frames/s of
``Tracker.integrate`` (TSDF view, 160 x 120) beside plain ``NeuralMap.integrate`` over the same frames.  HIP events,
median of 5 after 2 warm-up calls.  For a kernel breakdown, in a run of its own:
rocprofv3 --kernel-trace --stats -- python tools/track_bench.py"""
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
from bnv_fusion_amd import sequence, tracking  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--json")
    args = ap.parse_args()
    scale = sequence.DIMS[256][2]
    ts = range(96, 96 + 2 * args.frames, 2)
    frames = list(sequence.sweep_frames(ts, scale=scale, device=DEV))
    nm = new_map()
    for fr in frames:
        nm.integrate(fr)
    torch.cuda.synchronize()
    out = []
    fr = next(sequence.sweep_frames([ts[len(ts) // 2] + 1], scale=scale, device=DEV))
    K = np.asarray(fr["intr_mat"], dtype=np.float64)[:3, :3]
    T0 = tracking.se3_exp([0.01, -0.01, 0.01, 0.02, -0.01, 0.015]) @ fr["T_wc"]
    for source, render in (("neural", nm.render), ("tsdf", nm.render_tsdf)):
        for Hm, Wm in ((480, 640), (120, 160)):
            Km = tracking.scaled_intrinsics(K, W / Wm, H / Hm).astype(np.float32).astype(np.float64)
            Tm = T0.astype(np.float32).astype(np.float64)
            view = render(Tm, Km, Hm, Wm)
            res = tracking.icp_align(fr["depth"], K, view[0], view[1], Km, Tm, T0, max_depth=nm.max_depth)
            ms_render = timed(lambda: render(Tm, Km, Hm, Wm))
            ms_align = timed(lambda: tracking.icp_align(fr["depth"], K, view[0], view[1], Km, Tm, T0,
                                                        max_depth=nm.max_depth))
            dt = np.linalg.norm(res.T_wc[:3, 3] - fr["T_wc"][:3, 3])
            out.append({"case": "align", "source": source, "frame": [H, W], "view": [Hm, Wm], "iterations": 19,
                        "ms_render": ms_render, "ms_align": ms_align, "ms_total": ms_render + ms_align,
                        "status": tracking.STATUS_NAMES[res.status], "pairs": float(res.stats[-1, 0]),
                        "translation_error_mm": 1e3 * float(dt)})
    for name in ("integrate", "tracker"):
        m = new_map()
        step = m.integrate if name == "integrate" else tracking.Tracker(m, source="tsdf", model_size=(120, 160)).integrate
        step(frames[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in frames[1:]:
            step(f)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out.append({"case": "loop", "what": name, "frames": len(frames) - 1, "frames_per_s": (len(frames) - 1) / dt,
                    "ms_per_frame": 1e3 * dt / (len(frames) - 1)})
    for row in out:
        print(json.dumps(row))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
