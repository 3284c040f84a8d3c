"""The cost of volume planning (csrc/plan.hip; bnv_fusion_amd/plan.py) next to the fusion it precedes, one JSON line:

* pass 0 (VolumePlanner.add_normals, align="manhattan") with normal steps 1 and 8, frames/s, and the frame each finds
  (the sweep's world is the room's own, so the largest axis error is the frame's angle to the identity);
* pass 1 (VolumePlanner.add) with 3 and with 39 directions (align_yaw=18), frames/s;
* pass 2 (VolumePlanner.count) with 1 and with 4 candidate voxel sizes, frames/s, and the hash tables' device memory
  per candidate;
* for comparison in the same run: NeuralMap.integrate frames/s at 256^3 / 1 cm.

120 frames of the half-scale room sweep at 640 x 480, resident on the device; every figure is the median of 5 passes
over them, each timed with one pair of HIP events around the whole pass (host launch cost included: it is what a
caller sees), after one untimed pass.

    python tools/plan_bench.py [--frames N] [--out FILE]
"""
import argparse
import json
import math
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import bnv_fusion_amd as bnv  # noqa: E402
bnv.configure_runtime()      # the package's hardware queue count, before the first HIP call (streams.py)
from bnv_fusion_amd import sequence  # noqa: E402

DEV = "cuda:0"
SCALE = 0.5
REPEATS = 5
SIZES_4 = (0.005, 0.01, 0.02, 0.04)


def timed(fn, n_frames):
    fn()                                                      # warm-up: code objects, the allocator's pools
    torch.cuda.synchronize()
    rates = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        rates.append(n_frames / (a.elapsed_time(b) * 1e-3))
    return round(statistics.median(rates), 1), [round(r, 1) for r in rates]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--out", help="also append the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plan_bench.py measures on the GPU: no device found")
    frames = list(sequence.sweep_frames(range(args.frames), scale=SCALE, device=DEV))
    torch.cuda.synchronize()
    n = len(frames)
    res = {"image": "640x480", "frames": n, "repeats": REPEATS}

    def pass1(yaw):
        planner = bnv.VolumePlanner(device=DEV, align_yaw=yaw)
        for f in frames:
            planner.add(f)
        return planner

    for name, yaw in (("pass1_3_dirs", None), ("pass1_39_dirs", 18)):
        res[name + "_fps"], res[name + "_all"] = timed(lambda: pass1(yaw), n)

    def pass0(step):
        planner = bnv.VolumePlanner(device=DEV, align="manhattan", normal_step=step)
        for f in frames:
            planner.add_normals(f)
        return planner

    for name, step in (("pass0_step_1", 1), ("pass0_step_8", 8)):
        res[name + "_fps"], res[name + "_all"] = timed(lambda: pass0(step), n)
        try:
            frame = pass0(step).manhattan()
        except bnv.BnvError as e:
            res[name + "_frame"] = {"refused": str(e)}
            continue
        res[name + "_frame"] = {"confidence": round(frame.confidence, 3), "normals": frame.n_normals,
                                "largest_axis_error_deg": round(max(
                                    math.degrees(math.acos(min(1.0, float(np.abs(r).max())))) for r in frame.R), 3)}
    ext = pass1(None).extent()
    res["dimensions"] = [round(float(d), 2) for d in ext.dimensions]
    res["valid_points"] = ext.n_points
    counter = bnv.VolumePlanner(device=DEV)
    for name, sizes in (("pass2_1_size", (0.01,)), ("pass2_4_sizes", SIZES_4)):
        res[name + "_fps"], res[name + "_all"] = timed(
            lambda: counter.count(frames, sizes, dimensions=ext.dimensions, axis_align_mat=ext.axis_align_mat), n)
    cands = counter.count(frames, SIZES_4, dimensions=ext.dimensions, axis_align_mat=ext.axis_align_mat)
    res["table_mib_per_candidate"] = {f"{c.voxel_size:g}": round(c.table_bytes / 2 ** 20, 1) for c in cands}
    res["candidates"] = {f"{c.voxel_size:g}": {"min": round(c.min, 2), "mean": round(c.mean, 2), "ok": c.ok}
                         for c in cands}
    dims, voxel, _ = sequence.DIMS[256]
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)

    def integrate():
        nm = bnv.NeuralMap(np.array([dims] * 3), voxel, model, capacity=1 << 20, device=DEV)
        for f in frames:
            nm.integrate(f)

    res["integrate_256_fps"], res["integrate_256_all"] = timed(integrate, n)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
