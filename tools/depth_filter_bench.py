"""The figures of the depth filter (csrc/depth_filter.hip; frontend.filter_depth / DepthFilter), printed as one JSON
line per section:

* cost       microseconds per 640 x 480 frame: the median of single launches timed with HIP events after a warm-up, and
             the mean over a train of back-to-back launches between one pair of events (without the gaps between
             launches that a single-launch event pair includes); uint16 and float32 input, radius 2, 3 and 4;
* fusion     fuse_and_decode_async frames/s over 30 sweep frames at 256^3 / 1 cm, two frames in flight, resident
             inputs: without the filter (the rate of the code before the filter existed: nothing of it runs), without
             the filter but with inputs_resident off (what a filtered frame gives up besides the kernel: the encode
             stream waits for the caller's stream), and with the filter.  Alternating repeats, median;
* quality    a Kinect-noise scan of the half-scale room (sweep frames 96 .. 140 step 4), fused with the true poses at
             128^3 / 2 cm and 256^3 / 1 cm: evaluate_meshes of the extracted mesh (precision against the mesh, recall
             against the faces the scan saw) with and without the filter; and the tracked loop over drifting odometry
             (scan.drift_poses 5 mm / 3 mrad, seed 0): trajectory errors with and without the filter.

    python tools/depth_filter_bench.py [--out FILE] [--skip-quality]
"""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import bnv_fusion_amd as bnv  # noqa: E402
bnv.configure_runtime()      # the package's hardware queue count, before the first HIP call (streams.py)
from bnv_fusion_amd import _lib, evaluate, frontend, scan, sequence, tracking  # noqa: E402

DEV = "cuda:0"
SCALE, MAX_DEPTH = 0.5, 3.0
FRAMES = range(96, 141, 4)
GRIDS = {128: (2.54, 0.02), 256: (2.54, 0.01)}


def emit(out, section, payload):
    line = json.dumps({"section": section, **payload})
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def filter_cost(launches=50, train=200):
    lib = _lib.require_device(0)
    mm = sequence.depth_u16(250, scale=SCALE, device=DEV)
    inputs = {"uint16": mm, "float32": (mm.to(torch.float32) / 1000.0).contiguous()}
    out = torch.empty((480, 640), dtype=torch.float32, device=DEV)
    res = {}
    for name, d in inputs.items():
        for radius in (2, 3, 4):
            def launch():
                _lib.check(lib.bnv_depth_filter(_lib.ptr(d), frontend.DEPTH_DTYPES[d.dtype], 480, 640, MAX_DEPTH, radius,
                                                frontend.DEFAULT_SIGMA_DEPTH, 3.0, None, 0, _lib.ptr(out),
                                                _lib.stream_ptr()), "bnv_depth_filter")
            for _ in range(20):
                launch()
            torch.cuda.synchronize()
            singles = []
            for _ in range(launches):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                b.synchronize()
                singles.append(a.elapsed_time(b) * 1e3)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(train):
                launch()
            b.record()
            b.synchronize()
            res[f"{name}_r{radius}"] = {"median_single_launch_us": round(statistics.median(singles), 2),
                                        "min_single_launch_us": round(min(singles), 2),
                                        "mean_in_train_us": round(a.elapsed_time(b) * 1e3 / train, 2)}
    return {"image": "640x480", "single_launches": launches, "train_launches": train, "us": res}


def fusion_rate(model, n_frames=30, repeats=5):
    dims, voxel = GRIDS[256]
    frames = list(sequence.sweep_frames(range(n_frames), scale=SCALE, device=DEV))
    torch.cuda.synchronize()
    configs = {"no_filter_resident": (None, True), "no_filter_not_resident": (None, False),
               "filter_resident": (frontend.DepthFilter(), True)}

    def one(flt, resident):
        nm = bnv.NeuralMap(np.array([dims] * 3), voxel, model, capacity=1 << 20, device=DEV, tsdf=True,
                           depth_filter=flt)
        nm.inputs_resident = resident
        st = sequence.run(nm, frames, pipelined=True, in_flight=2, checksums=False)
        return st["frames"] / st["seconds"]

    for flt, resident in configs.values():       # warm-up: code objects, the allocator's pools, the pipeline's slots
        one(flt, resident)
    rates = {k: [] for k in configs}
    for _ in range(repeats):
        for k, (flt, resident) in configs.items():
            rates[k].append(one(flt, resident))
    return {"grid": "256^3 / 1 cm", "frames": n_frames, "repeats": repeats,
            "frames_per_s_median": {k: round(statistics.median(v), 1) for k, v in rates.items()},
            "frames_per_s_all": {k: [round(x, 1) for x in v] for k, v in rates.items()}}


def quality(models):
    scanner = scan.MeshScanner(sequence.gt_mesh(SCALE), device=DEV)
    truth = np.stack([sequence.sweep_pose(t, SCALE) for t in FRAMES])
    scanned = list(scan.scan_frames(scanner, truth, sequence.intrinsics(480, 640), 480, 640, noise="kinect"))
    visible, whole = scanner.visible_mesh(), sequence.gt_mesh(SCALE)
    drifted = scan.drift_poses(truth, sigma_t=0.005, sigma_r=0.003, seed=0)
    out = {}
    for grid, (dims, voxel) in GRIDS.items():
        for name, flt in (("raw", None), ("filtered", frontend.DepthFilter())):
            def new_map():
                return bnv.NeuralMap(np.array([dims] * 3), voxel, models[grid], capacity=1 << 20, device=DEV, tsdf=True,
                                     depth_filter=flt)
            nm = new_map()
            for fr in scanned:
                nm.integrate(fr)
            mesh = nm.extract_mesh()
            res = evaluate.evaluate_meshes(mesh, whole, gt_recall=visible, device=DEV,
                                           generator=torch.Generator(device=DEV).manual_seed(0))
            tracker = tracking.Tracker(new_map(), source="tsdf", model_size=(120, 160))
            for fr, T in zip(scanned, drifted):
                tracker.integrate(dict(fr, T_wc=T))
            torch.cuda.synchronize()
            err = evaluate.trajectory_errors(tracker.poses, truth)
            out[f"{grid}_{name}"] = {"mesh": evaluate.summary_line(res),
                                     "mesh_keys": "pred_gt/accuracy/gt_pred/recall/F1 at 2.5 cm",
                                     "tracked_translation_rmse_mm": round(err["translation_rmse"] * 1e3, 3),
                                     "tracked_rotation_mean_deg": round(err["rotation_mean_deg"], 4),
                                     "refused": int(tracker.failures), "frames": len(scanned)}
    given = evaluate.trajectory_errors(drifted, truth)
    out["odometry"] = {"translation_rmse_mm": round(given["translation_rmse"] * 1e3, 3),
                       "rotation_mean_deg": round(given["rotation_mean_deg"], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also append the JSON lines to this file")
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_filter_bench.py measures on the GPU: no device found")
    out = open(args.out, "a") if args.out else None
    emit(out, "cost", filter_cost())
    models = {g: bnv.load_pretrained(device=DEV, voxel_size=v) for g, (_, v) in GRIDS.items()}
    emit(out, "fusion", fusion_rate(models[256]))
    if not args.skip_quality:
        emit(out, "quality", quality(models))


if __name__ == "__main__":
    main()
