"""Timings of point-to-mesh registration (csrc/register.hip, bnv_fusion_amd/register.py) -> one JSON line.

    python tools/register_bench.py [--points 100000] [--json OUT]

The target is synthetic.gt_mesh(step_px=1) (~0.8 M faces, the mesh tools/mesh_ray_bench.py uses); the source is
``--points`` samples of its surface under a small known displacement (about 1 degree and 3 cm).  What an iteration
costs is what its search costs, and that depends on how far the points are from the mesh (rings of millimetre
cells), so two figures: a one-iteration call at the start (its init launch and the host's one read included) beside
``MeshSDF.query`` of the same points, and ``ms_per_iteration_converged``: a schedule of 10 iterations at stride 1 over
one of 2, divided by 8 -- iterations 3 to 10, the points on the surface by then; the init launch and the read
cancel --, beside ``MeshSDF.query`` of the points where they end up.  The queries are the floor: an iteration is that
search plus the sums.  HIP events, median of 5 after 2 warm-up calls, all in one run.  The tracker's per-iteration
cost as README.md records it is the overhead to expect of the second launch (the solve) and the reduction."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bnv_fusion_amd as bnv  # noqa: E402

bnv.configure_runtime()
from bnv_fusion_amd import evaluate, register, synthetic, tracking  # noqa: E402

DEV = "cuda:0"
TRACKER_US_PER_ITERATION = 36.0       # README.md, "Tracking": bnv_icp_align per iteration


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--json")
    args = ap.parse_args()
    v, f = evaluate._mesh_tensors(synthetic.gt_mesh(step_px=1), None, DEV)
    sdf = evaluate.MeshSDF(v, f)
    gen = torch.Generator(device=DEV).manual_seed(0)
    pts = evaluate.sample_surface(v, f, args.points, generator=gen)[0]
    M = tracking.se3_exp([0.01, -0.008, 0.012, 0.02, -0.015, 0.01])       # about 1 degree and 3 cm
    src = register.transform_points(tracking.rigid_inverse(M), pts)
    gate = 0.1
    res = register.register_points(src, sdf, levels=((1, 10, gate),))
    ms1 = timed(lambda: register.register_points(src, sdf, levels=((1, 1, gate),)))
    ms10 = timed(lambda: register.register_points(src, sdf, levels=((1, 10, gate),)))
    ms2 = timed(lambda: register.register_points(src, sdf, levels=((1, 2, gate),)))
    query_start_ms = timed(lambda: sdf.query(src))
    query_converged_ms = timed(lambda: sdf.query(pts))
    dT = res.T @ tracking.rigid_inverse(M)
    out = {"case": "synthetic.gt_mesh(step_px=1)", "faces": int(f.shape[0]), "points": args.points,
           "status": register.STATUS_NAMES[res.status], "inlier_share": round(res.inlier_share, 4),
           "residual_translation_mm": round(float(np.linalg.norm(dT[:3, 3])) * 1e3, 4),
           "ms_1_iteration_call_at_the_start": round(ms1, 3), "mesh_sdf_query_at_the_start_ms": round(query_start_ms, 4),
           "ms_10_iterations": round(ms10, 3), "ms_2_iterations": round(ms2, 3),
           "ms_per_iteration_converged": round((ms10 - ms2) / 8.0, 4),
           "mesh_sdf_query_converged_ms": round(query_converged_ms, 4),
           "tracker_us_per_iteration": TRACKER_US_PER_ITERATION}
    print(json.dumps(out), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
