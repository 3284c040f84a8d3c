"""Timings of the persistent cloud index and of cloud-to-cloud registration (csrc/cloud_register.hip,
bnv_fusion_amd/pointcloud.py: CloudIndex, bnv_fusion_amd/register.py: register_cloud) -> one JSON line.

    python tools/cloud_register_bench.py [--points 100000] [--targets 307200 1997568] [--json OUT]

The targets are ``--targets`` surface samples of synthetic.gt_mesh(step_px=1) (the mesh tools/register_bench.py
registers to) with their face normals; the source is ``--points`` other samples of it under a small known displacement
(about 1 degree and 3 cm).  Per target: ``index_build_ms`` (CloudIndex from the [N, 6] rows, its workspace allocation
included), ``nearest_ms`` of as many queries as the target has points beside ``nn_query_ms``
(evaluate.nn_d2, which builds the index on every call).  Against the largest target: a one-iteration call at the
start (its init launch and the host's one read included) and ``ms_per_iteration_converged`` -- a schedule of 10
iterations at stride 1 over one of 2, divided by 8, as tools/register_bench.py takes it -- beside the same two figures
of register_points against the mesh itself for the same points, and the converged iteration once more with the source
ordered by the cell of a grid of about the target's spacing at the guess (neighbouring threads then walk the same
cells) beside the order the sampler gave (random).  HIP events, median of 5 after 2 warm-up calls, all in one run."""
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
from bnv_fusion_amd import evaluate, pointcloud, register, synthetic, tracking  # noqa: E402

DEV = "cuda:0"


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


def cell_order(points, T, cell):
    """The permutation that sorts ``points`` at the pose ``T`` by the x-major cell of a grid of edge ``cell``."""
    q = register.transform_points(T, points).double()
    c = torch.floor((q - q.min(0).values) / cell).long()
    dims = c.max(0).values + 1
    return torch.argsort((c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2])


def per_iteration(run):
    """(a one-iteration call, a converged iteration) in ms; ``run(iterations)`` registers from the start."""
    ms1, ms2, ms10 = (timed(lambda k=k: run(k)) for k in (1, 2, 10))
    return ms1, (ms10 - ms2) / 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--targets", type=int, nargs="+", default=[307200, 1997568])
    ap.add_argument("--json")
    args = ap.parse_args()
    v, f = evaluate._mesh_tensors(synthetic.gt_mesh(step_px=1), None, DEV)
    gen = torch.Generator(device=DEV).manual_seed(0)
    out = {"case": "synthetic.gt_mesh(step_px=1)", "faces": int(f.shape[0]), "points": args.points, "targets": []}
    index = rows = None
    for n in sorted(args.targets):
        pos, _, nrm = evaluate.sample_surface(v, f, n, generator=gen, return_normals=True)
        rows = torch.cat([pos, nrm], 1).contiguous()
        queries = evaluate.sample_surface(v, f, n, generator=gen)[0]
        index = pointcloud.CloudIndex(input_pts=rows)
        d2, idx = index.nearest(queries)
        d2_q, idx_q = evaluate.nn_d2(queries, pos)
        same = bool(torch.equal(d2.view(torch.int32), d2_q.view(torch.int32)) and torch.equal(idx, idx_q))
        out["targets"].append({
            "points": n, "index_bytes": index._ws_bytes, "nearest_equals_nn_query": same,
            "index_build_ms": round(timed(lambda: pointcloud.CloudIndex(input_pts=rows)), 4),
            "nearest_ms": round(timed(lambda: index.nearest(queries)), 4),
            "nn_query_ms": round(timed(lambda: evaluate.nn_d2(queries, pos)), 4)})
    # the aligner against the largest target
    pts = evaluate.sample_surface(v, f, args.points, generator=gen)[0]
    M = tracking.se3_exp([0.01, -0.008, 0.012, 0.02, -0.015, 0.01])       # about 1 degree and 3 cm
    src = register.transform_points(tracking.rigid_inverse(M), pts)
    gate = 0.1
    res = register.register_cloud(src, index, levels=((1, 10, gate),))
    dT = res.T @ tracking.rigid_inverse(M)
    ms1, conv = per_iteration(lambda k: register.register_cloud(src, index, levels=((1, k, gate),)))
    sdf = evaluate.MeshSDF(v, f)
    mesh_ms1, mesh_conv = per_iteration(lambda k: register.register_points(src, sdf, levels=((1, k, gate),)))
    L = (rows[:, :3].max(0).values - rows[:, :3].min(0).values).double().cpu().numpy()
    spacing = float(np.sqrt(4.0 * (L[0] * L[1] + L[1] * L[2] + L[2] * L[0]) / index.n))   # cell_grid.hpp's edge rule
    ordered = src[cell_order(src, np.eye(4), spacing)].contiguous()
    ord_ms1, ord_conv = per_iteration(lambda k: register.register_cloud(ordered, index, levels=((1, k, gate),)))
    out.update({
        "target_points": index.n, "status": register.STATUS_NAMES[res.status],
        "inlier_share": round(res.inlier_share, 4),
        "residual_translation_mm": round(float(np.linalg.norm(dT[:3, 3])) * 1e3, 4),
        "cloud_ms_1_iteration_call_at_the_start": round(ms1, 4), "cloud_ms_per_iteration_converged": round(conv, 4),
        "mesh_ms_1_iteration_call_at_the_start": round(mesh_ms1, 4), "mesh_ms_per_iteration_converged": round(mesh_conv, 4),
        "order_cell_m": round(spacing, 5),
        "ordered_ms_1_iteration_call_at_the_start": round(ord_ms1, 4),
        "ordered_ms_per_iteration_converged": round(ord_conv, 4)})
    print(json.dumps(out), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
