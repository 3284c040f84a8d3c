"""Timings and quality of mesh simplification on the device (mesh.simplify_mesh_tensors) -> one JSON document.

    python tools/mesh_simplify_bench.py [--sweep-frames N] [--grids 256,512] [--cells 2,4] [--json OUT]

Meshes: the room sweep (sequence.py, its first N frames) extracted at each grid and post-processed on the device at
voxel / 4, as run_e2e.py does.  Per mesh: the device post-process's ms per call, and per cell size (in voxels) the
simplify's ms per call (HIP events, median of 5 after 2 warm-up calls; device tensors in and out), vertices and faces
in and out, whether the result is bit-identical to the host function, and evaluate_meshes(simplified, original) at
2.5 cm: the mean distance between the two surfaces (mean of both directions, between 100,000 surface samples of each;
``sampling_floor_mm`` is the same figure for two sample sets of the unsimplified mesh) and their F1; and, free of that
floor, the exact point-to-mesh distances (evaluate.MeshSDF) of 100,000 samples of each surface to the other mesh: the
two means and the two largest (a small component that collapses into one cell vanishes: its samples are
then as far from the simplified mesh as the component was from the rest).  For a kernel breakdown:
rocprofv3 --kernel-trace --stats -- python tools/mesh_simplify_bench.py; for the registers of the accumulate kernel
(k_ms_place): python bnv_fusion_amd/csrc/build.py --force --verbose."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_post_bench import DEV, sweep_mesh, timed  # noqa: E402

from bnv_fusion_amd import evaluate, mesh as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep-frames", type=int, default=600)
    ap.add_argument("--grids", default="256,512")
    ap.add_argument("--cells", default="2,4", help="cell sizes in voxels")
    ap.add_argument("--threshold", type=float, default=0.025, help="distance threshold of the F1, metres")
    ap.add_argument("--placement", default="quadric", choices=["quadric", "mean"])
    ap.add_argument("--json")
    args = ap.parse_args()
    out = {}
    for grid in [int(g) for g in args.grids.split(",")]:
        raw, voxel = sweep_mesh(grid, args.sweep_frames)
        rv, rf = torch.from_numpy(raw.vertices).to(DEV), torch.from_numpy(raw.faces).to(DEV)
        post_ms = timed(lambda: M.post_process_mesh_tensors(rv, rf, voxel / 4))
        v, f = M.post_process_mesh_tensors(rv, rf, voxel / 4)
        host_in = M.TriMesh(*M.to_host(v, f))
        row = {"frames": args.sweep_frames, "voxel": voxel, "V_in": int(v.shape[0]), "T_in": int(f.shape[0]),
               "post_process_gpu_ms": round(post_ms, 3), "placement": args.placement, "cells": {}}
        # the floor of the distance figures: two independent sample sets of the SAME mesh (100,000 samples each)
        res = evaluate.evaluate_meshes((v, f), (v, f), threshold=args.threshold,
                                       generator=torch.Generator(device=DEV).manual_seed(0))
        row["sampling_floor_mm"] = round(5e2 * (res["pred_gt"] + res["gt_pred"]), 4)
        for k in [float(c) for c in args.cells.split(",")]:
            cell = k * voxel
            ms = timed(lambda: M.simplify_mesh_tensors(v, f, cell, args.placement))
            sv, sf = M.simplify_mesh_tensors(v, f, cell, args.placement)
            want = M.simplify_mesh(host_in, cell, args.placement)
            gv, gf = M.to_host(sv, sf)
            same = bool(gv.shape == want.vertices.shape and np.array_equal(gv.view(np.uint32), want.vertices.view(np.uint32))
                        and np.array_equal(gf, want.faces))
            res = evaluate.evaluate_meshes((sv, sf), (v, f), threshold=args.threshold,
                                           generator=torch.Generator(device=DEV).manual_seed(0))
            # exact distances, free of the sampling floor: 100,000 samples of each surface to the other MESH
            gen = torch.Generator(device=DEV).manual_seed(1)
            d_so = evaluate.MeshSDF(v, f).query(evaluate.sample_surface(sv, sf, 100000, generator=gen)[0])[0].abs()
            d_os = evaluate.MeshSDF(sv, sf).query(evaluate.sample_surface(v, f, 100000, generator=gen)[0])[0].abs()
            exact = [d_so.double().mean(), d_os.double().mean(), d_so.max().double(), d_os.max().double()]
            exact = [round(1e3 * x, 4) for x in torch.stack(exact).tolist()]
            row["cells"][f"{k:g}_voxels"] = {
                "cell": cell, "gpu_ms": round(ms, 3), "V_out": int(sv.shape[0]), "T_out": int(sf.shape[0]),
                "faces_kept": round(int(sf.shape[0]) / max(int(f.shape[0]), 1), 4), "bit_identical_to_host": same,
                "mean_distance_mm": round(5e2 * (res["pred_gt"] + res["gt_pred"]), 4),
                "f1": round(res["F1"], 5), "evaluate": evaluate.summary_line(res),
                "to_original_mesh_mm": exact[0], "from_original_mesh_mm": exact[1],
                "to_original_mesh_max_mm": exact[2], "from_original_mesh_max_mm": exact[3]}
        out[f"sweep_{grid}"] = row
        print(json.dumps({f"sweep_{grid}": row}), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
