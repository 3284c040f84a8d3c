"""Timings of mesh post-processing (merge close vertices, clean, one smoothing pass) on the host
(mesh.post_process_mesh: numpy + scipy) against the device (mesh.post_process_mesh_tensors) -> one JSON document.

    python tools/mesh_post_bench.py [--sweep-frames N] [--grids 256,512] [--json OUT]

Meshes: the room sweep (sequence.py, its first N frames) extracted at each grid, vertex threshold
voxel / 4 as run_e2e.py:293 uses.  Per mesh: V / T in and out, the host's ms per call (wall clock, one call), the
device's ms per call (HIP events, median of 5 after 2 warm-up calls; device tensors in and out), and whether the two
results are bit-identical.  For a kernel breakdown: rocprofv3 --kernel-trace --stats -- python tools/mesh_post_bench.py"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bnv_fusion_amd as bnv  # noqa: E402

bnv.configure_runtime()
from bnv_fusion_amd import mesh as M, sequence  # noqa: E402

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


def sweep_mesh(grid, n_frames):
    dims, voxel, scale = sequence.DIMS[grid]
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)
    nm = bnv.NeuralMap(np.array([dims] * 3), voxel, model, device=DEV)
    for fr in sequence.sweep_frames(range(n_frames), scale=scale, device=DEV):
        nm.integrate(fr)
    return nm.extract_mesh(), voxel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep-frames", type=int, default=600)
    ap.add_argument("--grids", default="256,512")
    ap.add_argument("--json")
    args = ap.parse_args()
    out = {}
    for grid in [int(g) for g in args.grids.split(",")]:
        mesh, voxel = sweep_mesh(grid, args.sweep_frames)
        eps = voxel / 4
        t0 = time.perf_counter()
        host = M.post_process_mesh(mesh, eps)
        host_ms = 1e3 * (time.perf_counter() - t0)
        v = torch.from_numpy(mesh.vertices).to(DEV)
        f = torch.from_numpy(mesh.faces).to(DEV)
        dev_ms = timed(lambda: M.post_process_mesh_tensors(v, f, eps))
        gv, gf = M.to_host(*M.post_process_mesh_tensors(v, f, eps))
        same = bool(gv.shape == host.vertices.shape and np.array_equal(gv.view(np.uint32), host.vertices.view(np.uint32))
                    and np.array_equal(gf, host.faces))
        out[f"sweep_{grid}"] = {"frames": args.sweep_frames, "V_in": len(mesh.vertices), "T_in": len(mesh.faces),
                                "V_out": len(host.vertices), "T_out": len(host.faces), "host_ms": round(host_ms, 1),
                                "gpu_ms": round(dev_ms, 3), "bit_identical": same}
        print(json.dumps({f"sweep_{grid}": out[f"sweep_{grid}"]}), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
