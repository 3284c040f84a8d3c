"""Timings of mesh post-processing (merge close vertices, clean, one smoothing pass) on the host
(mesh.post_process_mesh: numpy + scipy) against the device (mesh.post_process_mesh_tensors) -> one JSON document.

    python tools/mesh_post_bench.py [--sweep-frames N] [--grids 256,512] [--json OUT]

Meshes: the room sweep (sequence.py, its first N frames) extracted at each grid, vertex threshold
voxel / 4 as run_e2e.py:293 uses.  Per mesh: V / T in and out, the host's ms per call (wall clock, one call), the
device's ms per call (HIP events, median of 5 after 2 warm-up calls; device tensors in and out), and whether the two
results are bit-identical.  On the post-processed mesh, the connected components (mesh.connected_components /
mesh.remove_small_components against their device versions): C, the largest component's share of the area, host and
device ms for labelling + areas and for the filter at --min-area (0.1 m^2), measured the same way, and a bit-identical
flag for each.  For a kernel breakdown: rocprofv3 --kernel-trace --stats -- python tools/mesh_post_bench.py"""
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


def components(host, gv, gf, min_area):
    """Connected components of the post-processed mesh: host against device."""
    t0 = time.perf_counter()
    labels, n_faces, areas = M.connected_components(host)
    host_cc_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    kept = M.remove_small_components(host, min_area=min_area)
    host_filter_ms = 1e3 * (time.perf_counter() - t0)
    v, f = torch.from_numpy(gv).to(DEV), torch.from_numpy(gf).to(DEV)
    cc_ms = timed(lambda: M.connected_components_tensors(v, f))
    filter_ms = timed(lambda: M.remove_small_components_tensors(v, f, min_area=min_area))
    dl, dn, da = M.to_host(*M.connected_components_tensors(v, f))
    kv, kf = M.to_host(*M.remove_small_components_tensors(v, f, min_area=min_area))
    same_cc = bool(np.array_equal(dl, labels) and np.array_equal(dn, n_faces)
                   and np.array_equal(da.view(np.uint64), areas.view(np.uint64)))
    same_filter = bool(kv.shape == kept.vertices.shape and np.array_equal(kv.view(np.uint32), kept.vertices.view(np.uint32))
                       and np.array_equal(kf, kept.faces))
    return {"components": len(areas), "largest_area_share": round(float(areas.max() / areas.sum()), 6) if len(areas) else None,
            "min_area": min_area, "T_removed": len(host.faces) - len(kept.faces),
            "area_removed": round(float(areas[areas < min_area].sum()), 6), "area_total": round(float(areas.sum()), 6),
            "host_components_ms": round(host_cc_ms, 1), "host_filter_ms": round(host_filter_ms, 1),
            "gpu_components_ms": round(cc_ms, 3), "gpu_filter_ms": round(filter_ms, 3),
            "components_bit_identical": same_cc, "filter_bit_identical": same_filter}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep-frames", type=int, default=600)
    ap.add_argument("--grids", default="256,512")
    ap.add_argument("--min-area", type=float, default=0.1, help="area threshold of the component filter")
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
        out[f"sweep_{grid}"].update(components(host, gv, gf, args.min_area))
        print(json.dumps({f"sweep_{grid}": out[f"sweep_{grid}"]}), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
