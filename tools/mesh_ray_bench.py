"""Timings of the mesh scanner (csrc/meshray.hip, bnv_fusion_amd/scan.py) -> one JSON line per case.

    python tools/mesh_ray_bench.py [--count] [--json OUT]

Cases: ``render_depth`` at 640 x 480 on sequence.gt_mesh() (96 faces, sweep poses) and on synthetic.gt_mesh(step_px=1)
(~0.8 M faces, the pan's poses), 8 poses per launch; ``simulate_sensor`` alone; beside them ``MeshSDF.query`` for
307,200 points on the same meshes.  HIP events, median of 5 after 2 warm-up calls.  --count: also the mean number of
cells stepped and triangles tested per ray, from a build of csrc/meshsdf.hip + csrc/meshray.hip alone with
-DBNV_MESHRAY_COUNT (tools/libbnv_meshray_count.so; compiled on first use).  For a kernel breakdown, in a run of its
own: rocprofv3 --kernel-trace --stats -- python tools/mesh_ray_bench.py"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bnv_fusion_amd as bnv  # noqa: E402

bnv.configure_runtime()
from bnv_fusion_amd import evaluate, scan, sequence, synthetic  # noqa: E402
from bnv_fusion_amd.csrc import build as hip_build  # noqa: E402

DEV = "cuda:0"
COUNT_LIB = os.path.join(ROOT, "tools", "libbnv_meshray_count.so")
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


def count_lib():
    if not os.path.exists(COUNT_LIB):
        subprocess.check_call([hip_build._hipcc()] + hip_build.FLAGS + ["-DBNV_MESHRAY_COUNT",
                              os.path.join(hip_build.HERE, "meshsdf.hip"), os.path.join(hip_build.HERE, "meshray.hip"),
                              os.path.join(ROOT, "tools", "mesh_sdf_count_stub.hip"), "-o", COUNT_LIB])
    return C.CDLL(COUNT_LIB)


def counts_per_ray(lib, v, f, K, poses):
    """Mean cells stepped and triangles tested per ray over ``poses``: the counting build's two counters."""
    n = C.c_int64()
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    assert lib.bnv_mesh_sdf_workspace_bytes(C.c_int64(v.shape[0]), C.c_int64(f.shape[0]), C.byref(n)) == 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.bnv_mesh_sdf_build(vp(v), C.c_int64(v.shape[0]), vp(f), C.c_int64(f.shape[0]), vp(ws), C.c_int64(n.value), s) == 0
    depth = torch.empty((len(poses), H, W), dtype=torch.float32, device=DEV)
    Kf = np.ascontiguousarray(K, np.float32).reshape(-1)
    Pf = np.ascontiguousarray(poses, np.float32).reshape(-1)
    out = (C.c_ulonglong * 2)()
    assert lib.bnv_mesh_ray_counts(out) == 0                     # (reads and clears)
    lib.bnv_mesh_render_depth.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_void_p]
    assert lib.bnv_mesh_render_depth(vp(ws), n.value, len(poses), Kf.ctypes.data, Pf.ctypes.data, H, W, 0.0,
                                     float("inf"), vp(depth), None, None, None, 0, s) == 0
    assert lib.bnv_mesh_ray_counts(out) == 0
    rays = len(poses) * H * W
    return out[0] / rays, out[1] / rays


def case(name, mesh, K, poses, lib):
    v, f = evaluate._mesh_tensors(mesh, None, DEV)
    sc = scan.MeshScanner(v, f)
    ms = timed(lambda: sc.render_depth(poses, K, H, W))
    ms_n = timed(lambda: sc.render_depth(poses, K, H, W, normals=True))
    depth, _ = sc.render_depth(poses, K, H, W)
    lo, hi = v.min(0).values, v.max(0).values
    q = lo + torch.rand((H * W, 3), generator=torch.Generator(device=DEV).manual_seed(0), device=DEV) * (hi - lo)
    sdf_ms = timed(lambda: sc.index.query(q))
    res = {"case": name, "faces": int(f.shape[0]), "poses_per_launch": len(poses), "render_ms_per_launch": round(ms, 3),
           "render_frames_per_s": round(len(poses) / ms * 1e3, 1),
           "render_with_normals_frames_per_s": round(len(poses) / ms_n * 1e3, 1),
           "Mrays_per_s": round(len(poses) * H * W / ms / 1e3, 1), "hit_fraction": round(float((depth > 0).float().mean()), 4),
           "mesh_sdf_query_307200_ms": round(sdf_ms, 3)}
    if lib is not None:
        cells, tests = counts_per_ray(lib, v, f, K, poses)
        res["cells_per_ray"], res["triangle_tests_per_ray"] = round(cells, 2), round(tests, 2)
    print(json.dumps(res), flush=True)
    return res, depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    lib = count_lib() if args.count else None
    out = []
    room_poses = np.stack([sequence.sweep_pose(t) for t in range(0, 800, 100)])
    r, depth = case("sequence.gt_mesh", sequence.gt_mesh(), sequence.intrinsics(), room_poses, lib)
    out.append(r)
    pan_poses = np.stack([synthetic.pose(t) for t in range(8)])
    r, _ = case("synthetic.gt_mesh(step_px=1)", synthetic.gt_mesh(step_px=1), synthetic.intrinsics(), pan_poses, lib)
    out.append(r)
    clean = depth[0].contiguous()
    ms = timed(lambda: scan.simulate_sensor(clean, 0, 0))
    res = {"case": "simulate_sensor 640x480", "ms": round(ms, 4), "frames_per_s": round(1e3 / ms, 1)}
    print(json.dumps(res), flush=True)
    out.append(res)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
