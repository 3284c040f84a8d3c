"""Timings of the mesh signed distance (csrc/meshsdf.hip) and of the patch cutter built on it -> one JSON line per case.

    python tools/mesh_sdf_bench.py [--queries 1000000] [--count-tests] [--json OUT]

Cases: sequence.gt_mesh() with uniform queries in its bounding box; synthetic.gt_mesh(step_px=1) (~0.8 M triangles)
with queries a Gaussian step of 2 cm off its vertices; a full patches.cut_local_patches of that mesh at voxel 0.01
beside one training epoch (batch 100) over the patches it gives.  The index build and the query are timed apart with
HIP events (median of 5 after 2 warm-up calls); the cut and the epoch by wall clock around a synchronise.
--count-tests: also the mean number of triangle tests per query, from a build of csrc/meshsdf.hip alone with
-DBNV_MESHSDF_COUNT_TESTS (tools/libbnv_meshsdf_count.so; compiled on first use).  For a kernel breakdown, in a run
of its own: rocprofv3 --kernel-trace --stats -- python tools/mesh_sdf_bench.py"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bnv_fusion_amd as bnv  # noqa: E402

bnv.configure_runtime()
from bnv_fusion_amd import evaluate, patches, sequence, synthetic, train  # noqa: E402
from bnv_fusion_amd.csrc import build as hip_build  # noqa: E402

DEV = "cuda:0"
COUNT_LIB = os.path.join(ROOT, "tools", "libbnv_meshsdf_count.so")


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
        subprocess.check_call([hip_build._hipcc()] + hip_build.FLAGS + ["-DBNV_MESHSDF_COUNT_TESTS",
                              os.path.join(hip_build.HERE, "meshsdf.hip"),
                              os.path.join(ROOT, "tools", "mesh_sdf_count_stub.hip"), "-o", COUNT_LIB])
    return C.CDLL(COUNT_LIB)


def tests_per_query(lib, v, f, q):
    """Mean triangle tests per query: the counting build's counter at byte 24 of the index."""
    n = C.c_int64()
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    assert lib.bnv_mesh_sdf_workspace_bytes(C.c_int64(v.shape[0]), C.c_int64(f.shape[0]), C.byref(n)) == 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    sdf = torch.empty(q.shape[0], dtype=torch.float32, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.bnv_mesh_sdf_build(vp(v), C.c_int64(v.shape[0]), vp(f), C.c_int64(f.shape[0]), vp(ws), C.c_int64(n.value), s) == 0
    assert lib.bnv_mesh_sdf_query(vp(ws), C.c_int64(n.value), vp(q), C.c_int64(q.shape[0]), vp(sdf), None, None, None, s) == 0
    torch.cuda.synchronize()
    return int(ws[24:32].view(torch.int64).item()) / q.shape[0]


def sdf_case(name, mesh, q, lib):
    v, f = evaluate._mesh_tensors(mesh, None, DEV)
    build_ms = timed(lambda: evaluate.MeshSDF(v, f))
    index = evaluate.MeshSDF(v, f)
    query_ms = timed(lambda: index.query(q))
    feature = index.query(q)[3]
    res = {"case": name, "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "queries": int(q.shape[0]),
           "index_MiB": round(index._ws_bytes / 2 ** 20, 1), "build_ms": round(build_ms, 3),
           "query_ms": round(query_ms, 3), "Mqueries_per_s": round(q.shape[0] / query_ms / 1e3, 1),
           "boundary_fraction": round(float(((feature & evaluate.FEATURE_BOUNDARY) != 0).float().mean()), 4)}
    if lib is not None:
        res["tests_per_query"] = round(tests_per_query(lib, v, f, q), 1)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000000)
    ap.add_argument("--count-tests", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    lib = count_lib() if args.count_tests else None
    g = torch.Generator(device=DEV).manual_seed(0)
    out = []
    room = sequence.gt_mesh()
    lo, hi = torch.from_numpy(room.vertices.min(0)).to(DEV), torch.from_numpy(room.vertices.max(0)).to(DEV)
    q = lo + torch.rand((args.queries, 3), generator=g, device=DEV) * (hi - lo)
    out.append(sdf_case("sequence.gt_mesh", room, q, lib))
    scene = synthetic.gt_mesh(step_px=1)
    sv = torch.from_numpy(scene.vertices).to(DEV)
    pick = torch.randint(0, sv.shape[0], (args.queries,), generator=g, device=DEV)
    q = sv[pick] + torch.randn((args.queries, 3), generator=g, device=DEV) * 0.02
    out.append(sdf_case("synthetic.gt_mesh(step_px=1)", scene, q, lib))
    # the cutter beside one training epoch over what it cuts
    v, f = evaluate._mesh_tensors(scene, None, DEV)
    cut = lambda: patches.cut_local_patches(v, 0.01, 1000000, faces=f, generator=g)   # noqa: E731
    cut()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p = cut()
    torch.cuda.synchronize()
    cut_s = time.perf_counter() - t0
    trainer = train.EmbeddingTrainer(seed=0, device=DEV)
    order = torch.randperm(len(p), generator=g, device=DEV)
    trainer.step(**p.batch(order[:100], generator=g))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = 0
    for s in range(0, len(p) - 99, 100):
        trainer.step(**p.batch(order[s:s + 100], generator=g))
        steps += 1
    torch.cuda.synchronize()
    epoch_s = time.perf_counter() - t0
    res = {"case": "cut_local_patches(synthetic.gt_mesh(step_px=1), voxel 0.01, 1M samples)", **p.stats,
           "cut_s": round(cut_s, 3), "epoch_steps": steps, "epoch_s": round(epoch_s, 3),
           "cut_over_epoch": round(cut_s / epoch_s, 4) if epoch_s > 0 else None}
    print(json.dumps(res), flush=True)
    out.append(res)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
