"""Timings of the point-cloud normals (bnv_fusion_amd/pointcloud.py, csrc/cloud.hip) on one GPU -> one JSON document.

    python tools/cloud_bench.py [--quick] [--json OUT]

Clouds: the valid points of synthetic.frame-like depth images of the pan scene at 640 x 480 (~300 k points) and at
1632 x 1224 (~2 M points).  Per cloud: estimate_normals for k = 8, 16, 32 (normals per second), and in the same run
nearest_neighbors of the same points against themselves and the encode of the same points (with the k = 16 normals),
each the median of 5 runs between HIP events after 2 warm-up runs.  --quick: 160 x 120 and 320 x 240."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bnv_fusion_amd as bnv  # noqa: E402

bnv.configure_runtime()
from bnv_fusion_amd import evaluate, synthetic  # noqa: E402

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


def cloud(H, W):
    """World points of the pan scene's clean depth at pose 0 (synthetic._clean_depth handles any image size)."""
    d = synthetic._clean_depth(0, H, W)
    K = synthetic.intrinsics(H, W)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pc = np.stack([(u - K[0, 2]) / K[0, 0] * d, (v - K[1, 2]) / K[1, 1] * d, d], -1).reshape(-1, 3)
    T = synthetic.pose(0)
    return torch.from_numpy((pc @ T[:3, :3].T + T[:3, 3]).astype(np.float32)).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sizes = [(120, 160), (240, 320)] if args.quick else [(480, 640), (1224, 1632)]
    origin = synthetic.pose(0)[:3, 3][None]
    dims, voxel = synthetic.GRID_DIMS[256]
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)
    vol = bnv.SparseVolume(8, voxel, np.array([dims] * 3), 8, device=DEV)
    out = {"device": torch.cuda.get_device_name(0), "clouds": []}
    for H, W in sizes:
        pts = cloud(H, W)
        n = int(pts.shape[0])
        row = {"points": n, "image": [H, W]}
        for k in (8, 16, 32):
            ms = timed(lambda: bnv.estimate_normals(pts, origin, k=k))
            row[f"normals_k{k}_ms"] = ms
            row[f"normals_k{k}_per_s"] = n / ms * 1e3
        rows, st = bnv.estimate_normals(pts, origin, k=16, return_stats=True)
        row["rejected_k16"] = int(st["status"][0])
        row["nearest_neighbors_ms"] = timed(lambda: evaluate.nn_d2(pts, pts))
        row["encode_ms"] = timed(lambda: model.encode_pointcloud_async(rows, vol.n_xyz, vol.min_coords, vol.max_coords,
                                                                      vol.voxel_size))
        out["clouds"].append(row)
        print(json.dumps(row))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
