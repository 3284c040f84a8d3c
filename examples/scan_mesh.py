"""Scan a triangle mesh into a depth sequence in the reference's layout, on the GPU.

    python examples/scan_mesh.py MESH.ply --out DATA_DIR --scan-id scans/chair --frames 200 --noise kinect
    python examples/run_e2e.py --data-dir DATA_DIR --scan-id scans/chair --out OUT \
        --eval-gt DATA_DIR/scans/chair/gt_mesh_visible.ply

MESH: a PLY or OBJ file.  --trajectory orbit (default): a circle around the mesh's box centre, radius --radius times
the box's half diagonal, --elevation of it above the centre, looking at the centre; or a text FILE of key poses, one
camera-to-world 4 x 4 matrix per line (16 numbers, row-major; +z forward, y down), interpolated to --frames poses.
Written under DATA_DIR/SCAN_ID: depth/ pose/ image/ as the reference's data sets have them (the mesh's box centre moved
to the origin), gt_mesh.ply, gt_mesh_visible.ply (the faces the frames saw: the ground truth for recall).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh")
    ap.add_argument("--out", required=True, help="data directory")
    ap.add_argument("--scan-id", required=True)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--trajectory", default="orbit", help="'orbit' or a file of key poses")
    ap.add_argument("--radius", type=float, default=1.5, help="orbit radius in half diagonals of the mesh's box")
    ap.add_argument("--elevation", type=float, default=0.4, help="orbit height above the centre, in half diagonals")
    ap.add_argument("--noise", default=None, choices=["kinect"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-depth", type=float, default=float("inf"))
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()

    import torch
    import bnv_fusion_amd as bnv
    bnv.configure_runtime()
    from bnv_fusion_amd import scan, synthetic
    from bnv_fusion_amd.mesh import load_obj, load_ply

    mesh = (load_obj if args.mesh.lower().endswith(".obj") else load_ply)(args.mesh)
    lo, hi = mesh.vertices.min(0).astype(np.float64), mesh.vertices.max(0).astype(np.float64)
    center, half = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2
    if args.trajectory == "orbit":
        poses = scan.orbit_poses(center, args.radius * half, args.frames, height=args.elevation * half)
    else:
        keys = np.loadtxt(args.trajectory).reshape(-1, 4, 4)
        poses = scan.interpolate_poses(keys, args.frames)
    scanner = scan.MeshScanner(mesh, device=args.device)
    K = synthetic.intrinsics(args.height, args.width)
    t0 = time.perf_counter()
    root = scan.write_scan(args.out, args.scan_id, scanner, poses, K, args.height, args.width, noise=args.noise,
                           seed=args.seed, max_depth=args.max_depth)
    torch.cuda.synchronize()
    seen = int((scanner.seen > 0).sum())
    print(f"{root}: {len(poses)} frames of {args.width} x {args.height} in {time.perf_counter() - t0:.1f} s (with the PNG "
          f"writes), {len(mesh.faces)} faces, {seen} of them seen, noise {args.noise}")


if __name__ == "__main__":
    main()
