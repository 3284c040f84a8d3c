"""Fuse a point cloud that comes without normals -- a LiDAR scan, an exported cloud, a PLY of points -- into a mesh.

    python examples/fuse_cloud.py CLOUD.ply --origin 0 0 0 --voxel 0.02 --out mesh.ply
    python examples/fuse_cloud.py CLOUD.ply --origins stations.txt --origin-index index.txt --out mesh.ply
    python examples/fuse_cloud.py --stations stations.txt --register --out mesh.ply
    python examples/fuse_cloud.py --synthetic --out mesh.ply

CLOUD.ply: vertices only are read (bnv_fusion_amd.load_cloud); with ``nx ny nz`` in the file those normals are used
as they are, unless --estimate is given.  Sensor positions: --origin X Y Z (one station), or --origins FILE with one
"x y z" per line and --origin-index FILE with one station number per point.  --stations FILE: a multi-station scan,
one line per station: a PLY in the station's own frame and the 16 numbers of its row-major 4x4 pose (station ->
common frame); the sensor sits at each station's origin.  With --register the poses are only rough: the scans are
aligned to each other first (pointcloud.align_scans: every scan to the union of those before it) and fused at the
aligned poses.  --synthetic: a four-station scan of a
box (scan.scan_cloud) instead of a file.  The volume is a cube around the cloud's box (--size to override) centred
on the cloud, which is shifted to the origin for fusion and back for the mesh.  --voxel and --min-pts have to suit
the cloud's density: a voxel with fewer than --min-pts points is not encoded."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cloud", nargs="?")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--origin", type=float, nargs=3, default=None)
    ap.add_argument("--origins", default=None, help="file: one sensor position per line")
    ap.add_argument("--origin-index", default=None, help="file: one station number per point")
    ap.add_argument("--stations", default=None, help="file: per line a PLY (relative to the file) and its 4x4 pose")
    ap.add_argument("--register", action="store_true", help="with --stations: align the scans to each other first")
    ap.add_argument("--estimate", action="store_true", help="estimate normals even if the file has them")
    ap.add_argument("-k", type=int, default=16)
    ap.add_argument("--max-radius", type=float, default=None)
    ap.add_argument("--min-neighbors", type=int, default=6)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--min-pts", type=int, default=2)
    ap.add_argument("--size", type=float, default=None, help="edge of the fusion volume in metres")
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()

    import torch
    import bnv_fusion_amd as bnv
    bnv.configure_runtime()
    from bnv_fusion_amd import scan, sequence
    dev = args.device

    normals = origin_index = None
    if args.synthetic:
        v, f = sequence._box_faces([-0.4, -0.3, -0.5], [0.4, 0.3, 0.5])
        scanner = scan.MeshScanner(bnv.TriMesh(v, f), device=dev)
        poses = scan.orbit_poses([0.0, 0.0, 0.0], 2.0, 4, height=0.7)
        K = np.array([[300.0, 0.0, 159.5], [0.0, 300.0, 119.5], [0.0, 0.0, 1.0]])
        points, origins, origin_index = scan.scan_cloud(scanner, poses, K, 240, 320)
    elif args.stations:
        from bnv_fusion_amd import register
        scans, poses = [], []
        with open(args.stations) as fh:
            for line in filter(None, (ln.split("#")[0].split() for ln in fh)):
                if len(line) != 17:
                    ap.error(f"--stations: expected 'SCAN.ply' and 16 numbers per line, got {len(line)} fields")
                path = os.path.join(os.path.dirname(os.path.abspath(args.stations)), line[0])
                scans.append(torch.from_numpy(bnv.load_cloud(path)[0]).to(dev))
                poses.append(np.array(line[1:], dtype=np.float64).reshape(4, 4))
        poses = np.stack(poses)
        if args.register:
            poses, statuses = bnv.align_scans(scans, poses)
            print("stations registered one after the other: " +
                  ", ".join(register.STATUS_NAMES.get(s, str(s)) for s in statuses))
        points = torch.cat([register.transform_points(T, s) for T, s in zip(poses, scans)])
        origins = poses[:, :3, 3].copy()
        origin_index = torch.cat([torch.full((len(s),), i, dtype=torch.int32, device=dev) for i, s in enumerate(scans)])
    else:
        if not args.cloud:
            ap.error("a PLY file, --stations, or --synthetic")
        pts, normals = bnv.load_cloud(args.cloud)
        points = torch.from_numpy(pts).to(dev)
        if args.origins:
            origins = np.loadtxt(args.origins, dtype=np.float64).reshape(-1, 3)
            if args.origin_index:
                origin_index = torch.from_numpy(np.loadtxt(args.origin_index, dtype=np.int64).astype(np.int32)).to(dev)
        elif args.origin is not None:
            origins = np.array([args.origin], dtype=np.float64)
        elif normals is None or args.estimate:
            ap.error("normals are oriented from sensor positions: give --origin or --origins")
        else:
            origins = None

    finite = torch.isfinite(points).all(1)
    lo, hi = points[finite].min(0).values.cpu().numpy(), points[finite].max(0).values.cpu().numpy()
    center = ((lo.astype(np.float64) + hi) / 2).astype(np.float32)
    size = args.size if args.size is not None else float((hi - lo).max()) + 8 * args.voxel
    shifted = points - torch.from_numpy(center).to(dev)
    model = bnv.load_pretrained(device=dev, voxel_size=args.voxel, min_pts_in_grid=args.min_pts)
    nm = bnv.NeuralMap(np.array([size] * 3), args.voxel, model, min_pts_in_grid=args.min_pts, device=dev)
    if normals is not None and not args.estimate:
        rows = torch.cat([shifted, torch.from_numpy(normals).to(dev)], 1)[None]
        for s, e in bnv.pointcloud.cloud_chunks(rows.shape[1]):
            nm.integrate({"input_pts": rows[:, s:e]})
        print(f"{rows.shape[1]} points with the file's normals")
    else:
        org = np.asarray(origins, dtype=np.float64) - center.astype(np.float64)
        rows, st = bnv.estimate_normals(shifted, org, origin_index, k=args.k, max_radius=args.max_radius,
                                        min_neighbors=args.min_neighbors, return_stats=True)
        for s, e in bnv.pointcloud.cloud_chunks(rows.shape[1]):
            nm.integrate({"input_pts": rows[:, s:e]})
        status = st["status"].cpu().numpy()
        print(f"{rows.shape[1]} points, {len(org)} station(s): {int(status[0])} rows rejected, {int(status[1])} bad "
              f"origin indices")
    mesh = nm.extract_mesh(post_process=args.voxel / 4)
    if mesh is None:
        sys.exit("nothing to mesh: no voxel holds --min-pts points (a larger --voxel or a smaller --min-pts?)")
    mesh.vertices = (mesh.vertices.astype(np.float64) + center.astype(np.float64)).astype(np.float32)
    mesh.export(args.out)
    print(f"{args.out}: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces")


if __name__ == "__main__":
    main()
