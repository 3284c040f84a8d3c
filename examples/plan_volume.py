"""Plan the fusion volume of a capture before fusing it: bounds, yaw and voxel size from the depth frames and poses
alone (bnv_fusion_amd/plan.py), printed as a table.

    python examples/plan_volume.py --data-dir DATA --scan-id scene3d/lounge                 # a sequence directory
    python examples/plan_volume.py --arkit --data-dir DATA --scan-id room --align-yaw 18    # an iPhone / iPad LiDAR capture
    python examples/plan_volume.py --mesh MESH.ply --frames 60 --noise kinect               # a mesh, scanned on the GPU
    python examples/plan_volume.py --data-dir DATA --scan-id SCAN --align manhattan         # a world with arbitrary axes
    python examples/plan_volume.py --sweep 24 --scale 0.5 --height 60 --width 80 --voxel-sizes 0.02 0.04 0.08

Neither ``pose/dimensions.txt`` nor ``export.obj`` is read.  The last line of the table is the recommended voxel size:
the smallest candidate whose per-frame mean number of points per voxel has min > 4 and mean >= 8, the rule of the
reference's README -- the figures ``SparseVolume.print_statistic`` prints after a full run, known before it.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data-dir")
    ap.add_argument("--scan-id")
    ap.add_argument("--arkit", action="store_true", help="--data-dir/--scan-id is a 3D Scanner app export")
    ap.add_argument("--confidence-level", type=int, default=2)
    ap.add_argument("--mesh", help="a PLY or OBJ file, scanned from an orbit with scan.scan_frames")
    ap.add_argument("--frames", type=int, default=60, help="--mesh: frames of the orbit")
    ap.add_argument("--noise", default=None, choices=["kinect"])
    ap.add_argument("--sweep", type=int, default=0, help="this many frames (every 30th time step) of the room sweep")
    ap.add_argument("--scale", type=float, default=1.0, help="--sweep: scene scale")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--skip-images", type=int, default=1)
    ap.add_argument("--voxel-sizes", type=float, nargs="+", default=[0.005, 0.01, 0.02, 0.04])
    ap.add_argument("--min-pts-in-grid", type=int, default=8)
    ap.add_argument("--max-depth", type=float, default=3.0)
    ap.add_argument("--bin-size", type=float, default=0.01)
    ap.add_argument("--trim", type=float, default=0.0, help="fraction of points ignored at each end of every direction")
    ap.add_argument("--margin", type=float, default=0.05)
    ap.add_argument("--align-yaw", type=int, help="try this many yaw angles in [0, 90) degrees about --up")
    ap.add_argument("--up", default="y", choices=["x", "y", "z"])
    ap.add_argument("--align", choices=["manhattan"],
                    help="manhattan: find the scene's own three axes and its vertical from the frames' normals (a world "
                         "that is the first camera's frame, or a capture's arbitrary one); not with --align-yaw")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()

    import bnv_fusion_amd as bnv
    bnv.configure_runtime()
    from bnv_fusion_amd import datasets, scan, sequence, synthetic

    if args.mesh:
        from bnv_fusion_amd.mesh import load_obj, load_ply
        mesh = (load_obj if args.mesh.lower().endswith(".obj") else load_ply)(args.mesh)
        lo, hi = mesh.vertices.min(0).astype(np.float64), mesh.vertices.max(0).astype(np.float64)
        half = float(np.linalg.norm(hi - lo)) / 2
        poses = scan.orbit_poses((lo + hi) / 2, 1.5 * half, args.frames, height=0.4 * half)
        frames = list(scan.scan_frames(scan.MeshScanner(mesh, device=args.device), poses,
                                       synthetic.intrinsics(args.height, args.width), args.height, args.width,
                                       noise=args.noise, max_depth=args.max_depth))
    elif args.sweep:
        frames = list(sequence.sweep_frames(range(0, 30 * args.sweep, 30), args.height, args.width, args.scale,
                                            device=args.device))
    elif not (args.data_dir and args.scan_id):
        ap.error("give --data-dir and --scan-id, --mesh, or --sweep")
    options = dict(bin_size=args.bin_size, trim=args.trim, margin=args.margin, align_yaw=args.align_yaw, up=args.up,
                   align=args.align)
    if args.mesh or args.sweep:
        plan = bnv.plan_volume(frames, voxel_sizes=args.voxel_sizes, min_pts_in_grid=args.min_pts_in_grid,
                               device=args.device, max_depth=args.max_depth, **options)
    else:
        # volume="plan": the loader runs pass 1 over its own frames and serves them aligned; the candidates are counted
        # in that frame
        from bnv_fusion_amd import plan as planning
        if args.arkit:
            data = datasets.ARKitDataset(args.data_dir, args.scan_id, confidence_level=args.confidence_level,
                                         max_depth=args.max_depth, skip_images=args.skip_images, device=args.device,
                                         volume="plan", plan_options=options)
        else:
            data = datasets.FusionInferenceDataset(args.data_dir, args.scan_id, skip_images=args.skip_images,
                                                   max_depth=args.max_depth, device=args.device, volume="plan",
                                                   plan_options=options)
        counter = planning.VolumePlanner(device=args.device, max_depth=args.max_depth)
        plan = planning.plan_from(data.extent, counter.count(data, args.voxel_sizes, args.min_pts_in_grid,
                                                             dimensions=data.dimensions, axis_align_mat=np.eye(4)),
                                  args.min_pts_in_grid)
    print(plan.table())
    print("axis_align_mat:")
    print(np.array2string(plan.axis_align_mat, precision=6, suppress_small=True))


if __name__ == "__main__":
    main()
