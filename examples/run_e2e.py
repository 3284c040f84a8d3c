"""The reference's end-to-end loop (src/run_e2e.py:196-293) on this package: local fusion of every frame of a
sequence directory, periodic global optimisation, mesh extraction, final artefacts.

    python examples/run_e2e.py --data-dir DATA --scan-id scene3d/lounge --out OUT          # the reference's layout
    python examples/run_e2e.py --synthetic 24 --out /tmp/bnv_demo                          # writes a synthetic scene first
    python examples/run_e2e.py ... --tsdf-mesh --eval-gt GT.ply                            # + the TSDF baseline, both scored
    python examples/run_e2e.py --arkit --data-dir DATA --scan-id room --tiny-cuda           # an iPhone / iPad LiDAR capture
    python examples/run_e2e.py --synthetic-arkit 24 --out /tmp/bnv_arkit                    # writes a synthetic one first
    python examples/run_e2e.py --sweep 60 --grid 256 --pose-drift 0.005 0.003 --track tsdf --no-optimize --out /tmp/trk
                                                    # drifting odometry, every frame aligned to the map before it is fused
    python examples/run_e2e.py --sweep 60 --grid 256 --odometry rgbd --track tsdf --no-optimize --out /tmp/odo
                                                    # no poses but the first: frame-to-frame odometry, then frame-to-model
    python examples/run_e2e.py ... --depth-filter                                           # smooth every depth image first
    python examples/run_e2e.py ... --plan-volume --plan-voxel-sizes 0.01 0.02 0.04         # extent and voxel size from the frames
    python examples/run_e2e.py ... --plan-volume --plan-align manhattan                    # ... in the scene's own axes
    python examples/run_e2e.py --sweep 600 --grid 512 --decode-frames --pipelined --no-optimize --out /tmp/sweep
                                                    # a moving-camera room sweep (bnv_fusion_amd/sequence.py), per-frame
                                                    # SDF decode of the touched voxels, two frames in flight

Frames are read from ``<data-dir>/<scan-id>/{depth/<i>.png, pose/T_wc_<i>.txt, pose/intr_mat_<i>.txt,
pose/dimensions.txt}`` (bnv_fusion_amd/datasets.py), the volume extent comes from ``dimensions.txt`` exactly as in
the reference; checkpoints default to the converted weights shipped with the package.  With ``--arkit`` they are read
from a *3D Scanner* app export (``depth_<n>.png``, ``conf_<n>.png``, ``frame_<n>.json``, ``export.obj``:
datasets.ARKitDataset, the reference's ``dataset=fusion_inference_dataset_arkit``); pixels whose depth confidence is
below ``--confidence-level`` become neither points nor training rays.  With ``--plan-volume`` neither
``dimensions.txt`` nor ``export.obj`` is read: the extent is planned from the frames (bnv_fusion_amd/plan.py), and
``--plan-voxel-sizes`` also chooses the voxel size among the given candidates.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bnv_fusion_amd as bnv                                   # noqa: E402
bnv.configure_runtime()                                       # optional: the package's hardware queue count
from bnv_fusion_amd import datasets, synthetic                # noqa: E402
from bnv_fusion_amd.mesh import (TriMesh, connected_components, connected_components_tensors,          # noqa: E402
                                 post_process_mesh, remove_small_components, remove_small_components_tensors, to_host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data-dir")
    ap.add_argument("--scan-id", default="synthetic/scene0")
    ap.add_argument("--synthetic", type=int, default=0, help="write this many synthetic 640x480 frames and use them")
    ap.add_argument("--out", required=True)
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--tiny-cuda", action="store_true", help="the reference's default tiny-cuda-nn checkpoint")
    ap.add_argument("--weights", metavar="PATH", help="embedding weights (.npz, e.g. examples/train_embedding.py's "
                    "last.npz; fp32 networks, or tiny-cuda-nn ones with --tiny-cuda) instead of the shipped checkpoint")
    ap.add_argument("--skip-images", type=int, default=1)
    ap.add_argument("--optim-interval", type=int, default=100)        # fusion_pointnet_model.yaml:48
    ap.add_argument("--mode", default="offline", choices=["demo", "offline"])
    ap.add_argument("--no-optimize", action="store_true")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--sweep", type=int, default=0, help="write this many frames of the moving-camera room sweep "
                                                          "(bnv_fusion_amd/sequence.py) and use them")
    ap.add_argument("--grid", type=int, default=512, choices=[256, 512], help="--sweep: volume of the sweep")
    ap.add_argument("--decode-frames", action="store_true",
                    help="decode the SDF lattice of every frame's touched voxels (the unit of the benchmark metric)")
    ap.add_argument("--pipelined", action="store_true",
                    help="with --decode-frames: two frames in flight (fuse_and_decode_async) instead of one "
                         "synchronous call per frame")
    ap.add_argument("--eval-gt", help="score the final mesh against this ground-truth mesh (PLY) and print the "
                                      "reference's summary line pred_gt/accuracy/gt_pred/recall/F1 at 2.5 cm")
    ap.add_argument("--tsdf-mesh", action="store_true",
                    help="also mesh the 2.5 cm TSDF side volume (observed cells only) into tsdf.ply; with --eval-gt "
                         "its summary line follows the neural mesh's: the TSDF baseline of the same run")
    ap.add_argument("--post-process", default="host", choices=["host", "gpu"],
                    help="where the written meshes are post-processed (merge close vertices, clean, smooth): the host "
                         "function or its device version (same output bit for bit)")
    ap.add_argument("--min-component-area", type=float, metavar="A",
                    help="remove connected components of the post-processed meshes whose surface is below A square "
                         "metres (the block the reference keeps commented out in o3d_helper.post_process_mesh, there "
                         "with 0.1), on either --post-process route; prints what the final mesh lost")
    ap.add_argument("--simplify", type=float, metavar="CELL",
                    help="simplify the final mesh on the GPU after post-processing and the component filter: one "
                         "vertex per grid cell of CELL metres, at its quadric position (mesh.simplify_mesh_gpu); "
                         "colours are computed on the simplified mesh")
    ap.add_argument("--arkit", action="store_true",
                    help="read --data-dir/--scan-id as an iPhone / iPad LiDAR capture (3D Scanner app, 'All Data')")
    ap.add_argument("--confidence-level", type=int, default=2,
                    help="--arkit: lowest ARKit depth confidence (0 / 1 / 2) a pixel needs to be fused and trained on")
    ap.add_argument("--synthetic-arkit", type=int, default=0,
                    help="write this many frames of a synthetic 256x192 LiDAR capture (flying pixels and outliers "
                         "marked confidence 0) and use them (implies --arkit)")
    ap.add_argument("--render", metavar="DIR",
                    help="after the run, render the map at every key frame's pose into DIR (16-bit PNGs, millimetres) "
                         "and print the mean depth errors against the observed frames")
    ap.add_argument("--track", choices=["neural", "tsdf"],
                    help="align every frame to the map built so far before fusing it (tracking.Tracker: frame-to-model "
                         "ICP against a render of the neural volume or of the TSDF side volume; the given poses serve "
                         "as odometry).  Off by default: poses are taken as given")
    ap.add_argument("--track-view", type=int, nargs=2, metavar=("H", "W"),
                    help="--track: size of the rendered model view (default: the frame's)")
    ap.add_argument("--odometry", choices=["rgbd"],
                    help="estimate the motion between consecutive frames from the frames themselves (odometry.RgbdOdometry: "
                         "joint photometric and depth alignment; depth only where the sequence has no colour images) "
                         "instead of reading it from the poses: only the first frame's pose is used.  With --track the "
                         "tracker predicts every pose from it; without, the chained motions are the poses.  Prints the "
                         "trajectory's errors against the sequence's own poses")
    ap.add_argument("--pose-drift", type=float, nargs=2, metavar=("SIGMA_T", "SIGMA_R"),
                    help="replace the poses by drifting odometry (scan.drift_poses: a random walk of SIGMA_T metres and "
                         "SIGMA_R radians per frame and axis, seed 0); the frames are held in memory.  With --track the "
                         "run fuses a second map from the drifted poses as they are and prints trajectory_errors (and, "
                         "with --eval-gt, the F-score) of both")
    ap.add_argument("--depth-filter", type=float, nargs="*", metavar="RADIUS SIGMA_DEPTH",
                    help="smooth every depth image on the GPU before fusion, tracking and optimisation "
                         "(frontend.DepthFilter: edge-preserving, range width SIGMA_DEPTH * z^2 metres).  Bare: radius 3 "
                         "and two disparity steps of the Kinect model at 1 m; or give both values.  Off by default")
    ap.add_argument("--color", action="store_true",
                    help="colour the final mesh from the sequence's colour images and write its vertex normals "
                         "(mesh.color_vertices; needs Pillow to decode them).  The synthetic sequences have none")
    ap.add_argument("--plan-volume", action="store_true",
                    help="place the volume from the frames themselves (plan.VolumePlanner: bounds of the valid depth "
                         "points plus a margin) instead of dimensions.txt / export.obj, and print the plan")
    ap.add_argument("--plan-voxel-sizes", type=float, nargs="+", metavar="V",
                    help="implies --plan-volume: count the per-frame points per voxel of these candidate sizes and use the "
                         "smallest with min > 4 and mean >= 8 (the reference README's rule) in place of --voxel-size")
    ap.add_argument("--plan-align", choices=["manhattan"],
                    help="implies --plan-volume: plan the volume in the scene's own axes, found from the frames' normals "
                         "(plan.ManhattanFrame), for a world whose axes are not the room's")
    args = ap.parse_args()
    args.plan_volume = args.plan_volume or bool(args.plan_voxel_sizes) or bool(args.plan_align)
    plan_options = {"align": args.plan_align} if args.plan_align else None
    if args.color and (args.synthetic or args.sweep or args.synthetic_arkit):
        sys.exit("--color: the sequences --synthetic, --sweep and --synthetic-arkit write hold depth only, there is no "
                 "colour image to take the colours from (a grey mesh is not written instead)")
    has_rgb = not (args.synthetic or args.sweep or args.synthetic_arkit)
    load_rgb = args.color or (bool(args.odometry) and has_rgb)
    depth_filter = None
    if args.depth_filter is not None:
        from bnv_fusion_amd import frontend
        if len(args.depth_filter) not in (0, 2):
            ap.error("--depth-filter takes no value or RADIUS SIGMA_DEPTH")
        if args.depth_filter and not (args.depth_filter[0].is_integer() and 1 <= args.depth_filter[0] <= 8):
            ap.error(f"--depth-filter: RADIUS must be an integer from 1 to 8, got {args.depth_filter[0]:g}")
        depth_filter = frontend.DepthFilter(*((int(args.depth_filter[0]), args.depth_filter[1])
                                              if args.depth_filter else ()))
    os.makedirs(args.out, exist_ok=True)
    dev = "cuda:0"

    if args.synthetic:
        args.data_dir = args.data_dir or os.path.join(args.out, "data")
        H, W = args.height, args.width
        dims = {0.01: 2.54, 0.02: 2.52}.get(args.voxel_size, 2.54)
        datasets.write_sequence(args.data_dir, args.scan_id,
                                [synthetic.depth_u16(t, H, W) for t in range(args.synthetic)],
                                synthetic.intrinsics(H, W), [synthetic.pose(t) for t in range(args.synthetic)],
                                [dims] * 3)
    if args.sweep:
        from bnv_fusion_amd import sequence
        args.data_dir = args.data_dir or os.path.join(args.out, "data")
        args.scan_id = "sweep/room"
        dims_m, args.voxel_size, scale = sequence.DIMS[args.grid]
        datasets.write_sequence(args.data_dir, args.scan_id,
                                (sequence.depth_u16(t, scale=scale, device=dev).cpu().numpy() for t in range(args.sweep)),
                                sequence.intrinsics(), (sequence.sweep_pose(t, scale) for t in range(args.sweep)),
                                [dims_m] * 3, filter_type=0, level=1)
    if args.synthetic_arkit:
        args.arkit = True
        args.data_dir = args.data_dir or os.path.join(args.out, "data")
        cap = synthetic.arkit_capture(args.synthetic_arkit, voxel_size=args.voxel_size)
        datasets.write_arkit_capture(args.data_dir, args.scan_id, cap["depths"], cap["confs"], cap["intrinsics"],
                                     cap["poses"], cap["dimensions"], center=cap["center"])
    if args.arkit:
        data = datasets.ARKitDataset(args.data_dir, args.scan_id, confidence_level=args.confidence_level,
                                     skip_images=args.skip_images, device=dev, load_rgb=load_rgb,
                                     volume="plan" if args.plan_volume else "file", plan_options=plan_options)
    else:
        data = datasets.FusionInferenceDataset(args.data_dir, args.scan_id, skip_images=args.skip_images, device=dev,
                                               load_rgb=load_rgb, volume="plan" if args.plan_volume else "file",
                                               plan_options=plan_options)
    plan = None
    if args.plan_volume:
        # the dataset planned its extent and serves aligned frames; the candidates are counted in that frame
        from bnv_fusion_amd import plan as planning
        counter = planning.VolumePlanner(device=dev, max_depth=data.max_depth)
        cands = counter.count(data, args.plan_voxel_sizes or [args.voxel_size], dimensions=data.dimensions,
                              axis_align_mat=np.eye(4))
        plan = planning.plan_from(data.extent, cands)
        print(plan.table())
        if args.plan_voxel_sizes:
            if plan.voxel_size is None:
                sys.exit("--plan-voxel-sizes: no candidate has min > 4 and mean >= 8 points per voxel; add larger sizes")
            args.voxel_size = plan.voxel_size
    model = bnv.load_pretrained(device=dev, voxel_size=args.voxel_size, tiny_cuda=args.tiny_cuda, path=args.weights)
    nm = bnv.NeuralMap(data.dimensions, args.voxel_size, model, capacity=1 << 20, device=dev, tsdf=True,
                       max_depth=data.max_depth, depth_filter=depth_filter)
    t_local = t_global = 0.0
    max_depth = data.max_depth
    truth = tracker = None
    if args.pose_drift:
        from bnv_fusion_amd import scan
        data = [fr for fr in data if not np.isnan(fr["T_wc"]).any()]
        truth = np.stack([np.asarray(fr["T_wc"], dtype=np.float64) for fr in data])
        drifted = scan.drift_poses(truth, args.pose_drift[0], args.pose_drift[1], seed=0)
        data = [dict(fr, T_wc=T) for fr, T in zip(data, drifted)]
    odo, odo_poses, given_poses = None, [], []
    if args.track:
        from bnv_fusion_amd import tracking
        tracker = tracking.Tracker(nm, source=args.track, model_size=args.track_view, odometry=args.odometry)
    elif args.odometry:
        from bnv_fusion_amd import odometry, tracking
        odo = odometry.RgbdOdometry(max_depth=data.max_depth)
    if args.decode_frames:
        # the per-frame loop of the benchmark metric: fuse + decode of the touched voxels, synchronous or pipelined
        from bnv_fusion_amd import sequence
        nm.volume.reset(100000)                  # the reference's initial capacity: the tables grow on demand
        # (prepare_frame: the key frames the optimiser reads later hold the filtered depth; the raw frame without one)
        st = sequence.run(nm, (nm.prepare_frame(fr) for fr in data), pipelined=args.pipelined, in_flight=2, checksums=False,
                          on_frame=lambda k, fr, c, s: nm.frames.append(fr))
        print(f"fused + decoded {st['frames']} frames ({st['empty_frames']} without a point inside the volume) at "
              f"{st['frames'] / st['seconds']:.1f} frames/s incl. file reading; {nm.volume.num_rows()} voxels")
        data = []
        t_local = st["seconds"]
    for idx, frame in enumerate(data):                                   # run_e2e.py:243-279
        t0 = time.perf_counter()
        frame = nm.prepare_frame(frame)             # --depth-filter: filtered once, for tracking, fusion and nm.frames
        if args.odometry and not np.isnan(frame["T_wc"]).any():
            given_poses.append(np.asarray(frame["T_wc"], dtype=np.float64))
        if odo is not None and not np.isnan(frame["T_wc"]).any():
            step = odo.step(frame)
            odo_poses.append(odo_poses[-1] @ tracking.rigid_inverse(step.T_wc) if odo_poses else given_poses[0])
            frame = dict(frame, T_wc=odo_poses[-1])
        if tracker is not None and not np.isnan(frame["T_wc"]).any():
            tracker.integrate(frame)
            frame = dict(frame, T_wc=tracker.poses[-1])              # the optimiser's rays start at the corrected pose
        else:
            nm.integrate(frame)
        torch.cuda.synchronize()
        t_local += time.perf_counter() - t0
        if np.isnan(frame["T_wc"]).any():
            continue
        nm.frames.append(frame)
        if args.mode == "demo" and not args.no_optimize and idx % args.optim_interval == 0:
            last = max(0, len(nm.frames) - args.optim_interval)
            n_iters = min(len(nm.frames), args.optim_interval) * args.skip_images
            t0 = time.perf_counter()
            nm.optimize(n_iters=n_iters, last_frame=last, ray_max_dist=max_depth)
            torch.cuda.synchronize()
            t_global += time.perf_counter() - t0
            if args.post_process == "gpu":
                mesh = nm.extract_mesh(post_process=0.005, min_component_area=args.min_component_area)
            else:
                mesh = nm.extract_mesh()
                mesh = None if mesh is None else post_process_mesh(mesh, surface_threshold=args.min_component_area)
            if mesh is not None:                                             # :277-280
                mesh.export(os.path.join(args.out, f"{idx}.ply"))
    mesh = nm.extract_mesh(os.path.join(args.out, "before_optim.ply"))   # :280-282
    if tracker is not None:
        print(f"tracking ({args.track}): {tracker.failures} of {len(tracker.poses)} frames refused by the aligner "
              "(fused with the predicted pose)")
    if args.odometry:
        from bnv_fusion_amd import evaluate
        runner = tracker.odometry if tracker is not None else odo
        e = evaluate.trajectory_errors(tracker.poses if tracker is not None else odo_poses, truth[:len(given_poses)]
                                       if truth is not None else given_poses)
        print(f"odometry (rgbd): {runner.failures} of {max(len(runner.statuses) - 1, 0)} pairs refused (the constant-velocity guess "
              f"stands in); trajectory against the sequence's poses: translation RMSE {e['translation_rmse'] * 1e3:.2f} "
              f"mm, mean rotation error {e['rotation_mean_deg']:.3f} deg over {e['n']} frames")
    if tracker is not None and truth is not None:
        compare_given_and_tracked(args, data, truth, tracker, mesh, model, nm, dev)
    steps = int(len(nm.frames) * args.skip_images) * (1 if args.mode == "demo" else 2)   # :283-284
    if not args.no_optimize:
        t0 = time.perf_counter()
        nm.optimize(n_iters=steps, last_frame=-1, ray_max_dist=max_depth)
        torch.cuda.synchronize()
        t_global += time.perf_counter() - t0
    print(f"speed on local fusion: {len(nm.frames) / max(t_local, 1e-9):.1f} fps"
          + ("" if args.no_optimize else f"; speed on global fusion: {steps / max(t_global, 1e-9):.1f} fps"))
    if args.post_process == "gpu":                                      # :291-294
        mesh = nm.extract_mesh(post_process=nm.voxel_size / 4)
    else:
        mesh = nm.extract_mesh()
        mesh = None if mesh is None else post_process_mesh(mesh, vertex_threshold=nm.voxel_size / 4)
    if mesh is not None and args.min_component_area is not None:
        # the same as extract_mesh(post_process=..., min_component_area=A) / post_process_mesh(surface_threshold=A),
        # in two steps: the figures below are about the components of the unfiltered mesh
        n_before = len(mesh.faces)
        if args.post_process == "gpu":                                   # one upload serves the statistics and the filter
            gv, gf = torch.from_numpy(mesh.vertices).to(dev), torch.from_numpy(mesh.faces).to(dev)
            areas = to_host(connected_components_tensors(gv, gf)[2])[0]
            mesh = TriMesh(*to_host(*remove_small_components_tensors(gv, gf, min_area=args.min_component_area)))
        else:
            _, _, areas = connected_components(mesh)
            mesh = remove_small_components(mesh, min_area=args.min_component_area)
        gone = areas < args.min_component_area
        share = f"{areas.max() / areas.sum():.4%}" if len(areas) and areas.sum() > 0 else "n/a"
        print(f"components: {len(areas)}, the largest holds {share} of the area; below "
              f"{args.min_component_area:g} m^2: {int(gone.sum())} components, {n_before - len(mesh.faces)} faces, "
              f"{areas[gone].sum():.6f} m^2 removed")
    if mesh is not None and args.simplify is not None:
        from bnv_fusion_amd.mesh import simplify_mesh_gpu
        n_v, n_f = len(mesh.vertices), len(mesh.faces)
        mesh = simplify_mesh_gpu(mesh, cell=args.simplify, device=dev)
        print(f"simplify ({args.simplify:g} m cells): {n_v} vertices / {n_f} faces -> {len(mesh.vertices)} / "
              f"{len(mesh.faces)}")
    if mesh is not None and args.color:
        from bnv_fusion_amd.mesh import color_vertices
        _, observed = color_vertices(mesh, nm.frames, max_depth=max_depth, device=dev)
        print(f"colour: {observed.mean():.2%} of {len(mesh.vertices)} vertices observed in {len(nm.frames)} frames")
    if mesh is not None:
        mesh.export(os.path.join(args.out, "final.ply"))
    nm.save(args.out, scan_id=args.scan_id.split("/")[-1])
    tsdf_mesh = None
    if args.tsdf_mesh:                                                   # fusion.py:323-341 + meshwrite (:366-399)
        from bnv_fusion_amd.tsdf import meshwrite
        tsdf_mesh = nm.tsdf_vol.mesh_tensors(observed_only=True)
        meshwrite(os.path.join(args.out, "tsdf.ply"), *to_host(*tsdf_mesh))
    if args.eval_gt and (mesh is not None or tsdf_mesh is not None):
        from bnv_fusion_amd import evaluate
        from bnv_fusion_amd.mesh import load_ply
        gt = load_ply(args.eval_gt)
        if plan is not None:        # the ground truth lives in the frames' world: bring it into the planned volume's
            gt = TriMesh(plan.apply_points(gt.vertices).astype(np.float32), gt.faces)
        if mesh is not None:
            res = evaluate.evaluate_meshes(mesh, gt, generator=torch.Generator(device=dev).manual_seed(0), device=dev)
            print(evaluate.summary_line(res))
        if tsdf_mesh is not None and len(tsdf_mesh[1]):
            res = evaluate.evaluate_meshes(tsdf_mesh[:2], gt, generator=torch.Generator(device=dev).manual_seed(0),
                                           device=dev)
            print(evaluate.summary_line(res), "(TSDF baseline)")
    if args.render:
        render_key_frames(nm, args.render, max_depth)
    print(f"{len(nm.frames)} frames, {nm.volume.num_rows()} voxels, "
          f"{0 if mesh is None else len(mesh.faces)} triangles -> {args.out}")


def compare_given_and_tracked(args, frames, truth, tracker, tracked_mesh, model, nm, dev):
    """--pose-drift with --track: the same frames fused once more with the drifted poses as they are; prints
    evaluate.trajectory_errors of both trajectories and, with --eval-gt, the F-score of both maps' meshes."""
    from bnv_fusion_amd import evaluate
    from bnv_fusion_amd.mesh import load_ply
    plain = bnv.NeuralMap(nm.dimensions, args.voxel_size, model, capacity=1 << 20, device=dev, tsdf=True,
                          max_depth=nm.max_depth, depth_filter=nm.depth_filter)
    for fr in frames:
        plain.integrate(fr)
    given = np.stack([fr["T_wc"] for fr in frames])
    for name, poses in (("given", given), ("tracked", np.stack(tracker.poses))):
        e = evaluate.trajectory_errors(poses, truth)
        print(f"trajectory ({name} poses): translation RMSE {e['translation_rmse'] * 1e3:.2f} mm, mean rotation error "
              f"{e['rotation_mean_deg']:.3f} deg over {e['n']} frames")
    if args.eval_gt:
        gt = load_ply(args.eval_gt)
        for name, m in (("given", plain.extract_mesh()), ("tracked", tracked_mesh)):
            if m is not None:
                res = evaluate.evaluate_meshes(m, gt, generator=torch.Generator(device=dev).manual_seed(0), device=dev)
                print(evaluate.summary_line(res), f"({name} poses, before optimisation)")


def render_key_frames(nm, out_dir, max_depth):
    """Renders the map at every key frame's pose, writes <frame_id>.png (uint16 mm) and prints the mean depth_errors
    against the observed depth (cut at max_depth like the fused frames)."""
    from bnv_fusion_amd import evaluate
    os.makedirs(out_dir, exist_ok=True)
    sums, counts = {}, {}
    for k, fr in enumerate(nm.frames):
        obs = fr["depth"]
        obs = obs.to(torch.float32) / 1000.0 if obs.dtype in (torch.uint16, torch.int16) else obs.to(torch.float32)
        obs = torch.where(obs < max_depth, obs, torch.zeros_like(obs))
        H, W = int(obs.shape[-2]), int(obs.shape[-1])
        depth, _ = nm.render(fr["T_wc"], fr["intr_mat"], H, W, normals=False)
        mm = torch.round(depth.double() * 1000.0).clamp(0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)
        datasets.write_png16(os.path.join(out_dir, f"{fr.get('frame_id', k)}.png"), mm)
        e = evaluate.depth_errors(depth, obs)
        for key, v in e.items():
            if not np.isnan(v):
                sums[key] = sums.get(key, 0.0) + v
                counts[key] = counts.get(key, 0) + 1
    if counts:
        print(f"rendered depth vs observed (mean over {counts.get('coverage', 0)} key frames): "
              + ", ".join(f"{key} {sums[key] / counts[key]:.4f}" for key in sums))
    else:
        print("rendered depth: no key frame with observed depth")


if __name__ == "__main__":
    main()
