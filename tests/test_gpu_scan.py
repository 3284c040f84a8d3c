"""Scanning a mesh into a depth sequence (bnv_fusion_amd/scan.py) end to end: the sequence on disk, the frames against
the analytic room, and fusion of scanned frames against fusion of analytic ones.

Millimetre counts.  ``scan_frames(noise=None, rounding="nearest")`` on ``sequence.gt_mesh()`` against
round(``sequence.render_depth`` * 1000) on frames 37, 195, 390, 777 and 1234 (frame 0 is left out here: 82 of its
pixels graze a box's top edge exactly and see either surface, 250 counts apart -- tests/test_mesh_ray_cpu.py): a depth
within a few fp32 ulp of a half millimetre rounds either way, so counts may differ by 1 and no more.  The float32 numpy
evaluation of the kernel's formulas (mesh_ray_restatement.woop) differs from the analytic counts at 55, 5, 0, 51 and 50
pixels of those frames, by 1 count each: 161 of 1,536,000 = 0.0105 %.  The kernel may differ at 4x that share, over the
five frames together: 0.0419 %.

Fusion.  Precision of the two reconstructions is estimated from n = 100,000 surface samples each, so the two figures
spread by sqrt(2 p (1 - p) / n) around the same value; three of those are allowed.
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNT_FRAMES = (37, 195, 390, 777, 1234)
COUNT_SHARE_FLOAT32 = 161 / (5 * 480 * 640)


def _room_scanner(scale=1.0):
    from bnv_fusion_amd import scan, sequence
    return scan.MeshScanner(sequence.gt_mesh(scale), device=DEV)


def test_write_scan_round_trips_through_the_dataset(tmp_path):
    from bnv_fusion_amd import datasets, scan, sequence
    from bnv_fusion_amd.mesh import load_ply
    sc = _room_scanner()
    K, H, W = sequence.intrinsics(120, 160), 120, 160
    poses = np.stack([sequence.sweep_pose(t) for t in (0, 40, 80, 120, 160)])
    frames = list(scan.scan_frames(sc, poses, K, H, W, noise="kinect", seed=3))
    root = scan.write_scan(str(tmp_path), "scans/room", sc, poses, K, H, W, noise="kinect", seed=3)
    data = datasets.FusionInferenceDataset(str(tmp_path), "scans/room", device=DEV)
    assert len(data) == len(poses)
    mesh = sequence.gt_mesh()
    lo, hi = mesh.vertices.astype(np.float64).min(0), mesh.vertices.astype(np.float64).max(0)
    assert np.allclose(data.dimensions, hi - lo, rtol=0, atol=0)
    for fr, ref, T in zip(data, frames, poses):
        assert fr["depth"].dtype == torch.uint16
        assert torch.equal(fr["depth"].cpu().to(torch.int32), ref["depth"].cpu().to(torch.int32))
        assert np.array_equal(fr["intr_mat"], K.astype(np.float32))
        shifted = T.copy()
        shifted[:3, 3] -= (lo + hi) / 2
        assert np.array_equal(fr["T_wc"], shifted.astype(np.float32))           # (the data set reads poses as fp32)
    assert set(frames[0]) == {"frame_id", "depth", "intr_mat", "T_wc"} and frames[0]["depth"].is_cuda
    gt, vis = load_ply(os.path.join(root, "gt_mesh.ply")), load_ply(os.path.join(root, "gt_mesh_visible.ply"))
    assert len(gt.faces) == len(mesh.faces) and 0 < len(vis.faces) < len(gt.faces)
    assert np.abs(gt.vertices.min(0) + gt.vertices.max(0)).max() < 1e-6           # recentred
    assert len(vis.faces) == int((sc.seen > 0).sum())


def test_clean_frames_against_the_analytic_room():
    from bnv_fusion_amd import scan, sequence
    sc = _room_scanner()
    K, H, W = sequence.intrinsics(), 480, 640
    poses = np.stack([sequence.sweep_pose(t) for t in COUNT_FRAMES])
    differing = 0
    for fr, t in zip(scan.scan_frames(sc, poses, K, H, W, noise=None, rounding="nearest"), COUNT_FRAMES):
        want = torch.round(sequence.render_depth(poses[fr["frame_id"]], K, H, W) * 1000.0).to(torch.int32)
        diff = (fr["depth"].cpu().to(torch.int32) - want).abs()
        print(f"\nframe {t}: {int((diff > 0).sum())} pixels differ, largest difference {int(diff.max())} count")
        assert int(diff.max()) <= 1
        differing += int((diff > 0).sum())
    share = differing / (len(COUNT_FRAMES) * H * W)
    print(f"share differing {100 * share:.4f} % (float32 numpy evaluation {100 * COUNT_SHARE_FLOAT32:.4f} %)")
    assert share <= 4 * COUNT_SHARE_FLOAT32
    # truncation, the reference's storage rule, never rounds up
    for fr in scan.scan_frames(sc, poses[:1], K, H, W):
        depth, _ = sc.render_depth(poses[0], K, H, W, count_seen=False)
        assert torch.equal(fr["depth"].to(torch.int32), torch.trunc(depth.double() * 1000).to(torch.int32))


def _fuse(frames, dims, voxel):
    import bnv_fusion_amd as bnv
    nm = bnv.NeuralMap(np.array([dims] * 3), voxel, bnv.load_pretrained(device=DEV, voxel_size=voxel), device=DEV)
    for fr in frames:
        nm.integrate(fr)
    return nm.extract_mesh()


def test_fusing_scanned_frames_equals_fusing_analytic_frames():
    from bnv_fusion_amd import evaluate, scan, sequence
    dims, voxel, scale = sequence.DIMS[256]
    K, H, W = sequence.intrinsics(), 480, 640
    times = list(range(0, 120, 15))
    poses = np.stack([sequence.sweep_pose(t, scale) for t in times])
    sc = _room_scanner(scale)
    scanned = list(scan.scan_frames(sc, poses, K, H, W, noise=None, rounding="nearest"))
    analytic = []
    for i, T in enumerate(poses):
        mm = torch.round(sequence.render_depth(T, K, H, W, scale) * 1000.0).to(torch.int32).to(torch.uint16)
        analytic.append({"frame_id": i, "depth": mm.to(DEV), "intr_mat": K, "T_wc": T})
    gt = sequence.gt_mesh(scale)
    n = 100000
    res = []
    for frames in (scanned, analytic):
        mesh = _fuse(frames, dims, voxel)
        res.append(evaluate.evaluate_meshes(mesh, gt, n_samples=n, gt_recall=sc.visible_mesh(),
                                            generator=torch.Generator(device=DEV).manual_seed(0)))
        res[-1]["recall_full"] = evaluate.evaluate_meshes(mesh, gt, n_samples=n,
                                                          generator=torch.Generator(device=DEV).manual_seed(0))["recall"]
    p = (res[0]["accuracy"] + res[1]["accuracy"]) / 2
    spread = math.sqrt(2 * p * (1 - p) / n)
    print(f"\nscanned: {evaluate.summary_line(res[0])}  analytic: {evaluate.summary_line(res[1])}  precision differs by "
          f"{abs(res[0]['accuracy'] - res[1]['accuracy']):.5f} (allowed {3 * spread:.5f}); recall against the visible "
          f"faces {res[0]['recall']:.4f}, against the whole mesh {res[0]['recall_full']:.4f}")
    assert abs(res[0]["accuracy"] - res[1]["accuracy"]) <= 3 * spread
    for r in res:
        assert r["recall"] >= r["recall_full"]
    assert 0 < len(sc.visible_mesh().faces) < len(gt.faces)


def test_kinect_noise_run_completes():
    """No bar: nothing exists to measure the sensor model's reconstruction against.  The precision is reported."""
    from bnv_fusion_amd import evaluate, scan, sequence
    dims, voxel, scale = sequence.DIMS[256]
    K, H, W = sequence.intrinsics(), 480, 640
    poses = np.stack([sequence.sweep_pose(t, scale) for t in range(0, 120, 15)])
    sc = _room_scanner(scale)
    frames = list(scan.scan_frames(sc, poses, K, H, W, noise="kinect", seed=1))
    assert all(f["depth"].dtype == torch.uint16 and f["depth"].shape == (H, W) for f in frames)
    mesh = _fuse(frames, dims, voxel)
    res = evaluate.evaluate_meshes(mesh, sequence.gt_mesh(scale), gt_recall=sc.visible_mesh(),
                                   generator=torch.Generator(device=DEV).manual_seed(0))
    print(f"\nkinect noise, 8 frames: {evaluate.summary_line(res)}")
    assert len(mesh.faces) > 0 and np.isfinite(res["accuracy"])


def test_trajectories():
    from bnv_fusion_amd import scan
    poses = scan.orbit_poses((0.3, -0.2, 0.4), 2.0, 12, height=0.5)
    assert poses.shape == (12, 4, 4)
    for T in poses:
        R = T[:3, :3]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0
        to_center = np.array([0.3, -0.2, 0.4]) - T[:3, 3]
        assert np.allclose(R[:, 2], to_center / np.linalg.norm(to_center), atol=1e-12)        # +z forward
        assert R[1, 1] > 0                                                                     # y down
        assert abs(T[1, 3] - (-0.2 - 0.5)) < 1e-12                                             # above: y is down
    mid = scan.interpolate_poses(poses[:3], 9)
    assert mid.shape == (9, 4, 4) and np.allclose(mid[0], poses[0]) and np.allclose(mid[4], poses[1]) and \
        np.allclose(mid[8], poses[2])
    for T in mid:
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12)
    assert np.allclose(mid[2][:3, 3], (poses[0][:3, 3] + poses[1][:3, 3]) / 2)
