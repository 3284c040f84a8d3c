"""iPhone / iPad LiDAR captures on the device: the depth front end's confidence gate (csrc/frontend.hpp: conf_ok /
pixel_valid; the *_gated C entries) against the reference and against the ungated front end, the three depth paths of
NeuralMap with the gate, the optimiser's key frames, and what the gate buys on a capture with wrong depth."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FEAT_TOL = 1e-4     # per-voxel encoder features (as tests/test_gpu_parity.py)


@pytest.fixture(scope="module", params=["split_f16", "fp32_exact"])
def bnv(request):
    """The tests that run the MLPs run in both arithmetic modes (include/bnv_fusion.h)."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    import bnv_fusion_amd
    bnv_fusion_amd.set_mlp_mode(1 if request.param == "split_f16" else 0)
    yield bnv_fusion_amd
    bnv_fusion_amd.set_mlp_mode(1)


def _golden_dataset(tmp_path, **kw):
    from bnv_fusion_amd import datasets
    z = np.load(os.path.join(GOLDEN, "arkit_capture.npz"))
    os.makedirs(tmp_path / "scan", exist_ok=True)
    for f in z["files"]:
        (tmp_path / "scan" / str(f)).write_bytes(z["file:" + str(f)].tobytes())
    return datasets.ARKitDataset(str(tmp_path), "scan", confidence_level=int(z["conf_level"]),
                                 max_depth=float(z["max_depth"]), device=DEV, **kw), z


def _synthetic_dataset(tmp_path, n_frames, confidence_level=2, voxel_size=0.01):
    from bnv_fusion_amd import datasets, synthetic
    cap = synthetic.arkit_capture(n_frames, voxel_size=voxel_size)
    datasets.write_arkit_capture(str(tmp_path), "syn", cap["depths"], cap["confs"], cap["intrinsics"], cap["poses"],
                                 cap["dimensions"], center=cap["center"])
    return datasets.ARKitDataset(str(tmp_path), "syn", confidence_level=confidence_level, device=DEV), cap


def test_gated_front_end_matches_the_reference(tmp_path):
    """The masked world points of FusionInferenceDatasetARKit (tests/golden/arkit_capture.npz), bit for bit."""
    from bnv_fusion_amd.frontend import depth_to_input_pts
    ds, z = _golden_dataset(tmp_path)
    k = int(z["pts_frame"])
    f = ds[k]
    pts = depth_to_input_pts(f["depth"], f["intr_mat"], f["T_wc"], max_depth=f["max_depth"], conf=f["conf"],
                             conf_level=f["conf_level"])[0].cpu().numpy()
    assert pts.shape == (int(z["counts"][k]), 6)
    assert np.array_equal(pts[:, :3], z["pts_w"])
    for k in range(len(ds)):                        # the row count of every frame (count and emit kernels agree)
        f = ds[k]
        pts, n = depth_to_input_pts(f["depth"], f["intr_mat"], f["T_wc"], max_depth=f["max_depth"], conf=f["conf"],
                                    conf_level=f["conf_level"], compact=False)
        assert int(n.item()) == int(z["counts"][k])
        assert torch.isnan(pts[0, int(z["counts"][k]):]).all() and not torch.isnan(pts[0, :int(z["counts"][k])]).any()


def test_gate_removes_rows_and_keeps_the_normals(tmp_path):
    """Gated output = the ungated output with its rows filtered by conf, bit for bit, normals included (and the oracle's
    unchanged depth_to_input_pts filtered the same way: points within 1 ulp, 99.9 % of all values equal).  Zeroing the rejected pixels' depth instead
    changes the normals of their neighbours: the Sobel stencil reads the unmasked depth."""
    from bnv_fusion_amd.frontend import depth_to_input_pts
    from oracle import bnv_oracle as orc
    ds, _ = _synthetic_dataset(tmp_path, 2)
    for k in range(len(ds)):
        f = ds[k]
        d, conf, lvl, md = f["depth"], f["conf"], f["conf_level"], f["max_depth"]
        gated = depth_to_input_pts(d, f["intr_mat"], f["T_wc"], max_depth=md, conf=conf, conf_level=lvl)[0]
        ungated = depth_to_input_pts(d, f["intr_mat"], f["T_wc"], max_depth=md)[0]
        dm = d.double() / 1000.0
        valid = ((dm > 0) & (dm < md)).reshape(-1)
        keep = (conf.reshape(-1) >= lvl)[valid]
        assert 0 < int(keep.sum()) < int(keep.numel())
        assert torch.equal(gated, ungated[keep])
        # (the oracle's criterion as in test_gpu_parity: the same float64 operation order, at most 1 ulp apart)
        ref = orc.depth_to_input_pts(dm.cpu().numpy(), f["intr_mat"], f["T_wc"], max_depth=md).astype(np.float32)
        ref = ref[keep.cpu().numpy()]
        got = gated.cpu().numpy()
        assert got.shape == ref.shape
        ulp = np.abs(got[:, :3].view(np.int32).astype(np.int64) - ref[:, :3].view(np.int32).astype(np.int64)).max()
        exact = float(np.mean(got == ref))      # (normals at the corrupted bands are ill-conditioned: a few differ)
        assert exact > 0.999 and ulp <= 1, (exact, ulp, float(np.abs(got - ref).max()))
        # the wrong way: depth zeroed where conf is low (both in float64 metres)
        gated = depth_to_input_pts(dm, f["intr_mat"], f["T_wc"], max_depth=md, conf=conf, conf_level=lvl)[0]
        zeroed = torch.where(conf >= lvl, dm, torch.zeros_like(dm))
        z = depth_to_input_pts(zeroed, f["intr_mat"], f["T_wc"], max_depth=md)[0]
        assert z.shape == gated.shape and torch.equal(z[:, :3], gated[:, :3])
        rej = (conf < lvl) & (dm > 0) & (dm < md)
        near = torch.zeros_like(rej)
        near[1:] |= rej[:-1]
        near[:-1] |= rej[1:]
        near[:, 1:] |= rej[:, :-1]
        near[:, :-1] |= rej[:, 1:]
        kept_mask = ((conf >= lvl) & (dm > 0) & (dm < md)).reshape(-1)
        at_border = near.reshape(-1)[kept_mask]
        diff = (z[:, 3:] != gated[:, 3:]).any(dim=1)
        assert bool(at_border.any())
        assert float(diff[at_border].float().mean()) > 0.9     # next to a rejected pixel the normals differ
        assert not bool(diff[~at_border & ~_near_ring(near, kept_mask)].any())


def _near_ring(near, kept_mask):
    """Pixels within 2 of a rejected one (diagonal stencil taps): a kept pixel outside this ring reads no rejected
    depth, so its normal is the same either way."""
    r = near.clone()
    r[1:] |= near[:-1]
    r[:-1] |= near[1:]
    r[:, 1:] |= near[:, :-1]
    r[:, :-1] |= near[:, 1:]
    return r.reshape(-1)[kept_mask]


def _run_three_paths(bnv, frames, dims, voxel, tsdf=True):
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)
    out = []
    for path in ("points", "fused", "pipe"):
        nm = bnv.NeuralMap(np.asarray(dims), voxel, model, device=DEV, tsdf=tsdf)
        coords = []
        if path == "points":                      # depth_to_input_pts(conf=...) -> encode_pointcloud
            for f in frames:
                c, _ = nm.fuse_and_decode(f)
                coords.append(c)
        else:                                     # encode_depth_async(conf=...) / the C frame pipe
            nm.frame_pipe = path == "pipe"
            hs = [nm.fuse_and_decode_async(f) for f in frames]
            coords = [h.result()[0] for h in hs]
        torch.cuda.synchronize()
        out.append((nm, coords))
    return out


def _assert_same_maps(runs):
    (a, ca), *rest = runs
    n = a.volume.num_rows()
    for b, cb in rest:
        for x, y in zip(ca, cb):
            assert (x is None and y is None) or torch.equal(x, y)
        assert b.volume.num_rows() == n
        assert torch.equal(a.volume._row_coords[:n], b.volume._row_coords[:n])
        assert torch.equal(a.volume._weights[:n], b.volume._weights[:n])
        assert float((a.volume._features[:n] - b.volume._features[:n]).abs().max()) < FEAT_TOL
        assert np.allclose(a.volume.n_pts_list, b.volume.n_pts_list)
        assert torch.equal(a.tsdf_vol.tsdf, b.tsdf_vol.tsdf) and torch.equal(a.tsdf_vol.weight, b.tsdf_vol.weight)


def test_three_depth_paths_agree_with_the_gate(bnv, tmp_path):
    ds, cap = _synthetic_dataset(tmp_path, 8, voxel_size=0.02)
    frames = list(ds)
    runs = _run_three_paths(bnv, frames, ds.dimensions, 0.02)
    _assert_same_maps(runs)
    # and the gate did something: the ungated map differs
    plain = _run_three_paths(bnv, [{k: v for k, v in f.items() if k != "conf"} for f in frames[:2]], ds.dimensions,
                             0.02)[0][0]
    gated2 = _run_three_paths(bnv, frames[:2], ds.dimensions, 0.02)[0][0]
    assert plain.volume.n_pts_list != gated2.volume.n_pts_list


def test_no_gate_no_change(bnv, tmp_path):
    """conf=None, and conf_level=0 with any map, give the ungated entries' results bit for bit on all three paths."""
    ds, _ = _synthetic_dataset(tmp_path, 4, voxel_size=0.02)
    frames = list(ds)
    plain = [{k: v for k, v in f.items() if k not in ("conf", "conf_level")} for f in frames]
    level0 = [dict(f, conf_level=0) for f in frames]
    ref = _run_three_paths(bnv, plain, ds.dimensions, 0.02)
    got = _run_three_paths(bnv, level0, ds.dimensions, 0.02)
    for (a, ca), (b, cb) in zip(ref, got):
        n = a.volume.num_rows()
        assert b.volume.num_rows() == n
        for x, y in zip(ca, cb):
            assert (x is None and y is None) or torch.equal(x, y)
        for t in ("_row_coords", "_weights", "_features"):
            assert torch.equal(getattr(a.volume, t)[:n], getattr(b.volume, t)[:n]), t
    _assert_same_maps(ref)
    from bnv_fusion_amd.frontend import depth_to_input_pts
    f = frames[0]
    for compact in (True, False):
        x = depth_to_input_pts(f["depth"], f["intr_mat"], f["T_wc"], 3.0, compact=compact)
        y = depth_to_input_pts(f["depth"], f["intr_mat"], f["T_wc"], 3.0, compact=compact, conf=f["conf"],
                               conf_level=0)
        x, y = (x, y) if compact else (x[0], y[0])
        assert torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0))
    with pytest.raises(Exception):
        depth_to_input_pts(f["depth"], f["intr_mat"], f["T_wc"], 3.0, conf_level=2)     # a level without a map


def test_tsdf_side_fusion_ignores_the_gate(bnv, tmp_path):
    """The TSDF side volume sees the range-masked depth: the same with and without the gate on frames that keep an
    in-bounds point (all of these do)."""
    ds, _ = _synthetic_dataset(tmp_path, 3, voxel_size=0.02)
    frames = list(ds)
    model = bnv.load_pretrained(device=DEV, voxel_size=0.02)
    vols = []
    for fr in (frames, [{k: v for k, v in f.items() if k != "conf"} for f in frames]):
        for pipe in (False, True):
            nm = bnv.NeuralMap(np.asarray(ds.dimensions), 0.02, model, device=DEV, tsdf=True)
            nm.frame_pipe = pipe
            [h.result() for h in [nm.fuse_and_decode_async(f) for f in fr]]
            nm.integrate(fr[0])
            torch.cuda.synchronize()
            vols.append(nm.tsdf_vol)
    for v in vols[1:]:
        assert torch.equal(v.tsdf, vols[0].tsdf) and torch.equal(v.weight, vols[0].weight)


def test_key_frames_match_the_reference_and_the_cache_keeps_gates_apart(bnv, tmp_path):
    from bnv_fusion_amd.optimize import key_frame_points, sample_key_frame
    ds, z = _golden_dataset(tmp_path)
    f = ds[0]
    d = f["depth"].to(torch.float32) / 1000.0
    pts = key_frame_points(d, f["intr_mat"], f["T_wc"], float(z["max_depth"]), conf=f["conf"],
                           conf_level=f["conf_level"])
    g = torch.Generator().manual_seed(int(z["key_seed"]))
    rays = sample_key_frame(None, None, None, int(z["key_sampling"]), float(z["max_depth"]), g, points=pts)
    assert np.array_equal(rays["mask"][0].cpu().numpy(), z["key_mask"])
    assert np.array_equal(rays["neighbor_masks"][0].cpu().numpy(), z["key_neighbor_masks"])
    # NeuralMap.optimize's key-frame cache: the same frame dict, gated then ungated then gated again
    model = bnv.load_pretrained(device=DEV, voxel_size=0.02)
    nm = bnv.NeuralMap(np.asarray(ds.dimensions), 0.02, model, device=DEV)
    nm.integrate(f)
    nm.frames.append(f)
    cache = nm.__dict__.setdefault("_key_frame_points", {})

    def cached_mask():
        nm.optimize(1, sampling_size=256, train_ray_splits=256, generator=torch.Generator().manual_seed(0))
        return cache[id(f)][1]["mask"]

    gated = cached_mask()
    assert torch.equal(gated, pts["mask"])
    conf, f["conf"] = f["conf"], None
    ungated = cached_mask()
    assert not torch.equal(ungated, gated)
    f["conf"] = conf
    f["conf_level"] = 1
    lvl1 = cached_mask()
    assert not torch.equal(lvl1, gated) and not torch.equal(lvl1, ungated)
    f["conf_level"] = 2
    assert torch.equal(cached_mask(), gated)


def test_frame_parallel_and_sharded_maps_honour_the_gate(bnv, tmp_path):
    """The distributed drivers on one rank: the same map as NeuralMap with the gate."""
    import socket
    import torch.distributed as dist
    from bnv_fusion_amd.distributed import FrameParallelNeuralMap, ShardedNeuralMap
    ds, _ = _synthetic_dataset(tmp_path, 4, voxel_size=0.02)
    frames = list(ds)
    dims = np.asarray(ds.dimensions)
    model = bnv.load_pretrained(device=DEV, voxel_size=0.02)
    ref = bnv.NeuralMap(dims, 0.02, model, device=DEV, tsdf=True)
    want = [ref.fuse_and_decode(f) for f in frames]
    created = False
    if not dist.is_initialized():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
        created = True
    try:
        fp = FrameParallelNeuralMap(dims, 0.02, model, device=DEV, tsdf=True)
        got_fp = [h.result() for h in fp.process_stream([[f] for f in frames])]
        fp.flush()
        sh = ShardedNeuralMap(dims, 0.02, model, device=DEV, tsdf=True)
        got_sh = [sh.fuse_and_decode_async(f).result() for f in frames]
        sh.flush()
        torch.cuda.synchronize()
    finally:
        if created:
            dist.destroy_process_group()
    for (c0, s0), (c1, s1), (c2, s2) in zip(want, got_fp, got_sh):
        assert torch.equal(c0, c1) and torch.equal(s0, s1)
        assert torch.equal(c0, c2) and float((s0 - s2).abs().max()) < 1e-4
    assert np.allclose(fp.volume.n_pts_list, ref.volume.n_pts_list)


def _fuse_and_score(bnv, tmp_path, level, n_frames=16, voxel=0.02):
    from bnv_fusion_amd import evaluate, synthetic
    ds, cap = _synthetic_dataset(tmp_path / f"l{level}", n_frames, confidence_level=level, voxel_size=voxel)
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)
    nm = bnv.NeuralMap(np.asarray(ds.dimensions), voxel, model, capacity=1 << 20, device=DEV, tsdf=True)
    for f in ds:
        nm.integrate(f)
    mesh = nm.extract_mesh()
    assert mesh is not None
    gt = synthetic.gt_mesh("union", step_px=2.0)
    gt.vertices = (gt.vertices.astype(np.float64) + ds.axis_align_mat[:3, 3]).astype(np.float32)
    res = evaluate.evaluate_meshes(mesh, gt, generator=torch.Generator(device=DEV).manual_seed(0), device=DEV)
    # world positions of the injected outliers (in the loader's frame)
    outl = []
    for k, f in enumerate(ds):
        rc = cap["outliers"][k]
        d = f["depth"].double().cpu().numpy()[rc[:, 0], rc[:, 1]] / 1000.0
        K, T = f["intr_mat"], f["T_wc"]
        pc = np.stack([(rc[:, 1] - K[0, 2]) / K[0, 0] * d, (rc[:, 0] - K[1, 2]) / K[1, 1] * d, d], -1)
        outl.append(pc @ T[:3, :3].T + T[:3, 3])
    return nm, res, np.concatenate(outl)


def _off_surface(volume, center, limit=0.1):
    """Voxel rows whose lattice point lies more than ``limit`` (along camera 0's ray) off the synthetic scene's surface."""
    from bnv_fusion_amd import synthetic
    n = volume.num_rows()
    c = (volume._row_coords[:n].double().cpu().numpy() * volume.voxel_size
         + volume.min_coords.double().cpu().numpy())
    p = c + center - synthetic.pose(0)[:3, 3]                  # loader frame -> camera 0 (pose(0) has R = I)
    K = synthetic.INTRINSICS
    u = K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2]
    v = K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]
    return int((np.abs(p[:, 2] - synthetic.scene_depth0(u, v)) > limit).sum()), n


def test_gate_keeps_wrong_depth_out_of_the_map(bnv, tmp_path):
    """16 frames of synthetic.arkit_capture (bands of flying pixels 15-25 % in front of the surface and 1.5 % outliers
    0.2-0.5 m off it, all at confidence 0), fused with confidence_level 2 and with 0.

    One measured run (both MLP modes alike): the meshes, scored against synthetic.gt_mesh (shifted by the capture's
    axis_align_mat) at 2.5 cm, reach precision 1.0000 either way -- the mesh extraction (min_pts_in_grid, the SDF zero
    crossing) already drops these thin ghost surfaces -- and recall 0.40 gated / 0.49 ungated (the gate also drops the
    correct confidence-1 pixels next to the corrupted ones).  The MAP is where the gate shows: without it 18,276 of
    41,904 voxel rows lie more than 10 cm off the surface; with it 0 of 22,255, and no gated voxel within 2 cm of any
    of the 9,998 injected outliers.  So: gated mesh precision not below the ungated one, no gated voxel more than 10 cm
    off the surface or within 2 cm of an outlier, and at least 5,000 such voxels without the gate."""
    nm2, r2, outl = _fuse_and_score(bnv, tmp_path, 2)
    nm0, r0, _ = _fuse_and_score(bnv, tmp_path, 0)
    from bnv_fusion_amd import synthetic
    off2, n2 = _off_surface(nm2.volume, synthetic.ARKIT_CENTER)
    off0, n0 = _off_surface(nm0.volume, synthetic.ARKIT_CENTER)
    v = nm2.volume
    centres = v._row_coords[:n2].double().cpu() * v.voxel_size + v.min_coords.double().cpu()
    near_outlier = int((torch.cdist(torch.from_numpy(outl), centres).min(dim=1).values < 0.02).sum())
    print(f"precision@2.5cm gated {r2['accuracy']:.4f} ungated {r0['accuracy']:.4f}; recall gated {r2['recall']:.4f} "
          f"ungated {r0['recall']:.4f}; voxels >10 cm off the surface: gated {off2} of {n2}, ungated {off0} of {n0}; "
          f"outliers with a gated voxel within 2 cm: {near_outlier} of {len(outl)}")
    assert r2["accuracy"] >= r0["accuracy"]
    assert off2 == 0 and near_outlier == 0
    assert off0 >= 5000


def test_run_e2e_example_on_an_arkit_capture(tmp_path, monkeypatch, capsys):
    """examples/run_e2e.py --synthetic-arkit (writes a capture, then reads it with --arkit), both checkpoints, run
    in-process (no exec from a process that has initialised the GPU)."""
    import importlib.util
    import sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    spec = importlib.util.spec_from_file_location("run_e2e_example", os.path.join(root, "examples", "run_e2e.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for extra in ([], ["--tiny-cuda"]):
        out = tmp_path / ("out" + "".join(extra))
        monkeypatch.setattr(sys, "argv", ["run_e2e.py", "--synthetic-arkit", "8", "--out", str(out), "--voxel-size",
                                          "0.02", "--mode", "demo", "--optim-interval", "4"] + extra)
        try:
            mod.main()
        finally:
            import bnv_fusion_amd
            bnv_fusion_amd.set_mlp_mode(1)
        printed = capsys.readouterr().out
        assert "speed on local fusion" in printed and "speed on global fusion" in printed, printed
        assert (out / "final.ply").exists() and (out / "final.ply").stat().st_size > 10000
        assert (out / "data" / "synthetic" / "scene0" / "conf_7.png").exists()
