"""ARKit captures (datasets.ARKitDataset / write_arkit_capture) on the host: the loader against values the reference's
FusionInferenceDatasetARKit produced (tests/golden/arkit_capture.npz, make_golden_arkit.py), the writer's round trip,
and the argument checks of the confidence-gated C entries.  CPU only."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

INVALID_ARGUMENT = -1       # BNV_ERR_INVALID_ARGUMENT (include/bnv_fusion.h)


def _golden():
    return np.load(os.path.join(GOLDEN, "arkit_capture.npz"))


def write_golden_capture(root):
    """The golden capture's files, byte for byte, under root/scan -> (data_dir, scan_id, npz)."""
    z = _golden()
    os.makedirs(os.path.join(root, "scan"), exist_ok=True)
    for f in z["files"]:
        with open(os.path.join(root, "scan", str(f)), "wb") as fh:
            fh.write(z["file:" + str(f)].tobytes())
    return str(root), "scan", z


def test_loader_matches_the_reference(tmp_path):
    from bnv_fusion_amd import datasets
    data_dir, scan, z = write_golden_capture(tmp_path)
    ds = datasets.ARKitDataset(data_dir, scan, confidence_level=int(z["conf_level"]), max_depth=float(z["max_depth"]),
                               device="cpu")
    assert [int(n) for n in ds.names] == list(z["order"])
    assert np.array_equal(ds.dimensions, z["dimensions"])
    assert np.array_equal(ds.axis_align_mat, z["axis_align_mat"])
    assert len(ds) == len(z["order"])
    for k in range(len(ds)):
        f = ds[k]
        assert f["depth"].dtype == torch.uint16 and f["conf"].dtype == torch.uint8
        assert f["conf_level"] == int(z["conf_level"]) and f["max_depth"] == float(z["max_depth"])
        assert np.array_equal(f["T_wc"], z["T_wc"][k]), k           # same float64 operations: equal, not just close
        assert np.array_equal(f["intr_mat"], z["intr_mat"][k]), k
        d = f["depth"].numpy().astype(np.float64) / 1000.0
        mask = (d > 0) & (d < f["max_depth"]) & (f["conf"].numpy() >= f["conf_level"])
        assert np.array_equal(mask, z["mask"][k]), k
        assert int(mask.sum()) == int(z["counts"][k])
    # the fixture exercises every part of the gate
    assert (z["mask"].sum() < z["mask"].size) and len(np.unique(ds[0]["conf"].numpy())) == 3


def test_key_frame_sampling_matches_the_reference_on_the_host(tmp_path):
    """optimize.key_frame_points with the confidence gate, sampled with the reference's seed: the golden's ray mask and
    3x3 neighbour masks (IterableInferenceDataset._sample_key_frame).  (tests/test_gpu_arkit.py repeats it on the
    device.)"""
    from bnv_fusion_amd import datasets
    from bnv_fusion_amd.optimize import key_frame_points, sample_key_frame
    data_dir, scan, z = write_golden_capture(tmp_path)
    f = datasets.ARKitDataset(data_dir, scan, device="cpu")[0]
    d = f["depth"].to(torch.float32) / 1000.0
    pts = key_frame_points(d, f["intr_mat"], f["T_wc"], float(z["max_depth"]), conf=f["conf"],
                           conf_level=f["conf_level"])
    g = torch.Generator().manual_seed(int(z["key_seed"]))
    rays = sample_key_frame(None, None, None, int(z["key_sampling"]), float(z["max_depth"]), g, points=pts)
    assert np.array_equal(rays["uv"][0].numpy(), z["key_uv"])
    assert np.array_equal(rays["mask"][0].numpy(), z["key_mask"])
    assert np.array_equal(rays["neighbor_masks"][0].numpy(), z["key_neighbor_masks"])
    # without the gate the mask differs (the fixture has low-confidence pixels among the sampled ones)
    ungated = key_frame_points(d, f["intr_mat"], f["T_wc"], float(z["max_depth"]))
    assert not torch.equal(ungated["mask"], pts["mask"])
    with pytest.raises(Exception, match="confidence"):
        key_frame_points(d, f["intr_mat"], f["T_wc"], 3.0, conf_level=2)


def test_writer_round_trip(tmp_path):
    from bnv_fusion_amd import datasets, synthetic
    rng = np.random.default_rng(0)
    H, W = 24, 32
    K = synthetic.intrinsics(H * 8, W * 8)
    K[:2] /= 8
    poses = [synthetic.pose(t) @ np.diag([1.0, 1.0, 1.0, 1.0]) for t in (0, 5)]
    poses[1][:3, 3] += [0.1, 0.2, -0.3]
    depths = [rng.integers(0, 4000, size=(H, W)).astype(np.uint16) for _ in poses]
    confs = [rng.integers(0, 3, size=(H, W)).astype(np.uint8) for _ in poses]
    center, dims = np.array([0.4, -1.25, 2.0]), np.array([3.1, 1.7, 2.3])
    datasets.write_arkit_capture(tmp_path, "cap", depths, confs, K, poses, dims, center=center)
    ds = datasets.ARKitDataset(tmp_path, "cap", confidence_level=1, device="cpu")
    assert len(ds) == 2
    assert np.allclose(ds.dimensions, dims, rtol=0, atol=1e-12)
    assert np.allclose(ds.axis_align_mat[:3, 3], -center, rtol=0, atol=1e-12)
    for k in range(2):
        f = ds[k]
        assert np.allclose(f["T_wc"], poses[k], rtol=0, atol=1e-12)
        assert np.allclose(f["intr_mat"], K, rtol=1e-14, atol=0)
        assert np.array_equal(f["depth"].numpy(), depths[k]) and np.array_equal(f["conf"].numpy(), confs[k])
        assert f["conf_level"] == 1
    # the JSON holds ARKit conventions: colour-resolution intrinsics, the un-aligned, un-flipped pose
    cam = json.load(open(os.path.join(tmp_path, "cap", "frame_1.json")))
    assert np.isclose(cam["intrinsics"][0], K[0, 0] * 7.5)
    raw = np.asarray(cam["cameraPoseARFrame"]).reshape(4, 4)
    assert np.allclose(raw[:3, 3], poses[1][:3, 3] + center)
    assert np.allclose(raw[:3, 1], -poses[1][:3, 1]) and np.allclose(raw[:3, 2], -poses[1][:3, 2])
    # downsampling: depth and confidence by the same nearest-neighbour rule, intrinsics scaled
    half = datasets.ARKitDataset(tmp_path, "cap", downsample_scale=0.5, device="cpu")[0]
    assert tuple(half["depth"].shape) == tuple(half["conf"].shape) == (H // 2, W // 2)
    assert np.array_equal(half["conf"].numpy(), confs[0][::2, ::2])
    assert np.array_equal(half["depth"].numpy(), depths[0][::2, ::2])
    assert np.allclose(half["intr_mat"][:2], K[:2] * 0.5)


def test_frames_are_in_numeric_order(tmp_path):
    from bnv_fusion_amd import datasets
    names = [10, 9, 100, 2, 11]
    z = np.zeros((4, 4), np.uint16)
    datasets.write_arkit_capture(tmp_path, "s", [z + i for i in range(5)], [z.astype(np.uint8)] * 5, np.eye(3),
                                 [np.eye(4)] * 5, [1.0, 1.0, 1.0], names=names)
    ds = datasets.ARKitDataset(tmp_path, "s", device="cpu")
    assert ds.names == ["2", "9", "10", "11", "100"]
    assert [int(ds[k]["depth"][0, 0]) for k in range(5)] == [3, 1, 0, 4, 2]
    assert datasets.ARKitDataset(tmp_path, "s", skip_images=2, device="cpu").names == ["2", "10", "100"]


def test_missing_files_are_named(tmp_path):
    from bnv_fusion_amd import datasets
    z = np.zeros((4, 4), np.uint16)
    root = datasets.write_arkit_capture(tmp_path, "s", [z, z], [z.astype(np.uint8)] * 2, np.eye(3), [np.eye(4)] * 2,
                                        [1.0, 1.0, 1.0], names=[3, 4])
    os.remove(os.path.join(root, "conf_4.png"))
    ds = datasets.ARKitDataset(tmp_path, "s", device="cpu")
    ds[0]
    with pytest.raises(FileNotFoundError, match="conf_4.png"):
        ds[1]
    os.remove(os.path.join(root, "export.obj"))
    with pytest.raises(FileNotFoundError, match="export.obj"):
        datasets.ARKitDataset(tmp_path, "s", device="cpu")


def test_obj_bounds_need_only_vertex_lines(tmp_path):
    from bnv_fusion_amd import datasets
    p = tmp_path / "m.obj"
    p.write_text("# comment\nv 1 2 3\nvn 0 0 1\nvt 0.5 0.5\nv -1 0.5 7 1.0\nv\t0 0 0\nf 1 2 3\n")
    v = datasets.read_obj_vertices(str(p))
    assert v.shape == (3, 3) and np.array_equal(v.max(0), [1, 2, 7]) and np.array_equal(v.min(0), [-1, 0, 0])


def _lib_loaded():
    from bnv_fusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib, _lib.load()


def test_gated_entries_refuse_a_level_without_a_map():
    """A null confidence map with conf_level > 0 is BNV_ERR_INVALID_ARGUMENT (checked before anything is launched, so
    no GPU is needed); so is a negative level."""
    _lib, lib = _lib_loaded()
    K = (C.c_double * 9)(*np.eye(3).reshape(-1))
    T = (C.c_double * 16)(*np.eye(4).reshape(-1))
    fake = C.c_void_p(256)
    for pad in (0, 1):
        for conf, level in ((None, 2), (None, 1), (fake, -1)):
            rc = lib.bnv_depth_to_points(fake, 0, 8, 8, K, T, 3.0, conf, level, pad, fake, 1 << 20, fake, fake, None)
            assert rc == INVALID_ARGUMENT, (pad, conf, level, rc)
    g = _lib.Grid()
    rc = lib.bnv_encode_begin_depth(fake, 0, 8, 8, K, T, 3.0, None, 2, C.byref(g), fake, 1 << 20, 64, fake, None)
    assert rc != 0      # (without bnv_init: BNV_ERR_NOT_INITIALISED comes first)
    assert lib.bnv_frame_begin_depth(None, 0, fake, 0, 8, 8, K, T, None, 2, None) == INVALID_ARGUMENT
