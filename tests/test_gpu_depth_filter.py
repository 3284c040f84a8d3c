"""The depth filter on the GPU (csrc/depth_filter.hip; include/bnv_fusion.h, "Depth filter"): bit for bit against the
numpy restatement of tests/depth_filter_restatement.py, the normals it is there for, and its way through NeuralMap
and the tracked fusion loop."""
import functools

import numpy as np
import pytest
import torch

import depth_filter_restatement as dfr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE, MAX_DEPTH = 0.5, 3.0


def as_device(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.astype(np.int32)).to(DEV).to(torch.uint16)
    return torch.from_numpy(np.array(a)).to(DEV)             # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def planted_image(H, W, dtype):
    """Room depth through the restated sensor (sweep frame 250 at H x W) with a planted 125 mm depth step down the
    right third, zeros, a pixel exactly at ``MAX_DEPTH`` and one above it; float32 also a NaN, +inf and -inf.
    -> (image, confidence map with four pixels below level 2), read-only."""
    _, mm, _ = dfr.room_frame(250, H, W)
    mm = mm.astype(np.int64)
    mm[:, W - max(W // 3, 1):] += 125
    mm = np.clip(mm, 0, 65535)
    flat = mm.reshape(-1)                               # (a view: the plants go into mm)
    n = H * W
    spots = [(k * n) // 11 for k in range(11)]          # 11 distinct pixels for n >= 11, spread over the image
    assert len(set(spots)) == 11
    flat[spots[0]] = 0
    flat[spots[1]] = 0
    flat[spots[2]] = 3000                               # == MAX_DEPTH: not valid
    flat[spots[3]] = 3500
    flat[spots[4]] = 65535
    if dtype == "u16":
        img = mm.astype(np.uint16)
    else:
        img = (mm.astype(np.float64) / 1000.0).astype(np.float32)
        f = img.reshape(-1)
        f[spots[5]], f[spots[6]], f[spots[7]], f[spots[8]] = np.nan, np.inf, -np.inf, -1.0
    conf = np.full((H, W), 2, np.uint8)
    c = conf.reshape(-1)
    c[spots[9]], c[spots[10]], c[n // 2], c[n - 1] = 1, 0, 1, 0
    img.setflags(write=False)
    conf.setflags(write=False)
    return img, conf


@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("radius", [1, 3, 4, 8])
@pytest.mark.parametrize("shape", [(3, 5), (13, 17), (37, 70)])
def test_bit_for_bit_against_restatement(shape, radius, dtype):
    """Smaller than a window, no multiple of the 32 x 8 tile, wider and taller than one tile."""
    from bnv_fusion_amd import frontend
    img, _ = planted_image(*shape, dtype)
    got = frontend.filter_depth(as_device(img), max_depth=MAX_DEPTH, radius=radius)
    ref = dfr.filter_depth(img, max_depth=MAX_DEPTH, radius=radius)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape and got.is_cuda
    got = got.cpu().numpy()
    assert (ref > 0).sum() >= shape[0] * shape[1] // 3 and np.isfinite(ref).all()
    assert got.tobytes() == ref.tobytes(), f"{(got.view(np.uint32) != ref.view(np.uint32)).sum()} pixels differ"


@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_bit_for_bit_with_a_confidence_gate_and_other_settings(dtype):
    from bnv_fusion_amd import frontend
    img, conf = planted_image(37, 70, dtype)
    kw = dict(max_depth=2.5, radius=4, sigma_depth=0.5 * dfr.DEFAULT_SIGMA_DEPTH, range_cut=2.0, conf_level=2)
    got = frontend.filter_depth(as_device(img)[None], conf=as_device(conf), **kw)         # [1, H, W] is taken too
    ref = dfr.filter_depth(img, conf=conf, **kw)
    assert tuple(got.shape) == (37, 70)
    assert got.cpu().numpy().tobytes() == ref.tobytes()
    assert (ref[conf < 2] == 0).all()
    ungated = frontend.filter_depth(as_device(img), **dict(kw, conf_level=0))
    assert ungated.cpu().numpy().tobytes() == dfr.filter_depth(img, **dict(kw, conf_level=0)).tobytes()
    assert ungated.cpu().numpy().tobytes() != ref.tobytes()


def test_float64_input_and_refusals():
    from bnv_fusion_amd import _lib, frontend
    img, conf = planted_image(13, 17, "f32")
    d64 = img.astype(np.float64)
    got = frontend.filter_depth(as_device(d64), max_depth=MAX_DEPTH)
    assert got.cpu().numpy().tobytes() == dfr.filter_depth(d64, max_depth=MAX_DEPTH).tobytes()
    with pytest.raises(_lib.BnvError):
        frontend.filter_depth(torch.from_numpy(np.array(img)))                          # a CPU tensor: no fallback
    with pytest.raises(_lib.BnvError):
        frontend.filter_depth(as_device(img), radius=9)
    with pytest.raises(_lib.BnvError):
        frontend.filter_depth(as_device(img), conf_level=1)                             # a level without a map
    with pytest.raises(_lib.BnvError):
        frontend.filter_depth(as_device(img).to(torch.int32))


def test_two_calls_give_identical_bits():
    from bnv_fusion_amd import frontend
    _, mm, _ = dfr.room_frame(250, 480, 640)
    d = as_device(mm)
    a = frontend.filter_depth(d, max_depth=MAX_DEPTH)
    b = frontend.filter_depth(d, max_depth=MAX_DEPTH)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_normals_of_a_sensor_frame_improve_by_half():
    """tests/test_depth_filter_cpu.py's claim on the kernel's own output, 480 x 640: the mean angle between the front
    end's Sobel normals and those of the clean depth is at most half of the raw image's after the filter."""
    from bnv_fusion_amd import frontend
    clean, mm, K = dfr.room_frame(250, 480, 640)
    got = frontend.filter_depth(as_device(mm), max_depth=MAX_DEPTH).cpu().numpy()
    assert got.tobytes() == dfr.filter_depth(mm, max_depth=MAX_DEPTH).tobytes()
    raw, filtered = dfr.mean_normal_error_deg(mm, clean, K), dfr.mean_normal_error_deg(got, clean, K)
    print(f"mean normal error: raw {raw:.2f} deg, filtered {filtered:.2f} deg")
    assert filtered <= 0.5 * raw


# ---- through NeuralMap: a 128^3 map at 2 cm (tests/test_gpu_track.py's recipe) -------------------------------------

@pytest.fixture(scope="module")
def model():
    import bnv_fusion_amd as bnv
    return bnv.load_pretrained(device=DEV, voxel_size=0.02)


@pytest.fixture(scope="module")
def frames():
    from bnv_fusion_amd import sequence
    out = list(sequence.sweep_frames([100, 104, 108], scale=SCALE, device=DEV))
    torch.cuda.synchronize()
    return out


def new_map(model, depth_filter=None):
    import bnv_fusion_amd as bnv
    return bnv.NeuralMap(np.array([2.54] * 3), 0.02, model, device=DEV, tsdf=True, depth_filter=depth_filter)


def volume_state(nm):
    from bnv_fusion_amd import sequence
    torch.cuda.synchronize()
    vol = nm.volume
    n = vol.num_rows()
    return (n, sequence.checksum(vol._row_coords[:n]), sequence.checksum(vol._features[:n]),
            sequence.checksum(vol._weights[:n]), sequence.checksum(nm.tsdf_vol.tsdf), sequence.checksum(nm.tsdf_vol.weight))


def test_integrate_filters_the_frame(model, frames):
    from bnv_fusion_amd import frontend
    f = frontend.DepthFilter()
    assert (f.radius, f.sigma_depth, f.range_cut) == (3, frontend.DEFAULT_SIGMA_DEPTH, 3.0)
    with pytest.raises(AttributeError):
        f.radius = 2
    fr = frames[0]
    with_filter, plain, raw = new_map(model, f), new_map(model), new_map(model)
    assert with_filter.depth_filter is f and plain.depth_filter is None
    c1 = with_filter.integrate(fr)
    applied = f.apply(fr, MAX_DEPTH)
    assert applied is not fr and applied["depth_filtered"] is True and applied["depth"].dtype == torch.float32
    assert "depth_filtered" not in fr and fr["depth"].dtype == torch.uint16              # the caller's frame is untouched
    assert applied["intr_mat"] is fr["intr_mat"] and applied["T_wc"] is fr["T_wc"]
    c2 = plain.integrate(applied)
    assert c1 is not None and torch.equal(c1, c2)
    assert volume_state(with_filter) == volume_state(plain)
    c3 = raw.integrate(fr)
    assert volume_state(raw) != volume_state(plain)                                      # the filter did something
    assert c3 is not None


def test_prepared_frame_is_not_filtered_twice(model, frames):
    from bnv_fusion_amd import frontend
    f = frontend.DepthFilter(radius=2)
    nm, other = new_map(model, f), new_map(model, f)
    fr = frames[1]
    p = nm.prepare_frame(fr)
    assert p is not fr and p["depth_filtered"] is True
    assert nm.prepare_frame(p) is p and f.apply(p, MAX_DEPTH) is p
    pts_only = {"input_pts": torch.zeros((1, 4, 6), device=DEV)}
    assert nm.prepare_frame(pts_only) is pts_only
    ref = frontend.filter_depth(fr["depth"], max_depth=MAX_DEPTH, radius=2)
    assert torch.equal(p["depth"].view(torch.int32), ref.view(torch.int32))
    c1, c2 = nm.integrate(p), other.integrate(fr)
    assert torch.equal(c1, c2) and volume_state(nm) == volume_state(other)
    assert torch.equal(p["depth"].view(torch.int32), ref.view(torch.int32))


def test_map_without_a_filter_is_unchanged(model, frames):
    a, b = new_map(model), new_map(model)
    fr = frames[2]
    assert a.prepare_frame(fr) is fr
    ca, cb = a.integrate(fr), b.integrate(dict(fr))
    assert torch.equal(ca, cb) and volume_state(a) == volume_state(b)


@pytest.mark.parametrize("frame_pipe", [True, False])
def test_async_gives_the_synchronous_bits(model, frames, frame_pipe):
    """inputs_resident=True promises that the caller's tensors are complete; the filtered image is made on the caller's
    stream inside the call, so the encode stream must still wait for it."""
    from bnv_fusion_amd import frontend
    f = frontend.DepthFilter()
    sync, pipe = new_map(model, f), new_map(model, f)
    ref = [sync.fuse_and_decode(fr) for fr in frames]
    pipe.inputs_resident, pipe.frame_pipe = True, frame_pipe
    handles = [pipe.fuse_and_decode_async(fr) for fr in frames]
    for (c_ref, s_ref), h in zip(ref, handles):
        c, s = h.result()
        assert c_ref is not None and torch.equal(c, c_ref)
        assert torch.equal(s.view(torch.int32), s_ref.view(torch.int32))
    assert volume_state(pipe) == volume_state(sync)
    assert all("depth_filtered" not in fr for fr in frames)
    # a frame the caller prepared a moment ago: its filter kernel may still be queued on the caller's stream
    prepared = new_map(model, f)
    prepared.inputs_resident, prepared.frame_pipe = True, frame_pipe
    handles = []
    for fr in frames:
        p = prepared.prepare_frame(fr)
        assert isinstance(p["depth_ready"], torch.cuda.Event)
        handles.append(prepared.fuse_and_decode_async(p))
    for (c_ref, s_ref), h in zip(ref, handles):
        c, s = h.result()
        assert torch.equal(c, c_ref) and torch.equal(s.view(torch.int32), s_ref.view(torch.int32))
    assert volume_state(prepared) == volume_state(sync)


def test_tracked_loop_with_and_without_the_filter(model):
    """The tracked fusion loop over a Kinect-noise scan of the room with drifting odometry, once with and once without
    the filter: every frame is fused and every pose is finite.  The trajectory errors are printed, not asserted."""
    from bnv_fusion_amd import evaluate, frontend, scan, sequence, tracking
    from test_gpu_track import FRAMES
    scanner = scan.MeshScanner(sequence.gt_mesh(SCALE), device=DEV)
    truth = np.stack([sequence.sweep_pose(t, SCALE) for t in FRAMES])
    scanned = list(scan.scan_frames(scanner, truth, sequence.intrinsics(480, 640), 480, 640, noise="kinect"))
    drifted = scan.drift_poses(truth, sigma_t=0.005, sigma_r=0.003, seed=0)
    for name, flt in (("raw", None), ("filtered", frontend.DepthFilter())):
        tracker = tracking.Tracker(new_map(model, flt), source="tsdf", model_size=(120, 160))
        fused = [tracker.integrate(dict(fr, T_wc=T)) for fr, T in zip(scanned, drifted)]
        torch.cuda.synchronize()
        err = evaluate.trajectory_errors(tracker.poses, truth)
        print(f"tracked loop, {name}: translation rmse {err['translation_rmse'] * 1e3:.2f} mm, rotation "
              f"{err['rotation_mean_deg']:.3f} deg, refused {tracker.failures} of {len(scanned)}: {tracker.statuses}")
        assert len(tracker.poses) == len(scanned) and all(c is not None and len(c) > 0 for c in fused)
        assert np.isfinite(np.stack(tracker.poses)).all()
