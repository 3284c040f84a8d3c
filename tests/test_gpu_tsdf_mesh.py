"""Dense marching cubes over the TSDF side volume on the GPU (csrc/mesh.hip k_tm_*, TSDFVolume.mesh_tensors /
get_mesh / get_point_cloud -- third_parties/fusion.py:302-341): bit for bit against the numpy restatement of
tests/test_tsdf_mesh_cpu.py, run-to-run determinism, geometry and topology on analytic spheres up to 512^3, the
workspace budget, and the F-score of the TSDF baseline on the synthetic pan scene."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
from test_tsdf_mesh_cpu import euler_characteristic, is_closed, restate_mesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def make_volume(shape, voxel=0.025, origin=(-0.6, 0.35, -1.1)):
    from bnv_fusion_amd.tsdf import TSDFVolume
    lo = np.asarray(origin, np.float64)
    vol = TSDFVolume(np.stack([lo, lo + (np.asarray(shape) - 0.5) * voxel], 1), voxel, device=DEV)
    assert tuple(int(v) for v in vol._vol_dim) == tuple(shape)
    return vol


def fill(vol, tsdf, weight=None, color=None):
    vol.tsdf.copy_(torch.from_numpy(np.ascontiguousarray(tsdf, F32)))
    if weight is not None:
        vol.weight.copy_(torch.from_numpy(np.ascontiguousarray(weight, F32)))
    if color is not None:
        vol.color.copy_(torch.from_numpy(np.ascontiguousarray(color, F32)))
    return vol


def folded_colors(shape, rng):
    """Random b * 65536 + g * 256 + r values, as TSDFVolume.integrate stores them (fusion.py:223-224)."""
    c = rng.integers(0, 256, size=tuple(shape) + (3,)).astype(np.float64)
    return (c[..., 2] * 65536 + c[..., 1] * 256 + c[..., 0]).astype(F32)


def sphere(shape, center, radius):
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return (np.sqrt((i - center[0]) ** 2 + (j - center[1]) ** 2 + (k - center[2]) ** 2) - radius).astype(F32)


def check_bitwise(vol, level=0.0, observed_only=False):
    from bnv_fusion_amd.mesh import to_host
    got = to_host(*vol.mesh_tensors(level, observed_only))
    ref = restate_mesh(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.color.cpu().numpy(), vol._vol_origin,
                       F32(vol._voxel_size), level, observed_only)
    names = ("vertices", "faces", "normals", "colors")
    for name, g, r in zip(names, got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, (name, g.dtype, g.shape, r.dtype, r.shape)
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), "vertices differ"
    assert np.array_equal(got[1], ref[1]), "faces differ"
    assert np.array_equal(got[3], ref[3]), "colors differ"
    if len(ref[2]):
        assert np.abs(got[2] - ref[2]).max() <= 1e-6, np.abs(got[2] - ref[2]).max()
    return got


@pytest.fixture(scope="module")
def pan_volume():
    """The TSDF of 20 synthetic pan frames at 2.5 cm in NeuralMap's TSDF extent (run_e2e.py:58-71), with seeded random
    colour images (the synthetic frames have none)."""
    from bnv_fusion_amd import synthetic
    from bnv_fusion_amd.sparse_volume import get_world_range
    from bnv_fusion_amd.tsdf import TSDFVolume
    dims, _ = synthetic.GRID_DIMS[256]
    mn, mx, _ = get_world_range(np.array([dims] * 3), 0.025)
    vol = TSDFVolume(np.stack([mn, mx], 1), 0.025, device=DEV)
    rng = np.random.default_rng(7)
    for t in range(20):
        rgb = rng.integers(0, 256, size=(480, 640, 3)).astype(np.float32)
        vol.integrate(rgb, synthetic.depth_image(t), synthetic.intrinsics(), synthetic.pose(t))
    torch.cuda.synchronize()
    return vol


# ---- bit for bit against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("observed_only", [False, True])
def test_sphere_with_holey_weights(observed_only):
    rng = np.random.default_rng(1)
    shape = (48, 40, 71)                       # Z = 71: tiles of 64 grid points straddle the rows
    w = rng.random(shape).astype(F32)
    w[w < 0.1] = 0
    vol = fill(make_volume(shape), sphere(shape, (22.7, 19.1, 35.4), 15.3), w, folded_colors(shape, rng))
    v, f, _, _ = check_bitwise(vol, 0.0, observed_only)
    assert len(f) > 1000


@pytest.mark.parametrize("observed_only", [False, True])
def test_uniform_noise_many_ambiguous_cells(observed_only):
    rng = np.random.default_rng(2)
    shape = (33, 70, 65)
    w = (rng.random(shape) > 0.05).astype(F32)
    vol = fill(make_volume(shape), rng.uniform(-1, 1, shape).astype(F32), w, folded_colors(shape, rng))
    _, f, _, _ = check_bitwise(vol, 0.1, observed_only)
    assert len(f) > 50000


@pytest.mark.parametrize("observed_only", [False, True])
def test_values_exactly_at_the_level(observed_only):
    rng = np.random.default_rng(3)
    shape = (30, 31, 64)
    tsdf = (rng.integers(-2, 3, size=shape) * 0.5).astype(F32)         # a third of the values equal a level below
    w = (rng.random(shape) > 0.2).astype(F32) * 3
    vol = fill(make_volume(shape), tsdf, w, folded_colors(shape, rng))
    for level in (0.0, 0.5, -0.5):
        check_bitwise(vol, level, observed_only)


@pytest.mark.parametrize("observed_only", [False, True])
def test_integrated_pan_frames(pan_volume, observed_only):
    _, f, _, c = check_bitwise(pan_volume, 0.0, observed_only)
    assert len(f) > 10000 and c.any()


@pytest.mark.parametrize("observed_only", [False, True])
def test_empty_and_degenerate_volumes(observed_only):
    rng = np.random.default_rng(4)
    cases = [(s, rng.uniform(-1, 1, s).astype(F32)) for s in ((1, 9, 9), (9, 1, 9), (9, 9, 1), (1, 1, 1))]
    cases += [((9, 10, 11), None), ((9, 10, 11), np.ones((9, 10, 11), F32))]   # all inside (-trunc_margin), outside
    for shape, tsdf in cases:
        vol = make_volume(shape)
        if tsdf is not None:
            fill(vol, tsdf, np.ones(shape, F32))
        v, f, n, c = vol.mesh_tensors(0.0, observed_only)
        assert (v.shape, f.shape, n.shape, c.shape) == ((0, 3),) * 4
        assert (v.dtype, f.dtype, n.dtype, c.dtype) == (torch.float32, torch.int64, torch.float32, torch.uint8)
        assert all(t.device == torch.device(DEV) for t in (v, f, n, c))
        hv, hf, hn, hc = vol.get_mesh(observed_only)
        assert (hv.dtype, hf.dtype, hn.dtype, hc.dtype) == (np.float32, np.int64, np.float32, np.uint8)
        assert hv.shape == (0, 3) and hf.shape == (0, 3)
        pc = vol.get_point_cloud(observed_only)
        assert pc.shape == (0, 6) and pc.dtype == np.float32
        check_bitwise(vol, 0.0, observed_only)


def test_determinism():
    rng = np.random.default_rng(5)
    shape = (40, 50, 60)
    vol = fill(make_volume(shape), rng.uniform(-1, 1, shape).astype(F32), (rng.random(shape) > 0.1).astype(F32),
               folded_colors(shape, rng))
    for obs in (False, True):
        a = [t.cpu() for t in vol.mesh_tensors(0.0, obs)]
        b = [t.cpu() for t in vol.mesh_tensors(0.0, obs)]
        for x, y in zip(a, b):
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


# ---- geometry --------------------------------------------------------------------------------------------------------
def _check_sphere(v_idx, faces, normals, center, radius, bound=0.02):
    d = v_idx - center
    r = np.linalg.norm(d, axis=1)
    assert np.abs(r - radius).max() <= bound, np.abs(r - radius).max()
    if normals is not None:
        assert (np.sum(normals * (d / r[:, None]), 1) >= 0.999).all()
    assert euler_characteristic(len(v_idx), faces) == 2
    assert is_closed(faces)


def test_sphere_geometry_and_topology():
    center, radius = np.array([31.37, 32.21, 30.83]), 20.0
    shape = (64, 64, 64)
    vol = fill(make_volume(shape, voxel=0.025, origin=(0.0, 0.0, 0.0)), sphere(shape, center, radius))
    v, f, n, c = vol.get_mesh()
    v_idx = v.astype(np.float64) / 0.025                   # back to index space (origin 0)
    _check_sphere(v_idx, f, n, center, radius)
    fn = np.cross(v_idx[f[:, 1]] - v_idx[f[:, 0]], v_idx[f[:, 2]] - v_idx[f[:, 0]])
    ok = np.linalg.norm(fn, axis=1) > 1e-3                  # non-degenerate: twice the area above 1e-3 voxel^2
    vn = n[f].astype(np.float64)                          # [T, 3 corners, 3]
    assert ok.mean() > 0.99
    assert (np.einsum("td,tcd->tc", fn[ok], vn[ok]) > 0).all()


@pytest.mark.parametrize("observed_only", [False, True])
def test_point_cloud_is_mesh_vertices_and_colors(observed_only):
    rng = np.random.default_rng(6)
    shape = (40, 41, 42)
    w = rng.random(shape).astype(F32)
    w[w < 0.2] = 0
    vol = fill(make_volume(shape), sphere(shape, (20.2, 19.7, 21.1), 12.9), w, folded_colors(shape, rng))
    v, _, _, c = vol.get_mesh(observed_only)
    pc = vol.get_point_cloud(observed_only)
    assert pc.dtype == np.float32 and np.array_equal(pc, np.hstack([v, c]))


def test_512_cubed_sphere_topology_and_workspace():
    shape = (512, 512, 512)
    center, radius = (255.3, 256.7, 254.9), 200.0
    vol = make_volume(shape, voxel=0.01, origin=(0.0, 0.0, 0.0))
    ar = torch.arange(512, dtype=torch.float32, device=DEV)
    vol.tsdf.copy_(torch.sqrt((ar[:, None, None] - center[0]) ** 2 + (ar[None, :, None] - center[1]) ** 2
                              + (ar[None, None, :] - center[2]) ** 2) - radius)
    vol.weight.fill_(1.0)
    vol.mesh_tensors(0.0, True)                           # warm: the table is on the device
    for obs in (False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = vol.mesh_tensors(0.0, obs)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        out_bytes = sum(t.numel() * t.element_size() for t in out)
        work = peak - base - out_bytes
        assert work <= 512 ** 3, f"workspace {work} B > 1 B per voxel"
        v, f = out[0].cpu().numpy(), out[1].cpu().numpy()
        del out
        _check_sphere(v.astype(np.float64) / F32(0.01), f, None, np.array(center), radius)


# ---- end to end: the TSDF baseline scored against the pan scene's ground truth ---------------------------------------
# Bars: the first MI355X measurement less 0.02 on each fraction.  20 frames, 2.5 cm, observed_only:
# 0.004/1.0000/0.004/0.9999/0.9999; without it the surface against unobserved space halves the precision:
# 0.202/0.4628/0.005/1.0000/0.6328.
PAN_BARS = {"accuracy": 0.98, "recall": 0.98, "F1": 0.98}


def test_pan_scene_tsdf_baseline_f_score(pan_volume):
    from bnv_fusion_amd import evaluate, synthetic
    gt, gt_common = synthetic.gt_mesh("union"), synthetic.gt_mesh("common")
    res = {}
    for obs in (False, True):
        v, f, _, _ = pan_volume.mesh_tensors(0.0, obs)
        res[obs] = evaluate.evaluate_meshes((v, f), gt, gt_recall=gt_common,
                                            generator=torch.Generator(device=DEV).manual_seed(0))
        print("pan scene TSDF baseline, observed_only", obs, evaluate.summary_line(res[obs]))
    assert res[True]["accuracy"] >= res[False]["accuracy"], res
    assert res[True]["accuracy"] >= PAN_BARS["accuracy"], res
    assert res[True]["recall"] >= PAN_BARS["recall"], res
    assert res[True]["F1"] >= PAN_BARS["F1"], res
