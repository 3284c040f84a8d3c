"""Rendering the map on the GPU (csrc/render.hip; include/bnv_fusion.h, "Rendering"): bit-exact against the float32
restatement of tests/render_restatement.py whose field is the volume's own decode_pts, acceleration-invariant, and
geometrically right on the room sweep (against the analytic depth and against the mesh of the same state)."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, WEIGHTS_FP32
import render_restatement as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 120, 160
NEAR, MAX_DEPTH, STEP = 0.1, 3.0, 0.5


def small_map(tiny_cuda=False, mode=None, n_frames=12, tsdf=True):
    """A 128^3 map (2.54 m at 2 cm) of the half-size room sweep fused at 640 x 480 (rendered at 160 x 120)."""
    import bnv_fusion_amd as bnv
    from bnv_fusion_amd import sequence
    model = bnv.load_pretrained(device=DEV, voxel_size=0.02, tiny_cuda=tiny_cuda)
    if mode is not None:
        model.set_mlp_mode(mode)
    nm = bnv.NeuralMap(np.array([2.54] * 3), 0.02, model, device=DEV, tsdf=tsdf)
    for fr in sequence.sweep_frames(range(0, 4 * n_frames, 4), scale=0.5, device=DEV):
        nm.integrate(fr)
    torch.cuda.synchronize()
    return nm


def view(t=10, H=H, W=W):
    from bnv_fusion_amd import sequence
    return sequence.sweep_pose(t, 0.5), sequence.intrinsics(H, W)


def restate_neural(vol, nerf, T, K, delta=None, H=H, W=W, rays=None):
    """The restatement with vol.decode_pts as the field (or the rays listed in ``rays`` only)."""
    vol.to_tensor()
    occ = rr.occupancy(vol.active_coordinates, vol._n_xyz_host)
    bmin = vol.min_coords.cpu().numpy()
    lo, hi = rr.box(bmin, vol._n_xyz_host, vol.voxel_size)
    ray = rr.ray_setup(T, K, H, W, lo, hi, NEAR, MAX_DEPTH)
    if rays is not None:
        ray = {k: (v[rays] if v.dim() and v.shape[0] == H * W else v) for k, v in ray.items()}
    s = rr.f32(STEP) * rr.f32(vol.voxel_size)

    def field(p):
        with torch.no_grad():
            return vol.decode_pts(p.to(DEV).reshape(1, -1, 1, 3), nerf, delta).reshape(-1).cpu()
    depth, th, hit = rr.render(ray, s, field, rr.neural_domain(occ, bmin, vol.voxel_size))
    normals = rr.central_difference_normals(ray, th, hit, field, vol.voxel_size)
    return depth, normals, hit, ray


MODELS = [("fp32-default", False, None), ("fp32-exact", False, 0), ("tcnn", True, None)]


@pytest.fixture(scope="module", params=MODELS, ids=[m[0] for m in MODELS])
def model_map(request):
    _, tiny, mode = request.param
    return small_map(tiny, mode)


def test_render_matches_restatement(model_map):
    """Hit masks identical, depth equal to the bit, normals within 1e-5.  k_decode_pts evaluates every query on its
    own (an MFMA column per input, fixed reduction order), so a sample decodes to the same bits in the render's
    compacted buffer as in the restatement's batch."""
    nm = model_map
    vol, nerf = nm.volume, nm.pointnet.nerf
    delta = nm.prepare_tsdf_volume()
    for t in (10, 26):
        T, K = view(t)
        depth, normals = vol.render_depth(T, K, H, W, nerf, delta, near=NEAR, max_depth=MAX_DEPTH, step=STEP)
        rd, rn, hit, _ = restate_neural(vol, nerf, T, K, delta)
        got = depth.cpu().reshape(-1)
        print(f"{t}: {int(hit.sum())} hits, depth not bit-equal at {int((got != rd).sum())} pixels, max "
              f"{float((got - rd).abs().max()):.3g} m")
        assert hit.float().mean() > 0.05, "too few hits for the comparison to mean anything"
        nerr = float((normals.cpu().reshape(-1, 3) - rn).abs().max())
        st = vol.last_render_stats
        print(f"   normals max diff {nerr:.3g}, stats {st}")
        assert torch.equal(got > 0, hit), f"hit masks differ at {int(((got > 0) != hit).sum())} pixels"
        assert torch.equal(got, rd), f"depth differs at {int((got != rd).sum())} pixels"
        assert nerr <= 1e-5
        assert st["hits"] == int(hit.sum()) and st["rounds"] >= 1 and 0 < st["live_samples"] <= st["samples"]


def test_render_matches_oracle_field():
    """A few hundred rays end to end with the CPU checker's decode_pts as the field, on a checker volume holding
    the HIP volume's rows (exact-fp32 MLP mode: the checker is fp32)."""
    from oracle import bnv_oracle as orc
    nm = small_map(mode=0, tsdf=False)
    vol, nerf = nm.volume, nm.pointnet.nerf
    coords, feats, weights, hits = vol.to_tensor()
    ovol = orc.OracleSparseVolume(8, vol.voxel_size, vol.dimensions, vol.min_pts_in_grid)
    ovol.insert(coords.cpu(), feats.cpu(), weights.cpu(), hits.cpu())
    sd = orc.load_weights(WEIGHTS_FP32)
    T, K = view(10)
    depth, _ = vol.render_depth(T, K, H, W, nerf, near=NEAR, max_depth=MAX_DEPTH, step=STEP, normals=False)
    g = torch.Generator().manual_seed(0)
    rays = torch.randperm(H * W, generator=g)[:300]
    occ = rr.occupancy(coords, vol._n_xyz_host)
    bmin = vol.min_coords.cpu().numpy()
    lo, hi = rr.box(bmin, vol._n_xyz_host, vol.voxel_size)
    ray = rr.ray_setup(T, K, H, W, lo, hi, NEAR, MAX_DEPTH)
    ray = {k: (v[rays] if v.dim() and v.shape[0] == H * W else v) for k, v in ray.items()}

    def field(p):
        out = ovol.decode_pts(p.reshape(1, -1, 1, 3).float(), sd, None, query_tensor=False)
        return out.reshape(-1).float()
    od, _, ohit = rr.render(ray, rr.f32(STEP) * rr.f32(vol.voxel_size), field,
                            rr.neural_domain(occ, bmin, vol.voxel_size))
    got = depth.cpu().reshape(-1)[rays]
    assert int(ohit.sum()) > 100
    agree = (got > 0) == ohit
    assert float(agree.float().mean()) >= 0.99, f"hit masks agree on {float(agree.float().mean()):.3f}"
    both = (got > 0) & ohit
    assert float((got[both] - od[both]).abs().max()) <= 1e-4


def test_brick_and_hash_render_identically():
    import bnv_fusion_amd as bnv
    nm = small_map(tsdf=False)
    vol, nerf = nm.volume, nm.pointnet.nerf
    coords, feats, weights, hits = vol.to_tensor()
    other = bnv.SparseVolume(8, vol.voxel_size, vol.dimensions, vol.min_pts_in_grid, capacity=len(coords) + 1024,
                             device=DEV, brick=vol._brick is None)
    other.insert(coords, feats, weights, hits)
    assert (vol._brick is None) != (other._brick is None)
    T, K = view(18)
    a = vol.render_depth(T, K, H, W, nerf)
    b = other.render_depth(T, K, H, W, nerf)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float((a[0] > 0).float().mean()) > 0.05


# ---- geometry on the room sweep (256^3, 60 frames, as test_gpu_eval.test_room_sweep_precision) ----------------------

@pytest.fixture(scope="module")
def sweep_map():
    import bnv_fusion_amd as bnv
    from bnv_fusion_amd import sequence
    dims, voxel, scale = sequence.DIMS[256]
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)
    nm = bnv.NeuralMap(np.array([dims] * 3), voxel, model, device=DEV, tsdf=True)
    for fr in sequence.sweep_frames(range(0, 120, 2), scale=scale, device=DEV):
        nm.integrate(fr)
    torch.cuda.synchronize()
    return nm, scale


def analytic(T, K, Hh, Ww, scale):
    """(z-depth [H, W] f64, world points [H W, 3] f64, ray directions [H W, 3]) of the scene."""
    from bnv_fusion_amd import sequence
    z = sequence.render_depth(T, K, Hh, Ww, scale).double()
    u = torch.arange(Ww, dtype=torch.float64)[None, :].expand(Hh, Ww).reshape(-1)
    v = torch.arange(Hh, dtype=torch.float64)[:, None].expand(Hh, Ww).reshape(-1)
    xy1 = torch.stack([(u - K[0][2]) / K[0][0], (v - K[1][2]) / K[1][1], torch.ones_like(u)], 1)
    R, o = torch.from_numpy(np.asarray(T)[:3, :3]), torch.from_numpy(np.asarray(T)[:3, 3])
    dirs = xy1 @ R.T
    return z, o + z.reshape(-1, 1) * dirs, dirs


# angle of box-face normals to the nearest axis; first MI355X measurement: median 0.27 deg, p90 1.12 / 1.15 deg
NORMAL_MEDIAN_DEG, NORMAL_P90_DEG = 0.5, 2.0


@pytest.mark.parametrize("t", [40, 41], ids=["fused-pose", "held-out-pose"])
def test_sweep_geometry(sweep_map, t):
    from bnv_fusion_amd import sequence
    nm, scale = sweep_map
    Hh, Ww = 480, 640
    T, K = sequence.sweep_pose(t, scale), sequence.intrinsics(Hh, Ww)
    depth, normals = nm.render(T, K, Hh, Ww)
    z, pts, dirs = analytic(T, K, Hh, Ww, scale)
    d = depth.double().cpu().reshape(-1)
    zf = z.reshape(-1)
    hit = d > 0
    err = (d - zf).abs()
    within = float((err[hit] <= 0.025).double().mean())
    half = float(nm.volume.dimensions[0]) / 2
    inside = (pts.abs() <= half - 3 * nm.voxel_size).all(1) & (zf < nm.max_depth) & torch.isfinite(zf)
    coverage = float(hit[inside].double().mean())
    n = normals.cpu().double().reshape(-1, 3)[hit]
    facing = float(((n * dirs[hit]).sum(1) < 0).double().mean())
    # box faces are axis-aligned: angle to the nearest axis, on hits whose analytic point is well inside the volume
    sel = inside[hit]
    ang = torch.rad2deg(torch.acos(n[sel].abs().max(1).values.clamp(max=1.0)))
    med, p90 = float(ang.median()), float(torch.quantile(ang, 0.9))
    print(f"sweep t={t}: within 2.5 cm {within:.4f}, coverage {coverage:.4f}, facing {facing:.4f}, "
          f"normal angle median {med:.2f} p90 {p90:.2f} deg, stats {nm.volume.last_render_stats}")
    assert within >= 0.97          # first MI355X measurement: 0.9993 at both poses
    # first MI355X measurement: 0.985 / 0.984 (the mesh of the same state: 0.992 within a voxel).  Without the runs' lead-in samples (include/bnv_fusion.h, "Hit") coverage was 0.69: in 95 % of the missed rays the
    # first in-domain sample was already inside the surface while the mesh of the same state covered 99.2 % of these
    # pixels within a voxel.
    assert coverage >= 0.9
    assert facing >= 0.99          # first MI355X measurement: 0.998
    assert med <= NORMAL_MEDIAN_DEG and p90 <= NORMAL_P90_DEG


def test_render_consistent_with_mesh(sweep_map):
    """Back-projected hits lie on the mesh extract_mesh makes of the same state: >= 0.99 within half a voxel of
    dense surface samples."""
    from bnv_fusion_amd import evaluate, sequence
    nm, scale = sweep_map
    T, K = sequence.sweep_pose(40, scale), sequence.intrinsics(240, 320)
    depth, _ = nm.render(T, K, 240, 320, normals=False)
    mesh = nm.extract_mesh()
    samples = evaluate.sample_surface(mesh, n=2_000_000, generator=torch.Generator(device=DEV).manual_seed(0),
                                      device=DEV)
    if isinstance(samples, tuple):
        samples = samples[0]
    _, _, dirs = analytic(T, K, 240, 320, scale)
    d = depth.double().cpu().reshape(-1)
    hit = d > 0
    p = (torch.from_numpy(np.asarray(T)[:3, 3])[None, :] + d[hit, None] * dirs[hit]).float().to(DEV)
    dist, _ = evaluate.nearest_neighbors(p, samples.float())
    frac = float((dist <= 0.5 * nm.voxel_size).double().mean())
    print(f"render vs mesh: {frac:.4f} of {int(hit.sum())} hits within half a voxel")
    assert frac >= 0.99


# ---- TSDF side volume ---------------------------------------------------------------------------------------------

def test_tsdf_render_matches_restatement():
    nm = small_map(tsdf=True)
    tv = nm.tsdf_vol
    for t in (10, 26):
        T, K = view(t)
        depth, normals = tv.render_depth(T, K, H, W, near=NEAR, max_depth=MAX_DEPTH, step=STEP)
        tsdf, weight = tv.tsdf.cpu(), tv.weight.cpu()
        lo, hi = rr.box(tv._vol_origin, tv._vol_dim, tv._voxel_size)
        ray = rr.ray_setup(T, K, H, W, lo, hi, NEAR, MAX_DEPTH)
        dom, field = rr.tsdf_field(tsdf, weight, tv._vol_origin, tv._voxel_size)
        rd, th, hit = rr.render(ray, rr.f32(STEP) * rr.f32(tv._voxel_size), field, dom, lead_in=False)
        got = depth.cpu().reshape(-1)
        print(f"TSDF {t}: {int(hit.sum())} hits, depth not bit-equal at {int((got != rd).sum())} pixels, max "
              f"{float((got - rd).abs().max()):.3g} m")
        assert hit.float().mean() > 0.05
        assert torch.equal(got > 0, hit)
        assert torch.equal(got, rd), f"depth differs at {int((got != rd).sum())} pixels"
        rn = torch.zeros((H * W, 3))
        rn[hit] = rr.tsdf_normals(tsdf, tv._vol_origin, tv._voxel_size, rr.hit_points(ray, th)[hit])
        assert float((normals.cpu().reshape(-1, 3) - rn).abs().max()) <= 1e-5


def test_tsdf_render_sweep_geometry(sweep_map):
    from bnv_fusion_amd import sequence
    nm, scale = sweep_map
    T, K = sequence.sweep_pose(40, scale), sequence.intrinsics(240, 320)
    depth, _ = nm.render_tsdf(T, K, 240, 320)
    z, _, _ = analytic(T, K, 240, 320, scale)
    d = depth.double().cpu().reshape(-1)
    hit = d > 0
    within = float(((d - z.reshape(-1)).abs()[hit] <= 0.05).double().mean())
    print(f"TSDF sweep: within 5 cm {within:.4f} of {int(hit.sum())} hits")
    assert int(hit.sum()) > 0.3 * 240 * 320
    assert within >= 0.9          # 2.5 cm TSDF voxels: two voxels


# ---- edge cases ---------------------------------------------------------------------------------------------------

def test_empty_volume_and_outward_pose_render_zeros():
    import bnv_fusion_amd as bnv
    model = bnv.load_pretrained(device=DEV, voxel_size=0.02)
    vol = bnv.SparseVolume(8, 0.02, np.array([1.24] * 3), 8, device=DEV)
    T, K = view(10)
    d, n = vol.render_depth(T, K, H, W, model.nerf)
    assert float(d.abs().max()) == 0.0 and float(n.abs().max()) == 0.0
    nm = small_map(tsdf=False, n_frames=4)
    T = np.eye(4)
    T[:3, 3] = [0.0, 0.0, 5.0]                 # outside the volume, looking along +z away from it
    d, n = nm.volume.render_depth(T, K, H, W, nm.pointnet.nerf)
    assert float(d.abs().max()) == 0.0 and float(n.abs().max()) == 0.0


def test_invalid_arguments_raise():
    import bnv_fusion_amd as bnv
    nm = small_map(tsdf=True, n_frames=2)
    vol, nerf = nm.volume, nm.pointnet.nerf
    T, K = view(10)
    bad_T = T.copy()
    bad_T[0, 3] = float("nan")
    for args in [(T, K[:2], H, W), (T[:3], K, H, W), (bad_T, K, H, W), (T, K, 0, W), (T, K, H, -1)]:
        with pytest.raises(bnv.BnvError):
            vol.render_depth(*args, nerf)
        with pytest.raises(bnv.BnvError):
            nm.tsdf_vol.render_depth(*args)
    with pytest.raises(bnv.BnvError):
        vol.render_depth(T, K, H, W, nerf, step=0.0)
    with pytest.raises(bnv.BnvError):
        vol.render_depth(T, K, H, W, nerf, step=0.01)          # below BNV_RENDER_MIN_STEP
    d32, _ = vol.render_depth(T, K, H, W, nerf, step=np.float32(0.5), normals=False)
    assert torch.equal(d32, vol.render_depth(T, K, H, W, nerf, step=0.5, normals=False)[0])
    vol.shard = (0, 2, 3)
    try:
        with pytest.raises(NotImplementedError):
            vol.render_depth(T, K, H, W, nerf)
    finally:
        vol.shard = (0, 1, 3)


def test_render_reads_only_and_is_deterministic():
    from bnv_fusion_amd import sequence
    nm = small_map(tsdf=True, n_frames=6)
    vol = nm.volume
    n = vol.num_rows()
    before = (sequence.checksum(vol._features[:n]), sequence.checksum(vol._weights[:n]), n)
    T, K = view(10)
    a = nm.render(T, K, H, W)
    b = nm.render(T, K, H, W)
    n2 = vol.num_rows()
    assert (sequence.checksum(vol._features[:n2]), sequence.checksum(vol._weights[:n2]), n2) == before
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_render_between_pipelined_frames_changes_nothing():
    import bnv_fusion_amd as bnv
    from bnv_fusion_amd import sequence

    def run(render):
        model = bnv.load_pretrained(device=DEV, voxel_size=0.02)
        nm = bnv.NeuralMap(np.array([2.54] * 3), 0.02, model, device=DEV, tsdf=True)
        outs, handles = [], []
        for k, fr in enumerate(sequence.sweep_frames(range(0, 40, 4), H=H, W=W, scale=0.5, device=DEV)):
            handles.append(nm.fuse_and_decode_async(fr))
            if render and k % 3 == 1:
                T, K = view(4 * k)
                nm.render(T, K, H, W)
        for h in handles:
            c, s = h.result()
            outs.append((None if c is None else c.clone(), None if s is None else s.clone()))
        torch.cuda.synchronize()
        return outs

    plain, rendered = run(False), run(True)
    for (c0, s0), (c1, s1) in zip(plain, rendered):
        assert (c0 is None) == (c1 is None)
        if c0 is not None:
            assert torch.equal(c0, c1) and torch.equal(s0, s1)
