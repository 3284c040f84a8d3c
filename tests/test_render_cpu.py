"""The render semantics (include/bnv_fusion.h, "Rendering") restated in float32 (tests/render_restatement.py) on
analytic fields -- they pin the pixel and z-depth conventions, the schedule's accuracy and the domain rule -- and
evaluate.depth_errors on constructed tensors.  CPU only."""
import math

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
import render_restatement as rr

H, W = 24, 32
K = np.array([[30.0, 0.0, 15.5], [0.0, 30.0, 11.5], [0.0, 0.0, 1.0]])
STEP = np.float32(0.005)
LO, HI = rr.box([-2.0, -2.0, -2.0], [401] * 3, 0.01)      # a 4 m cube of 1 cm voxels around the camera


def pose(yaw_deg=0.0, t=(0.0, 0.0, 0.0)):
    a = math.radians(yaw_deg)
    T = np.eye(4)
    T[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
    T[:3, 3] = t
    return T


def everywhere(p):
    return torch.ones(p.shape[0], dtype=torch.bool)


def test_plane_depth_is_exact():
    """f = z0 - z: linear along every ray, so interpolation is exact and z-depth is z0 to float32 precision at every
    pixel -- pixel centres at integer (u, v), z-depth (not range) as the output."""
    z0 = 1.3
    ray = rr.ray_setup(pose(), K, H, W, LO, HI, 0.1, 3.0)
    depth, _, hit = rr.render(ray, STEP, lambda p: rr.f32(z0) - p[:, 2], everywhere)
    assert bool(hit.all())
    assert float((depth - z0).abs().max()) < 4e-7


def test_plane_depth_tilted_camera():
    """The same plane seen from a yawed, offset camera: the hit's world z is z0, its z-depth follows the pose."""
    z0 = 1.3
    T = pose(20.0, (0.1, -0.05, 0.2))
    ray = rr.ray_setup(T, K, H, W, LO, HI, 0.1, 3.0)
    depth, t_hit, hit = rr.render(ray, STEP, lambda p: rr.f32(z0) - p[:, 2], everywhere)
    assert bool(hit.all())
    p = rr.hit_points(ray, t_hit).double()
    assert float((p[:, 2] - z0).abs().max()) < 2e-6
    # z-depth = the camera-frame z of the hit point
    R, o = torch.from_numpy(T[:3, :3]), torch.from_numpy(T[:3, 3])
    zc = ((p - o) @ R)[:, 2]
    assert float((depth.double() - zc).abs().max()) < 2e-6


def test_sphere_depth_within_schedule_bound():
    c, r = torch.tensor([0.1, -0.05, 1.5]), 0.5
    ray = rr.ray_setup(pose(), K, H, W, LO, HI, 0.1, 3.0)
    depth, _, hit = rr.render(ray, STEP, lambda p: torch.linalg.norm(p - c, dim=1) - r, everywhere)
    # analytic: smallest t with |o + t d - c| = r (float64), z-depth = t / nrm
    d = ray["d"].double()
    oc = -c.double()
    b = d @ oc
    disc = b * b - (oc @ oc - r * r)
    ok = disc > 1e-4
    t = -b - torch.sqrt(disc.clamp(min=0))
    z = t / ray["nrm"].double()
    assert bool((hit == ok).all()), "hit mask differs from the analytic sphere silhouette"
    # linear interpolation between samples h apart: |t error| <= h^2 f'' / (8 f'^2) with f' = cos(incidence) and
    # f'' <= 1 / r along the ray, so h^2 / (8 r cos^2) (+ float32 rounding); grazing rays (cos < 0.3) are left out
    cos = torch.sqrt(disc.clamp(min=0)) / r
    sel = ok & (cos >= 0.3)
    bound = float(STEP) ** 2 / (8 * r * cos[sel] ** 2) + 2e-6
    assert int(sel.sum()) > 100
    assert bool(((depth.double() - z)[sel].abs() <= bound).all())


def test_domain_gap_is_free_space():
    """No sample in a 2 cm gap around the surface.  The sample right before the run beyond the gap is that run's
    lead-in: it carries the field's masked constant (decode_pts' +voxel_size where a corner has no row), so the hit is
    taken between it and the run's first sample -- at the far edge of the gap, never inside it or across a run."""
    z0, gap = 1.3, 0.01
    ray = rr.ray_setup(pose(), K, H, W, LO, HI, 0.1, 3.0)
    depth, _, hit = rr.render(ray, STEP, lambda p: rr.f32(z0) - p[:, 2], lambda p: (p[:, 2] - z0).abs() > gap,
                              masked=lambda p: torch.full((p.shape[0],), 0.01))
    assert bool(hit.all())
    assert float(depth.min()) >= z0 + gap - float(STEP) and float(depth.max()) <= z0 + gap + float(STEP)
    # a lead-in whose value is not positive (a run that starts inside the surface) is no hit
    _, _, hit = rr.render(ray, STEP, lambda p: rr.f32(z0) - p[:, 2], lambda p: (p[:, 2] - z0).abs() > gap,
                          masked=lambda p: torch.full((p.shape[0],), -0.01))
    assert not bool(hit.any())


def test_run_starting_inside_is_not_a_hit():
    """f = z - z0: negative in front of the plane, positive behind -- the ray starts inside the surface (a back
    face), which is never a hit."""
    ray = rr.ray_setup(pose(), K, H, W, LO, HI, 0.1, 3.0)
    _, _, hit = rr.render(ray, STEP, lambda p: p[:, 2] - rr.f32(1.3), everywhere)
    assert not bool(hit.any())


def test_schedule_stops_at_max_depth_and_box():
    ray = rr.ray_setup(pose(), K, H, W, LO, HI, 0.1, 1.0)
    _, _, hit = rr.render(ray, STEP, lambda p: rr.f32(1.3) - p[:, 2], everywhere)
    assert not bool(hit.any())                                # the plane lies beyond max_depth
    lo, hi = rr.box([-2.0, -2.0, -2.0], [301] * 3, 0.01)      # box ends at z = 1.0
    ray = rr.ray_setup(pose(), K, H, W, lo, hi, 0.1, 3.0)
    _, _, hit = rr.render(ray, STEP, lambda p: rr.f32(1.3) - p[:, 2], everywhere)
    assert not bool(hit.any())
    t, valid = rr.schedule(ray, STEP)
    p = rr.positions(ray, t)
    assert float(p[valid][:, 2].max()) <= float(hi[2]) + 1e-6


def test_central_difference_normals_of_a_plane():
    ray = rr.ray_setup(pose(), K, H, W, LO, HI, 0.1, 3.0)
    field = lambda p: rr.f32(1.3) - p[:, 2]          # noqa: E731
    _, t_hit, hit = rr.render(ray, STEP, field, everywhere)
    n = rr.central_difference_normals(ray, t_hit, hit, field, 0.01)
    assert torch.allclose(n[hit], torch.tensor([0.0, 0.0, -1.0]).expand(int(hit.sum()), 3), atol=1e-6)


def test_depth_errors_on_constructed_tensors():
    from bnv_fusion_amd.evaluate import depth_errors
    gt = torch.tensor([[1.0, 2.0, 0.0, 1.5], [1.0, 1.0, 1.0, 0.0]])
    pred = torch.tensor([[1.01, 2.0, 0.7, 0.0], [1.1, 0.98, 1.0, 0.5]])
    e = depth_errors(pred, gt)
    # observed: 6 pixels; both > 0: 5 with |errors| 0.01, 0, 0.1, 0.02, 0
    err = np.array([0.01, 0.0, 0.1, 0.02, 0.0])
    assert e["coverage"] == pytest.approx(5 / 6)
    assert e["median"] == pytest.approx(float(np.float32(1.01) - 1.0), abs=1e-6)
    assert e["mean"] == pytest.approx(err.mean(), abs=1e-6)
    assert e["rmse"] == pytest.approx(math.sqrt((err ** 2).mean()), abs=1e-6)
    assert e["within"] == pytest.approx(4 / 5)
    assert depth_errors(pred, gt, threshold=0.15)["within"] == 1.0
    empty = depth_errors(torch.zeros(2, 2), torch.ones(2, 2))
    assert empty["coverage"] == 0.0 and math.isnan(empty["median"])
    with pytest.raises(ValueError):
        depth_errors(torch.zeros(2, 2), torch.zeros(3, 2))
