"""The restatements of tests/mesh_ray_restatement.py against what they restate; no GPU.

Ray caster.  The float64 brute force (all triangles, no grid) must reproduce the analytic ``sequence.render_depth`` on
``sequence.gt_mesh()`` at 640 x 480, on the sure pixels of frames 0, 37, 195, 390, 777 and 1234.  The mesh's vertices are
float32-rounded, a plane is off by at most 2^-24 L along its normal (L = 3.6), and a sure pixel's surface is no
steeper than SLOPE_MAX = 16 against the image plane, so the depths may differ by 16 * 2^-24 * 3.6 = 3.4e-6 m.
Measured: 1.1e-7 .. 3.1e-7 m on the sure pixels, no miss; unsure pixels 0.0309 % at frame 0 (row 452 grazes a box's
top edge: a 0.25 m jump), at most 0.0007 % at the others (two pixels, on surfaces steeper than SLOPE_MAX); the cap is
0.1 %.

DEPTH TOLERANCE of the kernel tests (tests/test_gpu_mesh_ray.py): the kernel's formulas in numpy float32, one rounding
per operation (``woop(dtype=float32)`` on ``camera_rays(dtype=float32)``), against the float64 brute force on the same
rays, sure pixels, in units of 2^-23 L (L: the largest absolute coordinate of vertices and camera):

    frame 0: 1.111   37: 3.207   195: 4.270   390: 1.819   777: 2.208   1234: 1.262     (no hit / miss flip)

The worst is 4.270 (1.8e-6 m; the error grows with the slope, and sure pixels go up to SLOPE_MAX); 4x for a different
but legitimate operation order: TOL_REL = 17.08 (7.3e-6 m in the room).  On the small views of the kernel tests the
same evaluation gives 0.17 .. 2.85, and 6.64 on the torus.

Second case, many triangles: ``synthetic.gt_mesh(step_px=4)`` (44,935 faces) from ``synthetic.pose(0)``, 1,500 seeded
pixels.  The piecewise-linear mesh deviates from the smooth ``synthetic._clean_depth`` by the chord error of
0.2 sin(u/40) cos(v/30) over 4 px: at most about 0.2 * (4^2 / 8) * (1/40^2 + 1/30^2) * 2 = 1.4e-3 m in depth; measured
in float64 below and asserted against that bound -- it is the tessellation's error, no part of the kernel's tolerance.
"""
import os

import numpy as np
import pytest

import mesh_ray_restatement as R
from conftest import GOLDEN

FRAMES = (0, 37, 195, 390, 777, 1234)
TOL_REL = 17.08
UNSURE_CAP = 1e-3
ANALYTIC_BOUND = R.SLOPE_MAX * 2.0 ** -24 * 3.6
TESSELLATION_BOUND = 1.4e-3
BARY_MARGIN = 1e-3          # barycentric: further than this inside a triangle, a hit is that triangle's in any arithmetic
GRAZING = 64                # TOL_REL is measured on surfaces up to SLOPE_MAX steep and fp32's error in t grows with the
#                             slope; rays cast from inside a closed surface meet it at any angle: 64 x admits slopes to
#                             1024 (0.06 degrees off tangent).  Beyond that a hit goes to ``legitimate_hit``, whose
#                             distance to the face's plane does not grow with the slope.


def synthetic_subset(n=1500, step_px=4, seed=7):
    """-> (mesh, K, T, H, W, pixel indices): the seeded pixels of the second case, away from the image border."""
    from bnv_fusion_amd import synthetic
    H, W = 480, 640
    rng = np.random.default_rng(seed)
    pix = rng.integers(8, H - 8, n) * W + rng.integers(8, W - 8, n)
    return synthetic.gt_mesh(step_px=step_px), synthetic.intrinsics(H, W), synthetic.pose(0), H, W, pix


@pytest.mark.parametrize("t", FRAMES)
def test_brute_force_reproduces_the_analytic_room(t):
    from bnv_fusion_amd import sequence
    m, K, T, H, W = sequence.gt_mesh(), sequence.intrinsics(), sequence.sweep_pose(t), 480, 640
    ok, c = R.sure(K, T, H, W, m.vertices, m.faces)
    analytic = sequence.render_depth(T, K, H, W).numpy().reshape(-1)
    hit = np.isfinite(c["t"])
    diff = np.abs(np.where(hit, c["t"], 0.0) - analytic)
    print(f"\nframe {t}: unsure {100 * (1 - ok.mean()):.4f} %, misses {(~hit).sum()}, max |brute force - analytic| on "
          f"sure pixels {diff[ok].max():.3e} m (all pixels {diff.max():.3e})")
    assert 1 - ok.mean() <= UNSURE_CAP
    assert hit[ok].all()
    assert diff[ok].max() <= ANALYTIC_BOUND
    # the float32 evaluation of the kernel's formulas stays inside the tolerance it sets, with the same hits
    o32, d32 = R.camera_rays(K, T, H, W, np.float32)
    ref = R.brute_force(o32, d32, m.vertices, m.faces)
    w32 = R.woop(o32, d32, m.vertices, m.faces)
    L = max(float(np.abs(m.vertices).max()), float(np.abs(T[:3, 3]).max()))
    assert np.array_equal(np.isfinite(w32)[ok], np.isfinite(ref["t"])[ok])
    err = np.abs(w32 - ref["t"])[ok].max() / (R.ULP32 * L)
    print(f"frame {t}: float32 formulas {err:.3f} x 2^-23 L (TOL_REL {TOL_REL})")
    assert err <= TOL_REL / 4 * 1.0001


def test_brute_force_on_many_triangles_against_the_smooth_surface():
    from bnv_fusion_amd import synthetic
    m, K, T, H, W, pix = synthetic_subset()
    o, d = R.camera_rays(K, T, H, W)
    c = R.brute_force(o, d[pix], m.vertices, m.faces)
    smooth = synthetic._clean_depth(0, H, W).reshape(-1)[pix]
    assert np.isfinite(c["t"]).all()
    dev = np.abs(c["t"] - smooth)
    print(f"\nsynthetic.gt_mesh(step_px=4): {len(m.faces)} faces, {len(pix)} pixels, tessellation error max "
          f"{dev.max():.3e} m, mean {dev.mean():.3e} m")
    assert dev.max() <= TESSELLATION_BOUND
    w64 = R.woop(o, d[pix], m.vertices, m.faces, dtype=np.float64)
    assert np.abs(w64 - c["t"]).max() < 1e-12                  # the two ray / triangle tests agree in float64


def legitimate_hits(o, d, V, F, t, face, ref):
    """The distances of a ray caster's hits (t, face: one per ray, all hits) against ``ref = brute_force(o, d, V, F)``,
    for rays that may run through edges and vertices and along silhouettes, where the reference is one legitimate
    answer among several and, being plain Moeller-Trumbore, sometimes none.  Within GRAZING * TOL_REL * 2^-23 L of the
    reference's distance a hit is fine; any other must pass ``mesh_ray_restatement.legitimate_hit`` with the same
    tolerance and BARY_MARGIN.  -> (differs from the reference bool [N], fine bool [N])"""
    d = np.asarray(d, np.float64)
    dn = np.linalg.norm(d, axis=1)
    tol = GRAZING * TOL_REL * R.ULP32 * max(float(np.abs(V).max()), float(np.abs(o).max()))
    with np.errstate(invalid="ignore"):
        differs = ~(np.abs(t - ref["t"]) * dn <= tol)
    fine = ~differs
    i = np.nonzero(differs)[0]
    if len(i):
        fine[i] = R.legitimate_hit(np.asarray(o, np.float64), d[i], V, F, t[i], face[i], tol, BARY_MARGIN)
    return differs, fine


def test_woop_is_watertight_where_moeller_trumbore_need_not_be():
    """Rays from inside a closed box and a closed torus aimed exactly at their vertices and edge midpoints, and within
    2^-20 of them: the float32 formulas hit on every one, at the reference's distance or at another legitimate one.
    Measured: the float64 Moeller-Trumbore reference loses 11 of the box's 3,028 rays and 15 of the torus's 16,128;
    the float32 formulas lose none.  Their distance differs from the reference's on 11 and 34 rays: the reference's
    leaks, rays that leaked in the reference and came back into the torus's far wall, and 4 rays grazing the torus's
    inner equator (see tests/test_gpu_mesh_ray.py::test_watertight_from_inside); all legitimate."""
    import mesh_sdf_restatement as S
    meshes = {name: (V, F) for name, V, F, _ in S.kernel_cases()}
    for name, origin in (("box", (1.02, -0.47, 2.03)), ("torus", (0.8, -0.2, 0.4))):
        V, F = meshes[name]
        o = np.asarray(origin, np.float32)
        d = R.aimed_directions(V, F, o)
        d = d[np.abs(d).max(1) > 0]
        ref = R.brute_force(o.astype(np.float64), d.astype(np.float64), V, F)
        t, face = R.woop(o, d, V, F, return_face=True)
        assert np.isfinite(t).all()
        differs, fine = legitimate_hits(o, d, V, F, t, face, ref)
        print(f"\n{name}: {len(d)} rays, the reference leaks {(~np.isfinite(ref['t'])).sum()}, distance differs on "
              f"{differs.sum()}, not legitimate {(~fine).sum()}")
        assert fine.all()
        # the check is no rubber stamp: a hit moved along its ray, or given to a face elsewhere, is refused
        k = np.nonzero(~differs)[0][::97]
        assert not R.legitimate_hit(o.astype(np.float64), d[k], V, F, t[k] * 1.01, face[k], 1e-4, BARY_MARGIN).any()
        assert not R.legitimate_hit(o.astype(np.float64), d[k], V, F, t[k], (face[k] + 100) % len(F), 1e-4, BARY_MARGIN).any()


PHILOX_KAT = (     # Random123's known-answer vectors for philox4x32-10: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def test_philox_known_answers():
    for ctr, key, out in PHILOX_KAT:
        assert R.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32)).tolist() == list(out)


def test_sensor_restatement_reproduces_the_reference_bit_for_bit():
    g = np.load(os.path.join(GOLDEN, "sensor_60x80.npz"))
    s = R.sensor(g["clean"], draws=g["draws"], table=np.ones((80, 80, 5)))
    assert np.array_equal(s["depth"].view(np.int64), g["depth"].view(np.int64))
    assert (g["depth"] == 0).sum() > 100 and (g["depth"] > 0).sum() > 3000


def test_sensor_properties():
    from bnv_fusion_amd import sequence
    clean = sequence.render_depth(sequence.sweep_pose(37), sequence.intrinsics(120, 160), 120, 160).numpy()
    clean[10:20, 30:50] = 0.0
    a = R.sensor(clean, seed=5, frame=3)
    nz = a["depth"] > 0
    k = 35.130 * 8 / a["depth"][nz]
    assert np.abs(k - np.rint(k)).max() < 1e-9                 # every non-zero output is bf 8 / k, k an integer
    assert (a["depth"][12:18:2, 32:48:2] == 0).all()           # zero stays zero (block origins well inside the hole)
    zero_src = R.sensor(np.zeros((16, 16)), seed=1, frame=0)
    assert (zero_src["mm"] == 0).all()
    assert np.array_equal(a["mm"], R.sensor(clean, seed=5, frame=3)["mm"])
    assert (a["mm"] != R.sensor(clean, seed=5, frame=4)["mm"]).mean() > 0.2
    assert (a["mm"] != R.sensor(clean, seed=6, frame=3)["mm"]).mean() > 0.2
    n = R.sensor_draws(240, 320, 9, 1)
    assert abs(n.mean()) < 0.01 and abs(n.std() - 1) < 0.01 and abs(np.corrcoef(n[..., 0].ravel(), n[..., 1].ravel())[0, 1]) < 0.01
    assert np.array_equal(a["mm"], np.trunc(a["depth"] * 1000).astype(np.uint16))


def test_float32_draws_leave_few_pixels_near_a_rounding_boundary():
    """What tests/test_gpu_mesh_ray.py's sensor test rests on: with the draws in float32 (as the kernel makes them), the
    three quantities before rounding differ from the float64 ones by at most DELTA / 4, and fewer than 0.1 % of a
    640 x 480 frame lie within DELTA of a rounding boundary.  Measured: largest difference 2.64e-7 (frame 37; 2.35e-7 at 777), so
    DELTA = 4 * 2.64e-7 = 1.06e-6; share within DELTA 0.0026 % and 0.0007 %; pixels whose float32 evaluation differs
    from float64: 0 in both frames."""
    from bnv_fusion_amd import sequence
    for t in (37, 777):
        clean = sequence.render_depth(sequence.sweep_pose(t), sequence.intrinsics(), 480, 640).numpy().astype(np.float32)
        n32 = R.sensor_draws(480, 640, 0, t, np.float32)
        a, b = R.sensor(clean, draws=n32), R.sensor(clean, seed=0, frame=t)
        with np.errstate(invalid="ignore"):
            diff = np.nanmax(np.abs(a["q"] - b["q"]))
        near = near_boundary(b["q"], SENSOR_DELTA)
        print(f"\nframe {t}: max |q32 - q64| {diff:.3e}, within DELTA of a boundary {100 * near.mean():.5f} %, "
              f"float32 evaluation differs at {(a['mm'] != b['mm']).sum()} pixels")
        assert 4 * diff <= SENSOR_DELTA
        assert near.mean() <= 1e-3
        assert (a["mm"] != b["mm"])[~near].sum() == 0


SENSOR_DELTA = 1.06e-6


def near_boundary(q, delta):
    """Pixels one of whose quantities lies within ``delta`` of a half-integer (rint's boundaries)."""
    with np.errstate(invalid="ignore"):
        frac = np.abs(q - np.floor(q) - 0.5)
    return (np.nan_to_num(frac, nan=1.0) <= delta).any(-1)
