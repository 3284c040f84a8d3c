"""Cloud-to-cloud registration without a GPU: the float64 restatement (tests/cloud_register_restatement.py) recovers a
known transform of box samples against 3,000 samples of the same box with their face normals, does not depend on the
sign of a target normal, never pairs with a rejected target row, refuses a target without a usable row, keeps fewer
pairs under the normal gate, and breaks ties towards the lower index.

Recovery, measured with this file's cases (3,000 target samples, 1,500 source samples, T_true = exp((.3, -.2, .25,
.05, -.04, .03)), stride 1, gates 0.2 / 0.05 / 0.02 m over 10 + 6 + 4 iterations; the figures are printed by the
test; the translation error is measured at the origin, 2.3 m from the box):

    near    start 70.7 mm / 6.99 deg   -> 2.69 mm / 0.073 deg   (1,435 of 1,500 paired at the 2 cm gate)
    far     start 142 mm / 21.6 deg    -> 2.69 mm / 0.073 deg   (steps 0 .. 4 and 6 clamped)
    noise   near with 2 mm noise       -> 3.36 mm / 0.098 deg   (1,423 paired)
    800 target / 400 source points, near: 2.12 mm / 0.057 deg

The target is sampled about 2 cm apart, so a source point near an edge of the box can pair with a sample of the
neighbouring face: that, not rounding, is the residual (the point-to-mesh registration of the same source points
ends at 1e-4 mm)."""
import functools

import numpy as np
import pytest

import cloud_register_restatement as cc
import register_restatement as rr
import track_restatement as tr


@functools.lru_cache(maxsize=None)
def restated(name):
    target, pts, T_true, T0 = cc.cloud_case(name)
    return cc.register(pts, target, T0, levels=cc.BOX_LEVELS), T_true, T0


@pytest.mark.parametrize("name", ["near", "far", "noise"])
def test_restatement_recovers_the_box(name):
    (T, status, stats, poses, scales), T_true, T0 = restated(name)
    e0, e = tr.pose_error(T0, T_true), tr.pose_error(T, T_true)
    print(f"{name}: start {e0[0] * 1e3:.3g} mm / {np.degrees(e0[1]):.3g} deg -> {e[0] * 1e3:.3g} mm / "
          f"{np.degrees(e[1]):.3g} deg; pairs at the last iteration {stats[-1, 0]:.0f}; clamped iterations "
          f"{np.nonzero(scales < 1.0)[0].tolist()}")
    assert status == cc.OK
    assert np.array_equal(poses[0], T0) and np.array_equal(poses[-1], T)
    assert e[0] <= e0[0] / 10 and e[1] <= e0[1] / 10
    if name == "far":
        assert scales[0] < 1.0


def test_the_sign_of_a_target_normal_changes_no_bit():
    target, pts, T_true, T0 = cc.cloud_case("near")
    turned = cc.flipped(target)
    assert 1000 < (turned[:, 3:] != target[:, 3:]).any(1).sum() < 2000
    levels = ((1, 4, 0.2), (1, 2, 0.05))
    a = cc.register(pts, target, T0, levels=levels)
    b = cc.register(pts, turned, T0, levels=levels)
    assert a[1] == b[1] == cc.OK
    assert a[3].tobytes() == b[3].tobytes() and a[2].tobytes() == b[2].tobytes()
    # with the unoriented normal gate too; the oriented gate does see the sign
    ns = cc.source_normals()
    c = cc.register(pts, target, T0, levels=levels, normals=ns, min_normal_cos=0.9)
    d = cc.register(pts, turned, T0, levels=levels, normals=ns, min_normal_cos=0.9)
    assert c[3].tobytes() == d[3].tobytes()
    o = cc.register(pts, turned, T0, levels=((1, 1, 0.2),), normals=ns, min_normal_cos=0.9, oriented=True)
    assert o[2][0, 0] < 0.7 * c[2][0, 0]


def test_a_rejected_target_row_is_never_paired():
    target, pts, T_true, T0 = cc.cloud_case("near")
    pos, nrm = cc.index_rows(target)
    q = rr.transform(T_true, pts)
    idx = cc.candidates(q, pos, 0.02)
    assert (idx >= 0).sum() > 1400
    hit = np.unique(idx[idx >= 0])[:200]                   # rows that are somebody's nearest neighbour
    broken = target.copy()
    broken[hit[:100], 4] = np.nan                          # a NaN normal
    broken[hit[100:150], 3:] = 0.0                         # no direction
    broken[hit[150:], 0] = np.inf                          # a position that is not finite
    pos_b, nrm_b = cc.index_rows(broken)
    assert np.isnan(pos_b[hit]).all() and np.isnan(nrm_b[hit]).all()
    keep = np.setdiff1d(np.arange(len(target)), hit)
    assert np.array_equal(pos_b[keep].view(np.uint32), pos[keep].view(np.uint32))
    idx_b = cc.candidates(q, pos_b, 0.02)
    assert not np.isin(idx_b, hit).any()
    # the point takes its next nearest: the answer over the rows that are left
    d2_left, idx_left = cc.nearest(q, pos[keep])
    want = np.where(d2_left <= cc.gate2(0.02), keep[idx_left], -1)
    assert np.array_equal(idx_b, want)
    moved = np.isin(idx, hit)
    assert moved.sum() >= 200 and (idx_b[moved] >= 0).sum() > 0.8 * moved.sum()
    J, r, pairs = cc.rows(q, idx_b, pos_b, nrm_b)
    assert np.isfinite(J).all() and np.isfinite(r).all() and pairs == (idx_b >= 0).sum()


def test_a_target_without_a_usable_row_is_lost():
    _, pts, T_true, T0 = cc.cloud_case("near")
    T, status, stats, poses, _ = cc.register(pts, np.full((50, 6), np.nan, np.float32), T0, levels=cc.BOX_LEVELS)
    assert status == cc.LOST and T.tobytes() == T0.tobytes() and not stats.any()
    # everything beyond the gate: lost too
    target = cc.box_target()
    T, status, stats, _, _ = cc.register(pts + np.float32(10.0), target, T0, levels=cc.BOX_LEVELS)
    assert status == cc.LOST and T.tobytes() == T0.tobytes() and stats[0, 0] == 0.0


def test_the_normal_gate_keeps_fewer_pairs_and_still_converges():
    target, pts, T_true, T0 = cc.cloud_case("near")
    ns = cc.source_normals()
    # the normals belong to the points: at the true pose they are the face normals of the box
    Rt = T_true[:3, :3]
    box_normals = cc.box_target()[:200, 3:].astype(np.float64)
    turned = ns.astype(np.float64) @ Rt.T
    assert all((np.abs(box_normals - t).max(1) < 1e-5).any() for t in turned[:50])
    T, status, stats, poses, _ = cc.register(pts, target, T0, levels=cc.BOX_LEVELS, normals=ns, min_normal_cos=0.9)
    plain = restated("near")[0]
    e0, e = tr.pose_error(T0, T_true), tr.pose_error(T, T_true)
    print(f"normal gate 0.9: pairs {stats[0, 0]:.0f} against {plain[2][0, 0]:.0f} at the first iteration, "
          f"{stats[-1, 0]:.0f} against {plain[2][-1, 0]:.0f} at the last; {e[0] * 1e3:.3g} mm / "
          f"{np.degrees(e[1]):.3g} deg")
    assert status == cc.OK
    assert stats[0, 0] < plain[2][0, 0] and stats[-1, 0] < plain[2][-1, 0]
    assert e[0] <= e0[0] / 10 and e[1] <= e0[1] / 10
    # a source normal that is not finite rejects its pair
    holes = ns.copy()
    holes[:7, 1] = np.nan
    (_, _, _, pairs_h, _), _ = cc.accumulate(pts, *cc.index_rows(target), T0, 1, 0.2, holes, -1.0)
    (_, _, _, pairs_a, _), _ = cc.accumulate(pts, *cc.index_rows(target), T0, 1, 0.2, ns, -1.0)
    assert pairs_h == pairs_a - 7


def test_ties_go_to_the_lower_index():
    # an integer lattice with queries at the cell centres: eight corners at the same fp32 distance
    g = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    perm = np.random.default_rng(3).permutation(len(g))
    pos = g[perm]
    centres = g[(g < 3).all(1)] + np.float32(0.5)
    d2, idx = cc.nearest(centres, pos)
    assert (d2 == np.float32(0.75)).all()
    for c, i in zip(centres, idx):
        corners = np.flatnonzero((np.abs(pos - c) == 0.5).all(1))
        assert len(corners) == 8 and i == corners.min()
    # two copies of the same point
    twice = np.concatenate([pos, pos[:10]])
    d2, idx = cc.nearest(pos[:10] + np.float32(0.125), twice)
    assert np.array_equal(idx, np.arange(10))
    # the gate is inclusive: d2 == float32(dist * dist) pairs, the next float below does not
    dist = float(np.sqrt(0.75))
    assert (cc.candidates(centres, pos, dist) >= 0).all() == bool(cc.gate2(dist) >= np.float32(0.75))
    assert (cc.candidates(centres, pos, 0.8660) == -1).all() and (cc.candidates(centres, pos, 0.8661) >= 0).all()
    # a non-finite query has no answer
    d2, idx = cc.nearest(np.array([[np.nan, 0, 0], [0, np.inf, 0]], np.float32), pos)
    assert np.isinf(d2).all() and (idx == -1).all()
