"""The optimiser's ray kernels (csrc/rays.hip) restated for the tests: the oracle's torch formulation of
render_utils.py (camera_rays -> hierarchical_samples -> ray_targets, oracle/bnv_oracle.py) run in a chosen dtype on
given uniforms, the ray sets and parameter cases the CPU and GPU tests share, the comparison both use
(``assert_samples_close``) with the seeded corruptions it must reject, and a float32 numpy restatement of k_ray_loss.

Everything here runs on the CPU; the GPU tests feed the kernels' outputs to the same comparison."""
import functools
import os
from collections import namedtuple

import numpy as np
import torch

from conftest import GOLDEN
from oracle import bnv_oracle as orc

DELTA = 1e-5            # a sample whose float64 decision value lies this close to a threshold may decide either way
FLAGGED_CAP = 0.01      # ... and at most this share of a case's samples may be such samples
# (n_fine, n_coarse, truncated_dist)
PARAMS = ((20, 15, 0.1), (2, 2, 0.1), (3, 2, 0.05), (62, 2, 0.1), (2, 62, 0.1), (33, 31, 0.2), (20, 15, 0.02))
RAY_KEYS = ("uv", "gt_pts", "mask", "neighbor_pts", "neighbor_masks", "T_wc", "intr_mat")

Case = namedtuple("Case", "id set_name rays u_f u_c n_fine n_coarse truncated_dist")


# --------------------------------------------------------------------------- #
# the float formulation
# --------------------------------------------------------------------------- #


def run(rays, u_f, u_c, n_fine, n_coarse, truncated_dist, dtype):
    """camera_rays -> hierarchical_samples -> ray_targets on the uniforms u_f [1, n, n_fine], u_c [1, n, n_coarse] in
    ``dtype`` -> dict of numpy arrays: pts [n, S, 3], dists [n, S], target, weight, raw_sdf [n, S], gt_depth [n],
    centre [3].  The inputs are the float32 values the kernel reads (``truncated_dist`` too), cast to ``dtype``."""
    r = {k: rays[k].to(dtype) for k in RAY_KEYS}
    td = float(np.float32(truncated_dist))
    dirs, centre = orc.camera_rays(r["uv"], r["T_wc"], r["intr_mat"])
    gt_depth = torch.sqrt(torch.sum((r["gt_pts"] - centre.unsqueeze(1)) ** 2, dim=-1))
    draws = iter((u_f.to(dtype), u_c.to(dtype)))            # hierarchical_samples draws fine, then coarse
    pts, dists = orc.hierarchical_samples(n_fine, n_coarse, gt_depth, r["gt_pts"], dirs, centre, td,
                                          lambda *shape: next(draws))
    target, weight, raw = orc.ray_targets(r, pts, centre, td)
    return {"pts": pts[0].numpy(), "dists": dists[0, ..., 0].numpy(), "target": target[0].numpy(),
            "weight": weight[0].numpy(), "raw_sdf": raw[0].numpy(), "gt_depth": gt_depth[0].numpy(),
            "centre": centre[0].numpy()}


# --------------------------------------------------------------------------- #
# ray sets (CPU float32 tensors, batch 1) and cases
# --------------------------------------------------------------------------- #


def fixture_rays():
    """(a) the 160 rays of tests/golden/optimize_64.npz."""
    op = np.load(os.path.join(GOLDEN, "optimize_64.npz"))
    return {k: torch.from_numpy(op["rays_" + k]) for k in RAY_KEYS}


def edge_rays():
    """(b) 203 rays of an 80x60 synthetic frame with what the fixture lacks: invalid pixels (six zeroed rows, five
    columns beyond ray_max_dist: their surface point is the camera centre), a skewed camera, 20 rays whose surface and
    neighbours lie 0.03-0.09 m from the camera (closer than truncated_dist), 15 rays without a valid neighbour."""
    from bnv_fusion_amd import optimize, synthetic
    H, W = 60, 80
    depth = torch.from_numpy(synthetic.depth_u16(3, H, W).astype(np.float32)) / 1000.0
    depth[[4, 17, 18, 33, 47, 59]] = 0.0
    depth[:, [0, 21, 22, 50, 79]] = 3.5
    K = synthetic.intrinsics(H, W)
    K[0, 1] = 0.7
    full = optimize.sample_key_frame(depth, K, synthetic.pose(3), 203, 3, generator=torch.Generator().manual_seed(11))
    rays = {k: full[k].clone().float() for k in RAY_KEYS}
    cam = rays["T_wc"][0, :3, 3]
    rng = np.random.default_rng(5)
    chosen = rng.choice(np.flatnonzero(rays["mask"][0].numpy() == 1), 35, replace=False)
    pulled, no_nb = torch.from_numpy(chosen[:20]), torch.from_numpy(chosen[20:])
    gt = rays["gt_pts"][0, pulled] - cam
    s = torch.from_numpy(rng.uniform(0.03, 0.09, 20).astype(np.float32)) / gt.norm(dim=-1)
    rays["gt_pts"][0, pulled] = cam + gt * s[:, None]
    rays["neighbor_pts"][0, pulled] = cam + (rays["neighbor_pts"][0, pulled] - cam) * s[:, None, None]
    rays["neighbor_masks"][0, no_nb] = 0.0
    return rays


def cut(rays, n):
    return {k: (v if k in ("T_wc", "intr_mat") else v[:, :n].clone()) for k, v in rays.items()}


def with_neighbours(rays, n_nb):
    """The neighbour arrays cut (n_nb < 9) or tiled (n_nb > 9) to n_nb per ray."""
    reps = -(-n_nb // int(rays["neighbor_masks"].shape[2]))
    out = dict(rays)
    out["neighbor_pts"] = rays["neighbor_pts"].repeat(1, 1, reps, 1)[:, :, :n_nb].clone()
    out["neighbor_masks"] = rays["neighbor_masks"].repeat(1, 1, reps)[:, :, :n_nb].clone()
    return out


@functools.lru_cache(maxsize=None)
def ray_sets():
    b = edge_rays()
    return {"a": fixture_rays(), "b": b, "c1": cut(b, 1), "c37": cut(b, 37), "d1": with_neighbours(b, 1),
            "d25": with_neighbours(b, 25)}


@functools.lru_cache(maxsize=None)
def cases():
    """Every ray set at every parameter triple on seeded uniforms, plus one case per set in which a fine and a coarse
    column of the uniforms are exactly 0 (samples on stratum edges; on a camera-centre ray a fine / coarse tie)."""
    out = []
    for si, (name, rays) in enumerate(ray_sets().items()):
        n = int(rays["uv"].shape[1])
        for pi, (nf, nc, td) in enumerate(PARAMS + (PARAMS[0],)):
            g = torch.Generator().manual_seed(4000 + 10 * si + pi)
            u_f, u_c = torch.rand(1, n, nf, generator=g), torch.rand(1, n, nc, generator=g)
            zero = pi == len(PARAMS)
            if zero:
                u_f[..., 0] = 0.0
                u_c[..., 0] = 0.0
            out.append(Case(f"{name}-" + ("zero-columns" if zero else f"{nf}-{nc}-{td}"), name, rays, u_f, u_c, nf, nc, td))
    return tuple(out)


def case_ids():
    return [c.id for c in cases()]


def deviation(a, b, keep=None):
    """Largest |a - b| (over the samples ``keep``)."""
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    if keep is not None:
        d = d[keep]
    return float(d.max()) if d.size else 0.0


def flagged(ref, case):
    """Samples whose target sign or validity hangs on less than DELTA in float64: ray not at the camera centre and
    |raw_sdf| or |raw_sdf - max(-off / 2, -0.05)| below DELTA.  They are left out of the target / weight comparison."""
    off = float(np.float32(case.truncated_dist))
    raw = ref["raw_sdf"]
    near = (np.abs(raw) < DELTA) | (np.abs(raw - max(-off / 2, -0.05)) < DELTA)
    return near & ~centre_rays(case)[:, None]


def centre_rays(case):
    """[n] bool: the ray's surface point IS the camera centre (what an invalid pixel gives)."""
    return (case.rays["gt_pts"][0] == case.rays["T_wc"][0, :3, 3]).all(-1).numpy()


def no_neighbour_rays(case):
    return (case.rays["neighbor_masks"][0] == 0).all(-1).numpy()


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """-> (float64 run, float32 run, E): E = the float32 oracle's own deviation from float64 on the case, for pts and
    for target (outside the flagged samples)."""
    case = next(c for c in cases() if c.id == case_id)
    args = (case.rays, case.u_f, case.u_c, case.n_fine, case.n_coarse, case.truncated_dist)
    r64, r32 = run(*args, torch.float64), run(*args, torch.float32)
    keep = ~flagged(r64, case)
    E = {"pts": deviation(r32["pts"], r64["pts"]), "target": deviation(r32["target"], r64["target"], keep)}
    for r in (r64, r32):
        for v in r.values():
            v.setflags(write=False)
    return r64, r32, E


# --------------------------------------------------------------------------- #
# the comparison
# --------------------------------------------------------------------------- #


def assert_samples_close(got, ref, E, case):
    """``got``: pts [n, S, 3], target, weight [n, S] in float32 (numpy) of ``case``; ``ref``: its float64 run;
    ``E``: the float32 oracle's deviation from float64 on the case.  Raises AssertionError unless
      - no slot is NaN (a rank collision leaves one unwritten);
      - the distances from the camera centre, recomputed from pts, do not decrease along a ray (each float32 coordinate
        carries the roundings of d * dir and of cam + ., <= 1 ulp together, so a distance moves by <= sqrt(3) ulp and
        a gap by < 4 ulp of the largest coordinate: that much is allowed);
      - pts (every sample) and target (outside the flagged samples) are within max(4 E, 2 ulp of the largest
        coordinate) of float64, and weight (outside the flagged samples) is equal exactly;
      - the flagged samples are at most FLAGGED_CAP of all;
      - a ray at the camera centre has weight 0, its n_coarse smallest distances exactly 0 with pts the camera centre
        there, and target <= 0;
      - a ray without a valid neighbour has |target| == float32(truncated_dist) exactly.
    -> {"pts", "target": largest deviations from float64, "flagged": share}."""
    pts, target, weight = (np.asarray(got[k]) for k in ("pts", "target", "weight"))
    assert pts.dtype == target.dtype == weight.dtype == np.float32
    assert pts.shape == ref["pts"].shape and target.shape == weight.shape == ref["target"].shape
    assert not (np.isnan(pts).any() or np.isnan(target).any() or np.isnan(weight).any()), "a slot was left NaN"
    centre = ref["centre"].astype(np.float32)
    ulp = float(np.spacing(np.float32(max(np.abs(ref["pts"]).max(), np.abs(centre).max()))))
    d = np.sqrt(((pts.astype(np.float64) - centre.astype(np.float64)) ** 2).sum(-1))
    assert (np.diff(d, axis=1) >= -4 * ulp).all(), ("distances decrease along a ray", float(np.diff(d, axis=1).min()))
    dev_pts = deviation(pts, ref["pts"])
    assert dev_pts <= max(4 * E["pts"], 2 * ulp), ("pts", dev_pts, E["pts"], ulp)
    flag = flagged(ref, case)
    share = float(flag.mean())
    assert share <= FLAGGED_CAP, ("flagged share", share)
    dev_target = deviation(target, ref["target"], ~flag)
    assert dev_target <= max(4 * E["target"], 2 * ulp), ("target", dev_target, E["target"], ulp)
    assert np.array_equal(weight[~flag], ref["weight"][~flag].astype(np.float32)), "weight"
    at_centre = centre_rays(case)
    if at_centre.any():
        assert (case.rays["mask"][0].numpy()[at_centre] == 0).all()      # (an invalid pixel is a masked ray)
        assert (weight[at_centre] == 0).all(), "weight on a camera-centre ray"
        assert (pts[at_centre, :case.n_coarse] == centre).all(), "coarse samples of a camera-centre ray"
        assert (d[at_centre, :case.n_coarse] == 0).all()
        assert (target[at_centre] <= 0).all(), "target on a camera-centre ray"
    alone = no_neighbour_rays(case)
    if alone.any():
        assert (np.abs(target[alone]) == np.float32(case.truncated_dist)).all(), "target of a no-neighbour ray"
    return {"pts": dev_pts, "target": dev_target, "flagged": share}


def _pick(rng, mask):
    idx = np.argwhere(mask)
    return tuple(idx[rng.integers(len(idx))]) if len(idx) else None


def corruptions(good, ref, case, seed=0):
    """Seeded corruptions of a good output that ``assert_samples_close`` must reject -> {name: corrupted copy}; a
    corruption the case has no ray for is absent."""
    rng = np.random.default_rng(seed)
    off32 = np.float32(case.truncated_dist)
    flag = flagged(ref, case)
    out = {}

    def fresh():
        return {k: np.array(good[k], dtype=np.float32, copy=True) for k in ("pts", "target", "weight")}

    at = _pick(rng, (good["weight"] > 0) & ~flag & (np.abs(good["target"]) > 1e-3))
    if at is not None:
        c = fresh()
        c["target"][at] = -c["target"][at]
        out["live target negated"] = c
    at = _pick(rng, np.broadcast_to(no_neighbour_rays(case)[:, None], flag.shape))
    if at is not None:
        c = fresh()
        c["target"][at] = np.copysign(np.nextafter(off32, np.float32(0)), c["target"][at])
        out["no-neighbour target off the truncation"] = c
    valid = (np.clip(ref["raw_sdf"], -float(off32), float(off32)) > max(-float(off32) / 2, -0.05)).astype(np.float32)
    masked = (case.rays["mask"][0].numpy() == 0) & (valid.sum(1) > 0) & ~flag.any(1)
    at = _pick(rng, masked)
    if at is not None:
        c = fresh()
        c["weight"][at[0]] = valid[at[0]]
        out["masked ray weighted by validity alone"] = c
    gap = np.diff(ref["dists"], axis=1) > DELTA
    at = _pick(rng, gap & ~centre_rays(case)[:, None])
    if at is not None:
        c = fresh()
        r, j = at
        for k in c:
            c[k][r, [j, j + 1]] = c[k][r, [j + 1, j]]
        out["neighbouring samples swapped"] = c
    c = fresh()
    at = _pick(rng, np.ones(flag.shape, bool))
    c[("pts", "target", "weight")[int(rng.integers(3))]][at] = np.nan
    out["slot left NaN"] = c
    return out


# --------------------------------------------------------------------------- #
# k_ray_loss
# --------------------------------------------------------------------------- #


def ray_loss(pred, target, weight, n_valid, split_samples):
    """k_ray_loss restated on float32 numpy arrays: -> (grad = sign(pred - target) * weight * (1 / n_valid) in float32,
    operation for operation; the loss sum w |pred - target| / n_valid in float64; sum |terms| in float64).  Sample i
    reads n_valid[i // split_samples] (split_samples 0: n_valid[0])."""
    m = len(pred)
    split = (np.arange(m) // split_samples) if split_samples > 0 else np.zeros(m, np.int64)
    inv = (np.float32(1) / n_valid.astype(np.float32))[split]
    w = weight.astype(np.float32) * inv
    d = pred.astype(np.float32) - target.astype(np.float32)
    grad = np.where(d > 0, w, np.where(d < 0, -w, np.float32(0))).astype(np.float32)
    terms = np.abs(pred.astype(np.float64) - target.astype(np.float64)) * weight.astype(np.float64) \
        / n_valid.astype(np.float64)[split]
    return grad, float(terms.sum()), float(np.abs(terms).sum())
