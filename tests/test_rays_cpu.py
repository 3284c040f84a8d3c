"""The float64 formulation the GPU ray tests compare against, and their comparison function, checked on the CPU
(tests/rays_restatement.py; the kernels themselves: tests/test_gpu_rays.py).

Float64 against the reference's golden vectors (tests/golden/optimize_64.npz, the reference's random stream): the
float64 run deviates from the golden pts by 1.19e-7 and from the golden dists by 8.4e-8; the float32 oracle
deviates from the same float64 run by 1.19e-7 (pts) and 8.4e-8 (dists); the bar is 4 x the latter.

Flagged shares (samples whose sign / validity decision hangs on less than 1e-5 in float64, cap 1 %) over the 48 cases:
at most 0.123 % (d1-2-2-0.1: 1 of 812 samples), none in 30 of them; the float32 oracle's deviation from float64 is
6.4e-8 ... 3.75e-7 for pts and up to 3.65e-7 for targets (-s prints the table)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import rays_restatement as rr


def test_float64_run_reproduces_the_golden_samples():
    op = np.load(os.path.join(GOLDEN, "optimize_64.npz"))
    rays = rr.fixture_rays()
    n_fine, n_coarse = int(op["truncated_units"]) * 2, int(op["ray_max_dist"]) * 5
    gen = torch.Generator().manual_seed(int(op["seed"]))
    u_f = torch.rand(1, 160, n_fine, generator=gen)                  # the reference's stream: fine, then coarse
    u_c = torch.rand(1, 160, n_coarse, generator=gen)
    args = (rays, u_f, u_c, n_fine, n_coarse, float(op["truncated_dist"]))
    r64, r32 = rr.run(*args, torch.float64), rr.run(*args, torch.float32)
    for key, golden in (("pts", op["pts"][0]), ("dists", op["dists"][0, ..., 0])):
        own = rr.deviation(r32[key], r64[key])
        dev = rr.deviation(golden, r64[key])
        print(f"{key}: float64 vs golden {dev:.3g}, float32 oracle vs float64 {own:.3g}")
        assert own > 0 and dev <= 4 * own, (key, dev, own)


def test_every_ray_set_has_what_it_is_for():
    """The edge set really holds the rays the fixture lacks (else the cases below check nothing new)."""
    sets = rr.ray_sets()
    assert {k: int(v["uv"].shape[1]) for k, v in sets.items()} == \
        {"a": 160, "b": 203, "c1": 1, "c37": 37, "d1": 203, "d25": 203}
    assert int(sets["d1"]["neighbor_masks"].shape[2]) == 1 and int(sets["d25"]["neighbor_pts"].shape[2]) == 25
    b = next(c for c in rr.cases() if c.id == "b-20-15-0.1")
    depth = rr.reference(b.id)[0]["gt_depth"]
    assert rr.centre_rays(b).sum() >= 20 and (b.rays["mask"][0].numpy() == 0).sum() == rr.centre_rays(b).sum()
    assert ((depth > 0) & (depth < 0.1)).sum() == 20                  # hierarchical_sampling's back = gt_depth branch
    assert (rr.no_neighbour_rays(b) & ~rr.centre_rays(b)).sum() == 15
    assert float(b.rays["intr_mat"][0, 0, 1]) == pytest.approx(0.7)
    a = next(c for c in rr.cases() if c.id == "a-20-15-0.1")
    assert not rr.centre_rays(a).any() and not rr.no_neighbour_rays(a).any() and (a.rays["mask"] == 0).sum() == 16


@pytest.mark.parametrize("case_id", rr.case_ids())
def test_comparison_accepts_the_float32_oracle_and_rejects_corruptions(case_id):
    case = next(c for c in rr.cases() if c.id == case_id)
    r64, r32, E = rr.reference(case_id)
    stats = rr.assert_samples_close(r32, r64, E, case)
    print(f"{case_id}: E pts {E['pts']:.3g} target {E['target']:.3g}, flagged {100 * stats['flagged']:.3f} %")
    assert stats["flagged"] <= rr.FLAGGED_CAP
    bad = rr.corruptions(r32, r64, case, seed=3)
    expected = {"slot left NaN"}
    if case.set_name != "c1":
        expected |= {"live target negated", "neighbouring samples swapped"}
    if case.set_name in ("a", "b", "c37", "d1", "d25"):
        expected.add("masked ray weighted by validity alone")
    if case.set_name in ("b", "c37", "d1", "d25"):
        expected.add("no-neighbour target off the truncation")
    assert expected <= set(bad), (expected - set(bad))
    for name, c in bad.items():
        with pytest.raises(AssertionError):
            rr.assert_samples_close(c, r64, E, case)
            pytest.fail(f"{name} was accepted")


def test_ray_loss_restatement_signs_and_sum():
    pred = np.array([1.0, -2.0, 0.5, 0.25], np.float32)
    target = np.array([0.5, -1.0, 0.5, 1.0], np.float32)
    weight = np.array([1.0, 1.0, 1.0, 0.0], np.float32)
    grad, loss, total = rr.ray_loss(pred, target, weight, np.array([2.0, 4.0], np.float32), 2)
    assert grad.tolist() == [0.5, -0.5, 0.0, 0.0] and np.signbit(grad).tolist() == [False, True, False, True]
    assert loss == total == 0.5 / 2 + 1.0 / 2
