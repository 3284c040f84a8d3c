"""The optimiser's ray kernels (csrc/rays.hip) and the loss half of k_optim_step, element by element against float64.

k_ray_samples: pts, L1 target and sample weight of every case of tests/rays_restatement.py (6 ray sets x 7 parameter
triples + one zero-uniform case per set; output buffers pre-filled with NaN) through ``assert_samples_close`` against
the float64 run of the oracle's formulation.  The bar per case is 4 x the float32 oracle's own deviation from float64
(floor: 2 ulp of the largest coordinate).  Measured on an MI355X over the 48 cases, largest deviation from float64:
  kernel          pts 3.52e-7 (d25-62-2-0.1)   target 3.65e-7 (b-20-15-0.02)   [ray set (a): 1.29e-7 / 1.18e-7]
  float32 oracle  pts 3.75e-7 (d25-20-15-0.02) target 3.65e-7 (b-20-15-0.02)   [ray set (a): 1.29e-7 / 1.20e-7]
(the kernel never exceeds 1.3 x the oracle's deviation on a case and equals it to three digits on about half of them).
Flagged samples (sign or validity decided by less than 1e-5 in float64; left out of the target and weight checks only):
at most 0.123 % of a case (d1-2-2-0.1: 1 of 812), none in 30 of the 48 cases; the asserted cap is 1 %.

k_ray_loss: gradient bit for bit against a float32 restatement, loss against the float64 sum.  The deferred
count_optim kernels: exact against the oracle volume and against split-by-split calls.  k_optim_step: its loss and
feature gradient against restatements formed from its own ``pred``."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import rays_restatement as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def bnv():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    import bnv_fusion_amd
    from bnv_fusion_amd import _lib
    _lib.require_device(0)
    return bnv_fusion_amd


def _dev(a):
    return torch.as_tensor(a).float().contiguous().to(DEV)


def _kernel_samples(case):
    """bnv_ray_samples on a case, straight through the C entry, into NaN-filled buffers."""
    from bnv_fusion_amd import _lib
    r = case.rays
    uv, gt, rm, nb, nbm = (_dev(r[k][0]) for k in ("uv", "gt_pts", "mask", "neighbor_pts", "neighbor_masks"))
    u_f, u_c = _dev(case.u_f[0]), _dev(case.u_c[0])
    n, S = int(uv.shape[0]), case.n_fine + case.n_coarse
    T = (C.c_float * 16)(*r["T_wc"][0].reshape(-1).tolist())
    K = (C.c_float * 9)(*r["intr_mat"][0].reshape(-1).tolist())
    pts = torch.full((n, S, 3), NAN, dtype=torch.float32, device=DEV)
    target = torch.full((n, S), NAN, dtype=torch.float32, device=DEV)
    weight = torch.full((n, S), NAN, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().bnv_ray_samples(
        _lib.ptr(uv), _lib.ptr(gt), _lib.ptr(rm), _lib.ptr(nb), _lib.ptr(nbm), int(nb.shape[1]), T, K, _lib.ptr(u_f),
        _lib.ptr(u_c), n, case.n_fine, case.n_coarse, float(case.truncated_dist), _lib.ptr(pts), _lib.ptr(target),
        _lib.ptr(weight), _lib.stream_ptr()), "bnv_ray_samples")
    return {"pts": pts.cpu().numpy(), "target": target.cpu().numpy(), "weight": weight.cpu().numpy()}


@pytest.mark.parametrize("case_id", rr.case_ids())
def test_ray_samples_match_float64(bnv, case_id):
    case = next(c for c in rr.cases() if c.id == case_id)
    r64, _, E = rr.reference(case_id)
    got = _kernel_samples(case)
    print(f"{case_id}: kernel vs float64 pts {rr.deviation(got['pts'], r64['pts']):.3g} "
          f"target {rr.deviation(got['target'], r64['target'], ~rr.flagged(r64, case)):.3g}; float32 oracle vs float64 "
          f"pts {E['pts']:.3g} target {E['target']:.3g}; flagged {100 * float(rr.flagged(r64, case).mean()):.3f} %")
    rr.assert_samples_close(got, r64, E, case)


# --------------------------------------------------------------------------- #
# k_ray_loss
# --------------------------------------------------------------------------- #
SPLIT = 35 * 40


def _ray_loss_inputs(m, split_samples, dead_split):
    """Random pred / target, weight with zeros, 5 % of pred bit-equal to target; per split one n_valid.  ``dead_split``:
    that split has every weight 0 and n_valid = 1e-4 (a split of masked rays: render_utils.py:553)."""
    rng = np.random.default_rng(100 + m)
    target = np.clip(rng.normal(0, 0.05, m), -0.1, 0.1).astype(np.float32)
    pred = rng.normal(0, 0.05, m).astype(np.float32)
    weight = (rng.random(m) < 0.7).astype(np.float32)
    same = rng.random(m) < 0.05
    same[m // 2] = True
    pred[same] = target[same]
    n_splits = -(-m // split_samples) if split_samples else 1
    n_valid = (rng.integers(1, 40, n_splits) + 1e-4).astype(np.float32)
    if dead_split is not None:
        lo = dead_split * split_samples
        weight[lo: lo + split_samples if split_samples else m] = 0.0
        n_valid[dead_split] = np.float32(1e-4)
    return pred, target, weight, n_valid


@pytest.mark.parametrize("m,split_samples,dead_split", [
    (1, 0, None), (255, 0, None), (256, 0, None), (257, 0, None), (1295, 0, None), (257, 0, 0),
    (1, SPLIT, None), (255, SPLIT, None), (256, SPLIT, None), (257, SPLIT, None), (1295, SPLIT, None),
    (2 * SPLIT + 35 * 13, SPLIT, None), (2 * SPLIT + 35 * 13, SPLIT, 1), (2 * SPLIT + 35 * 13, 0, None)])
def test_ray_loss_grad_bitwise_and_loss_vs_float64(bnv, m, split_samples, dead_split):
    from bnv_fusion_amd import _lib
    pred, target, weight, n_valid = _ray_loss_inputs(m, split_samples, dead_split)
    want_grad, want_loss, total = rr.ray_loss(pred, target, weight, n_valid, split_samples)
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    grad = torch.full((m,), NAN, dtype=torch.float32, device=DEV)
    p, t, w, nv = _dev(pred), _dev(target), _dev(weight), _dev(n_valid)
    _lib.check(_lib.load().bnv_ray_loss(_lib.ptr(p), _lib.ptr(t), _lib.ptr(w), _lib.ptr(nv), m, split_samples,
                                        _lib.ptr(loss), _lib.ptr(grad), _lib.stream_ptr()), "bnv_ray_loss")
    got = grad.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want_grad.view(np.int32)), int((got != want_grad).sum())
    assert (got[pred == target] == 0).all()
    print(f"m {m} split_samples {split_samples}: loss {float(loss):.9g} float64 {want_loss:.9g} sum|terms| {total:.6g}")
    assert abs(float(loss) - want_loss) <= 1e-6 * total


# --------------------------------------------------------------------------- #
# count_optim on sample points: direct, and deferred as split masks
# --------------------------------------------------------------------------- #


def _oracle_volume():
    from oracle import bnv_oracle as orc
    z = np.load(os.path.join(GOLDEN, "sequence_64.npz"))
    pos = {tuple(k): i for i, k in enumerate(z["keys_sorted"].tolist())}
    perm = np.array([pos[tuple(k)] for k in z["keys_insertion"].tolist()])
    ovol = orc.OracleSparseVolume(8, float(z["voxel_size"]), z["dims"], 8)
    ovol.insert(torch.from_numpy(z["keys_insertion"]), torch.from_numpy(z["features_sorted"][perm]),
                torch.from_numpy(z["weights_sorted"][perm]), torch.from_numpy(z["num_hits_sorted"][perm]))
    ovol.to_tensor()
    return ovol


@pytest.fixture(scope="module")
def count_points():
    """5,700 world points: the 5,600 float32 samples of ray set (a), 60 points on integer voxel coordinates (all eight
    corners are ONE row) and 40 outside the grid -> (world [m, 3], voxel coordinates [m, 3]) float32 CPU tensors."""
    ovol = _oracle_volume()
    pts = torch.from_numpy(rr.reference("a-20-15-0.1")[1]["pts"].reshape(-1, 3).copy())
    on_grid = ovol.active_coordinates[::25][:60].float() * ovol.voxel_size + ovol.min_coords
    g = torch.Generator().manual_seed(21)
    outside = torch.cat([torch.rand(20, 3, generator=g) * 4 + 1.5, -torch.rand(19, 3, generator=g) * 4 - 1.5,
                         torch.tensor([[1e4, -1e4, 0.0]])])
    world = torch.cat([pts, on_grid, outside]).float().contiguous()
    coords = torch.cat([(pts - ovol.min_coords) / ovol.voxel_size, ovol.active_coordinates[::25][:60].float(),
                        (outside - ovol.min_coords) / ovol.voxel_size]).float().contiguous()
    assert world.shape == (5700, 3)
    return world, coords


def _oracle_counts(ovol, coords):
    """The oracle volume's weights after count_optim(get_neighbors(coords)) (render_utils.py:488-493)."""
    from oracle import bnv_oracle as orc
    ovol.count_optim(orc.get_neighbors(coords.reshape(1, -1, 1, 3)))
    return ovol.weights.clone()


@pytest.mark.parametrize("is_coords", [False, True])
def test_count_optim_pts_equals_the_oracle_volume(bnv, count_points, is_coords):
    from test_gpu_optimize import _insertion_order_volume
    world, coords = count_points
    vol, ovol = _insertion_order_volume(bnv), _oracle_volume()
    assert torch.equal(vol.weights.cpu(), ovol.weights)
    # what the oracle counts: its own float32 voxel coordinates of the world points, or the given ones
    given = coords if is_coords else (world - ovol.min_coords) / ovol.voxel_size
    before = ovol.weights.clone()
    once = _oracle_counts(ovol, given)
    assert 100 < int((once != before).sum()) < len(before)
    vol.count_optim_pts((coords if is_coords else world).to(DEV), is_coords=is_coords)
    assert torch.equal(vol.weights.cpu(), once)
    twice = _oracle_counts(ovol, given)
    vol.count_optim_pts((coords if is_coords else world).to(DEV), is_coords=is_coords)      # a fresh epoch: +1 again
    assert torch.equal(vol.weights.cpu(), twice) and torch.equal(twice - once, once - before)


@pytest.mark.parametrize("split_samples,n_splits", [(1400, 5), (185, 31)])
@pytest.mark.parametrize("is_coords", [False, True])
def test_deferred_split_counts_equal_split_by_split(bnv, count_points, is_coords, split_samples, n_splits):
    from test_gpu_optimize import _insertion_order_volume
    p = count_points[1 if is_coords else 0].to(DEV)
    m = int(p.shape[0])
    assert -(-m // split_samples) == n_splits and m % split_samples != 0            # an uneven last split
    va, vb = _insertion_order_volume(bnv), _insertion_order_volume(bnv)
    for lo in range(0, m, split_samples):
        va.count_optim_pts(p[lo: lo + split_samples], is_coords=is_coords)
    w0 = vb.weights.clone()
    vb.count_optim_splits(p, split_samples, is_coords=is_coords)
    assert torch.equal(vb.weights, w0)                                   # deferred: nothing added yet
    mask = vb._split_mask()[: int(w0.shape[0])].clone()
    assert int(mask.max()) > 0 and int(mask.min()) >= 0                  # (31 splits: bit 30 is the highest)
    vb.apply_split_counts()
    assert torch.equal(va.weights, vb.weights)
    assert int((vb.weights - w0).max()) > 1                              # some row is touched by several splits
    assert not vb._split_mask().any()


def test_thirty_two_splits_are_refused(bnv, count_points):
    from bnv_fusion_amd import _lib, optimize
    from test_gpu_optimize import _insertion_order_volume
    vol = _insertion_order_volume(bnv)
    p = count_points[0].to(DEV)
    assert -(-int(p.shape[0]) // 179) == 32
    w0 = vol.weights.clone()
    status = _lib.load().bnv_volume_count_optim_splits(
        C.byref(vol._struct()), C.byref(vol._grid), _lib.ptr(p), int(p.shape[0]), 0, int(w0.shape[0]), 179,
        _lib.ptr(vol._split_mask()), _lib.stream_ptr())
    assert status != 0
    with pytest.raises(_lib.BnvError):
        vol.count_optim_splits(p, 179)
    assert not vol._split_mask().any() and torch.equal(vol.weights, w0)
    model = bnv.load_pretrained(device=DEV, voxel_size=0.02)
    rays = {k: v.to(DEV) for k, v in rr.ray_sets()["a"].items()}
    with pytest.raises(ValueError):
        optimize.ray_batch_step(vol, rays, model.nerf, 10, 0.1, 3, train_ray_splits=5)       # 160 rays / 5 = 32
    assert not vol._split_mask().any() and torch.equal(vol.weights, w0)


# --------------------------------------------------------------------------- #
# the loss half of k_optim_step
# --------------------------------------------------------------------------- #


@pytest.mark.parametrize("mode", ["split_f16", "fp32_exact"])
@pytest.mark.parametrize("per", [40, 48])
def test_optim_step_loss_and_gradient_from_its_own_pred(bnv, mode, per):
    """bnv_optim_step on the samples of ray set (a), ``per`` rays a split (48: an uneven last split of 16): loss[0]
    against sum w |pred - target| / n_valid in float64 formed from the kernel's own pred, grad_features against
    bnv_decode_pts_backward fed the restated d loss / d pred (same split masks); then again with target bit-equal to
    pred on a tenth of the live samples, which must send no gradient."""
    from test_gpu_optimize import _insertion_order_volume
    bnv.set_mlp_mode(1 if mode == "split_f16" else 0)
    try:
        model = bnv.load_pretrained(device=DEV, voxel_size=0.02)
        case = next(c for c in rr.cases() if c.id == "a-20-15-0.1")
        s = _kernel_samples(case)
        n, S = s["target"].shape
        pts, weight = _dev(s["pts"]), _dev(s["weight"].reshape(-1))
        split_samples = per * S
        rm = case.rays["mask"][0].numpy()
        n_valid = np.array([rm[lo: lo + per].sum() for lo in range(0, n, per)], np.float32) + np.float32(1e-4)
        vol = _insertion_order_volume(bnv)
        vol.count_optim_splits(pts, split_samples)
        voxel = np.float32(vol.voxel_size)

        def step(target):
            loss2 = torch.zeros(2, dtype=torch.float32, device=DEV)
            grad = torch.zeros_like(vol.features)
            pred = torch.full((n * S,), NAN, dtype=torch.float32, device=DEV)
            vol.optim_step(pts, model.nerf, None, split_samples, _dev(target), weight, _dev(n_valid), loss2, grad, pred)
            pred = pred.cpu().numpy()
            assert not np.isnan(pred).any()
            g, want_loss, total = rr.ray_loss(pred, target, s["weight"].reshape(-1), n_valid, split_samples)
            print(f"{mode} per {per}: loss {float(loss2[0]):.9g} float64 {want_loss:.9g} sum|terms| {total:.6g}")
            assert total > 0 and abs(float(loss2[0]) - want_loss) <= 1e-6 * total
            want = torch.zeros_like(vol.features)
            vol.decode_pts_backward_splits(pts, model.nerf, _dev(g), want, split_samples)
            top = float(want.abs().max())
            print(f"  grad_features: largest {top:.6g}, deviation {float((grad - want).abs().max()):.3g}")
            assert top > 0 and float((grad - want).abs().max()) <= 2e-5 * top
            return pred, g, grad

        target = s["target"].reshape(-1)
        pred, g, grad = step(target)
        live = np.flatnonzero((pred != voxel) & (g != 0))
        assert len(live) > 200
        quiet = live[::10]
        target2 = target.copy()
        target2[quiet] = pred[quiet]
        pred2, g2, grad2 = step(target2)
        assert np.array_equal(pred2.view(np.int32), pred.view(np.int32))
        assert (g2[quiet] == 0).all() and float((grad2 - grad).abs().max()) > 0
        vol.apply_split_counts()
        assert not vol._split_mask().any()
    finally:
        bnv.set_mlp_mode(1)
