"""Embedding training, the parts that run without a GPU: the float64 restatement against the reference's golden
step (train_step.npz), the patch dataset (pickle layout, split, _resize_input_pts), the synthetic patch generator,
and the trainer's weight layouts (npz keys, reference checkpoint keys)."""
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLDEN, WEIGHTS_FP32
import train_restatement as rs


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "train_step.npz"))


def _rows(g, k, a):
    return a[g["rows"]] if k in ("nerf.geo_layer1.weight", "nerf.geo_layer2.weight", "nerf.geo_layer3.weight") else a


def test_restatement_matches_reference_golden(golden):
    from bnv_fusion_amd import weights
    sd = weights.load_npz(WEIGHTS_FP32)
    batch = (golden["input_pts"], golden["training_pts"], golden["gt"], int(golden["n"]))
    losses, grads, final = rs.train_steps(sd, [batch] * 3)
    np.testing.assert_allclose(np.array(losses), golden["losses"], rtol=1e-5)
    for k, g in grads.items():
        want = golden["grad/" + k]
        scale = float(golden["gmax/" + k])
        if ".conv" in k and k.endswith(".bias"):     # zero in exact arithmetic under train-mode BatchNorm
            conv_w = float(golden["gmax/" + k.replace(".bias", ".weight")])
            assert np.abs(_rows(golden, k, g.numpy())).max() < 1e-6 * conv_w, k
            continue
        err = np.abs(_rows(golden, k, g.numpy()) - want).max()
        assert err <= 1e-4 * scale, (k, err, scale)
    for k, v in final.items():
        got = _rows(golden, k, v.numpy())
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(golden["after/" + k]) == int(sd[k]) + 3
            continue
        g1 = _rows(golden, k, grads[k].numpy()) if k in grads else None
        assert_params_close(k, got, golden, g1)


def noise_tolerance(k, g1, gmax, lr=1e-3, steps=3, base=1e-6):
    """Per-element tolerance of a parameter after ``steps`` Adam steps.  1e-6 in general.  Adam normalises every
    gradient element, so an element whose gradient is at the rounding-noise level moves by about +-lr per step whatever
    the noise's sign: the four conv biases (zero gradient in exact arithmetic: train-mode BatchNorm removes them, so
    they have no effect on the output), the running means that absorb them, and any weight element whose step-1
    gradient is below 1e-2 of its tensor's largest (fp32 rounding of the gradient, up to 1e-4 of the largest entry, is
    then >= 1e-2 relative and Adam passes it on at that size) -- those get 2 lr steps."""
    loose = 2 * lr * steps
    if (".conv" in k and k.endswith(".bias")) or k.endswith("running_mean"):
        return np.full(np.shape(g1) if g1 is not None else (), loose)
    if g1 is None:
        return base
    return np.where(np.abs(g1) < 1e-2 * gmax, loose, base)


def assert_params_close(k, got, golden, g1, base=1e-6):
    want = golden["after/" + k]
    gmax = float(golden["gmax/" + k]) if ("gmax/" + k) in golden.files else 0.0
    tol = noise_tolerance(k, g1, gmax, base=base)
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.all(err <= tol), (k, float(err.max()))


def _patch(rng, k, M):
    return {"input_pts": rng.normal(size=(k, 6)).astype(np.float32), "center": rng.normal(size=(1, 3)),
            "training_pts": rng.uniform(-1, 1, (M, 3)).astype(np.float32),
            "gt_sdf": rng.normal(size=M).astype(np.float32)}


def test_local_patch_dataset_layout_split_and_resize(tmp_path):
    from bnv_fusion_amd import datasets
    rng = np.random.default_rng(0)
    written = {}
    for cat in datasets.PATCH_CATEGORIES:
        for s in range(12):
            seq = f"seq{s:02d}"
            ks = [5 if s == 0 else 80, 12, 64]             # seq00: small patches (val skips < 16)
            written[(cat, seq)] = [_patch(rng, k, 7) for k in ks]
            datasets.write_local_patches(str(tmp_path), cat, seq, written[(cat, seq)])
    tr = datasets.LocalPatchDataset(str(tmp_path), "train", seed=1)
    va = datasets.LocalPatchDataset(str(tmp_path), "val", seed=1)
    assert len(tr) == 2 * 2 * 3 and len(va) == 2 * 10       # train = sorted(seqs)[10:], val = [:10] per category
    assert all(os.path.basename(os.path.dirname(p)) in ("seq10", "seq11") for p in tr.file_paths)
    item = tr[0]
    src = written[(datasets.PATCH_CATEGORIES[0], "seq10")][0]
    assert item["input_pts"].shape == (64, 6)
    # resize: 80 points -> a permutation's first 64 (distinct rows of the source)
    rows = {r.tobytes() for r in src["input_pts"]}
    assert all(r.tobytes() in rows for r in item["input_pts"])
    assert len({r.tobytes() for r in item["input_pts"]}) == 64
    np.testing.assert_array_equal(item["training_pts"], src["training_pts"])
    np.testing.assert_array_equal(item["gt"], src["gt_sdf"])
    # 12 points -> drawn with replacement to 64
    small = tr[1]["input_pts"]
    assert small.shape == (64, 6) and len({r.tobytes() for r in small}) <= 12
    v0 = va[0]                                     # seq00: the 5- and 12-point patches are skipped
    assert v0["input_pts"].shape == (1, 64, 6)
    assert va[1]["input_pts"].shape == (2, 64, 6)
    b = next(tr.batches(5))
    assert b["input_pts"].shape == (5, 64, 6) and b["training_pts"].shape == (5, 7, 3) and b["gt"].shape == (5, 7)


def test_patch_unpickler_admits_only_plain_data(tmp_path):
    from bnv_fusion_amd import datasets

    class Evil:
        def __reduce__(self):
            return (os.getcwd, ())
    p = tmp_path / "evil.pkl"
    with open(p, "wb") as fh:
        pickle.dump({"input_pts": Evil()}, fh)
    with pytest.raises(pickle.UnpicklingError):
        datasets.read_local_patch(str(p))


def _dense_surface(s, step=0.02):
    """An independent dense sampling of the shape's surface near the cube [-1, 1]^3 (parametric, not the
    generator's closest-point map)."""
    k = s["kind"]
    if k == "plane":
        n = s["normal"]
        u = np.cross(n, [1.0, 0, 0] if abs(n[0]) < 0.9 else [0, 1.0, 0])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        t = np.arange(-3.5, 3.5, step)
        a, b = np.meshgrid(t, t, indexing="ij")
        return s["point"] + a.reshape(-1, 1) * u + b.reshape(-1, 1) * v
    if k == "sphere":
        r = s["radius"]
        nt = int(np.pi * r / step) + 8
        th = np.linspace(0, np.pi, nt)
        ph = np.linspace(0, 2 * np.pi, 2 * nt)
        a, b = np.meshgrid(th, ph, indexing="ij")
        d = np.stack([np.sin(a) * np.cos(b), np.sin(a) * np.sin(b), np.cos(a)], -1).reshape(-1, 3)
        return s["center"] + r * d
    if k == "cylinder":
        ax, r = s["axis"], s["radius"]
        u = np.cross(ax, [1.0, 0, 0] if abs(ax[0]) < 0.9 else [0, 1.0, 0])
        u /= np.linalg.norm(u)
        v = np.cross(ax, u)
        c0 = s["center"] - (s["center"] @ ax) * ax          # the axis point nearest the origin
        ph = np.linspace(0, 2 * np.pi, int(2 * np.pi * r / step) + 8)
        t = np.arange(-3.5, 3.5, step)
        a, b = np.meshgrid(ph, t, indexing="ij")
        a, b = a.reshape(-1, 1), b.reshape(-1, 1)
        return c0 + b * ax + r * (np.cos(a) * u + np.sin(a) * v)
    R, h = s["rotation"], s["half"]
    pts = []
    for axis in range(3):
        o = [i for i in range(3) if i != axis]
        ta = np.arange(-h[o[0]], h[o[0]] + step, step).clip(-h[o[0]], h[o[0]])
        tb = np.arange(-h[o[1]], h[o[1]] + step, step).clip(-h[o[1]], h[o[1]])
        a, b = np.meshgrid(ta, tb, indexing="ij")
        for sign in (-1, 1):
            q = np.zeros((a.size, 3))
            q[:, o[0]], q[:, o[1]], q[:, axis] = a.ravel(), b.ravel(), sign * h[axis]
            pts.append(q)
    return s["center"] + np.concatenate(pts) @ R.T


def test_synthetic_local_patches():
    from scipy.spatial import cKDTree
    from bnv_fusion_amd import synthetic
    d = synthetic.local_patches(24, 40, seed=3)
    assert d["input_pts"].shape == (24, 64, 6) and d["training_pts"].shape == (24, 40, 3) and d["gt"].shape == (24, 40)
    assert np.abs(d["input_pts"][..., :3]).max() <= 1.0 and np.abs(d["training_pts"]).max() <= 1.0
    np.testing.assert_allclose(np.linalg.norm(d["input_pts"][..., 3:], axis=-1), 1.0, atol=1e-5)
    kinds = set()
    for i, s in enumerate(d["shapes"]):
        kinds.add(s["kind"])
        # input points lie on the surface, their normals are the SDF gradient
        p = d["input_pts"][i, :, :3].astype(np.float64)
        assert np.abs(synthetic.shape_sdf(s, p)).max() < 1e-5, s["kind"]
        e = 1e-4
        grad = np.stack([(synthetic.shape_sdf(s, p + e * np.eye(3)[a]) - synthetic.shape_sdf(s, p - e * np.eye(3)[a]))
                         / (2 * e) for a in range(3)], -1)
        agree = np.sum(grad * d["input_pts"][i, :, 3:], -1)
        assert np.mean(agree > 0.99) > 0.9, s["kind"]       # box edges / corners excepted
        # |gt| = distance to a dense sampling of the shape (within the sampling's resolution)
        dist, _ = cKDTree(_dense_surface(s)).query(d["training_pts"][i].astype(np.float64))
        np.testing.assert_allclose(np.abs(d["gt"][i]), dist, atol=0.03, err_msg=s["kind"])
    assert kinds == set(synthetic.PATCH_KINDS)


def test_trainer_state_dict_layout_matches_checkpoint():
    from bnv_fusion_amd import train
    want = np.load(WEIGHTS_FP32)
    assert train.state_dict_keys() == list(want.files)
    sd = train.default_state_dict(seed=0)
    assert list(sd) == list(want.files)
    for k in want.files:
        assert sd[k].shape == want[k].shape and sd[k].dtype == want[k].dtype, k
    assert sum(int(np.prod(s)) for _, s in train.PARAM_SHAPES) == sum(
        want[k].size for k in want.files if k.endswith((".weight", ".bias")))
    # default init: torch's bounds, seeded
    assert np.abs(sd["nerf.geo_layer1.weight"]).max() <= 1 / 16 and np.abs(sd["nerf.geo_layer1.weight"]).max() > 0.06
    assert np.array_equal(train.default_state_dict(seed=0)["nerf.fc_alpha.weight"], sd["nerf.fc_alpha.weight"])
    assert not np.array_equal(train.default_state_dict(seed=1)["nerf.fc_alpha.weight"], sd["nerf.fc_alpha.weight"])


def test_ckpt_keys_match_reference_model(golden):
    from bnv_fusion_amd import train
    keys = [k for k, _ in train.PARAM_SHAPES] + list(np.load(WEIGHTS_FP32).files) + [k for k, _ in train.COLOR_HEAD_SHAPES]
    shapes = dict(train.PARAM_SHAPES + train.RUNNING_SHAPES + train.COLOR_HEAD_SHAPES)
    ref = dict(zip(golden["ref_keys"].tolist(), golden["ref_shapes"].tolist()))
    assert set(keys) == set(ref)
    for k, s in shapes.items():
        assert ",".join(str(x) for x in s) == ref[k], k


def test_trainer_shape_guards():
    from bnv_fusion_amd import train
    x, p, g = torch.zeros(2, 64, 6), torch.zeros(2, 5, 3), torch.zeros(2, 5)
    assert train.check_shapes(x, p, g, 4) == (2, 5)
    for bad in [(x, p, g, 65), (x, p, g, 0), (x[:1], p[:1], g[:1], 1), (x, p, torch.zeros(2, 6), 4),
                (torch.zeros(2, 63, 6), p, g, 4), (x, torch.zeros(3, 5, 3), g, 4)]:
        with pytest.raises(ValueError):
            train.check_shapes(*bad)
