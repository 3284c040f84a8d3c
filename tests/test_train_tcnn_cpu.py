"""Training of the tiny-cuda-nn embedding, the parts that run without a GPU: the torch restatement
(tcnn_train_restatement.py) against the oracle's inference restatement and against finite differences, the weight
layouts of train.TcnnEmbeddingTrainer, the learning bar of the GPU test, and the shape guards."""
import numpy as np
import pytest
import torch

from conftest import WEIGHTS_TCNN
import tcnn_train_restatement as rs

# Held-out L1 (voxel units) after 300 steps of B = 100, M = 256 from tcnn_default_state_dict(0), on the batches and
# n draws of test_gpu_train_tcnn.test_learns_synthetic_patches.  Chosen from the fp32 restatement's own run
# (test_restatement_learns_synthetic_patches below): 0.576 untrained -> 0.115 after 300 steps; the bar sits 30 % above
# the trained value, far below the untrained one.
LEARN_BAR = 0.15
LEARN_STEPS = 300


def _weights():
    from bnv_fusion_amd import weights
    return weights.load_npz(WEIGHTS_TCNN)


def test_restatement_forward_is_the_inference_restatement():
    from bnv_fusion_amd import synthetic
    from oracle import bnv_oracle as orc
    sd = {k: torch.from_numpy(v) for k, v in _weights().items()}
    d = synthetic.local_patches(6, 50, seed=2, noise=0.02)
    n = 17
    _, _, _, feats, pred = rs.forward(sd, d["input_pts"], d["training_pts"], d["gt"], n, dtype=torch.float32)
    enc = orc.tcnn_point_encoder(sd[rs.KEYS[0]])
    x = torch.from_numpy(d["input_pts"][:, :n]).reshape(-1, 6)
    want_f = enc(x.t()[None])[0].t().reshape(6, n, 8).mean(1).half().float()
    assert torch.equal(feats.detach(), want_f)
    pts = torch.from_numpy(d["training_pts"])
    geo_in = torch.cat([orc.xyz_encoding(pts), want_f[:, None, :].expand(6, 50, 8)], -1)
    want_p = orc.tcnn_geo_forward(sd[rs.KEYS[1]])(geo_in)[..., 0]
    assert torch.equal(pred.detach(), want_p)


def test_float64_gradients_match_finite_differences():
    from bnv_fusion_amd import synthetic, train
    d = synthetic.local_patches(2, 4, seed=4, noise=0.02)
    sd = train.tcnn_default_state_dict(seed=1)
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
    args = (d["input_pts"], d["training_pts"], d["gt"], 3)
    loss = rs.forward(p, *args, half=False)[0]
    loss.backward()
    rng = np.random.default_rng(0)
    eps = 1e-6
    for k in rs.KEYS:
        g = p[k].grad.numpy()
        idx = np.concatenate([rng.choice(g.size, 40, replace=False), np.argsort(-np.abs(g))[:10]])
        for i in idx:
            q = {kk: v.detach().clone() for kk, v in p.items()}
            q[k][i] += eps
            up = float(rs.forward(q, *args, half=False)[0])
            q[k][i] -= 2 * eps
            dn = float(rs.forward(q, *args, half=False)[0])
            fd = (up - dn) / (2 * eps)
            assert abs(fd - g[i]) <= 1e-6 + 1e-5 * np.abs(g).max(), (k, int(i), fd, float(g[i]))


def test_state_dict_layout_matches_checkpoint():
    from bnv_fusion_amd import train
    want = np.load(WEIGHTS_TCNN)
    assert [k for k, _ in train.TCNN_SHAPES] == list(want.files) == list(rs.KEYS)
    sd = train.tcnn_default_state_dict(seed=0)
    assert list(sd) == list(want.files)
    for k in want.files:
        assert sd[k].shape == want[k].shape and sd[k].dtype == want[k].dtype, k
    # Xavier bounds per matrix, seeded
    w1 = sd[rs.KEYS[1]][32 * 64: 32 * 64 + 64 * 64]
    assert np.abs(w1).max() <= np.sqrt(6 / 128) and np.abs(w1).max() > 0.95 * np.sqrt(6 / 128)
    assert np.array_equal(train.tcnn_default_state_dict(seed=0)[rs.KEYS[0]], sd[rs.KEYS[0]])
    assert not np.array_equal(train.tcnn_default_state_dict(seed=1)[rs.KEYS[0]], sd[rs.KEYS[0]])


def test_ckpt_layout_is_what_the_reference_loads(tmp_path):
    """save_ckpt / save_npz, written without a GPU (the trainer's methods on a host-side stand-in): the reference's
    LitFusionPointNet(tiny_cuda=True) state_dict holds exactly the two flat vectors (tests/golden/
    convert_checkpoints.py)."""
    from bnv_fusion_amd import fusion, train
    stand_in = object.__new__(train.TcnnEmbeddingTrainer)
    stand_in.params = torch.from_numpy(np.concatenate([v for v in _weights().values()]))
    ck, npz = str(tmp_path / "w.ckpt"), str(tmp_path / "w.npz")
    stand_in.save_ckpt(ck)
    stand_in.save_npz(npz)
    sd = torch.load(ck)["state_dict"]
    want = np.load(WEIGHTS_TCNN)
    assert list(sd) == list(want.files)
    z = np.load(npz)
    for k in want.files:
        assert sd[k].dtype == torch.float32 and tuple(sd[k].shape) == want[k].shape
        assert np.array_equal(sd[k].numpy(), want[k]) and np.array_equal(z[k], want[k]) and z[k].dtype == want[k].dtype
    model = fusion.LitFusionPointNet({"trainer": {"dense_volume": False},
                                      "model": {"feature_vector_size": 8, "voxel_size": 0.01, "tiny_cuda": True,
                                                "min_pts_in_grid": 8,
                                                "nerf": {"hidden_size": 256, "num_layers": 4, "num_encoding_fn_xyz": 1,
                                                         "interpolate_decode": True}}})
    assert sorted(model.state_dict()) == sorted(sd)


def test_restatement_learns_synthetic_patches():
    from bnv_fusion_amd import synthetic, train
    B, M = 100, 256
    d = synthetic.local_patches(40 * B, M, seed=11, noise=0.02)
    batches = [{k: d[k][i * B:(i + 1) * B] for k in ("input_pts", "training_pts", "gt")} for i in range(40)]
    held = synthetic.local_patches(400, M, seed=12345, noise=0.02)
    sd = train.tcnn_default_state_dict(0)
    rng = np.random.default_rng(0)      # TcnnEmbeddingTrainer(seed=0).draw_n
    ns = [int(rng.integers(train.MIN_PTS_IN_GRID // 2, train.N_LOCAL_SAMPLES)) for _ in range(LEARN_STEPS)]
    p0 = {k: torch.from_numpy(v) for k, v in sd.items()}
    before = float(rs.forward(p0, held["input_pts"], held["training_pts"], held["gt"], 64, dtype=torch.float32)[1])
    steps = [(batches[i % 40]["input_pts"], batches[i % 40]["training_pts"], batches[i % 40]["gt"], ns[i])
             for i in range(LEARN_STEPS)]
    _, _, final, skipped, _ = rs.train_steps(sd, steps, dtype=torch.float32)
    after = float(rs.forward(final, held["input_pts"], held["training_pts"], held["gt"], 64, dtype=torch.float32)[1])
    print(f"\nrestatement: held-out L1 {before:.4f} -> {after:.4f} (bar {LEARN_BAR})")
    assert not any(skipped)
    assert before > 2 * LEARN_BAR and after < 0.8 * LEARN_BAR, (before, after)


def test_tcnn_shape_guards():
    from bnv_fusion_amd import train
    x, p, g = torch.zeros(2, 64, 6), torch.zeros(2, 5, 3), torch.zeros(2, 5)
    assert train.check_tcnn_shapes(x, p, g, 4) == (2, 5)
    assert train.check_tcnn_shapes(x[:1], p[:1], g[:1], 1) == (1, 5)      # no BatchNorm: B n = 1 is valid
    for bad in [(x, p, g, 65), (x, p, g, 0), (x, p, torch.zeros(2, 6), 4), (torch.zeros(2, 63, 6), p, g, 4),
                (x, torch.zeros(3, 5, 3), g, 4), (x, torch.zeros(2, 0, 3), torch.zeros(2, 0), 4),
                (torch.zeros(0, 64, 6), torch.zeros(0, 5, 3), torch.zeros(0, 5), 4),
                (torch.zeros(2, 64, 6), torch.zeros(2, 1 << 23 | 1, 3)[:, :, :], torch.zeros(2, 1 << 23 | 1), 4)]:
        with pytest.raises(ValueError):
            train.check_tcnn_shapes(*bad)
