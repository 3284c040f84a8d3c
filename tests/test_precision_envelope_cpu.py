"""The error envelope of the MLP arithmetics, derived on the CPU: the bars of tests/test_gpu_precision.py rest on it.

The three arithmetics of the fp32 checkpoint (exact fp32 = mode 0, split f16 = mode 1, f16 operands = mode 3) are
emulated layer by layer with numpy (oracle/precision.py) on the shipped checkpoint, on decoder and encoder inputs
built from the feature rows and points of tests/golden/sequence_64.npz, and compared with a float64 run of the same
network.  Units as on the GPU: decoder errors in alpha (= SDF / voxel), encoder errors relative to max |feature|,
feature gradients per evaluation relative to the row's largest component.  Emulated maxima (20,000 inputs):

  decoder forward   exact 4.8e-7   split 1.1e-6   f16 2.2e-3      alpha
  encoder forward   exact 4.0e-7   split 4.7e-7   f16 7.1e-4      relative
  decoder backward  exact 2.6e-6   split 2.2e-6   (f16 unusable)  relative, evaluations off the ReLU kinks
  hidden pre-activations, split: 1.0e-6 (|z| up to ~2)
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, WEIGHTS_FP32
from oracle import bnv_oracle as orc
from oracle import precision as P

N = 20000
# bounds the emulation must stay below; the GPU bars (test_gpu_precision.py) sit ~4-10x above them
DEC_FP32_CLASS = 2.5e-6       # alpha, modes 0 / 1        (GPU bar 1e-5)
ENC_FP32_CLASS = 1.5e-6       # relative, modes 0 / 1     (GPU bar 5e-6)
BWD_FP32_CLASS = 5e-6         # relative per evaluation   (GPU bar 2e-5)
KINK_DELTA = 4e-6             # test_gpu_precision.KINK_DELTA: 4x the largest split pre-activation error


@pytest.fixture(scope="module")
def sd():
    return orc.load_weights(WEIGHTS_FP32)


@pytest.fixture(scope="module")
def decoder_inputs():
    z = np.load(os.path.join(GOLDEN, "sequence_64.npz"))
    live = z["features_sorted"][z["weights_sorted"][:, 0] >= 8]
    rng = np.random.default_rng(0)
    feats = live[rng.integers(len(live), size=N)]
    local = rng.uniform(-1, 1, size=(N, 3)).astype(np.float32)
    local[: N // 4] = rng.choice([-0.5, 0.0, 0.5], size=(N // 4, 3))          # the lattice offsets too
    return P.sdf_inputs(local, feats)


@pytest.fixture(scope="module")
def encoder_inputs():
    z = np.load(os.path.join(GOLDEN, "sequence_64.npz"))
    pts = z["frames"].reshape(-1, 6)
    rng = np.random.default_rng(1)
    rel = rng.uniform(-1, 1, size=(N, 3))
    return np.concatenate([rel, pts[rng.integers(len(pts), size=N), 3:]], axis=1).astype(np.float32)


def test_decoder_forward_envelope(sd, decoder_inputs):
    L = P.sdf_layers(sd)
    ref = P.mlp(L, decoder_inputs, "f64")
    # the float64 oracle network is the same function as the float64 emulation
    o64 = orc.geo_forward(P.state_dict_f64(sd), torch.from_numpy(decoder_inputs)).numpy()
    assert P.max_err(o64, ref) < 1e-12
    err = {m: P.max_err(P.mlp(L, decoder_inputs, m, fp32_last=True), ref) for m in ("exact", "split", "f16")}
    assert err["exact"] < DEC_FP32_CLASS and err["split"] < DEC_FP32_CLASS, err
    assert err["f16"] >= 100 * err["split"], err
    assert 1e-4 <= err["f16"] <= 1e-2, err                        # the mode-3 window of the GPU tests
    # a split kernel that lost its lo products IS the f16 arithmetic: it cannot pass the fp32-class bar
    assert err["f16"] > 10 * 1e-5


def test_encoder_forward_envelope(sd, encoder_inputs):
    L = P.pointnet_layers(sd)
    ref = orc.pointnet_encoder(P.state_dict_f64(sd), torch.from_numpy(encoder_inputs.T[None])).numpy()[0].T
    scale = np.abs(ref).max()
    err = {m: P.max_err(P.mlp(L, encoder_inputs, m), ref) / scale for m in ("exact", "split", "f16")}
    assert err["exact"] < ENC_FP32_CLASS and err["split"] < ENC_FP32_CLASS, err
    assert err["f16"] >= 100 * err["split"], err


def test_decoder_backward_envelope(sd, decoder_inputs):
    L = P.sdf_layers(sd)
    g = np.random.default_rng(2).uniform(-1, 1, size=N)
    pre = []
    P.mlp(L, decoder_inputs, "f64", preacts=pre)
    pre_s = []
    P.mlp(L, decoder_inputs, "split", fp32_last=True, preacts=pre_s)
    pre_err = max(P.max_err(a, b) for a, b in zip(pre_s, pre))
    assert 4 * pre_err <= KINK_DELTA, pre_err                   # a mask flip needs |z| below the pre-activation error
    near = np.zeros(N, bool)
    for z in pre:
        near |= (np.abs(z) < KINK_DELTA).any(1)
    assert near.mean() < 0.05, near.mean()                        # per evaluation; a query blends 8
    ref = P.mlp_input_grad(L, decoder_inputs, g, "f64")[:, 9:]
    for m in ("exact", "split"):
        got = P.mlp_input_grad(L, decoder_inputs, g, m)[:, 9:]
        rel = np.abs(got - ref).max(1) / np.abs(ref).max(1).clip(1e-30)
        assert rel[~near].max() < BWD_FP32_CLASS, (m, rel[~near].max())


def _f32_and_f64_volumes(sd):
    z = np.load(os.path.join(GOLDEN, "sequence_64.npz"))
    vols = []
    for dt in (torch.float32, torch.float64):
        v = orc.OracleSparseVolume(8, float(z["voxel_size"]), z["dims"], 8, dtype=dt)
        n = len(z["keys_sorted"])
        v.insert(torch.from_numpy(z["keys_sorted"]), torch.from_numpy(z["features_sorted"]).to(dt),
                 torch.from_numpy(z["weights_sorted"]).to(dt), torch.zeros(n, 1, dtype=dt))
        v.to_tensor()
        vols.append(v)
    return vols


def test_float64_oracle_agrees_with_reference_decode_goldens(sd):
    """The float64 decode (fp32 voxel geometry, float64 from the MLP inputs on) against the reference's own outputs,
    to within the fp32 oracle's distance to them -- or, where that is 0 (bitwise equal), within the fp32-class
    envelope: the reference ran fp32 itself; mask decisions identical."""
    v32, v64 = _f32_and_f64_volumes(sd)
    sd64 = P.state_dict_f64(sd)
    z = np.load(os.path.join(GOLDEN, "decode_64.npz"))
    delta = torch.from_numpy(z["sdf_delta"])
    cases = {"lattice_qt": (z["lattice_coords"], None, True, True), "lattice_q": (z["lattice_coords"], None, True, False),
             "lattice_delta": (z["lattice_coords"], delta, True, True), "random_qt": (z["random_coords"], None, True, True),
             "random_world_out": (z["random_world_coords"], None, False, False),
             "random_delta": (z["random_coords"], delta, True, True)}
    voxel = float(v32.voxel_size)
    for key, (c, d, is_coords, qt) in cases.items():
        c = torch.from_numpy(c)
        o32 = v32.decode_pts(c, sd, d, is_coords=is_coords, query_tensor=qt)
        o64 = v64.decode_pts(c, sd64, d, is_coords=is_coords, query_tensor=qt)
        assert o32.dtype == torch.float32 and o64.dtype == torch.float64
        e32, e64 = P.max_err(o32, z[key]), P.max_err(o64, z[key])
        assert e64 <= max(2 * e32, DEC_FP32_CLASS * voxel), (key, e32, e64)
        if d is None:
            assert torch.equal(o64 == voxel, torch.from_numpy(z[key]) == np.float32(voxel)), key


def test_float64_oracle_agrees_with_reference_dense_and_encode_goldens(sd):
    sd64 = P.state_dict_f64(sd)
    z = np.load(os.path.join(GOLDEN, "dense_decode_64.npz"))
    mn, mx, n_xyz = orc.get_world_range(z["dims"], float(z["voxel_size"]))
    voxel = float(z["voxel_size"])
    mn, mx = torch.from_numpy(mn).float(), torch.from_numpy(mx).float()
    n_xyz = torch.tensor(n_xyz)
    pts = torch.from_numpy(z["input_pts"])
    fg32, mask, _, _ = orc.encode_pointcloud(sd, pts, n_xyz, mn, mx, voxel, return_dense=True)
    fg64, mask64, _, _ = orc.encode_pointcloud(sd64, pts, n_xyz, mn, mx, voxel, return_dense=True)
    assert fg64.dtype == torch.float64 and torch.equal(mask64, mask.double())
    q = torch.from_numpy(z["queries"])
    s32, _ = orc.decode_feature_grid_w_pts(sd, q, fg32, mask, voxel)
    s64, _ = orc.decode_feature_grid_w_pts(sd64, q, fg64, mask64, voxel)
    e32, e64 = P.max_err(s32, z["sdf"]), P.max_err(s64, z["sdf"])
    assert e64 <= max(2 * e32, DEC_FP32_CLASS * voxel), (e32, e64)
    assert torch.equal(s64 == voxel, torch.from_numpy(z["sdf"]) == np.float32(voxel))

    e = np.load(os.path.join(GOLDEN, "encode_64.npz"))
    args = (torch.from_numpy(e["input_pts"]), torch.from_numpy(e["n_xyz"]), torch.from_numpy(e["min_coords"]),
            torch.from_numpy(e["max_coords"]), float(e["voxel_size"]))
    f32, c32, ids32, _, _ = orc.encode_pointcloud(sd, *args)
    f64, c64, ids64, _, _ = orc.encode_pointcloud(sd64, *args)
    assert f64.dtype == torch.float64
    assert torch.equal(ids64, ids32) and torch.equal(c64, c32)                # integer decisions unchanged
    assert np.array_equal(ids64.numpy(), e["flat_ids"])
    e32, e64 = P.max_err(f32, e["feats"]), P.max_err(f64, e["feats"])
    assert e64 <= max(2 * e32, ENC_FP32_CLASS * float(np.abs(e["feats"]).max())), (e32, e64)
