"""Training of the tiny-cuda-nn embedding on the GPU (csrc/train_tcnn.hip, train.TcnnEmbeddingTrainer): the forward
against the fp32 restatement, one step against float64 across shapes, three Adam steps, bit-reproducibility,
learning on synthetic patches, the skip of an overflowing step, the trained weights feeding fusion, shape guards."""
import numpy as np
import pytest
import torch

from conftest import WEIGHTS_TCNN
import tcnn_train_restatement as rs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# declared end-to-end precision of a gradient, of its tensor's largest |gradient| (include/bnv_fusion.h): the hi + lo
# f16 backward itself is near fp32; what remains is the f16 forward's rounding decisions -- a value one f16 ulp from
# the float64 restatement's flips sign(pred - gt) or a ReLU downstream (the fp32 restatement flips at other places)
BACKWARD_BOUND = 5e-3


def _trainer(sd=None, seed=0):
    from bnv_fusion_amd import train, weights
    init = weights.load_npz(WEIGHTS_TCNN) if sd == "pretrained" else (None if sd == "scratch" else sd)
    return train.TcnnEmbeddingTrainer(init, seed=seed, device=DEV)


def _init(kind, seed=0):
    from bnv_fusion_amd import train, weights
    return weights.load_npz(WEIGHTS_TCNN) if kind == "pretrained" else train.tcnn_default_state_dict(seed)


def _batches(n_batches, B, M, seed):
    from bnv_fusion_amd import synthetic
    d = synthetic.local_patches(n_batches * B, M, seed=seed, noise=0.02)
    return [{k: d[k][i * B:(i + 1) * B] for k in ("input_pts", "training_pts", "gt")} for i in range(n_batches)]


def _ulp16(x):
    return np.spacing(np.abs(x).astype(np.float16)).astype(np.float64)


@pytest.mark.parametrize("init", ["pretrained", "scratch"])
def test_forward_matches_fp32_restatement(init):
    b = _batches(1, 37, 300, seed=5)[0]
    t = _trainer(init)
    feats, pred = t.forward(b["input_pts"], b["training_pts"], n=64)
    from oracle import bnv_oracle as orc
    p = {k: torch.from_numpy(v) for k, v in _init(init).items()}
    _, _, _, f_ref, _ = rs.forward(p, b["input_pts"], b["training_pts"], b["gt"], 64, dtype=torch.float32)
    # the decoder on the GPU's feats: one f16 ulp of a feature moves pred by far more than an ulp of pred, so each
    # network is checked on the same inputs
    pts = torch.from_numpy(b["training_pts"])
    f_gpu = feats.cpu()
    geo_in = torch.cat([orc.xyz_encoding(pts), f_gpu[:, None, :].expand(-1, pts.shape[1], 8)], -1)
    p_ref = orc.tcnn_geo_forward(p[rs.KEYS[1]])(geo_in)[..., 0]
    for name, got, want in (("feats", feats, f_ref), ("pred", pred, p_ref)):
        got = got.cpu().numpy().astype(np.float64)
        want = want.detach().numpy().astype(np.float64)
        err = np.abs(got - want)
        ulp = np.maximum(_ulp16(got), _ulp16(want))
        print(f"\n{init} {name}: bit-equal {np.mean(got == want):.4f}, max err {err.max():.3g}, "
              f"max err / ulp {float((err / ulp).max()):.2f}")
        if name == "pred":
            # the hidden layers run at unit scale: one of their values an f16 ulp off (an fp32 accumulation order
            # on the other side of a rounding boundary) moves a small pred by up to an ulp at that scale
            ulp = np.maximum(ulp, _ulp16(np.ones(1)))
        assert np.all(err <= ulp), (name, float((err / ulp).max()))


def _grad_check(t, sd, batch, label):
    _, g64, _, _, _ = rs.train_steps(sd, [batch])
    losses, _, _, _, _ = rs.train_steps(sd, [batch])
    _, g32, _, _, _ = rs.train_steps(sd, [batch], dtype=torch.float32)
    got = t.gradients()
    for k in rs.KEYS:
        w = g64[k].numpy()
        err32 = float(np.abs(g32[k].double().numpy() - w).max())
        err = float(np.abs(got[k].cpu().numpy().astype(np.float64) - w).max())
        tol = 2 * err32 + BACKWARD_BOUND * float(np.abs(w).max())
        print(f"{label} {k}: max err {err:.3g} (fp32 restatement {err32:.3g}, tol {tol:.3g}, "
              f"max |g| {np.abs(w).max():.3g})")
        assert err <= tol, (label, k, err, tol)
    return losses


SHAPES = [(1, 1, 1), (3, 5, 7), (37, 64, 1000), (100, 64, 256)]


@pytest.mark.parametrize("init", ["pretrained", "scratch"])
@pytest.mark.parametrize("B,n,M", SHAPES)
def test_one_step_matches_float64(init, B, n, M):
    b = _batches(1, B, M, seed=B * 1000 + n * 10 + M)[0]
    sd = _init(init)
    t = _trainer(init)
    out = t.step(**b, n=n)
    batch = (b["input_pts"], b["training_pts"], b["gt"], n)
    losses = _grad_check(t, sd, batch, f"{init} B={B} n={n} M={M}")
    got = np.array([float(out["loss"]), float(out["bce_loss"]), float(out["reg_loss"])])
    np.testing.assert_allclose(got, np.array(losses[0]), rtol=1e-4, atol=1e-6)
    assert not bool(out["skipped"])
    # output rows nothing reads: exactly zero
    g = t.gradients()
    enc = g["pointnet_backbone.model.params"].cpu().numpy()[-16 * 64:].reshape(16, 64)
    dec = g["nerf.model.params"].cpu().numpy()[-16 * 64:].reshape(16, 64)
    assert np.all(enc[8:] == 0) and np.all(dec[1:] == 0)


def _params_close(got, want, g1, steps, base=1e-5, lr=1e-3):
    """``base`` in general; an element whose step-1 gradient is under 1e-2 of its tensor's largest gets 2 lr steps
    (Adam passes its rounding noise on at about lr per step; test_train_cpu.noise_tolerance)."""
    for k in rs.KEYS:
        g = np.abs(g1[k])
        tol = np.where(g < 1e-2 * g.max(), 2 * lr * steps, base)
        err = np.abs(got[k].astype(np.float64) - want[k].numpy())
        assert np.all(err <= tol), (k, float(err.max()))


def test_three_adam_steps_match_restatement():
    bs = _batches(3, 20, 64, seed=3)
    sd = _init("pretrained")
    t = _trainer("pretrained")
    for b in bs:
        t.step(**b, n=33)
    _, g1, final, skipped, _ = rs.train_steps(sd, [(b["input_pts"], b["training_pts"], b["gt"], 33) for b in bs])
    assert not any(skipped)
    assert int(t.adam_step.item()) == 3
    _params_close(t.state_dict(), final, {k: v.numpy() for k, v in g1.items()}, 3)


def test_fifty_steps_are_bit_reproducible():
    bs = _batches(5, 40, 64, seed=7)
    runs = []
    for _ in range(2):
        t = _trainer(seed=3)
        losses = [t.step(**bs[i % 5])["loss"] for i in range(50)]
        runs.append((torch.stack(losses).cpu().numpy(), t.state_dict()))
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    for k in rs.KEYS:
        assert runs[0][1][k].tobytes() == runs[1][1][k].tobytes(), k


LEARN_STEPS = 300
# Held-out L1 bar after LEARN_STEPS steps of B = 100, M = 256 from scratch (seed 0).  Fixed from the fp32 torch
# restatement on the CPU (test_train_tcnn_cpu.test_restatement_learns_synthetic_patches; tools-free, same batches,
# same n draws): see LEARN_BAR there.
from test_train_tcnn_cpu import LEARN_BAR  # noqa: E402


def test_learns_synthetic_patches():
    from bnv_fusion_amd import synthetic
    B, M = 100, 256
    train_b = _batches(40, B, M, seed=11)
    held = synthetic.local_patches(400, M, seed=12345, noise=0.02)
    held = {k: held[k] for k in ("input_pts", "training_pts", "gt")}
    t = _trainer(seed=0)
    before = float(t.eval_loss(held))
    ns = [t.draw_n() for _ in range(20)]
    t.rng = np.random.default_rng(0)
    tb = [(b["input_pts"], b["training_pts"], b["gt"], n) for b, n in zip(train_b, ns)]
    torch_losses, _, _, _, _ = rs.train_steps(_init("scratch"), tb, dtype=torch.float32)
    curve = []
    for i in range(LEARN_STEPS):
        out = t.step(**train_b[i % len(train_b)], n=ns[i] if i < 20 else None)
        if i < 20:
            curve.append(float(out["loss"]))
    after = float(t.eval_loss(held))
    print(f"\nlearning: held-out L1 {before:.4f} -> {after:.4f} after {LEARN_STEPS} steps (bar {LEARN_BAR})")
    for i in range(20):
        print(f"  {i:2d} {curve[i]:.6f} {torch_losses[i][0]:.6f}")
    np.testing.assert_allclose(curve, [x[0] for x in torch_losses], rtol=1e-2)
    assert before > LEARN_BAR, "the untrained model must fail the bar"
    assert after < LEARN_BAR, (before, after)


def test_overflow_step_is_skipped():
    b1, b2, b3 = _batches(3, 10, 32, seed=9)
    sd = _init("pretrained")
    t = _trainer("pretrained")
    t.step(**b1, n=20)
    good = t.params.clone()
    snap = [x.clone() for x in (t.exp_avg, t.exp_avg_sq, t.adam_step)]
    # decoder hidden matrices 1 and 2 (64 x 64) times 1e4: the activations pass 65504 and the f16 forward overflows
    o = 10240 + 32 * 64
    t.params[o: o + 2 * 64 * 64] *= 1e4
    bad = t.params.clone()
    out = t.step(**b2, n=20)
    assert bool(out["skipped"]), [float(v) for v in (out["loss"], out["bce_loss"])]
    assert torch.equal(t.params.view(torch.int32), bad.view(torch.int32))
    for x, y in zip((t.exp_avg, t.exp_avg_sq, t.adam_step), snap):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y)
    t.params.copy_(good)
    out = t.step(**b3, n=20)
    assert not bool(out["skipped"]) and int(t.adam_step.item()) == 2
    _, g1, final, skipped, _ = rs.train_steps(sd, [(b["input_pts"], b["training_pts"], b["gt"], 20) for b in (b1, b3)])
    assert not any(skipped)
    _params_close(t.state_dict(), final, {k: v.numpy() for k, v in g1.items()}, 2)


def test_trained_weights_feed_fusion(tmp_path):
    """save_npz -> load_pretrained(tiny_cuda=True, path=...) -> NeuralMap on a synthetic frame, against the oracle's
    tcnn restatement of inference with the trained weights; then a mesh."""
    import bnv_fusion_amd as bnv
    from bnv_fusion_amd import synthetic
    from oracle import bnv_oracle as orc
    t = _trainer("pretrained")
    for b in _batches(5, 50, 64, seed=21):
        t.step(**b)
    path = str(tmp_path / "trained.npz")
    t.save_npz(path)
    z = np.load(path)
    for k, v in np.load(WEIGHTS_TCNN).items():
        assert z[k].shape == v.shape and z[k].dtype == v.dtype, k
    assert not np.array_equal(z[rs.KEYS[1]], np.load(WEIGHTS_TCNN)[rs.KEYS[1]])
    dims, voxel = np.array([1.24] * 3), 0.02
    pts = torch.from_numpy(synthetic.frame(0, H=120, W=160))
    pts[..., :3] *= 0.3
    sd = orc.load_weights(path)
    enc = orc.tcnn_point_encoder(sd[rs.KEYS[0]])
    geo = orc.tcnn_geo_forward(sd[rs.KEYS[1]])
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel, path=path, tiny_cuda=True)
    nm = bnv.NeuralMap(dims, voxel, model, device=DEV)
    ovol = orc.OracleSparseVolume(8, voxel, dims, 8)
    for _ in range(9):
        coords, sdf = nm.fuse_and_decode({"input_pts": pts.to(DEV)})
        f, c, ids, g, n = orc.encode_pointcloud(None, pts, ovol.n_xyz, ovol.min_coords, ovol.max_coords, voxel,
                                                encoder=enc)
        orc.integrate(ovol, g, f, c)
    torch.cuda.synchronize()
    assert torch.equal(coords.cpu(), g)
    # decode on an oracle volume holding the GPU volume's values, so that only the decoder differs (as the shipped
    # checkpoint's tcnn parity test does: the f16 encoders may differ by an ulp)
    nm.volume.to_tensor()
    ov2 = orc.OracleSparseVolume(8, voxel, dims, 8)
    ov2.insert(nm.volume.active_coordinates.cpu(), nm.volume.features.cpu(), nm.volume.weights.cpu(),
               nm.volume.num_hits.cpu())
    ref = ov2.decode_pts(orc.lattice_coords(g.numpy()), None, None, is_coords=True, query_tensor=False, geo=geo)
    err = float((sdf.cpu() - ref[0, :, :, 0]).abs().max())
    print(f"\ntrained tcnn weights: SDF max-abs-err {err:.3g} against the oracle")
    assert err < 1e-4, err
    assert float((ref != voxel).float().mean()) > 0.05
    mesh = nm.extract_mesh()
    assert mesh is not None and len(mesh.vertices) > 0 and len(mesh.faces) > 0
    m2 = t.to_model(voxel_size=voxel)
    assert torch.equal(m2.pointnet_pack, model.pointnet_pack)
    assert torch.equal(m2.nerf.sdf_pack, model.nerf.sdf_pack)
    assert torch.equal(m2.nerf.sdf_bwd_pack, model.nerf.sdf_bwd_pack)


def test_bad_shapes_raise():
    t = _trainer(seed=0)
    x, p, g = torch.zeros(2, 64, 6), torch.zeros(2, 5, 3), torch.zeros(2, 5)
    before = t.params.clone()
    for bad in [dict(n=65), dict(n=0)]:
        with pytest.raises(ValueError):
            t.step(x, p, g, **bad)
    with pytest.raises(ValueError):
        t.step(x, p, torch.zeros(2, 6), n=4)        # ragged M
    with pytest.raises(ValueError):
        t.step(torch.zeros(2, 63, 6), p, g, n=4)
    with pytest.raises(ValueError):
        t.step(x, torch.zeros(2, 0, 3), torch.zeros(2, 0), n=4)
    with pytest.raises(ValueError):
        t.eval_loss({"input_pts": x, "training_pts": torch.zeros(2, 7, 3), "gt": g})
    assert torch.equal(t.params, before) and int(t.adam_step.item()) == 0
    out = t.step(x[:1], p[:1], g[:1], n=1)          # B n = 1 is valid here; a valid step after the refused ones runs
    assert torch.isfinite(out["loss"]).item() and int(t.adam_step.item()) == 1
