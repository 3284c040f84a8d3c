"""Golden vectors for embedding training (train_step.npz), captured from the reference.

Build-container only (needs /root/reference):  python tests/golden/make_golden_train.py
Runs the reference's own LitFusionPointNet(tiny_cuda=False) with pointnet.ckpt in TRAIN mode on a fixed batch
(B = 12, n = 37, M = 97: neither B n nor M is a tile multiple): forward(input_pts[:, :n], normalize=False),
compute_loss with the config's loss weights (bce 1.0, reg 0.001), torch autograd and torch.optim.Adam(lr=1e-3), for
three steps on the same batch.  Records the inputs, the loss terms of every step, every gradient of step 1, the
parameters / running stats / num_batches_tracked after step 3, and the reference model's state_dict keys and shapes.

To stay small, the three 256 x 256 decoder weights are recorded on every 8th output row (their max-abs over the full
tensor is recorded too).  Only DATA is written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

B, N, M, STEPS = 12, 37, 97, 3
BIG = ("nerf.geo_layer1.weight", "nerf.geo_layer2.weight", "nerf.geo_layer3.weight")
ROWS = np.arange(0, 256, 8)


def make_batch(seed=5):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-0.9, 0.9, (B, 64, 3))
    nrm = rng.normal(size=(B, 64, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    inp = np.concatenate([pts, nrm], -1).astype(np.float32)
    tp = rng.uniform(-1, 1, (B, M, 3)).astype(np.float32)
    gt = (0.6 * tp[..., 2] + 0.2 * np.sin(2 * tp[..., 0])).astype(np.float32)
    return inp, tp, gt


def main():
    torch.set_num_threads(8)
    model, _ = ref_shims.build_reference_model(0.01, "/tmp/refwork")
    for p in model.parameters():
        p.requires_grad_(True)
    model.train()
    inp, tp, gt = make_batch()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-3)
    w = model.loss_weight
    out = {"input_pts": inp, "training_pts": tp, "gt": gt, "n": np.array(N), "rows": ROWS}
    losses = []
    for step in range(STEPS):
        opt.zero_grad()
        data = {"input_pts": torch.from_numpy(inp), "training_pts": torch.from_numpy(tp), "gt": torch.from_numpy(gt)}
        feats = model(data["input_pts"][:, :N, :].clone(), normalize=False)
        lo = model.compute_loss(data, feats)
        loss = lo["bce_loss"] * w.bce_loss + lo["reg_loss"] * w.reg_loss
        loss.backward()
        losses.append([float(loss), float(lo["bce_loss"]), float(lo["reg_loss"])])
        if step == 0:
            for k, p in model.named_parameters():
                if p.grad is None or k.startswith("nerf.color") or k.startswith("nerf.fc_rgb"):
                    continue
                g = p.grad.detach().numpy().astype(np.float32)
                out["gmax/" + k] = np.array(np.abs(g).max(), np.float32)
                out["grad/" + k] = g[ROWS] if k in BIG else g
        opt.step()
    out["losses"] = np.array(losses, np.float64)
    sd = model.state_dict()
    for k, v in sd.items():
        if k.startswith("nerf.color") or k.startswith("nerf.fc_rgb"):
            continue
        a = v.detach().numpy()
        out["after/" + k] = a[ROWS] if k in BIG else a
    out["ref_keys"] = np.array(list(sd.keys()))
    out["ref_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    path = os.path.join(HERE, "train_step.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; losses", losses)


if __name__ == "__main__":
    main()
