"""Torch restatement of one training step of the tiny-cuda-nn embedding (csrc/train_tcnn.hip,
train.TcnnEmbeddingTrainer), for the tests only: float64 for the reference values, fp32 for the autograd baseline.

Forward = the inference restatement (oracle.bnv_oracle.tcnn_mlp(half=True, ste=True), xyz_encoding): encoder on the
B n points, outputs 0..7, feats = f16(mean over the patch's n points); decoder on [p, sin p, cos p, feats_b] (17 of 32
columns), pred = output 0.  Every f16 rounding is straight-through in the backward.  ``half=False`` drops the
roundings (the finite-difference check).  Loss: mean |pred - gt| + 0.001 mean_b |feats_b|.  Adam: torch's, with the
step skipped when the loss or a gradient is not finite (the reference's AMP gradient scaler).
"""
import numpy as np
import torch

from oracle.bnv_oracle import tcnn_mlp, xyz_encoding

KEYS = ("pointnet_backbone.model.params", "nerf.model.params")
W_L1, W_REG = 1.0, 0.001


def _q(t, half):
    return t + (t.half().to(t.dtype) - t).detach() if half else t


def forward(params, input_pts, training_pts, gt, n, dtype=torch.float64, half=True):
    """params: {key: flat tensor}.  Returns (loss, l1, reg, feats [B, 8], pred [B, M])."""
    dev = params[KEYS[0]].device
    x = torch.as_tensor(np.asarray(input_pts)).to(dev, dtype)[:, :n, :]
    B = x.shape[0]
    y = tcnn_mlp(params[KEYS[0]], x.reshape(B * n, 6), 16, 8, half=half, ste=True)
    feats = _q(y.reshape(B, n, 8).mean(1), half)
    pts = torch.as_tensor(np.asarray(training_pts)).to(dev, dtype)
    M = pts.shape[1]
    # sin / cos in fp32, as the kernels and the inference decode path evaluate them, then widened
    enc = xyz_encoding(pts.float()).to(dtype) if dtype == torch.float64 else xyz_encoding(pts)
    d = torch.cat([enc, feats[:, None, :].expand(B, M, 8)], -1)
    pred = tcnn_mlp(params[KEYS[1]], d.reshape(B * M, 17), 32, 1, half=half, ste=True).reshape(B, M)
    l1 = (pred - torch.as_tensor(np.asarray(gt)).to(dev, dtype).reshape(B, M)).abs().mean()
    reg = torch.norm(feats, dim=1).mean()
    return W_L1 * l1 + W_REG * reg, l1, reg, feats, pred


def train_steps(state_dict, batches, lr=1e-3, dtype=torch.float64, device="cpu", half=True, state=None):
    """Runs len(batches) steps of (input_pts, training_pts, gt, n) from ``state_dict``; returns (losses, grads of the
    first step, final params, skipped flags, Adam state).  ``state``: an Adam state to resume from (the returned one)."""
    params = {k: torch.as_tensor(np.asarray(state_dict[k])).to(device, dtype).clone().requires_grad_(True)
              for k in KEYS}
    opt = torch.optim.Adam([params[k] for k in KEYS], lr=lr)
    if state is not None:
        opt.load_state_dict(state)
    losses, first_grads, skipped = [], None, []
    for input_pts, training_pts, gt, n in batches:
        opt.zero_grad()
        loss, l1, reg, _, _ = forward(params, input_pts, training_pts, gt, n, dtype=dtype, half=half)
        loss.backward()
        if first_grads is None:
            first_grads = {k: v.grad.detach().clone() for k, v in params.items()}
        ok = bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v.grad).all()) for v in params.values())
        if ok:
            opt.step()
        skipped.append(not ok)
        losses.append((float(loss.detach()), float(l1.detach()), float(reg.detach())))
    return losses, first_grads, {k: v.detach() for k, v in params.items()}, skipped, opt.state_dict()
