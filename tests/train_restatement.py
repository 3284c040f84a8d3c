"""Float64 restatement of one embedding training step (the reference's LitFusionPointNet.training_step with
training_global=False, local_point_fusion.py:381-460), for the tests only.

Encoder: Conv1d(k=1) 6 -> 128 -> 128 -> 128 -> 8, each followed by BatchNorm1d (train mode: batch statistics over
the B n rows, biased variance, eps 1e-5; eval mode: running stats), ReLU after the first three, mean over the n
points.  Decoder: [xyz, sin xyz, cos xyz, feat] -> 4 x (Linear 256, ReLU) -> fc_alpha.  Loss: L1 + 0.001 mean_b
|feats_b|.  Adam: torch defaults.
"""
import numpy as np
import torch

EPS, MOMENTUM = 1e-5, 0.1
W_L1, W_REG = 1.0, 0.001


def to_torch(sd, dtype=torch.float64, device="cpu"):
    return {k: (torch.as_tensor(np.asarray(v)).to(device, dtype) if np.asarray(v).dtype != np.int64
                else torch.as_tensor(np.asarray(v)).to(device)) for k, v in sd.items()}


def forward(sd, input_pts, training_pts, gt, n, train=True, running=None, dtype=torch.float64):
    """Returns (loss, l1, reg, feats, pred).  ``running``: dict to receive the updated running stats (train).
    ``dtype``: float64 for the reference values; float32 (on the GPU) is the torch autograd baseline."""
    dev = sd["nerf.fc_alpha.bias"].device
    x = torch.as_tensor(input_pts).to(dev, dtype)[:, :n, :]
    B = x.shape[0]
    h = x.reshape(B * n, 6)
    for i in range(4):
        p = f"pointnet_backbone.conv{i + 1}"
        q = f"pointnet_backbone.bn{i + 1}"
        z = h @ sd[p + ".weight"][:, :, 0].T + sd[p + ".bias"]
        if train:
            mean = z.mean(0)
            var = z.var(0, unbiased=False)
            if running is not None:
                R = z.shape[0]
                running[q + ".running_mean"] = (1 - MOMENTUM) * sd[q + ".running_mean"] + MOMENTUM * mean.detach()
                running[q + ".running_var"] = ((1 - MOMENTUM) * sd[q + ".running_var"]
                                               + MOMENTUM * var.detach() * R / (R - 1))
        else:
            mean, var = sd[q + ".running_mean"], sd[q + ".running_var"]
        y = (z - mean) / torch.sqrt(var + EPS) * sd[q + ".weight"] + sd[q + ".bias"]
        h = torch.relu(y) if i < 3 else y
    feats = h.reshape(B, n, 8).mean(1)
    pts = torch.as_tensor(training_pts).to(dev, dtype)
    M = pts.shape[1]
    d = torch.cat([pts, torch.sin(pts), torch.cos(pts), feats[:, None, :].expand(B, M, 8)], -1)
    for i in range(4):
        d = torch.relu(d @ sd[f"nerf.geo_layer{i}.weight"].T + sd[f"nerf.geo_layer{i}.bias"])
    pred = (d @ sd["nerf.fc_alpha.weight"].T + sd["nerf.fc_alpha.bias"])[..., 0]
    l1 = (pred - torch.as_tensor(gt).to(dev, dtype).reshape(B, M)).abs().mean()
    reg = torch.norm(feats, dim=1).mean()
    return W_L1 * l1 + W_REG * reg, l1, reg, feats, pred


PARAM_SUFFIXES = (".weight", ".bias")


def trainable_keys(sd):
    return [k for k in sd if k.endswith(PARAM_SUFFIXES)]


def train_steps(state_dict, batches, lr=1e-3, dtype=torch.float64, device="cpu"):
    """Runs len(batches) steps of (input_pts, training_pts, gt, n) from ``state_dict``; returns (losses, grads of
    the first step, final state dict with running stats and num_batches_tracked)."""
    sd = to_torch(state_dict, dtype, device)
    params = {k: sd[k].clone().requires_grad_(True) for k in trainable_keys(sd)}
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    losses, first_grads = [], None
    for input_pts, training_pts, gt, n in batches:
        cur = dict(sd)
        cur.update(params)
        running = {}
        opt.zero_grad()
        loss, l1, reg, _, _ = forward(cur, input_pts, training_pts, gt, n, train=True, running=running, dtype=dtype)
        loss.backward()
        if first_grads is None:
            first_grads = {k: v.grad.detach().clone() for k, v in params.items()}
        opt.step()
        sd.update(running)
        for i in range(4):
            k = f"pointnet_backbone.bn{i + 1}.num_batches_tracked"
            sd[k] = sd[k] + 1
        losses.append((float(loss.detach()), float(l1.detach()), float(reg.detach())))
    final = dict(sd)
    final.update({k: v.detach() for k, v in params.items()})
    return losses, first_grads, final
