"""Throughput of one embedding training step (csrc/train.hip via train.EmbeddingTrainer) at the reference's batch
(B = 100, n = 64, M = 256), against torch eager autograd in fp32 on the same GPU (same model, loss and Adam).
--tiny-cuda: the tiny-cuda-nn networks (csrc/train_tcnn.hip via train.TcnnEmbeddingTrainer) against torch eager
autograd of the same f16 arithmetic (f16 casts of inputs, weights and layer outputs, f16 GEMMs) plus Adam on the fp32
masters.  Prints one JSON line.  The kernel split: run it under
`rocprofv3 --kernel-trace --stats -- python tools/train_bench.py`.

    python tools/train_bench.py [--tiny-cuda] [--steps 50] [--warmup 10] [--B 100] [--n 64] [--M 256]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def flops(B, n, M):
    """Multiply-adds x 2 of forward + backward: every layer's forward GEMM, its dW GEMM and (but for the encoder's
    first layer) its dX GEMM."""
    Re, Rd = B * n, B * M
    enc = [(6, 128), (128, 128), (128, 128), (128, 8)]
    dec = [(17, 256), (256, 256), (256, 256), (256, 256), (256, 1)]
    f = 0
    for i, (a, b) in enumerate(enc):
        f += 2 * Re * a * b * (2 if i == 0 else 3)
    for a, b in dec:
        f += 2 * Rd * a * b * 3
    return f


TCNN_ENC, TCNN_DEC = (16, 64, 64, 64, 16), (32, 64, 64, 64, 16)


def tcnn_flops(B, n, M, padded=True):
    """Multiply-adds x 2 of forward + backward of the tiny-cuda-nn networks: every layer's forward product, its dW
    product and (but for the encoder's first layer) its dX product.  ``padded``: on the widths the MFMAs execute
    (16 / 32 inputs, 16 outputs); otherwise on the widths that carry data (6 / 17 inputs, 8 / 1 outputs)."""
    Re, Rd = B * n, B * M
    enc = TCNN_ENC if padded else (6, 64, 64, 64, 8)
    dec = TCNN_DEC if padded else (17, 64, 64, 64, 1)
    f = 0
    for i, (a, b) in enumerate(zip(enc[:-1], enc[1:])):
        f += 2 * Re * a * b * (2 if i == 0 else 3)
    for a, b in zip(dec[:-1], dec[1:]):
        f += 2 * Rd * a * b * 3
    return f


def torch_tcnn_trainer(dev):
    """Torch eager autograd of the tiny-cuda-nn step: f16 casts where the kernels round, f16 GEMMs, Adam on fp32."""
    import torch
    from bnv_fusion_amd import train
    sd = train.tcnn_default_state_dict(0)
    params = [torch.from_numpy(sd[k]).to(dev).requires_grad_(True) for k in train.TCNN_KEYS]
    opt = torch.optim.Adam(params, lr=1e-3)

    def mlp(flat, x, widths):
        h = torch.cat([x, torch.ones(x.shape[0], widths[0] - x.shape[1], device=dev)], 1).half()
        off = 0
        for i, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
            w = flat[off: off + a * b].view(b, a).half()
            off += a * b
            h = h @ w.t()
            if i < len(widths) - 2:
                h = torch.relu(h)
        return h

    def step(x, pts, gt):
        opt.zero_grad()
        B, n = x.shape[:2]
        y = mlp(params[0], x.reshape(B * n, 6), TCNN_ENC)[:, :8].float()
        feats = y.view(B, n, 8).mean(1).half().float()
        M = pts.shape[1]
        d = torch.cat([pts, torch.sin(pts), torch.cos(pts), feats[:, None].expand(-1, M, -1)], -1).reshape(B * M, 17)
        pred = mlp(params[1], d, TCNN_DEC)[:, 0].float().view(B, M)
        loss = (pred - gt).abs().mean() + 0.001 * torch.norm(feats, dim=1).mean()
        loss.backward()
        opt.step()
        return loss
    return step


def torch_trainer(B, M, dev):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.convs = nn.ModuleList([nn.Conv1d(a, b, 1) for a, b in ((6, 128), (128, 128), (128, 128), (128, 8))])
            self.bns = nn.ModuleList([nn.BatchNorm1d(c) for c in (128, 128, 128, 8)])
            self.geo = nn.ModuleList([nn.Linear(17, 256)] + [nn.Linear(256, 256) for _ in range(3)])
            self.alpha = nn.Linear(256, 1)

        def forward(self, x, pts):
            h = x.permute(0, 2, 1)
            for i in range(4):
                h = self.bns[i](self.convs[i](h))
                h = F.relu(h) if i < 3 else h
            feats = h.mean(2)
            d = torch.cat([pts, torch.sin(pts), torch.cos(pts), feats[:, None].expand(-1, pts.shape[1], -1)], -1)
            for lin in self.geo:
                d = F.relu(lin(d))
            return self.alpha(d)[..., 0], feats

    net = Net().to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)

    def step(x, pts, gt):
        opt.zero_grad()
        pred, feats = net(x, pts)
        loss = F.l1_loss(pred, gt) + 0.001 * torch.norm(feats, dim=1).mean()
        loss.backward()
        opt.step()
        return loss
    return step


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--B", type=int, default=100)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--M", type=int, default=256)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--tiny-cuda", action="store_true", help="the tiny-cuda-nn networks (TcnnEmbeddingTrainer)")
    a = ap.parse_args()
    import bnv_fusion_amd as bnv
    bnv.configure_runtime()
    import torch
    from bnv_fusion_amd import synthetic, train
    dev = "cuda:0"
    d = synthetic.local_patches(a.B, a.M, seed=0, noise=0.02)
    x = torch.from_numpy(d["input_pts"]).to(dev)
    p = torch.from_numpy(d["training_pts"]).to(dev)
    g = torch.from_numpy(d["gt"]).to(dev)
    if a.tiny_cuda:
        t = train.TcnnEmbeddingTrainer(seed=0, device=dev)
        f = tcnn_flops(a.B, a.n, a.M)
        workload = "tcnn_embedding_train_step"
    else:
        t = train.EmbeddingTrainer(seed=0, device=dev)
        f = flops(a.B, a.n, a.M)
        workload = "embedding_train_step"
    hip_s = timed(lambda: t.step(x, p, g, n=a.n), a.steps, a.warmup)
    out = {"workload": workload, "B": a.B, "n": a.n, "M": a.M, "gflop_per_step": round(f / 1e9, 3),
           "hip_ms_per_step": round(hip_s * 1e3, 4), "hip_steps_per_s": round(1.0 / hip_s, 2),
           "hip_tflops": round(f / hip_s / 1e12, 2)}
    if a.tiny_cuda:
        out["gflop_per_step_unpadded"] = round(tcnn_flops(a.B, a.n, a.M, padded=False) / 1e9, 3)
    if not a.skip_torch:
        ts = torch_tcnn_trainer(dev) if a.tiny_cuda else torch_trainer(a.B, a.M, dev)
        xs = x[:, : a.n].contiguous()
        torch_s = timed(lambda: ts(xs, p, g), a.steps, a.warmup)
        out.update({"torch_ms_per_step": round(torch_s * 1e3, 4), "torch_steps_per_s": round(1.0 / torch_s, 2),
                    "torch_tflops": round(f / torch_s / 1e12, 2), "speedup_vs_torch": round(torch_s / hip_s, 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
