"""Throughput of one embedding training step (csrc/train.hip via train.EmbeddingTrainer) at the reference's batch
(B = 100, n = 64, M = 256), against torch eager autograd in fp32 on the same GPU (same model, loss and Adam).
Prints one JSON line.  The kernel split: run it under `rocprofv3 --kernel-trace --stats -- python tools/train_bench.py`.

    python tools/train_bench.py [--steps 50] [--warmup 10] [--B 100] [--n 64] [--M 256]
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
    t = train.EmbeddingTrainer(seed=0, device=dev)
    hip_s = timed(lambda: t.step(x, p, g, n=a.n), a.steps, a.warmup)
    f = flops(a.B, a.n, a.M)
    out = {"workload": "embedding_train_step", "B": a.B, "n": a.n, "M": a.M, "gflop_per_step": round(f / 1e9, 3),
           "hip_ms_per_step": round(hip_s * 1e3, 4), "hip_steps_per_s": round(1.0 / hip_s, 2),
           "hip_tflops": round(f / hip_s / 1e12, 2)}
    if not a.skip_torch:
        ts = torch_trainer(a.B, a.M, dev)
        xs = x[:, : a.n].contiguous()
        torch_s = timed(lambda: ts(xs, p, g), a.steps, a.warmup)
        out.update({"torch_ms_per_step": round(torch_s * 1e3, 4), "torch_steps_per_s": round(1.0 / torch_s, 2),
                    "torch_tflops": round(f / torch_s / 1e12, 2), "speedup_vs_torch": round(torch_s / hip_s, 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
