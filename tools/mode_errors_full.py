"""End-to-end SDF difference between the MLP modes at the benchmark configuration (256^3, 640x480):
every frame fused + decoded in each mode from scratch; compares the decoded lattice of EVERY touched voxel of
the last frames against mode 1 (fp32-class arithmetic, itself 1e-8 from the oracle)."""
import sys, numpy as np, torch
sys.path.insert(0, '.')
import bnv_fusion_amd as bnv
bnv.configure_runtime()      # the package's hardware queue count, before the first HIP call (streams.py)
from bnv_fusion_amd import synthetic
dims, voxel = synthetic.GRID_DIMS[256]
frames = [{"depth": torch.from_numpy(synthetic.depth_u16(t)).cuda(), "intr_mat": synthetic.intrinsics(), "T_wc": synthetic.pose(t)} for t in range(45)]
out = {}
for mode in (1, 3, 0):
    bnv.set_mlp_mode(mode)
    model = bnv.load_pretrained(device="cuda:0", voxel_size=voxel)
    nm = bnv.NeuralMap(np.array([dims]*3), voxel, model, capacity=1<<20, device="cuda:0", tsdf=True)
    res = []
    for t, f in enumerate(frames):
        c, s = nm.fuse_and_decode(f)
        if t >= 35: res.append((c.clone(), s.clone()))
    out[mode] = res
bnv.set_mlp_mode(1)
for mode in (3, 0):
    worst, n, masks = 0.0, 0, True
    for (c1, s1), (c2, s2) in zip(out[1], out[mode]):
        assert torch.equal(c1, c2)
        worst = max(worst, float((s1 - s2).abs().max())); n += s1.numel()
        masks &= bool(torch.equal(s1 == voxel, s2 == voxel))
    print(f"mode {mode} vs mode 1: {n} SDF values of 10 frames after 35-45 fusions: max |diff| = {worst:.3e}, mask decisions equal: {masks}")
