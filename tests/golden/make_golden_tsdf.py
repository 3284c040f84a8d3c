"""Golden vectors for the TSDF side fusion, captured from the reference's own
CPU path.

Build-container only (needs /root/reference):  python tests/golden/make_golden_tsdf.py
third_parties/fusion.py falls back to a CPU implementation when pycuda is missing (FUSION_GPU_MODE = 0,
:225-291).  Its helpers are numba kernels; numba is not installed here, so ``njit`` is shimmed as the identity and
``prange`` as ``range`` -- the SAME Python source then runs un-jitted (numba's float32 arithmetic is IEEE like
numpy's).  Three 120x160 synthetic depth frames are integrated into a 1.0 m volume at 0.025 m (40^3 voxels).

The CPU path and the CUDA kernel the reference runs on a GPU box are two formulations of the same update: the CPU
path inverts the pose with numpy (float64) and rounds pixel coordinates half-to-even (np.round), the kernel applies
the transposed rotation in float32 and rounds half away from zero (roundf).  The HIP kernel follows the CUDA kernel;
tests compare against these goldens with a small tolerance and allow the handful of voxels whose projection lands
exactly between two pixels.

tsdf_color.npz is a second capture from the same fallback, for the colour volume and the options: a non-cubic
15 x 17 x 20 volume at 0.04 m (5,100 voxels: 19 blocks of 256 threads and a partial one) with the camera INSIDE it, so
some voxels lie behind the camera; six 24 x 32 frames of uint16-millimetre depth with a zeroed patch, random 8-bit
colour from a seeded generator, ``obs_weight`` 2.5, generic (non-axis-aligned) poses so that no projection ties
between two pixels.  The fallback rounds channel averages half to even (np.round), the CUDA kernel half away from
zero (roundf): integer channels and small weights make exact .5 averages common, so the two differ in about half of
the observed voxels -- which is what lets a test tell the two roundings apart.

Only DATA is written (tests/golden/tsdf_40.npz, tests/golden/tsdf_color.npz).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import ref_shims  # noqa: E402


def _rodrigues(r):
    """Rotation matrix of the axis-angle vector r."""
    a = float(np.linalg.norm(r))
    k = r / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def color_capture(ref_fusion):
    bounds = np.array([[-0.30, 0.27], [-0.35, 0.33], [-0.2, 0.6]])
    voxel, H, W, obs_weight = 0.04, 24, 32, 2.5
    vol = ref_fusion.TSDFVolume(bounds.copy(), voxel_size=voxel, use_gpu=False)
    assert tuple(vol._vol_dim) == (15, 17, 20)
    rng = np.random.default_rng(2024)
    intr = np.array([[27.3, 0.0, 15.37], [0.0, 26.9, 11.61], [0.0, 0.0, 1.0]])
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depths_mm, colors, poses = [], [], []
    for t in range(6):
        T = np.eye(4)
        T[:3, :3] = _rodrigues(rng.uniform(-0.12, 0.12, 3))
        T[:3, 3] = np.array([0.013, -0.021, -0.047]) + rng.uniform(-0.03, 0.03, 3)      # inside the volume
        mm = np.round(1000.0 * (0.34 + 0.07 * np.sin(u / 5.0 + 0.4 * t) * np.cos(v / 4.0) + 0.01 * t)).astype(np.uint16)
        mm[5 + t:10 + t, 8:15] = 0                                                       # invalid patch
        rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        d = mm.astype(np.float32) / np.float32(1000)          # the float32 metres the HIP kernel makes of the uint16
        vol.integrate(rgb, d, intr, T, obs_weight=obs_weight)
        depths_mm.append(mm)
        colors.append(rgb)
        poses.append(T)
    tsdf, color = vol.get_volume()
    assert tsdf.dtype == np.float32 and color.dtype == np.float32 and vol._weight_vol_cpu.dtype == np.float32
    np.savez_compressed(os.path.join(HERE, "tsdf_color.npz"), bounds=bounds, voxel_size=voxel, intr=intr,
                        poses=np.stack(poses), depths_mm=np.stack(depths_mm), colors=np.stack(colors),
                        obs_weight=obs_weight, tsdf=tsdf, weight=vol._weight_vol_cpu, color=color,
                        origin=vol._vol_origin)
    print("tsdf_color:", tsdf.shape, "observed voxels", int((vol._weight_vol_cpu > 0).sum()),
          "weights up to", float(vol._weight_vol_cpu.max()))


def main():
    ref_shims.install()
    nb = types.ModuleType("numba")
    nb.njit = lambda *a, **k: (a[0] if (a and callable(a[0]) and not k) else (lambda f: f))
    nb.prange = range
    sys.modules["numba"] = nb
    sys.path.insert(0, "/root/reference")
    from third_parties import fusion as ref_fusion
    assert ref_fusion.FUSION_GPU_MODE == 0
    from oracle import bnv_oracle as orc
    color_capture(ref_fusion)

    bounds = np.array([[-0.5, 0.5], [-0.5, 0.5], [-0.5, 0.5]])
    vol = ref_fusion.TSDFVolume(bounds.copy(), voxel_size=0.025, use_gpu=False)
    H, W = 120, 160
    intr = orc.SYNTHETIC_INTRINSICS.copy()
    intr[:2] *= 0.25
    depths, poses = [], []
    for t in (0, 3, 7):
        d = (orc.synthetic_depth(t, H, W) * 0.5).astype(np.float32)          # surface at ~0.75 m: inside the volume
        T = orc.synthetic_pose(t).copy()
        T[:3, 3] = [0.0, 0.0, -0.95]
        vol.integrate(np.zeros((H, W, 3)), d, intr, T, obs_weight=1.0)
        depths.append(d)
        poses.append(T)
    tsdf, _ = vol.get_volume()
    np.savez_compressed(os.path.join(HERE, "tsdf_40.npz"), bounds=bounds, voxel_size=0.025, intr=intr,
                        depths=np.stack(depths), poses=np.stack(poses), tsdf=tsdf.astype(np.float32),
                        weight=vol._weight_vol_cpu.astype(np.float32), origin=vol._vol_origin)
    print("tsdf_40:", tsdf.shape, "observed voxels", int((vol._weight_vol_cpu > 0).sum()),
          "weights up to", float(vol._weight_vol_cpu.max()))


if __name__ == "__main__":
    main()
