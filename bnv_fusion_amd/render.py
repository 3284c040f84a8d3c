"""Argument checks and camera packing shared by SparseVolume.render_depth and TSDFVolume.render_depth (the kernels:
csrc/render.hip; the semantics: include/bnv_fusion.h, "Rendering")."""
import ctypes as C
import math
import numbers

import numpy as np
import torch

from ._lib import BnvError

MIN_STEP = 0.05        # BNV_RENDER_MIN_STEP: smallest sample spacing, in voxels


def _host_f64(x, what):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().double().numpy()
    try:
        return np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError):
        raise BnvError(f"render: {what} is not a numeric matrix")


def camera_args(T_wc, K, H, W, near, max_depth, step):
    """Validates a render request before any launch and returns the float32 (T_wc [16], K [9]) ctypes arrays."""
    T = _host_f64(T_wc, "T_wc")
    Km = _host_f64(K, "K")
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise BnvError(f"render: T_wc must be a finite 4x4 matrix (got shape {T.shape})")
    if Km.shape != (3, 3) or not np.isfinite(Km).all() or Km[0, 0] == 0 or Km[1, 1] == 0:
        raise BnvError(f"render: K must be a finite 3x3 pinhole matrix with fx, fy != 0 (got shape {Km.shape})")
    if int(H) != H or int(W) != W or int(H) <= 0 or int(W) <= 0:
        raise BnvError(f"render: H and W must be positive integers (got {H} x {W})")
    if not (isinstance(step, numbers.Real) and math.isfinite(step) and step >= MIN_STEP):
        raise BnvError(f"render: step must be at least {MIN_STEP} voxels (got {step})")
    if not (math.isfinite(near) and near >= 0) or math.isnan(max_depth) or max_depth < 0:
        raise BnvError(f"render: need near >= 0 and max_depth >= 0 (got {near}, {max_depth})")
    t = (C.c_float * 16)(*T.astype(np.float32).reshape(-1).tolist())
    k = (C.c_float * 9)(*Km.astype(np.float32).reshape(-1).tolist())
    return t, k
