"""Depth image -> ``input_pts`` on the GPU (the producer side of the hot path).

Replaces the float64 numpy/kornia code of FusionInferenceAbstractDataset.__getitem__
(src/datasets/fusion_inference_dataset.py:40-90) that the reference runs on DataLoader workers and
then uploads (7.4 MB/frame): here the 0.6 MB uint16 depth image is what crosses PCIe.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib

DEPTH_DTYPES = {torch.uint16: 0, torch.int16: 0, torch.float32: 1, torch.float64: 2}


def conf_arg(conf, conf_level, shape, device, what):
    """The (conf, conf_level) pair of a depth entry for a confidence map [H, W] (uint8 on the depth's device) or None
    (a NULL pointer: with level 0, no gate).  Returns (tensor kept alive by the caller or None, pointer, level)."""
    level = int(conf_level)
    if conf is None:
        return None, None, level            # level > 0 without a map: the entry refuses it (BNV_ERR_INVALID_ARGUMENT)
    if not (torch.is_tensor(conf) and conf.is_cuda and conf.device == device):
        raise _lib.BnvError(f"{what}: conf must be a tensor on {device}")
    if conf.dtype != torch.uint8 or tuple(conf.shape[-2:]) != tuple(shape) or conf.numel() != shape[0] * shape[1]:
        raise _lib.BnvError(f"{what}: conf must be uint8 [{shape[0]}, {shape[1]}], got {conf.dtype} "
                            f"{list(conf.shape)}")
    c = conf.contiguous()
    return c, _lib.ptr(c), level


def depth_to_input_pts(depth, intr_mat, T_wc, max_depth=10.0, compact=True, conf=None, conf_level=0):
    """depth [H, W] on the GPU: uint16/int16 millimetres (the dataset PNGs), or float32/float64 metres.
    intr_mat 3x3, T_wc 4x4 (host, float64).  Returns input_pts [1, N, 6] float32 (valid pixels in
    row-major order) -- what ``frame['input_pts'].cuda().float()`` is in run_e2e.py:247-249.
    ``compact=False`` skips the host read of N and returns ([1, H*W, 6], n_valid device tensor) with the
    rows past n_valid filled with NaN (encode_pointcloud's bounds mask drops them).
    ``conf`` [H, W] uint8 on the device (an ARKit confidence map, datasets.ARKitDataset): only pixels with
    ``conf >= conf_level`` become rows; the normals are those of the ungated front end (the Sobel stencil still
    reads rejected neighbours, as in the reference)."""
    if not depth.is_cuda:
        raise _lib.BnvError("depth_to_input_pts runs on the GPU only")
    lib = _lib.require_device(depth.device.index or 0)
    d = depth.contiguous()
    H, W = int(d.shape[-2]), int(d.shape[-1])
    c, c_ptr, level = conf_arg(conf, conf_level, (H, W), d.device, "depth_to_input_pts")
    dt = DEPTH_DTYPES[d.dtype]
    K = (C.c_double * 9)(*np.asarray(intr_mat, dtype=np.float64)[:3, :3].reshape(-1))
    T = (C.c_double * 16)(*np.asarray(T_wc, dtype=np.float64).reshape(-1))
    ws = torch.empty(int(lib.bnv_depth_workspace_bytes(H, W)), dtype=torch.uint8, device=d.device)
    out = torch.empty((H * W, 6), dtype=torch.float32, device=d.device)
    n = torch.empty(1, dtype=torch.int32, device=d.device)           # written by the scan kernel
    # compact=False: NaN rows behind n (pad)
    _lib.check(lib.bnv_depth_to_points(_lib.ptr(d), dt, H, W, K, T, float(max_depth), c_ptr, level, 0 if compact else 1,
                                       _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.ptr(n), _lib.stream_ptr()),
               "bnv_depth_to_points")
    if not compact:
        return out.unsqueeze(0), n
    return out[: int(n.item())].unsqueeze(0)


# ---- depth filter (csrc/depth_filter.hip; include/bnv_fusion.h, "Depth filter") ---------------------------------------

DEFAULT_SIGMA_DEPTH = 2.0 / (8 * 35.130)    # two disparity steps of the reference's sensor model at 1 m (geometry.py:54-69)


def filter_depth(depth, max_depth=3.0, radius=3, sigma_depth=DEFAULT_SIGMA_DEPTH, range_cut=3.0, conf=None,
                 conf_level=0):
    """Edge-preserving smoothing of a depth image on the GPU, for the front end's normals and the tracker: a bilateral
    filter with Tukey biweight kernels, ``radius`` 1..8 pixels, whose range width is ``sigma_depth * z^2`` metres (the
    sensor's disparity noise grows with z^2) and which ignores taps further than ``range_cut`` widths from the centre
    pixel's depth.  depth [H, W] or [1, H, W] on the GPU: uint16/int16 millimetres or float32/float64 metres.  Pixels
    outside (0, max_depth), non-finite ones and, with ``conf`` ([H, W] uint8), those below ``conf_level`` are neither
    smoothed nor used: they come back as 0.  Returns float32 metres [H, W]; float64 arithmetic in a fixed order, the
    same bits on every call (tests/depth_filter_restatement.py is the definition in numpy).  GPU only."""
    if not (torch.is_tensor(depth) and depth.is_cuda):
        raise _lib.BnvError("filter_depth runs on the GPU only: depth must be a device tensor (no CPU fallback)")
    if depth.dtype not in DEPTH_DTYPES:
        raise _lib.BnvError(f"filter_depth: depth must be uint16 millimetres or float32 / float64 metres, got "
                            f"{depth.dtype}")
    d = depth[0] if depth.dim() == 3 and depth.shape[0] == 1 else depth
    if d.dim() != 2 or d.numel() == 0:
        raise _lib.BnvError(f"filter_depth: expected a non-empty [H, W] image, got {tuple(depth.shape)}")
    lib = _lib.require_device(d.device.index or 0)
    d = d.contiguous()
    H, W = int(d.shape[0]), int(d.shape[1])
    c, c_ptr, level = conf_arg(conf, conf_level, (H, W), d.device, "filter_depth")
    with torch.cuda.device(d.device):
        out = torch.empty((H, W), dtype=torch.float32, device=d.device)
        _lib.check(lib.bnv_depth_filter(_lib.ptr(d), DEPTH_DTYPES[d.dtype], H, W, float(max_depth), int(radius),
                                        float(sigma_depth), float(range_cut), c_ptr, level, _lib.ptr(out),
                                        _lib.stream_ptr()), "bnv_depth_filter")
    return out


class DepthFilter(collections.namedtuple("DepthFilter", "radius sigma_depth range_cut",
                                         defaults=(3, DEFAULT_SIGMA_DEPTH, 3.0))):
    """The settings of ``filter_depth`` as one immutable object (``NeuralMap(..., depth_filter=DepthFilter())``)."""
    __slots__ = ()

    def apply(self, frame, max_depth):
        """A shallow copy of the frame dict whose ``depth`` is the filtered image (float32 metres) and whose
        ``depth_filtered`` is True (``depth_ready``: an event behind the filter kernel on the current stream); the
        frame's ``conf`` / ``conf_level`` gate the filter and stay in the frame.  A
        frame that already carries ``depth_filtered``, and one with ``input_pts`` and no ``depth``, is returned as it
        is."""
        if frame.get("depth_filtered") or frame.get("depth") is None:
            return frame
        gate = {}
        if frame.get("conf") is not None:
            gate = {"conf": frame["conf"], "conf_level": int(frame.get("conf_level", 0))}
        out = dict(frame)
        out["depth"] = filter_depth(frame["depth"], max_depth=max_depth, radius=self.radius,
                                    sigma_depth=self.sigma_depth, range_cut=self.range_cut, **gate)
        out["depth_filtered"] = True
        # behind the filter kernel on the stream that runs it: NeuralMap.fuse_and_decode_async does not treat the
        # frame as resident (inputs_resident) before this event has completed
        out["depth_ready"] = torch.cuda.Event()
        out["depth_ready"].record()
        return out
