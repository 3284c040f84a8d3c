"""Float64 reference and numpy emulations of the MLP arithmetics of the HIP kernels (TEST INFRASTRUCTURE ONLY).

The kernels run the fp32 checkpoint's networks in one of three arithmetics (include/bnv_fusion.h, bnv_set_mlp_mode):
  * mode 0, exact fp32: fp32 products, fp32 accumulation;
  * mode 1, split f16: every fp32 operand x is split into f16 hi = f16(x), lo = f16(x - hi), and a.b is taken as
    ah.bh + ah.bl + al.bh (three f16 products, exact in fp32) with fp32 accumulation; biases enter the accumulator
    in fp32; the SDF decoder's last layer (256 -> 1) is an fp32 dot product;
  * mode 3, f16 operands: ah.bh only.
The emulations below restate that arithmetic layer by layer on the CPU (the summation order of the MFMA is not
restated: numpy's fp32 matmul stands in for it), so that tests/test_precision_envelope_cpu.py can derive, without a
GPU, the error envelope each mode should land in against a float64 run of the same network -- the bars of
tests/test_gpu_precision.py rest on it.  The float64 network itself is bnv_oracle's, fed a float64 state dict
(``state_dict_f64``).
"""
import numpy as np
import torch

BN_EPS = 1e-5
MODES = ("f64", "exact", "split", "f16")     # f64 reference, then MLP modes 0, 1, 3


def state_dict_f64(sd):
    """The checkpoint's tensors as float64 (exact casts of the fp32 values)."""
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _np64(v):
    return v.detach().cpu().numpy().astype(np.float64) if hasattr(v, "detach") else np.asarray(v, np.float64)


def sdf_layers(sd):
    """(W [out, in], b [out]) of nerf.geo_layer0..3 and fc_alpha, float32."""
    names = [f"nerf.geo_layer{i}" for i in range(4)] + ["nerf.fc_alpha"]
    return [(_np64(sd[n + ".weight"]).astype(np.float32), _np64(sd[n + ".bias"]).astype(np.float32)) for n in names]


def pointnet_layers(sd):
    """conv1d(k=1) + eval-mode BatchNorm1d folded into one affine map per layer (float64 fold, stored fp32: what the
    kernels' weight pack holds)."""
    out = []
    p = "pointnet_backbone."
    for i in (1, 2, 3, 4):
        W = _np64(sd[f"{p}conv{i}.weight"])[:, :, 0]
        s = _np64(sd[f"{p}bn{i}.weight"]) / np.sqrt(_np64(sd[f"{p}bn{i}.running_var"]) + BN_EPS)
        b = (_np64(sd[f"{p}conv{i}.bias"]) - _np64(sd[f"{p}bn{i}.running_mean"])) * s + _np64(sd[f"{p}bn{i}.bias"])
        out.append(((W * s[:, None]).astype(np.float32), b.astype(np.float32)))
    return out


def split(x):
    """fp32 -> (hi, lo) as f16 values held in fp32: x ~ hi + lo to ~22 bits."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


def matmul(x, W, mode):
    """x [n, k] @ W[out, k].T in the arithmetic of ``mode`` (products exact in fp32 for the f16 modes)."""
    if mode == "f64":
        return np.asarray(x, np.float64) @ np.asarray(W, np.float64).T
    x = np.asarray(x, np.float32)
    W = np.asarray(W, np.float32)
    if mode == "exact":
        return x @ W.T
    xh, xl = split(x)
    Wh, Wl = split(W)
    if mode == "f16":
        return xh @ Wh.T
    assert mode == "split", mode
    return (xh @ Wh.T + xh @ Wl.T) + xl @ Wh.T


def mlp(layers, x, mode, fp32_last=False, preacts=None):
    """ReLU MLP (no ReLU after the last layer).  ``fp32_last``: the last layer is an fp32 dot product in every
    fp32-class mode (the SDF decoder's 256 -> 1).  ``preacts``: list that receives every hidden pre-activation."""
    h = np.asarray(x, np.float64 if mode == "f64" else np.float32)
    for i, (W, b) in enumerate(layers):
        last = i == len(layers) - 1
        m = "exact" if (last and fp32_last and mode != "f64") else mode
        z = matmul(h, W, m) + (b.astype(np.float64) if mode == "f64" else b)
        if last:
            return z
        if preacts is not None:
            preacts.append(z)
        h = np.maximum(z, 0)


def mlp_input_grad(layers, x, g_out, mode):
    """d(g_out . mlp(x)) / dx with the ReLU masks of a ``mode`` forward; the backward products in ``mode`` as well.
    As the decoder's backward kernel does: the Jacobian is propagated with a unit seed (operands O(1), no f16
    underflow) through the transposed layers, and g_out multiplies it in fp32 at the end."""
    pre = []
    mlp(layers, x, mode, fp32_last=True, preacts=pre)
    dt = np.float64 if mode == "f64" else np.float32
    g = np.repeat(np.asarray(layers[-1][0], dt), len(pre[0]), axis=0)
    for (W, _), z in zip(layers[-2::-1], pre[::-1]):
        g = g * (z > 0)
        g = matmul(g, np.asarray(W).T, mode)
    return g * np.asarray(g_out, dt)[:, None]


def sdf_inputs(local, feats):
    """Decoder input rows [n, 17]: local coordinates, sin, cos (fp32, as the kernels compute them), features."""
    t = np.asarray(local, np.float32)
    return np.concatenate([t, np.sin(t), np.cos(t), np.asarray(feats, np.float32)], axis=1)


def max_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())
