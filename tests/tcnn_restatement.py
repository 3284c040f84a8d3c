"""The tiny-cuda-nn networks (MLP mode 2) against float64, for the tests only: the ideal R, the restatement E, the
arithmetics a correct kernel may have, seeded defects, and the bars derived from them (TEST INFRASTRUCTURE ONLY).

The network is oracle.bnv_oracle.tcnn_mlp: inputs padded with 1.0 to 16 (encoder) or 32 (SDF decoder), three hidden
layers of 64 with ReLU, no bias, 16 outputs; weights row-major [out, in] in one flat vector.

  R  (ideal)        stored parameters rounded to f16 (as ``half=True`` does) and widened to float64; the fp32 inputs
                    the kernels form widened to float64; float64 accumulation, no activation rounding, output not
                    rounded.
  E  (restatement)  tcnn_mlp(half=True) in fp32, bit for bit (tests/test_tcnn_envelope_cpu.py asserts it).
  OK variants       E; "acc32": one fp32 accumulator over the 16-deep K-steps in the order of tcnn_hidden_layer
                    (csrc/tcnn_mlp.hpp, g = 0..3), each step's 16 products summed exactly; "acc32_rev": the same with
                    the K-steps in reverse order.
  defects           one-line changes of E:
                      a "drop_k"      K-step 2 of the first 64 -> 64 layer is dropped
                      b "pad0"        the input padding is 0.0 instead of 1.0
                      c "no_relu"     the ReLU after the last hidden layer is missing
                      d "swap_slots"  slots 0 and 1 of lane half 0 (tcnn_slot_feature: features 0 and 1) are swapped in
                                      the input fragment of K-step 0
                      e "trunc"       activations are truncated to f16 instead of rounded to nearest even
                      f "no_round"    activations are not rounded at all (the defect on the other side: a kernel that
                                      silently runs a higher-precision path)
  "acc16"           (accumulator rounded to f16 after every K-step) stays a sensitivity figure, NOT an OK variant: the
                    kernels accumulate in fp32.

Metrics, in the units of tests/test_gpu_precision.py: max and rms error against R; decoder in alpha (= SDF / voxel:
the network's output, for every arithmetic but R through the f16 product with the voxel size the decode kernels and
oracle.decode_pts(geo=) keep), encoder relative to max |feature|, gradients (d alpha / d features, f16 roundings
straight through as tcnn_geo_forward(ste=True) has them) per evaluation row relative to the largest gradient.

Backward: "jac16" restates k_decode_pts_bwd_t (csrc/decode_pts.hip) -- E's forward and masks, the Jacobian rounded to
f16 between the transposed layers, fp32 accumulation; tiny-cuda-nn itself back-propagates in fp16.  It is an OK
variant of the two gradient entries.

Bars (``bars()``; computed, never typed in).  Per entry and metric m, over every input set and both checkpoints
(weights/pointnet_tcnn.npz and train.tcnn_default_state_dict(0)), with B the entry's baseline (``BASELINE``: E; for
the gradients off the ReLU kinks jac16, because E's straight-through gradient is exact up to fp32 there and its
distance to R is matmul noise):
    ok_max = max over the OK variants of m(V) / m(B)                     (>= 1: B is one of them)
    bad    = m(defect) / m(B); for defect f, m(B) / m(f), against ok_lo = max over the OK variants of m(B) / m(V)
    a defect is PINNED by m when bad >= 2 ok_max (f: >= 2 ok_lo) on every input set and both checkpoints
    BAR[m]    = sqrt(ok_max * min over the pinned defects a..e of bad)
    BAR_lo[m] = sqrt(ok_lo * min bad of f)                               (None when f is not pinned by m)
A GPU result passes when m(GPU) <= BAR m(B), and m(GPU) >= m(B) / BAR_lo, with B evaluated on the same inputs at
test time.  The margin is the geometric midpoint: the two sides are a ratio apart.

Derived (tests/test_tcnn_envelope_cpu.py prints every ratio; min over input sets and checkpoints):
  decoder      max ok_max 1.029 ok_lo 1.000  a 475  b 624  c 328  d 297  e 1.41   f 1.37   pinned abcd   BAR 17.49
  decoder      rms ok_max 1.006 ok_lo 1.000  a 931  b 1340 c 625  d 375  e 2.18   f 1.24   pinned abcde  BAR 1.481
  encoder      max ok_max 1.000 ok_lo 1.000  a 515  b 589  c 1250 d 386  e 1.76   f 1.51   pinned abcd   BAR 19.65
  encoder      rms ok_max 1.000 ok_lo 1.000  a 874  b 1130 c 2260 d 375  e 1.74   f 1.31   pinned abcd   BAR 19.36
  gradient     max ok_max 1.000 ok_lo 5392   a 3120 b 3650 c 1850 d 2100 e 8.1e-4 f 962    pinned abcd   BAR 43.02
  gradient     rms ok_max 1.000 ok_lo 5145   a 3490 b 4330 c 2210 d 1640 e 5.7e-4 f 1670   pinned abcd   BAR 40.45
  gradient_all max ok_max 1.000 ok_lo 1.000  a 4.5  b 5.6  c 3.3  d 3.0  e 0.85   f 1.00   pinned abcd   BAR 1.721
  gradient_all rms ok_max 1.000 ok_lo 1.000  a 32.7 b 39.7 c 36.5 d 23.1 e 1.01   f 1.11   pinned abcd   BAR 4.810
"gradient": evaluations off the ReLU kinks (``kink_flags``), baseline jac16 (2.2e-4 .. 4.3e-4 of the largest gradient;
E and the fp32 accumulations sit 3,000 .. 5,400 x closer to R: that is ok_lo, and why f, which equals E there, is not
pinned against it).  "gradient_all": every evaluation, where flipped ReLUs carry the error.  No BAR_lo exists: f is
pinned nowhere.
"""
import functools
import os

import numpy as np
import torch

from conftest import GOLDEN, WEIGHTS_TCNN
from oracle import bnv_oracle as orc
from oracle import precision as P

N = 8192
OK_VARIANTS = ("E", "acc32", "acc32_rev")
GRAD_OK_VARIANTS = OK_VARIANTS + ("jac16",)      # the gradient entries: the backward kernel's own arithmetic as well
DEFECTS = {"a": "drop_k", "b": "pad0", "c": "no_relu", "d": "swap_slots", "e": "trunc", "f": "no_round"}
MUST_PIN_MAX = ("a", "b", "c", "d")
MUST_PIN_RMS = ("e", "f")
PIN_FACTOR = 2.0
ENTRIES = ("decoder", "encoder", "gradient", "gradient_all")
VOXEL = 0.02                  # of every golden volume the GPU tests decode
KINK_FACTOR = 4.0
DEC = dict(n_in_padded=32, n_out=1)
ENC = dict(n_in_padded=16, n_out=8)


def round_f16(t):
    return t.half().to(t.dtype)


def trunc_f16(t):
    """Round toward zero to f16: where nearest-even went away from zero, one f16 step back (sign-magnitude bits)."""
    r = t.half()
    away = r.to(t.dtype).abs() > t.abs()
    return (r.view(torch.int16) - away.to(torch.int16)).view(torch.float16).to(t.dtype)


def net(params, x, n_in_padded, n_out, variant="E", ste=False, width=64, n_hidden=3, preacts=None):
    """The network on fp32 inputs x [n, n_in] in the arithmetic of ``variant`` ("R", an OK variant, a defect or
    "acc16").  R returns float64; the others fp32.  ``ste``: roundings are identity in the backward pass.
    ``preacts``: list that receives every hidden pre-activation."""
    params = torch.as_tensor(np.asarray(params)).float()
    x = torch.as_tensor(x)
    ideal = variant == "R"
    assert x.dtype == torch.float32 or ideal, "fp32 inputs (R also takes them already widened)"
    rnd = trunc_f16 if variant == "trunc" else round_f16
    if ste:
        q = lambda t: t + (round_f16(t) - t).detach()
        qa = lambda t: t + (rnd(t) - t).detach()
    else:
        q, qa = round_f16, rnd
    if variant == "no_round":
        qa = lambda t: t
    pad = torch.full((x.shape[0], n_in_padded - x.shape[1]), 0.0 if variant == "pad0" else 1.0, dtype=x.dtype)
    h = torch.cat([x, pad], 1)
    if variant == "swap_slots":
        h = h[:, [1, 0] + list(range(2, n_in_padded))]
    h = h.double() if ideal else q(h)
    dims = [n_in_padded] + [width] * n_hidden + [16]
    off = 0
    for i in range(len(dims) - 1):
        w = round_f16(params[off: off + dims[i + 1] * dims[i]].reshape(dims[i + 1], dims[i]))
        off += dims[i + 1] * dims[i]
        if ideal:
            w = w.double()
        steps = list(range(0, dims[i], 16))
        if variant == "drop_k" and i == 1:
            h = torch.cat([h[:, :32], torch.zeros_like(h[:, 32:48]), h[:, 48:]], 1)
        if variant in ("acc32", "acc32_rev", "acc16"):
            acc = torch.zeros((x.shape[0], dims[i + 1]))
            for k0 in (steps[::-1] if variant == "acc32_rev" else steps):
                # the 16 products of a K-step are exact in fp32 and float64; their sum enters the accumulator once
                acc = acc + (h[:, k0: k0 + 16].double() @ w[:, k0: k0 + 16].double().t()).float()
                if variant == "acc16":
                    acc = q(acc)
            h = acc
        else:
            h = h @ w.t()
        last = i == len(dims) - 2
        if not last:
            if preacts is not None:
                preacts.append(h.detach())
            if not (variant == "no_relu" and i == n_hidden - 1):
                h = torch.relu(h)
        if not ideal:
            h = q(h) if last else qa(h)
    return h[:, :n_out]


def sdf_alpha(out, voxel=VOXEL, ste=False):
    """The decode kernels' per-evaluation value in alpha units: the network's f16 output times the voxel size stays
    f16 (a half tensor times a python float, sparse_volume.py:813; csrc/decode_pts.hip), widened and divided back."""
    r = (out.half() * voxel).double() / voxel
    return out.double() + (r - out.double()).detach() if ste else r


def decoder_alpha(params, x, variant, ste=False):
    """[n] float64 alpha of the SDF decoder: R as it is, every other arithmetic through the f16 product."""
    out = net(params, x, variant=variant, ste=ste, **DEC)[:, 0]
    return out if variant == "R" else sdf_alpha(out, ste=ste)


def feature_grad_jac16(params, x):
    """The backward arithmetic of k_decode_pts_bwd_t (csrc/decode_pts.hip): E's forward decides the ReLU masks; the
    Jacobian d alpha / d input starts from row 0 of the output layer and goes through the transposed layers with f16
    operands and fp32 accumulation, ROUNDED TO F16 between them (tiny-cuda-nn itself back-propagates in fp16)."""
    x = torch.as_tensor(x).detach().float()
    pre = []
    net(params, x, variant="E", preacts=pre, **DEC)
    p = torch.as_tensor(np.asarray(params)).float()
    dims, W, off = [32, 64, 64, 64, 16], [], 0
    for i in range(4):
        W.append(round_f16(p[off: off + dims[i + 1] * dims[i]].reshape(dims[i + 1], dims[i])))
        off += dims[i + 1] * dims[i]
    d = round_f16(W[3][0:1].expand(x.shape[0], 64) * (pre[2] > 0))
    d = round_f16((d @ W[2]) * (pre[1] > 0))
    d = round_f16((d @ W[1]) * (pre[0] > 0))
    return (d @ W[0])[:, 9:17].double()


def feature_grad(params, x, variant):
    """d alpha / d features (columns 9..16 of the decoder input) per evaluation, straight through the roundings."""
    if variant == "jac16":
        return feature_grad_jac16(params, x)
    x = torch.as_tensor(x).clone().requires_grad_(True)
    decoder_alpha(params, x, variant, ste=True).sum().backward()
    return x.grad[:, 9:17].double()


def kink_flags(params, x):
    """[n] bool: evaluations in which some hidden unit's float64 pre-activation lies within KINK_FACTOR x E's own
    error of zero -- a correct f16 kernel may put that unit on the other side of its ReLU.  E's error: at that unit,
    or the rms over the layer's 64 units of this evaluation where the unit's own happens to be smaller (the
    fp32-checkpoint tests use an absolute KINK_DELTA; f16 errors scale with the activations, so the margin is taken
    from the restatement, per evaluation)."""
    pr, pe = [], []
    x = torch.as_tensor(x).detach()
    net(params, x, variant="R", preacts=pr, **DEC)
    net(params, x.float(), variant="E", preacts=pe, **DEC)
    flag = torch.zeros(x.shape[0], dtype=torch.bool)
    for zr, ze in zip(pr, pe):
        err = (ze.double() - zr).abs()
        err = torch.maximum(err, err.pow(2).mean(1, keepdim=True).sqrt())
        flag |= (zr.abs() <= KINK_FACTOR * err).any(1)
    return flag


def max_rms(got, ref, scale=1.0, per_row=False):
    """(max, rms) of |got - ref| / scale; ``per_row``: of each row's largest component."""
    d = (torch.as_tensor(got).double() - torch.as_tensor(ref).double()).abs()
    if per_row:
        d = d.reshape(d.shape[0], -1).amax(1)
    d = d.reshape(-1) / scale
    if d.numel() == 0:
        return 0.0, 0.0
    return float(d.max()), float(d.pow(2).mean().sqrt())


# ---- callables for the oracle's ``geo=`` / ``encoder=`` hooks ----------------------------------------------------------
def geo(params, variant, voxel=VOXEL, product=True, ste=False):
    """nerf.geo_forward for oracle.decode_pts / decode_feature_grid_w_pts: [..., 17] -> [..., 1] FLOAT64 (the oracle
    scales a float64 output without rounding it).  R: the ideal.  Any other arithmetic: the network in fp32 on the
    fp32 values of the input; ``product``: through the f16 product with the voxel size (``sdf_alpha``) -- the branches
    that return the unscaled prediction pass False."""
    def f(x):
        flat = x.reshape(-1, x.shape[-1])
        if variant == "R":
            a = net(params, flat, variant="R", **DEC)[:, 0]
        else:
            out = net(params, flat.float(), variant=variant, ste=ste, **DEC)[:, 0]
            a = sdf_alpha(out, voxel, ste) if product else out.double()
        return a.reshape(list(x.shape[:-1]) + [1])
    return f


def encoder(params, variant):
    """Point encoder for oracle.encode_pointcloud: x [1, 6, P] fp32 -> [1, 8, P] FLOAT64 (the scatter mean is then
    float64 for the restatement as well: only the network differs from R)."""
    return lambda x: net(params, x[0].t().contiguous(), variant=variant, **ENC).double().t()[None]


# ---- inputs and checkpoints -------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def checkpoints():
    from bnv_fusion_amd import train
    return {"shipped": {k: np.asarray(v) for k, v in orc.load_weights(WEIGHTS_TCNN).items()},
            "default0": train.tcnn_default_state_dict(0)}


@functools.lru_cache(None)
def decoder_input_sets():
    """fp32 decoder rows [N, 17] from the feature rows of the sequence_64 golden volume (as
    test_precision_envelope_cpu.decoder_inputs): uniform local offsets, and the offsets of the 3x3x3 lattice."""
    z = np.load(os.path.join(GOLDEN, "sequence_64.npz"))
    live = z["features_sorted"][z["weights_sorted"][:, 0] >= 8]
    rng = np.random.default_rng(0)
    feats = live[rng.integers(len(live), size=N)]
    uniform = rng.uniform(-1, 1, size=(N, 3)).astype(np.float32)
    lattice = rng.choice([-0.5, 0.0, 0.5], size=(N, 3)).astype(np.float32)
    return {"uniform": torch.from_numpy(P.sdf_inputs(uniform, feats)),
            "lattice": torch.from_numpy(P.sdf_inputs(lattice, feats))}


@functools.lru_cache(None)
def encoder_input_sets():
    """fp32 encoder rows [N, 6] exactly as encode_pointcloud forms them from the encode_64 golden points."""
    e = np.load(os.path.join(GOLDEN, "encode_64.npz"))
    seen = []

    def spy(x):
        seen.append(x[0].t().contiguous())
        return torch.zeros((1, 8, x.shape[2]))

    orc.encode_pointcloud(None, torch.from_numpy(e["input_pts"]), torch.from_numpy(e["n_xyz"]),
                          torch.from_numpy(e["min_coords"]), torch.from_numpy(e["max_coords"]),
                          float(e["voxel_size"]), encoder=spy)
    rows = seen[0]
    pick = torch.from_numpy(np.random.default_rng(1).permutation(len(rows))[:N])
    return {"encode_64": rows[pick].float()}


# what the bars scale: E; for gradients off the ReLU kinks the restatement of the backward kernel's own arithmetic --
# there E's straight-through gradient is exact up to fp32, its distance to R is the noise of an fp32 matmul (acc32 is
# 3 .. 5 x closer to R than E) and no property of the network
BASELINE = {"decoder": "E", "encoder": "E", "gradient": "jac16", "gradient_all": "E"}


def ok_variants(entry):
    return GRAD_OK_VARIANTS if entry.startswith("gradient") else OK_VARIANTS


def _measure(entry, params, x, variant, ref):
    if entry == "decoder":
        return max_rms(decoder_alpha(params, x, variant), ref)
    if entry == "encoder":
        return max_rms(net(params, x, variant=variant, **ENC), ref, float(ref.abs().max()))
    g = feature_grad(params, x, variant)
    keep = ~kink_flags(params, x) if entry == "gradient" else slice(None)
    return max_rms(g[keep], ref[keep], float(ref.abs().max()), per_row=True)


@functools.lru_cache(None)
def measurements():
    """{entry: {(checkpoint, input set): {variant: (max, rms)}}} against R, every OK variant, defect and acc16."""
    out = {e: {} for e in ENTRIES}
    for ck, sd in checkpoints().items():
        for entry in ENTRIES:
            enc = entry == "encoder"
            params = sd["pointnet_backbone.model.params" if enc else "nerf.model.params"]
            for name, x in (encoder_input_sets() if enc else decoder_input_sets()).items():
                if entry.startswith("gradient"):
                    ref = feature_grad(params, x, "R")
                elif enc:
                    ref = net(params, x, variant="R", **ENC)
                else:
                    ref = decoder_alpha(params, x, "R")
                out[entry][(ck, name)] = {v: _measure(entry, params, x, v, ref)
                                          for v in ok_variants(entry) + tuple(DEFECTS.values()) + ("acc16",)}
    return out


@functools.lru_cache(None)
def ratios():
    """{entry: {metric: {"ok_max", "ok_lo", "bad": {defect letter: min over sets and checkpoints}, "pinned": [...]}}}"""
    out = {}
    for entry, sets in measurements().items():
        out[entry] = {}
        for mi, metric in enumerate(("max", "rms")):
            b = BASELINE[entry]
            ok_max = max(m[v][mi] / m[b][mi] for m in sets.values() for v in ok_variants(entry))
            ok_lo = max(m[b][mi] / m[v][mi] for m in sets.values() for v in ok_variants(entry))
            bad = {}
            for letter, v in DEFECTS.items():
                if letter == "f":
                    bad[letter] = min(m[b][mi] / m[v][mi] for m in sets.values())
                else:
                    bad[letter] = min(m[v][mi] / m[b][mi] for m in sets.values())
            pinned = [k for k, r in bad.items() if r >= PIN_FACTOR * (ok_lo if k == "f" else ok_max)]
            out[entry][metric] = {"ok_max": ok_max, "ok_lo": ok_lo, "bad": bad, "pinned": pinned}
    return out


@functools.lru_cache(None)
def bars():
    """{entry: {"max": BAR, "rms": BAR, "rms_lo": BAR_lo or None, "max_lo": ...}}: the one export the GPU tests use."""
    out = {}
    for entry, by_metric in ratios().items():
        out[entry] = {}
        for metric, r in by_metric.items():
            up = [r["bad"][k] for k in r["pinned"] if k != "f"]
            out[entry][metric] = float(np.sqrt(r["ok_max"] * min(up))) if up else None
            out[entry][metric + "_lo"] = float(np.sqrt(r["ok_lo"] * r["bad"]["f"])) if "f" in r["pinned"] else None
    return out


def table():
    lines = []
    for entry, by_metric in ratios().items():
        for metric, r in by_metric.items():
            b = bars()[entry]
            lo = b[metric + "_lo"]
            lines.append("  %-8s %-3s ok_max %.3f ok_lo %.3f  bad %s  pinned %s  BAR %s  BAR_lo %s" % (
                entry, metric, r["ok_max"], r["ok_lo"], " ".join("%s %.3g" % kv for kv in r["bad"].items()),
                "".join(r["pinned"]) or "-", "%.3f" % b[metric] if b[metric] else "-", "%.3f" % lo if lo else "-"))
    return "\n".join(lines)
