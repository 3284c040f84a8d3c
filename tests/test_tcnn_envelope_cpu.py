"""The bars of tests/test_gpu_precision_tcnn.py, derived on the CPU and proven able to see a broken kernel.

tests/tcnn_restatement.py holds the float64 ideal R of the tiny-cuda-nn networks, their restatement E
(oracle.bnv_oracle.tcnn_mlp(half=True)), the arithmetics a correct kernel may have and six seeded defects.  Here the
ratios m(variant) / m(E) are measured on decoder inputs gathered from the sequence_64 golden volume and encoder inputs
taken from encode_64, with the shipped checkpoint and train.tcnn_default_state_dict(0); the bars follow from them
(tcnn_restatement.bars) and every ratio is printed (pytest -s).

Conditions (not measurements): defects a, b, c, d are pinned by the max metric of every entry; e and f by the rms
metric, or they are listed below.

Residual (unpinned): not separable from the OK variants by 2 x ok_max, with the ratios found (min over input sets and
checkpoints; rms unless noted):
  * f (no activation rounding) at every entry: decoder m(E) / m(f) = 1.24 (max 1.37), encoder 1.31 (max 1.51).  The
    output rounding to f16 and the f16 product with the voxel size remain in f and carry most of E's distance to
    float64; a kernel that kept its activations in fp32 would pass.  No lower bar (BAR_lo) exists.
  * e (activations truncated) at the encoder: 1.74 (max 1.76); pinned at the decoder (2.18).
  * e and f at the gradient entries: on evaluations off the ReLU kinks the straight-through gradient does not see a
    forward rounding at all (e and f equal E there, 1e-3 of the backward kernel's own f16-Jacobian arithmetic that
    scales this entry; ok_lo = 5,400: E and the fp32 accumulations are that much closer to R than it); over all
    evaluations one flipped ReLU dominates both metrics (e 1.01, f 1.11).

The off-kinks gradient entry is scaled by "jac16", the restatement of k_decode_pts_bwd_t's backward (Jacobian rounded
to f16 between the transposed layers), not by E: E's gradient is exact up to fp32 there, so its distance to R is the
noise of an fp32 matmul.  jac16 is an OK variant of both gradient entries.
"""
import numpy as np
import pytest
import torch

import tcnn_restatement as T
from oracle import bnv_oracle as orc

RESIDUAL = {("decoder", "f"), ("encoder", "e"), ("encoder", "f"), ("gradient", "e"), ("gradient", "f"),
            ("gradient_all", "e"), ("gradient_all", "f")}


def test_E_is_the_oracle_restatement_bit_for_bit_and_R_is_its_float64_network():
    for ck, sd in T.checkpoints().items():
        for key, sets, shape in (("nerf.model.params", T.decoder_input_sets(), T.DEC),
                                 ("pointnet_backbone.model.params", T.encoder_input_sets(), T.ENC)):
            params = torch.as_tensor(sd[key]).float()
            for name, x in sets.items():
                e = T.net(params, x, variant="E", **shape)
                assert torch.equal(e, orc.tcnn_mlp(params, x, shape["n_in_padded"], shape["n_out"])), (ck, name)
                # R: the same layout with no rounding but the stored parameters', written out in numpy float64
                h = np.concatenate([x.numpy().astype(np.float64),
                                    np.ones((len(x), shape["n_in_padded"] - x.shape[1]))], 1)
                dims = [shape["n_in_padded"], 64, 64, 64, 16]
                off = 0
                for i in range(4):
                    w = params[off: off + dims[i + 1] * dims[i]].reshape(dims[i + 1], dims[i]).half().double().numpy()
                    off += dims[i + 1] * dims[i]
                    h = h @ w.T
                    if i < 3:
                        h = np.maximum(h, 0)
                r = T.net(params, x, variant="R", **shape)
                assert r.dtype == torch.float64
                assert float(np.abs(r.numpy() - h[:, :shape["n_out"]]).max()) <= 1e-12 * max(1.0, np.abs(h).max())
                # the straight-through forward is the plain forward
                assert torch.equal(T.net(params, x, variant="E", ste=True, **shape), e)


def test_truncation_and_the_f16_product():
    x = torch.from_numpy(np.random.default_rng(3).normal(size=20000).astype(np.float32)) * 3
    t, r = T.trunc_f16(x), T.round_f16(x)
    assert bool((t.abs() <= x.abs()).all()) and torch.equal(t.half().float(), t)
    assert bool(((t == r) | (t.abs() < r.abs())).all())
    assert float(((t - x).abs() / x.abs().clamp(min=1e-3)).max()) <= 2.0 ** -10
    assert float((t != r).float().mean()) > 0.4                                  # half of all roundings went away
    out = T.round_f16(x)
    assert torch.equal(T.sdf_alpha(out) * T.VOXEL, (out.half() * T.VOXEL).double() / T.VOXEL * T.VOXEL)
    assert float((T.sdf_alpha(out) - out.double()).abs().max()) <= 2.0 ** -11 * 1.001 * float(out.abs().max())


def test_bars_are_derived_and_the_defects_pinned():
    print()
    for entry, sets in T.measurements().items():
        for key, m in sets.items():
            print("%-12s %-22s " % (entry, "/".join(key)) + "  ".join(
                "%s %.2e/%.2e" % (v, *mm) for v, mm in m.items()))
    print(T.table())
    ratios, bars = T.ratios(), T.bars()
    unpinned = set()
    for entry in T.ENTRIES:
        r = ratios[entry]
        assert r["max"]["ok_max"] >= 1 and r["rms"]["ok_max"] >= 1
        for d in T.MUST_PIN_MAX:
            assert d in r["max"]["pinned"], (entry, d, r["max"])         # else the harness is inadequate
        for d in T.MUST_PIN_RMS:
            if d not in r["rms"]["pinned"]:
                unpinned.add((entry, d))
        # the bar sits a factor sqrt(2) or more from either side
        for metric in ("max", "rms"):
            rr = r[metric]
            worst = min(rr["bad"][k] for k in rr["pinned"] if k != "f")
            assert rr["ok_max"] * np.sqrt(T.PIN_FACTOR) <= bars[entry][metric] * (1 + 1e-12)
            assert bars[entry][metric] * np.sqrt(T.PIN_FACTOR) <= worst * (1 + 1e-12)
    assert unpinned == RESIDUAL, (unpinned ^ RESIDUAL, "update the residual list of the module docstring")
    # acc16 is a sensitivity figure: reported, never an OK variant
    for entry, sets in T.measurements().items():
        print("acc16 / E, %-12s max %.2f rms %.2f" % (entry, max(m["acc16"][0] / m["E"][0] for m in sets.values()),
                                                      max(m["acc16"][1] / m["E"][1] for m in sets.values())))


@pytest.mark.parametrize("ck", ["shipped", "default0"])
def test_the_bars_see_every_pinned_defect_on_fresh_inputs(ck):
    """On inputs the bars were not derived from (another seed): every OK variant passes m(V) <= BAR m(baseline) and
    every pinned defect fails it, per entry and metric."""
    import os
    from conftest import GOLDEN
    from oracle import precision as P
    z = np.load(os.path.join(GOLDEN, "sequence_64.npz"))
    live = z["features_sorted"][z["weights_sorted"][:, 0] >= 8]
    rng = np.random.default_rng(77)
    n = 4096
    xd = torch.from_numpy(P.sdf_inputs(rng.uniform(-1, 1, size=(n, 3)).astype(np.float32),
                                       live[rng.integers(len(live), size=n)]))
    rows = np.concatenate([rng.uniform(-1, 1, size=(n, 3)), z["frames"].reshape(-1, 6)[rng.integers(
        z["frames"].size // 6, size=n), 3:]], 1).astype(np.float32)
    sd = T.checkpoints()[ck]
    ratios, bars = T.ratios(), T.bars()
    for entry in T.ENTRIES:
        enc = entry == "encoder"
        params = sd["pointnet_backbone.model.params" if enc else "nerf.model.params"]
        x = torch.from_numpy(rows) if enc else xd
        if entry.startswith("gradient"):
            ref = T.feature_grad(params, x, "R")
        else:
            ref = T.net(params, x, variant="R", **T.ENC) if enc else T.decoder_alpha(params, x, "R")
        m = {v: T._measure(entry, params, x, v, ref) for v in T.ok_variants(entry) + tuple(T.DEFECTS.values())}
        for mi, metric in enumerate(("max", "rms")):
            bar = bars[entry][metric] * m[T.BASELINE[entry]][mi]
            for v in T.ok_variants(entry):
                assert m[v][mi] <= bar, (entry, metric, v, m[v][mi], bar)
            for d in ratios[entry][metric]["pinned"]:
                if d != "f":
                    assert m[T.DEFECTS[d]][mi] > bar, (entry, metric, d, m[T.DEFECTS[d]][mi], bar)
