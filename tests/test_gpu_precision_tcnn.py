"""Every kernel that runs the tiny-cuda-nn networks (MLP mode 2), against a float64 run of the same network.

The mode-2 tests elsewhere hold these kernels to flat tolerances against the oracle's fp16 restatement E (features
3e-3, SDF 1e-4 = 0.5 % of a voxel, gradients 2e-2) or to each other bit for bit.  Here the reference is R
(tests/tcnn_restatement.py): the f16-rounded parameters and the fp32 inputs the kernels form, widened to float64,
with float64 accumulation and no rounding anywhere, run through bnv_oracle on a float64 copy of the volume (``geo=`` /
``encoder=``).  A result passes when its max and rms error against R stay within BAR x the error of E against R on
the very same inputs, E evaluated on the CPU at test time.  The bars are computed from seeded defects
(tcnn_restatement.bars; tests/test_tcnn_envelope_cpu.py proves on the CPU that they see them); none is typed in here.
Units: decoder errors in alpha = SDF / voxel; encoder features relative to max |feature|; feature gradients per row,
relative to the largest gradient.  Mask decisions, ids and counts identical.  With fewer than MIN_LIVE_FOR_F16 live
values only the max bar is asserted, against m(E) of the full-size input of the same test.

No per-ulp or bit-equality claim against E is made: the outputs are scatter means and trilinear blends of network
outputs, and the GPU's fp32 accumulation order legitimately lands on the other side of an f16 rounding now and then.

Bars (BAR = sqrt(ok_max x the smallest ratio of a pinned defect); ok_max over E and fp32 accumulation over the K-steps
in either order; defects a dropped K-step, b padding 0.0, c missing last ReLU, d two input slots swapped, e
activations truncated, f no activation rounding):
  decoder   max: ok_max 1.029, a 475 b 624 c 328 d 297 (e 1.41 f 1.37)     BAR 17.49
            rms: ok_max 1.006, a 931 b 1340 c 625 d 375 e 2.18 (f 1.24)    BAR 1.481
  encoder   max: ok_max 1.000, a 515 b 589 c 1250 d 386 (e 1.76 f 1.51)    BAR 19.65
            rms: ok_max 1.000, a 874 b 1130 c 2260 d 375 (e 1.74 f 1.31)   BAR 19.36
  gradient, rows off the ReLU kinks, scaled by the backward kernel's own arithmetic restated ("jac16": Jacobian rounded
  to f16 between the transposed layers; E's straight-through gradient is exact up to fp32 there and 3,000 .. 5,400 x
  closer to R -- ok_lo -- so its distance is matmul noise and scales nothing)
            max: ok_max 1.000, a 3120 b 3650 c 1850 d 2100 (e, f: 1e-3)      BAR 43.02
            rms: ok_max 1.000, a 3490 b 4330 c 2210 d 1640 (e, f: 1e-3)      BAR 40.45
  gradient, all rows, scaled by E
            max: ok_max 1.000, a 4.5 b 5.6 c 3.3 d 3.0 (e 0.85 f 1.00)     BAR 1.721
            rms: ok_max 1.000, a 32.7 b 39.7 c 36.5 d 23.1 (e 1.01 f 1.11) BAR 4.810
Residual (unpinned; test_tcnn_envelope_cpu.py): f everywhere (no lower bar exists: the output rounding and the f16
product with the voxel size carry most of E's distance to float64), e at the encoder and in the gradients.  Parity
with tiny-cuda-nn's own CUDA arithmetic stays unpinned as before.

Gradients: a corner evaluation is kink-flagged when a hidden unit's float64 pre-activation lies within 4 x E's own
error of zero (tcnn_restatement.kink_flags; at most a quarter of the live evaluations, asserted).  A row's gradient
sums the evaluations AT that row, so a row is off the kinks when none of them is flagged: a quarter of the rows or
more at 129 queries and up (asserted), enough for both metrics.  Those rows are held to the "off the kinks" bars
against jac16 on the same rows, all rows to the "all rows" bars against E on the same rows: their errors are flipped
ReLUs, which the f16 roundings decide and E shares with a correct kernel.  Few rows (one query: 8): the max bar alone,
against the 2,400-query case of the same test.

Measured on an MI355X, m(GPU) / m(baseline) as max / rms (the baseline's own max error in brackets):
  decode_pts, every n                     1.000 / 0.999 .. 1.000          (5.8e-5 .. 6.7e-4 alpha)
  lattice, lattice_pipe 1 and 0 alike     1.000 / 1.000 .. 1.004          (1.8e-4 .. 6.7e-4 alpha)
  lattice, two rows exchanged             2533 / 1358: refused
  dense corners / nearest / global        1.000 / 0.998, 1.000 / 1.000, 1.000 / 1.000   (6.2e-4, 2.0e-3, 1.1e-3)
  encoder from points, three settings     1.000 / 1.000                   (1.4e-4 .. 2.1e-4 relative)
  encoder from depth, three settings      1.000 / 1.000 .. 1.001          (1.4e-4 .. 2.8e-4 relative)
  frame pipe                              1.000 / 1.000                   (7.6e-4 alpha)
  default initialisation, decode / encode 1.000 / 1.000, 1.000 / 1.001    (5.0e-4 alpha, 5.7e-4 relative)
  backward, all rows (against E)          1.000 .. 1.001 / 1.000 .. 1.003 at 33 .. 2,400 queries (E: 7.7e-3 .. 2.4e-2 of
                                          the largest gradient); one query: 1.5e-4, no ReLU flipped, held to the
                                          few-rows bar 1.721 x 2.4e-2
  backward, rows off the kinks (jac16)    1.000 .. 1.001 / 1.000 on 7, 70, 196 and 368 rows (jac16: 1.0e-4 .. 1.5e-4):
                                          the kernel's f16 Jacobian is the restated one
"""
import os

import numpy as np
import pytest
import torch

import tcnn_restatement as T
from conftest import GOLDEN, WEIGHTS_TCNN
from oracle import bnv_oracle as orc
from test_gpu_precision import DEV, MIN_LIVE_FOR_F16, VOXEL, _oracle64, _same_mask, bnv, golden  # noqa: F401

pytestmark = pytest.mark.gpu
SETTINGS = ((1, 1), (1, 0), (0, 1))          # (tcnn_block_encoder, tcnn_shared_table)
LATTICE_DELTA_ROWS = 120                     # decode_lattice with sdf_delta: origins up to this prefix


# ---------------------------------------------------------------------------------------------------------------
# fixtures and helpers
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def BARS():
    assert T.VOXEL == VOXEL
    return T.bars()


@pytest.fixture(scope="module")
def golden64(golden):
    return _oracle64(orc, golden, np.load(os.path.join(GOLDEN, "sequence_64.npz"))["dims"])


@pytest.fixture(scope="module")
def tsd():
    return {k: torch.as_tensor(v).float() for k, v in orc.load_weights(WEIGHTS_TCNN).items()}


@pytest.fixture(scope="module")
def dec(tsd):
    p = tsd["nerf.model.params"]
    return {"R": T.geo(p, "R"), "E": T.geo(p, "E"), "E_raw": T.geo(p, "E", product=False),
            "E_ste": T.geo(p, "E", ste=True), "params": p}


@pytest.fixture(scope="module")
def enc(tsd):
    p = tsd["pointnet_backbone.model.params"]
    return {"R": T.encoder(p, "R"), "E": T.encoder(p, "E")}


@pytest.fixture(scope="module")
def model_t(bnv):
    m = bnv.load_pretrained(device=DEV, voxel_size=VOXEL, tiny_cuda=True)
    assert m.mlp_mode == 2
    yield m
    bnv.set_mlp_mode(1)


@pytest.fixture(scope="module")
def lib(bnv):
    from bnv_fusion_amd import _lib
    handle = _lib.load()
    yield handle
    for name in (b"lattice_pipe", b"tcnn_block_encoder", b"tcnn_shared_table"):
        handle.bnv_set_option(name, 1)


def _errs(got, ref, keep=None, scale=VOXEL):
    """|got - ref| / scale over the kept values, float64 [k]."""
    d = (got.detach().cpu().double().reshape(-1) - ref.detach().cpu().double().reshape(-1)).abs() / scale
    return d if keep is None else d[keep.reshape(-1)]


def _m(errs):
    """(max, rms) of a list of error vectors taken together."""
    e = torch.cat([x.reshape(-1) for x in errs]) if len(errs) else torch.zeros(0)
    return (float(e.max()), float(e.pow(2).mean().sqrt())) if e.numel() else (0.0, 0.0)


def _check(m_gpu, m_e, bars, n_live, what, m_e_full=None):
    """m(GPU) <= BAR m(E) for max and rms (and >= m(E) / BAR_lo where a lower bar exists); few live values: the max
    bar alone, against m(E) of the full-size input."""
    ratio = tuple(g / e if e > 0 else float("nan") for g, e in zip(m_gpu, m_e))
    print(f"{what}: live {n_live}, GPU max/rms {m_gpu[0]:.3e}/{m_gpu[1]:.3e}, baseline {m_e[0]:.3e}/{m_e[1]:.3e}, "
          f"ratio {ratio[0]:.3f}/{ratio[1]:.3f}")
    if n_live < MIN_LIVE_FOR_F16:
        assert m_e_full is not None and m_e_full[0] > 0, what
        assert m_gpu[0] <= bars["max"] * m_e_full[0], (what, m_gpu, m_e_full, bars)
        return ratio
    assert m_e[0] > 0 and m_e[1] > 0, what
    for i, metric in enumerate(("max", "rms")):
        assert m_gpu[i] <= bars[metric] * m_e[i], (what, metric, m_gpu, m_e, bars)
        lo = bars[metric + "_lo"]
        if lo is not None:
            assert m_gpu[i] >= m_e[i] / lo, (what, metric, "higher precision than the network's", m_gpu, m_e, bars)
    return ratio


# ---------------------------------------------------------------------------------------------------------------
# k_decode_pts, PREC 2
# ---------------------------------------------------------------------------------------------------------------
def _decode_pts_queries(vol, n):
    """The query sets of test_gpu_precision.test_decode_pts_vs_float64: mixed, live and all-masked."""
    g = torch.Generator().manual_seed(1000 + n)
    valid = vol.active_coordinates.cpu()[(vol.weights[:, 0] >= 8).cpu()]
    out = []
    # (the large size is there for the index range and the grid: one kind, so that its references stay quick)
    for kind in (("mixed", "live", "masked") if n < 1000 else ("mixed",)):
        if kind == "masked":
            q = torch.rand(1, n, 1, 3, generator=g) * 3 + 1.0
        else:
            base = valid[torch.randint(len(valid), (n,), generator=g)].float()
            spread = 1.6 if kind == "mixed" else 0.0
            q = (base + (torch.rand(n, 3, generator=g) - 0.5) * spread).reshape(1, n, 1, 3)
        out.append((kind, q))
    return out


def _decode_pts_refs(vol, ovol, dec, delta, n):
    """[(kind, coords, is_coords, delta or None, R, E, live)] of one n, on the CPU."""
    cases = []
    for kind, q in _decode_pts_queries(vol, n):
        qw = q * vol.voxel_size + ovol.min_coords
        live = {}
        for coords, is_coords, d in ((q, True, None), (qw, False, None), (q, True, delta), (qw, False, delta)):
            r = ovol.decode_pts(coords, None, d, is_coords=is_coords, query_tensor=True, geo=dec["R"])
            if d is None:
                live[is_coords] = r.reshape(-1) != vol.voxel_size
            # (all-masked queries: E has nothing to add, the mask is R's)
            e = r if kind == "masked" else ovol.decode_pts(coords, None, d, is_coords=is_coords, query_tensor=True,
                                                           geo=dec["E"])
            assert r.dtype == torch.float64 and e.dtype == torch.float64
            cases.append((kind, coords, is_coords, d, r, e, live[is_coords]))
    return cases


@pytest.fixture(scope="module")
def delta():
    return torch.from_numpy(np.load(os.path.join(GOLDEN, "decode_64.npz"))["sdf_delta"])


@pytest.fixture(scope="module")
def decode_pts_full(golden, golden64, dec, delta):
    """The n = 4097 references, and m(E) over them: the scale of the few-live-values cases."""
    cases = _decode_pts_refs(golden, golden64, dec, delta, 4097)
    return cases, _m([_errs(e, r, live) for _, _, _, _, r, e, live in cases])


@pytest.mark.parametrize("n", [1, 15, 16, 17, 127, 128, 129, 4097])
def test_decode_pts_vs_float64(bnv, model_t, golden, golden64, dec, delta, decode_pts_full, BARS, n):
    """k_decode_pts<PREC 2> (stage_input_t, sdf_mlp_tile_t, 128 evaluations per workgroup) around its 16-query tile
    and its 128-evaluation chunk; mixed, live and all-masked queries; voxel and world coordinates; with and without
    sdf_delta."""
    vol = golden
    cases = decode_pts_full[0] if n == 4097 else _decode_pts_refs(vol, golden64, dec, delta, n)
    gpu, rest, n_live = [], [], 0
    for kind, coords, is_coords, d, r, e, live in cases:
        out = vol.decode_pts(coords.to(DEV), model_t.nerf, None if d is None else d.to(DEV), is_coords=is_coords,
                             query_tensor=True)
        if d is None:
            assert _same_mask(out, r), (kind, is_coords)
            n_live += int(live.sum())
        if kind == "masked":
            assert not bool(live.any())
        gpu.append(_errs(out, r, live))
        rest.append(_errs(e, r, live))
    _check(_m(gpu), _m(rest), BARS["decoder"], n_live, f"decode_pts n={n}", decode_pts_full[1])


def test_default_initialisation_vs_float64(bnv, golden, golden64, encode_full, BARS):
    """The other checkpoint of the CPU derivation, train.tcnn_default_state_dict(0) (what a training run starts from),
    through decode_pts (n = 129, no sdf_delta) and the point encoder (all of encode_64)."""
    from bnv_fusion_amd import train
    sd = train.tcnn_default_state_dict(0)
    try:
        model = bnv.load_pretrained(device=DEV, voxel_size=VOXEL, tiny_cuda=True, state_dict=sd)
        p = torch.as_tensor(sd["nerf.model.params"]).float()
        geo = {"R": T.geo(p, "R"), "E": T.geo(p, "E")}
        gpu, rest, n_live = [], [], 0
        for kind, q in _decode_pts_queries(golden, 129):
            r = golden64.decode_pts(q, None, None, is_coords=True, query_tensor=True, geo=geo["R"])
            e = golden64.decode_pts(q, None, None, is_coords=True, query_tensor=True, geo=geo["E"])
            out = golden.decode_pts(q.to(DEV), model.nerf, None, is_coords=True, query_tensor=True)
            assert _same_mask(out, r), kind
            live = r.reshape(-1) != VOXEL
            n_live += int(live.sum())
            gpu.append(_errs(out, r, live))
            rest.append(_errs(e, r, live))
        assert n_live >= MIN_LIVE_FOR_F16
        _check(_m(gpu), _m(rest), BARS["decoder"], n_live, "default initialisation, decode_pts n=129")
        z, pts, (n_xyz, mn, mx, voxel), _, _, _, _ = encode_full
        pe = torch.as_tensor(sd["pointnet_backbone.model.params"]).float()
        r, e = _encode_refs({"R": T.encoder(pe, "R"), "E": T.encoder(pe, "E")}, pts, n_xyz, mn, mx, voxel)
        vol = bnv.SparseVolume(8, voxel, z["dims"], 8, device=DEV)
        f, c, ids, _, _ = model.encode_pointcloud(pts.to(DEV), vol.n_xyz, vol.min_coords, vol.max_coords, voxel,
                                                  return_dense=False)
        _encode_check(f, c, ids, r, e, BARS["encoder"], "default initialisation, encode points", None, None)
    finally:
        bnv.set_mlp_mode(1)


# ---------------------------------------------------------------------------------------------------------------
# decode_lattice: k_lattice_table_t (lattice_pipe 1) and k_decode<LATTICE, PREC 2> (lattice_pipe 0), then the blend
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice_full(golden, golden64, dec, delta):
    """Origins (live voxels first, then the rest, then 40 dead ones with no live lattice point), R and E for all of
    them with and without sdf_delta -- a lattice is decoded per origin, so a prefix's reference is the prefix."""
    vol, ovol = golden, golden64
    keys = vol.active_coordinates.cpu()
    ok = (vol.weights[:, 0] >= 8).cpu()
    taken = torch.zeros(64, 64, 64, dtype=torch.bool)
    for dx in range(-2, 3):
        for dy in range(-2, 3):
            for dz in range(-2, 3):
                c = (keys + torch.tensor([dx, dy, dz])).clamp(0, 63)
                taken[c[:, 0], c[:, 1], c[:, 2]] = True
    free = (~taken[2:62, 2:62, 2:62]).nonzero() + 2
    dead = free[torch.linspace(0, len(free) - 1, 40).long()]
    origins = torch.cat([keys[ok], keys[~ok], dead]).contiguous()
    n_keys = len(keys)
    lat = orc.lattice_coords(origins.numpy())
    ref = {"plain": tuple(ovol.decode_pts(lat, None, None, is_coords=True, query_tensor=True, geo=dec[k])[0, :, :, 0]
                          for k in ("R", "E"))}
    # with sdf_delta: the prefixes up to LATTICE_DELTA_ROWS origins and the dead ones (keeps the references quick)
    part = torch.cat([torch.arange(LATTICE_DELTA_ROWS), torch.arange(n_keys, len(origins))])
    ref["delta"] = []
    for k in ("R", "E"):
        full = torch.full_like(ref["plain"][0], float("nan"))
        full[part] = ovol.decode_pts(lat[:, part], None, delta, is_coords=True, query_tensor=True,
                                     geo=dec[k])[0, :, :, 0]
        ref["delta"].append(full)
    live = ref["plain"][0] != vol.voxel_size
    assert not bool(live[n_keys:].any()) and int(live.sum()) > 1000
    m_e = _m([_errs(ref["plain"][1], ref["plain"][0], live)])
    return origins, ref, live, n_keys, m_e


def _lattice_run(vol, model_t, lib, delta, lattice_full, pipe, rows):
    origins, ref, live, _, _ = lattice_full
    assert lib.bnv_set_option(b"lattice_pipe", pipe) == 0
    o = origins[rows].contiguous().to(DEV)
    out = vol.decode_lattice(o, model_t.nerf, None, query_tensor=True)
    assert _same_mask(out, ref["plain"][0][rows]), pipe
    lv = live[rows]
    gpu = [_errs(out, ref["plain"][0][rows], lv)]
    rest = [_errs(ref["plain"][1][rows], ref["plain"][0][rows], lv)]
    if not bool(torch.isnan(ref["delta"][0][rows]).any()):
        out_d = vol.decode_lattice(o, model_t.nerf, delta.to(DEV), query_tensor=True)
        gpu.append(_errs(out_d, ref["delta"][0][rows], lv))
        rest.append(_errs(ref["delta"][1][rows], ref["delta"][0][rows], lv))
    return out, gpu, rest, int(lv.sum())


@pytest.mark.parametrize("pipe", [1, 0])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 120, "all", "33+dead", "all+dead"])
def test_decode_lattice_vs_float64(bnv, model_t, golden, lib, delta, lattice_full, BARS, n, pipe):
    """Both lattice kernels against R (not only against each other): whole and ragged work lists of the wave-per-32-
    entries table kernel, with dead voxels appended (origins that add no entry)."""
    origins, _, _, n_keys, m_e_full = lattice_full
    k = n_keys if str(n).startswith("all") else int(str(n).split("+")[0])
    rows = torch.arange(k)
    if str(n).endswith("+dead"):
        rows = torch.cat([rows, torch.arange(n_keys, len(origins))])
    try:
        out, gpu, rest, n_live = _lattice_run(golden, model_t, lib, delta, lattice_full, pipe, rows)
    finally:
        lib.bnv_set_option(b"lattice_pipe", 1)
    if str(n).endswith("+dead"):
        assert bool((out[k:] == np.float32(VOXEL)).all())
    _check(_m(gpu), _m(rest), BARS["decoder"], n_live, f"lattice pipe={pipe} n={n}", m_e_full)


def test_decode_lattice_bar_sees_a_permuted_row(bnv, model_t, golden, lib, delta, lattice_full, BARS):
    """The comparison compares what it claims to: the lattice_pipe 0 result at n = 33 passes, and the same result
    with two of its rows exchanged does not.  Runs no kernel the test above does not."""
    rows = torch.arange(33)
    _, ref, live, _, m_e_full = lattice_full
    try:
        out, gpu, rest, n_live = _lattice_run(golden, model_t, lib, delta, lattice_full, 0, rows)
    finally:
        lib.bnv_set_option(b"lattice_pipe", 1)
    assert n_live >= MIN_LIVE_FOR_F16
    _check(_m(gpu), _m(rest), BARS["decoder"], n_live, "lattice pipe=0 n=33", m_e_full)
    r = ref["plain"][0][rows]
    lv = live[rows]
    a = int(lv.sum(1).argmax())
    b = int((r[:, lv[a]] - r[a, lv[a]]).abs().amax(1).argmax())
    assert float((r[b, lv[a]] - r[a, lv[a]]).abs().max()) > 0.1 * VOXEL        # 0.1 alpha, E's own error: ~1e-3
    swapped = out.clone()
    swapped[[a, b]] = out[[b, a]]
    with pytest.raises(AssertionError):
        _check(_m([_errs(swapped, r, lv)]), _m(rest[:1]), BARS["decoder"], n_live, "lattice, rows exchanged", m_e_full)


# ---------------------------------------------------------------------------------------------------------------
# dense decode: every branch accepts a mode-2 model
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", ["corners", "nearest", "global"])
def test_dense_decode_vs_float64(bnv, model_t, dec, BARS, branch):
    """bnv_decode_dense with a tiny-cuda-nn model: k_decode<DENSE, PREC 2> (8 corners) and k_decode<DENSE1, PREC 2>
    (nearest, global) on the tcnn encoder's own fp32 feature grids.  No branch refuses mode 2.  The global branch
    returns the unscaled f16 prediction: its error is alpha itself, and E has no product with the voxel size."""
    z0 = np.load(os.path.join(GOLDEN, "dense_decode_64.npz"))
    zq = np.load(os.path.join(GOLDEN, "dense_modes_64.npz"))
    voxel = float(z0["voxel_size"])
    assert np.float32(voxel) == np.float32(VOXEL)
    vol = bnv.SparseVolume(8, voxel, z0["dims"], 8, device=DEV)
    fg, mask, _, _ = model_t.encode_pointcloud(torch.from_numpy(z0["input_pts"]).to(DEV), vol.n_xyz, vol.min_coords,
                                               vol.max_coords, voxel, return_dense=True)
    q = torch.from_numpy(z0["queries"] if branch == "corners" else zq["queries"])
    kw = dict(global_coords=branch == "global", interpolate_decode=branch != "nearest")
    r, _ = orc.decode_feature_grid_w_pts(None, q, fg.cpu(), mask.cpu(), voxel, geo=dec["R"], **kw)
    e, _ = orc.decode_feature_grid_w_pts(None, q, fg.cpu(), mask.cpu(), voxel,
                                         geo=dec["E_raw" if branch == "global" else "E"], **kw)
    assert r.dtype == torch.float64 and e.dtype == torch.float64
    live = r.reshape(-1) != voxel
    try:
        model_t.interpolate_decode = branch != "nearest"
        out, _ = model_t.decode_feature_grid_w_pts(q.to(DEV), fg, mask, voxel, vol.min_coords,
                                                   global_coords=branch == "global")
    finally:
        model_t.interpolate_decode = True
    assert _same_mask(out, r, voxel)
    scale = 1.0 if branch == "global" else voxel
    assert int(live.sum()) >= MIN_LIVE_FOR_F16
    _check(_m([_errs(out, r, live, scale)]), _m([_errs(e, r, live, scale)]), BARS["decoder"], int(live.sum()),
           f"dense {branch}")


# ---------------------------------------------------------------------------------------------------------------
# encoder: k_pointnet_scatter_tb<SHARED> (block encoder) and k_pointnet_scatter_t
# ---------------------------------------------------------------------------------------------------------------
def _encode_refs(enc, pts, n_xyz, mn, mx, voxel):
    r = orc.encode_pointcloud(None, pts, n_xyz, mn, mx, voxel, encoder=enc["R"])
    e = orc.encode_pointcloud(None, pts, n_xyz, mn, mx, voxel, encoder=enc["E"])
    return r, e


def _encode_check(f, c, ids, r, e, bars, what, m_e_full, scale_full):
    fr, cr, idr = r[0], r[1], r[2]
    assert fr.dtype == torch.float64 and e[0].dtype == torch.float64
    assert torch.equal(ids.cpu(), idr) and torch.equal(c.reshape(-1).cpu(), cr.reshape(-1)), what
    scale = float(fr.abs().max()) if fr.numel() >= MIN_LIVE_FOR_F16 else scale_full
    return _check(_m([_errs(f, fr, None, scale)]), _m([_errs(e[0], fr, None, scale)]), bars, fr.numel(), what,
                  m_e_full)


@pytest.fixture(scope="module")
def encode_full(enc):
    """encode_64's points ordered by the voxel they fall in (a prefix then fills voxels past min_pts_in_grid), and R,
    E of all of them."""
    z = np.load(os.path.join(GOLDEN, "encode_64.npz"))
    voxel = float(z["voxel_size"])
    mn, mx, n_xyz = orc.get_world_range(z["dims"], voxel)
    mn, mx, n_xyz = torch.from_numpy(mn).float(), torch.from_numpy(mx).float(), torch.tensor(n_xyz)
    pts = torch.from_numpy(z["input_pts"])
    xyz = pts[0, :, :3]
    cell = torch.floor((xyz - mn) / voxel).long()
    inside = ((xyz < mx - voxel) & (xyz > mn + voxel)).all(1)
    key = (cell[:, 0] * 64 + cell[:, 1]) * 64 + cell[:, 2]
    order = torch.argsort(torch.where(inside, key, torch.full_like(key, 2 ** 40)), stable=True)
    pts = pts[:, order].contiguous()
    r, e = _encode_refs(enc, pts, n_xyz, mn, mx, voxel)
    scale = float(r[0].abs().max())
    return z, pts, (n_xyz, mn, mx, voxel), r, e, _m([_errs(e[0], r[0], None, scale)]), scale


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65, "all"])
@pytest.mark.parametrize("setting", SETTINGS)
def test_encode_pointcloud_vs_float64(bnv, model_t, enc, lib, encode_full, BARS, setting, n):
    """The point entry under the three (tcnn_block_encoder, tcnn_shared_table) settings: blocks of 32 consecutive
    points, whole and ragged; voxel ids and counts identical to the float64 encoder's.  One point fills no voxel past
    min_pts_in_grid: that case compares no feature value, only that ids and counts come back empty."""
    z, pts, (n_xyz, mn, mx, voxel), r_all, e_all, m_e_full, scale_full = encode_full
    vol = bnv.SparseVolume(8, voxel, z["dims"], 8, device=DEV)
    p = pts if n == "all" else pts[:, :n].contiguous()
    r, e = (r_all, e_all) if n == "all" else _encode_refs(enc, p, n_xyz, mn, mx, voxel)
    try:
        assert lib.bnv_set_option(b"tcnn_block_encoder", setting[0]) == 0
        assert lib.bnv_set_option(b"tcnn_shared_table", setting[1]) == 0
        f, c, ids, _, _ = model_t.encode_pointcloud(p.to(DEV), vol.n_xyz, vol.min_coords, vol.max_coords, voxel,
                                                    return_dense=False)
    finally:
        lib.bnv_set_option(b"tcnn_block_encoder", 1)
        lib.bnv_set_option(b"tcnn_shared_table", 1)
    if n != "all" and n >= 31:
        assert r[0].numel() > 0                        # the prefix does fill a voxel
    _encode_check(f, c, ids, r, e, BARS["encoder"], f"encode points n={n} setting={setting}", m_e_full, scale_full)


@pytest.fixture(scope="module")
def depth_frame():
    """A 240 x 320 synthetic frame; the images of the depth tests are its top-left corners under ITS intrinsics, so
    that a 5 x 9 image still fills voxels past min_pts_in_grid."""
    from bnv_fusion_amd import synthetic
    dims, voxel = synthetic.GRID_DIMS[128]
    assert voxel == VOXEL
    return synthetic.depth_u16(7, 240, 320), synthetic.intrinsics(240, 320), synthetic.pose(7), dims


def _depth_case(bnv, model_t, enc, depth_frame, hw):
    from bnv_fusion_amd.frontend import depth_to_input_pts
    d16, intr, T_wc, dims = depth_frame
    vol = bnv.SparseVolume(8, VOXEL, np.array([dims] * 3), 8, device=DEV)
    depth = torch.from_numpy(np.ascontiguousarray(d16[:hw[0], :hw[1]])).to(DEV)
    pts = depth_to_input_pts(depth, intr, T_wc, max_depth=3.0).cpu()
    args = (vol.n_xyz.cpu(), vol.min_coords.cpu(), vol.max_coords.cpu(), VOXEL)
    r, e = _encode_refs(enc, pts, *args)

    def run():
        f, c, ids, _, cnt, _, _ = model_t.encode_depth_async(depth, intr, T_wc, 3.0, vol.n_xyz, vol.min_coords,
                                                             vol.max_coords, VOXEL)
        h = cnt.cpu()
        assert int(h[4]) == 0
        n_out = int(h[2])
        return f[:n_out], c[:n_out], ids[:n_out]

    return r, e, run


@pytest.fixture(scope="module")
def depth_full(bnv, model_t, enc, depth_frame):
    r, e, _ = _depth_case(bnv, model_t, enc, depth_frame, (75, 100))
    scale = float(r[0].abs().max())
    return _m([_errs(e[0], r[0], None, scale)]), scale


@pytest.mark.parametrize("hw", [(1, 1), (5, 9), (16, 16), (37, 53), (75, 100)])
def test_encode_depth_vs_float64(bnv, model_t, enc, lib, depth_frame, depth_full, BARS, hw):
    """The depth entry (8 x 4-pixel blocks, 16 x 16 patches per workgroup) under the three settings, against the
    float64 encoder run on the points the front end produced: until now the settings were compared with each other
    only.  The 1 x 1 image fills no voxel past min_pts_in_grid: it compares no feature value, only that the output
    is empty under every setting."""
    r, e, run = _depth_case(bnv, model_t, enc, depth_frame, hw)
    try:
        for setting in SETTINGS:
            assert lib.bnv_set_option(b"tcnn_block_encoder", setting[0]) == 0
            assert lib.bnv_set_option(b"tcnn_shared_table", setting[1]) == 0
            f, c, ids = run()
            if r[0] is None:
                assert len(ids) == 0, (hw, setting)
                continue
            _encode_check(f, c, ids, r, e, BARS["encoder"], f"encode depth {hw} setting={setting}", *depth_full)
    finally:
        lib.bnv_set_option(b"tcnn_block_encoder", 1)
        lib.bnv_set_option(b"tcnn_shared_table", 1)
    if hw[0] * hw[1] >= 45:
        assert r[0] is not None and r[0].numel() > 0, hw


# ---------------------------------------------------------------------------------------------------------------
# the frame pipe
# ---------------------------------------------------------------------------------------------------------------
def test_frame_pipe_lattice_vs_float64(bnv, model_t, dec, BARS):
    """A few 75 x 100 frames of a tiny-cuda-nn NeuralMap through the frame pipe, against a float64 decode of the very
    volume the last frame decoded."""
    from bnv_fusion_amd import synthetic
    dims = np.array([1.24] * 3)
    frames = []
    for t in range(3):
        p = torch.from_numpy(synthetic.frame(t, H=75, W=100))
        p[..., :3] *= 0.3
        frames.append(p.to(DEV))
    nm = bnv.NeuralMap(dims, VOXEL, model_t, device=DEV)
    for k in range(10):
        coords, sdf = nm.fuse_and_decode_async({"input_pts": frames[k % 3]}).result()
    torch.cuda.synchronize()
    nm.volume.to_tensor()
    ovol = _oracle64(orc, nm.volume, dims)
    lat = orc.lattice_coords(coords.cpu().numpy())
    r = ovol.decode_pts(lat, None, None, is_coords=True, query_tensor=True, geo=dec["R"])[0, :, :, 0]
    e = ovol.decode_pts(lat, None, None, is_coords=True, query_tensor=True, geo=dec["E"])[0, :, :, 0]
    live = r != VOXEL
    assert int(live.sum()) > 1000
    assert _same_mask(sdf, r)
    _check(_m([_errs(sdf, r, live)]), _m([_errs(e, r, live)]), BARS["decoder"], int(live.sum()), "frame pipe")


# ---------------------------------------------------------------------------------------------------------------
# k_decode_pts_bwd_t
# ---------------------------------------------------------------------------------------------------------------
BWD_FULL = 2400                 # the full-size query count: scales the few-rows cases
MIN_CLEAN_FRACTION = 0.25       # of the rows that receive gradient, at 129 queries and more
MAX_FLAGGED_FRACTION = 0.25     # of the live corner evaluations (the guard of test_gpu_precision.py)


def _row_errs(got, ref, rows, gmax):
    return (got - ref).abs().amax(-1)[rows] / gmax


def _backward_refs(vol, dec, n):
    """CPU side of one query count: queries, incoming gradients, the float64 gradient through R, E's straight-through
    gradient (autograd through the oracle), the backward kernel's own arithmetic (tcnn_restatement.feature_grad_jac16
    per corner evaluation, summed into the rows in float64), and the rows off the ReLU kinks.  A row's gradient is the
    sum over the corner evaluations AT THAT ROW: it is off the kinks when none of those is flagged."""
    g = torch.Generator().manual_seed(50 + n)
    valid = vol.active_coordinates.cpu()[(vol.weights[:, 0] >= 8).cpu()]
    dims = np.load(os.path.join(GOLDEN, "sequence_64.npz"))["dims"]
    m = max(n, 64)
    q = (valid[torch.randint(len(valid), (m,), generator=g)].float()
         + (torch.rand(m, 3, generator=g) - 0.5) * 1.6).reshape(1, m, 1, 3)
    if n == 1:                                                               # the one query is a live one
        out = _oracle64(orc, vol, dims).decode_pts(q, None, None, is_coords=True, query_tensor=True, geo=dec["R"])
        q = q[:, (out.reshape(-1) != vol.voxel_size).nonzero()[:1, 0]]
    q = q[:, :n].contiguous()
    gs = torch.rand(n, generator=g) * 2 - 1
    grads = {}
    for k in ("R", "E_ste"):
        ovol = _oracle64(orc, vol, dims)
        ovol.features.requires_grad_(True)
        out = ovol.decode_pts(q, None, None, is_coords=True, query_tensor=True, geo=dec[k])
        (out.reshape(-1) * gs.double()).sum().backward()
        grads[k] = ovol.features.grad.detach()
        if k == "R":
            live = out.detach().reshape(-1) != vol.voxel_size
    ref, rest = grads["R"], grads["E_ste"]
    nb = orc.get_neighbors(q)[0, :, :, 0]                                    # [8, n, 3] float corners
    local = q[0, :, 0][None] - nb                                            # [8, n, 3]
    rows = torch.tensor(ovol._rows(nb, ovol._tensor_map)).reshape(8, n)
    feats = ovol.features.detach()[rows.clamp(min=0)].reshape(-1, 8)
    x = torch.cat([orc.xyz_encoding(local.reshape(-1, 3)), feats.float()], -1)
    live_eval = live[None].expand(8, n)
    flagged = T.kink_flags(dec["params"], x).reshape(8, n) & live_eval
    dirty = torch.zeros(len(ref), dtype=torch.bool)
    dirty[rows[flagged]] = True
    # d (sum gs out) / d features[row] = sum over its evaluations of gs w voxel d alpha / d features
    w = torch.prod(1 - local.abs(), -1).double()
    w = w / w.sum(0, keepdim=True)
    coef = (w * gs.double()[None] * vol.voxel_size * live_eval).reshape(-1, 1)
    jac = torch.zeros_like(ref).index_add_(0, rows.reshape(-1).clamp(min=0),
                                           T.feature_grad_jac16(dec["params"], x) * coef)
    has = ref.abs().amax(-1) > 0
    assert torch.equal(rest.abs().amax(-1) > 0, has) and torch.equal(jac.abs().amax(-1) > 0, has)
    n_eval = int(live_eval.sum())
    if n_eval:
        assert int(flagged.sum()) <= MAX_FLAGGED_FRACTION * n_eval, (int(flagged.sum()), n_eval)
    clean = has & ~dirty
    gmax = float(ref.abs().max())
    m_e = {"all": _m([_row_errs(rest, ref, has, gmax)]) if bool(has.any()) else (0.0, 0.0),
           "clean": _m([_row_errs(jac, ref, clean, gmax)]) if bool(clean.any()) else (0.0, 0.0)}
    return dict(q=q, gs=gs, ref=ref, live=live, has=has, clean=clean, gmax=gmax, m_e=m_e,
                flagged=int(flagged.sum()), n_eval=n_eval)


@pytest.fixture(scope="module")
def backward_full(golden, dec):
    return _backward_refs(golden, dec, BWD_FULL)


@pytest.mark.parametrize("n", [1, 33, 129, BWD_FULL])
def test_decode_pts_backward_vs_float64(bnv, model_t, golden, dec, backward_full, BARS, n):
    """Feature gradients of k_decode_pts_bwd_t against float64 autograd through R; the same rows receive gradient.
    All rows: within the bar of E's straight-through gradient (tcnn_geo_forward(ste=True)'s convention) on the same
    rows -- their errors are flipped ReLUs.  Rows off the kinks: within the bar of the backward kernel's own
    arithmetic restated on the same rows (f16 Jacobian between the transposed layers; E is exact up to fp32 there).
    At 129 queries and more a quarter of the rows or more is off the kinks and both metrics are asserted; one query
    has 8 rows or none, 33 queries a few dozen: the max bar alone, against the full-size (2,400-query) case."""
    vol = golden
    c = backward_full if n == BWD_FULL else _backward_refs(vol, dec, n)
    ref, has, clean, gmax = c["ref"], c["has"], c["clean"], c["gmax"]
    grad = torch.zeros_like(vol.features)
    vol.decode_pts_backward(c["q"].to(DEV), model_t.nerf, c["gs"].to(DEV), grad, is_coords=True)
    got = grad.cpu().double()
    assert torch.equal(got.abs().amax(-1) > 0, has)
    print(f"backward n={n}: rows {int(has.sum())}, off the kinks {int(clean.sum())}, flagged evaluations "
          f"{c['flagged']} / {c['n_eval']}")
    assert int(has.sum()) >= 8
    assert bool(c["live"].any()) and bool(has.any())
    if n >= 129:
        assert int(clean.sum()) >= max(MIN_LIVE_FOR_F16, MIN_CLEAN_FRACTION * int(has.sum())), int(clean.sum())
    _check(_m([_row_errs(got, ref, has, gmax)]), c["m_e"]["all"], BARS["gradient_all"], int(has.sum()),
           f"backward n={n}, all rows", backward_full["m_e"]["all"])
    if n >= 33:
        assert bool(clean.any())
    if bool(clean.any()):
        _check(_m([_row_errs(got, ref, clean, gmax)]), c["m_e"]["clean"], BARS["gradient"], int(clean.sum()),
               f"backward n={n}, rows off the kinks", backward_full["m_e"]["clean"])


def test_optimiser_takes_the_split_path_for_mode_2(bnv, model_t, golden):
    """bnv_optim_step (the fused forward + loss + backward of the fp32 decoders) refuses MLP mode 2 with
    invalid-argument; the Python optimiser never calls it for a tiny-cuda-nn decoder and runs its own forward, ray
    loss and backward launches instead."""
    from bnv_fusion_amd import _lib, optimize
    op = np.load(os.path.join(GOLDEN, "optimize_64.npz"))
    rays = {k[5:]: torch.from_numpy(op[k]).to(DEV) for k in op.files if k.startswith("rays_")}
    args = (int(op["truncated_units"]), float(op["truncated_dist"]), int(op["ray_max_dist"]))
    z = np.load(os.path.join(GOLDEN, "sequence_64.npz"))
    vol = bnv.SparseVolume(8, float(z["voxel_size"]), z["dims"], 8, device=DEV)
    n = len(z["keys_sorted"])
    vol.insert(torch.from_numpy(z["keys_sorted"]).to(DEV), torch.from_numpy(z["features_sorted"]).to(DEV),
               torch.from_numpy(z["weights_sorted"]).to(DEV), torch.zeros(n, 1, device=DEV))
    vol.to_tensor()
    calls = []
    fused = vol.optim_step
    vol.optim_step = lambda *a, **k: calls.append(1) or fused(*a, **k)
    grad = torch.zeros_like(vol.features)
    loss, pts = optimize.ray_batch_step(vol, rays, model_t.nerf, *args, grad=grad,
                                        generator=torch.Generator().manual_seed(int(op["seed"])))
    assert not calls
    assert bool(torch.isfinite(loss).all()) and float(grad.abs().max()) > 0 and bool(torch.isfinite(grad).all())
    S = pts.shape[1]
    m = pts.shape[0] * S
    zeros = torch.zeros(m, device=DEV)
    with pytest.raises(_lib.BnvError, match="invalid argument"):
        fused(pts, model_t.nerf, None, m, zeros, zeros, torch.ones(1, device=DEV), torch.zeros(2, device=DEV),
              torch.zeros_like(grad))
