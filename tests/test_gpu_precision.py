"""Every MLP kernel in every arithmetic mode it runs in, against a float64 run of the same network.

The SDF parity tests elsewhere hold decodes to 1e-4 absolute (~2 % of a typical value): a split-f16 kernel that lost
its lo products would pass them.  Here the reference is bnv_oracle fed a float64 checkpoint: voxel ids, masks, local
coordinates, trilinear weights and sin / cos are the fp32 values the kernels pin bit for bit; from the MLP inputs on
everything is float64 (oracle/precision.py).  Units: decoder errors in alpha = SDF / voxel; encoder features relative
to max |feature|; feature gradients per row, relative.

Bars (tests/test_precision_envelope_cpu.py derives the envelope on the CPU: split 1.1e-6 alpha, f16 2.2e-3 alpha):
  * modes 0 / 1 forward <= FWD_BAR = 1e-5 alpha (~9x the emulated split error, ~200x below f16);
  * mode 3 forward inside [1e-4, 1e-2] alpha, and it FAILS the mode-1 bar on the same inputs: the bar can see a
    split kernel that lost its lo products (mode 3 is exactly that arithmetic);
  * encoder modes 0 / 1 <= ENC_BAR = 5e-6 relative (emulated 4.7e-7), mode 3 >= 2e-5;
  * backward (split arithmetic in every mode) <= BWD_BAR = 2e-5 relative per feature row on rows that no query near a
    ReLU kink touches (emulated 2.2e-6); the others <= 1e-3 of the largest gradient (test_gpu_optimize's bar);
  * mask decisions identical everywhere.

Measured on an MI355X (max error; modes 0 / 1 / 3):
  decode_pts (all n)           2.6e-7 / 5.4e-7 / 8.8e-4 alpha
  lattice, lattice_pipe 1      -      / 6.4e-7 / 8.8e-4      lattice_pipe 0: 2.6e-7 / 5.4e-7 / 8.8e-4
  dense corners / nearest      1.5e-7 / 6.0e-7 / 1.1e-3      3.5e-7 / 9.6e-7 / 1.7e-3
  dense global                 3.2e-7 / 1.2e-6 / 1.3e-3
  encoder (points, depth)      1.6e-7 / 3.4e-7 / 4.5e-4 relative
  frame pipe                   mode 1 7.4e-7, mode 3 1.6e-3
  backward, clean rows         4.1e-6 / 3.7e-6 / 3.9e-6 relative (169 of 913 live queries flagged)
  tile geometry (all cases)    <= 6.4e-7 (mode 1)
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, WEIGHTS_FP32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL = 0.02

FWD_BAR = 1e-5                 # alpha, modes 0 / 1
F16_WINDOW = (1e-4, 1e-2)      # alpha, mode 3
ENC_BAR = 5e-6                 # relative to max |feature|, modes 0 / 1
ENC_F16_MIN = 2e-5             # mode 3 encoder: at least this far off
BWD_BAR = 2e-5                 # relative per row, unflagged rows
BWD_FLAGGED_BAR = 1e-3         # relative to the largest gradient (today's bar, test_gpu_optimize.py)
KINK_DELTA = 4e-6              # |hidden pre-activation| below which a split forward may flip the ReLU mask: 4x the
                               # largest split pre-activation error of the CPU emulation (1.0e-6)
MIN_LIVE_FOR_F16 = 64          # fewer live values: the f16 window is not asserted (one value can land anywhere)


# ---------------------------------------------------------------------------------------------------------------
# fixtures and helpers
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bnv():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    import bnv_fusion_amd
    bnv_fusion_amd.set_mlp_mode(1)
    yield bnv_fusion_amd
    bnv_fusion_amd.set_mlp_mode(1)


@pytest.fixture(scope="module")
def model(bnv):
    m = bnv.load_pretrained(device=DEV, voxel_size=VOXEL)
    yield m
    m.set_mlp_mode(None)


@pytest.fixture(scope="module")
def orc():
    from oracle import bnv_oracle
    return bnv_oracle


@pytest.fixture(scope="module")
def P():
    from oracle import precision
    return precision


@pytest.fixture(scope="module")
def sd(orc):
    return orc.load_weights(WEIGHTS_FP32)


@pytest.fixture(scope="module")
def sd64(P, sd):
    return P.state_dict_f64(sd)


@pytest.fixture(scope="module")
def golden(bnv):
    z = np.load(os.path.join(GOLDEN, "sequence_64.npz"))
    vol = bnv.SparseVolume(8, float(z["voxel_size"]), z["dims"], 8, device=DEV)
    n = len(z["keys_sorted"])
    vol.insert(torch.from_numpy(z["keys_sorted"]).to(DEV), torch.from_numpy(z["features_sorted"]).to(DEV),
               torch.from_numpy(z["weights_sorted"]).to(DEV), torch.zeros(n, 1, device=DEV))
    vol.to_tensor()
    return vol


def _oracle64(orc, vol, dims):
    """Float64 oracle volume holding exactly the rows of the HIP volume's to_tensor() snapshot, in its order."""
    o = orc.OracleSparseVolume(8, vol.voxel_size, dims, vol.min_pts_in_grid, dtype=torch.float64)
    o.insert(vol.active_coordinates.cpu(), vol.features.detach().cpu().double(), vol.weights.cpu().double(),
             vol.num_hits.cpu().double())
    o.to_tensor()
    return o


@pytest.fixture(scope="module")
def golden64(orc, golden):
    z = np.load(os.path.join(GOLDEN, "sequence_64.npz"))
    return _oracle64(orc, golden, z["dims"])


class Modes:
    """Pins the model to an arithmetic mode for a block; restores the package default after."""

    def __init__(self, model):
        self.model = model

    def __call__(self, mode):
        self.model.set_mlp_mode(mode)
        return self

    def __enter__(self):
        return self.model

    def __exit__(self, *exc):
        self.model.set_mlp_mode(None)


def _alpha_err(got, ref, voxel=VOXEL):
    got = got.detach().cpu().double().reshape(-1)
    ref = ref.detach().cpu().double().reshape(-1)
    return float((got - ref).abs().max()) / voxel if got.numel() else 0.0


def _check_modes(errs, n_live, what):
    """errs {mode: alpha error}: the fp32-class modes under the bar, mode 3 inside its window and above the bar."""
    for m in (0, 1):
        if m in errs:
            assert errs[m] <= FWD_BAR, (what, m, errs)
    if 3 in errs and n_live >= MIN_LIVE_FOR_F16:
        assert errs[3] > FWD_BAR, (what, "mode 3 passes the mode-1 bar: the bar cannot see lost lo products", errs)
        assert F16_WINDOW[0] <= errs[3] <= F16_WINDOW[1], (what, errs)


def _same_mask(got, ref, voxel=VOXEL):
    return torch.equal(got.detach().cpu().reshape(-1) == np.float32(voxel), ref.detach().cpu().reshape(-1) == voxel)


# ---------------------------------------------------------------------------------------------------------------
# k_decode_pts
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 127, 128, 129, 4097])
def test_decode_pts_vs_float64(bnv, model, golden, golden64, sd64, n):
    """k_decode_pts at sizes around its 16-query tile and 128-query chunk; mixed, live and all-masked queries;
    voxel and world coordinates, with and without sdf_delta; modes 0, 1, 3."""
    vol, ovol = golden, golden64
    dec = np.load(os.path.join(GOLDEN, "decode_64.npz"))
    delta = torch.from_numpy(dec["sdf_delta"])
    g = torch.Generator().manual_seed(1000 + n)
    valid = vol.active_coordinates.cpu()[(vol.weights[:, 0] >= 8).cpu()]
    errs, n_live = {0: 0.0, 1: 0.0, 3: 0.0}, 0
    for kind in ("mixed", "live", "masked"):
        if kind == "masked":
            q = torch.rand(1, n, 1, 3, generator=g) * 3 + 1.0
        else:
            base = valid[torch.randint(len(valid), (n,), generator=g)].float()
            spread = 1.6 if kind == "mixed" else 0.0
            q = (base + (torch.rand(n, 3, generator=g) - 0.5) * spread).reshape(1, n, 1, 3)
        qw = q * vol.voxel_size + ovol.min_coords
        for coords, is_coords, d in ((q, True, None), (qw, False, delta), (q, True, delta), (qw, False, None)):
            ref = ovol.decode_pts(coords, sd64, d, is_coords=is_coords, query_tensor=True)
            assert ref.dtype == torch.float64
            live = ref.reshape(-1) != vol.voxel_size if d is None else None
            if d is None:
                n_live += int(live.sum())
            for m in (0, 1, 3):
                with Modes(model)(m):
                    out = vol.decode_pts(coords.to(DEV), model.nerf, None if d is None else d.to(DEV),
                                         is_coords=is_coords, query_tensor=True)
                errs[m] = max(errs[m], _alpha_err(out, ref))
                if d is None:
                    assert _same_mask(out, ref), (kind, m, is_coords)
            if kind == "masked" and d is None:
                assert not bool(live.any())
    _check_modes(errs, n_live, f"decode_pts n={n}")
    print(f"decode_pts n={n}: alpha err {errs}, live values {n_live}")


# ---------------------------------------------------------------------------------------------------------------
# decode_lattice: k_lattice_table_x (lattice_pipe 1) and k_decode<LATTICE> (lattice_pipe 0), then the blend
# ---------------------------------------------------------------------------------------------------------------
def test_decode_lattice_vs_float64(bnv, model, golden, golden64, sd64, orc):
    """All 1,577 voxels of the golden volume (and 300 repeated: 5,131 origins, ~34 tiles of 128) through both lattice
    kernels, with and without sdf_delta, against the float64 8-corner decode of their 3x3x3 lattices."""
    from bnv_fusion_amd import _lib
    lib = _lib.load()
    vol, ovol = golden, golden64
    dec = np.load(os.path.join(GOLDEN, "decode_64.npz"))
    delta = torch.from_numpy(dec["sdf_delta"])
    o = vol.active_coordinates
    o = torch.cat([o, o[:300]]).contiguous()
    lat = orc.lattice_coords(o.cpu().numpy())
    ref = ovol.decode_pts(lat, sd64, None, is_coords=True, query_tensor=True)[0, :, :, 0]
    ref_d = ovol.decode_pts(lat, sd64, delta, is_coords=True, query_tensor=True)[0, :, :, 0]
    n_live = int((ref != vol.voxel_size).sum())
    assert n_live > 1000
    errs = {}
    try:
        for pipe, modes in ((1, (1, 3)), (0, (0, 1, 3))):
            assert lib.bnv_set_option(b"lattice_pipe", pipe) == 0
            e = {}
            for m in modes:
                with Modes(model)(m):
                    out = vol.decode_lattice(o, model.nerf, None, query_tensor=True)
                    out_d = vol.decode_lattice(o, model.nerf, delta.to(DEV), query_tensor=True)
                assert _same_mask(out, ref), (pipe, m)
                e[m] = max(_alpha_err(out, ref), _alpha_err(out_d, ref_d))
            _check_modes(e, n_live, f"lattice pipe={pipe}")
            errs[pipe] = e
    finally:
        lib.bnv_set_option(b"lattice_pipe", 1)
    print(f"decode_lattice: alpha err by lattice_pipe {errs}, live values {n_live}")


# ---------------------------------------------------------------------------------------------------------------
# dense decode, the three branches of decode_feature_grid_w_pts
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", ["corners", "nearest", "global"])
def test_dense_decode_vs_float64(bnv, model, orc, sd64, branch):
    """k_decode<DENSE> (8 corners) and k_decode<DENSE1> (nearest, global) on the encoder's fp32 feature grids: the
    float64 reference samples the same grids (nearest / trilinear in fp32) and runs the MLP in float64.  The global
    branch returns the unscaled prediction: its error is alpha itself."""
    z0 = np.load(os.path.join(GOLDEN, "dense_decode_64.npz"))
    zq = np.load(os.path.join(GOLDEN, "dense_modes_64.npz"))
    voxel = float(z0["voxel_size"])
    vol = bnv.SparseVolume(8, voxel, z0["dims"], 8, device=DEV)
    with Modes(model)(1):
        fg, mask, _, _ = model.encode_pointcloud(torch.from_numpy(z0["input_pts"]).to(DEV), vol.n_xyz, vol.min_coords,
                                                 vol.max_coords, voxel, return_dense=True)
    q = torch.from_numpy(z0["queries"] if branch == "corners" else zq["queries"])
    kw = dict(global_coords=branch == "global", interpolate_decode=branch != "nearest")
    ref, _ = orc.decode_feature_grid_w_pts(sd64, q, fg.cpu(), mask.cpu(), voxel, **kw)
    assert ref.dtype == torch.float64
    n_live = int((ref != voxel).sum())
    errs = {}
    for m in (0, 1, 3):
        with Modes(model)(m):
            try:
                model.interpolate_decode = branch != "nearest"
                out, _ = model.decode_feature_grid_w_pts(q.to(DEV), fg, mask, voxel, vol.min_coords,
                                                         global_coords=branch == "global")
            finally:
                model.interpolate_decode = True
        assert _same_mask(out, ref, voxel), m
        errs[m] = _alpha_err(out, ref, 1.0 if branch == "global" else voxel)
    _check_modes(errs, n_live, f"dense {branch}")
    print(f"dense {branch}: alpha err {errs}, live values {n_live}")


# ---------------------------------------------------------------------------------------------------------------
# encoder: k_pointnet_scatter (mode 0), k_pointnet_scatter_x (modes 1, 3)
# ---------------------------------------------------------------------------------------------------------------
def _enc_errs(model, sd64, orc, run, pts_cpu, n_xyz, mn, mx, voxel):
    ref, rc, rids, _, _ = orc.encode_pointcloud(sd64, pts_cpu, n_xyz, mn, mx, voxel)
    assert ref.dtype == torch.float64
    scale = float(ref.abs().max())
    errs = {}
    for m in (0, 1, 3):
        with Modes(model)(m):
            f, c, ids = run()
        assert torch.equal(ids.cpu(), rids) and torch.equal(c.reshape(-1).cpu(), rc.reshape(-1)), m
        errs[m] = float((f.cpu().double() - ref).abs().max()) / scale
    assert errs[0] <= ENC_BAR and errs[1] <= ENC_BAR, errs
    assert errs[3] > ENC_BAR and errs[3] >= ENC_F16_MIN, errs
    return errs


@pytest.mark.parametrize("name", ["encode_64", "encode_128"])
def test_encode_pointcloud_vs_float64(bnv, model, orc, sd64, name):
    """encode_pointcloud's features (PointNet per point, scatter mean per voxel) against the float64 encoder with a
    float64 scatter mean; voxel ids and counts identical."""
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    voxel = float(z["voxel_size"])
    vol = bnv.SparseVolume(8, voxel, z["dims"], 8, device=DEV)
    pts = torch.from_numpy(z["input_pts"])

    def run():
        f, c, ids, _, _ = model.encode_pointcloud(pts.to(DEV), vol.n_xyz, vol.min_coords, vol.max_coords, voxel,
                                                  return_dense=False)
        return f, c, ids

    mn, mx, n_xyz = orc.get_world_range(z["dims"], voxel)
    errs = _enc_errs(model, sd64, orc, run, pts, torch.tensor(n_xyz), torch.from_numpy(mn).float(),
                     torch.from_numpy(mx).float(), voxel)
    print(f"encode {name}: relative err {errs}")


def test_encode_depth_vs_float64(bnv, model, orc, sd64):
    """The depth entry (front end fused into the voxelisation, bnv_encode_finish with an image width) against the
    float64 encoder run on the points that front end produced."""
    from bnv_fusion_amd import synthetic
    from bnv_fusion_amd.frontend import depth_to_input_pts
    dims, voxel = synthetic.GRID_DIMS[128]
    vol = bnv.SparseVolume(8, voxel, np.array([dims] * 3), 8, device=DEV)
    depth = torch.from_numpy(synthetic.depth_u16(2, 240, 320)).to(DEV)
    intr, T = synthetic.intrinsics(240, 320), synthetic.pose(2)
    pts = depth_to_input_pts(depth, intr, T, max_depth=3.0)

    def run():
        f, c, ids, _, cnt, _, _ = model.encode_depth_async(depth, intr, T, 3.0, vol.n_xyz, vol.min_coords,
                                                           vol.max_coords, voxel)
        h = cnt.cpu()
        assert int(h[4]) == 0
        n_out = int(h[2])
        return f[:n_out], c[:n_out], ids[:n_out]

    errs = _enc_errs(model, sd64, orc, run, pts.cpu(), vol.n_xyz.cpu(), vol.min_coords.cpu(), vol.max_coords.cpu(),
                     voxel)
    print(f"encode depth: relative err {errs}")


# ---------------------------------------------------------------------------------------------------------------
# the frame pipe's stamped / persistent tables
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 3])
def test_frame_pipe_lattice_vs_float64(bnv, model, orc, sd64, mode):
    """A NeuralMap frame through the frame pipe (the prestamped lattice decode without its blend + a blend on a side
    stream) against a float64 decode of the very volume the frame decoded."""
    from bnv_fusion_amd import synthetic
    dims = np.array([1.24] * 3)
    frames = []
    for t in range(3):
        p = torch.from_numpy(synthetic.frame(t, H=120, W=160))
        p[..., :3] *= 0.3
        frames.append(p.to(DEV))
    with Modes(model)(mode) as m:
        nm = bnv.NeuralMap(dims, VOXEL, m, device=DEV)
        for k in range(10):
            coords, sdf = nm.fuse_and_decode_async({"input_pts": frames[k % 3]}).result()
        torch.cuda.synchronize()
    nm.volume.to_tensor()
    ovol = _oracle64(orc, nm.volume, dims)
    ref = ovol.decode_pts(orc.lattice_coords(coords.cpu().numpy()), sd64, None, is_coords=True, query_tensor=True)
    ref = ref[0, :, :, 0]
    n_live = int((ref != VOXEL).sum())
    assert n_live > 1000
    assert _same_mask(sdf, ref)
    err = _alpha_err(sdf, ref)
    if mode == 1:
        assert err <= FWD_BAR, err
    else:
        assert FWD_BAR < err and F16_WINDOW[0] <= err <= F16_WINDOW[1], err
    print(f"frame pipe mode {mode}: alpha err {err:.3e}, live values {n_live}")


# ---------------------------------------------------------------------------------------------------------------
# k_decode_pts_bwd
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_decode_pts_backward_vs_float64(bnv, model, golden, golden64, sd, sd64, orc, P, mode):
    """Feature gradients of k_decode_pts_bwd (split arithmetic whatever the mode: the backward kernel has no other)
    against float64 autograd through the oracle.  Queries whose any hidden pre-activation (float64, any of the 8
    corner evaluations) lies within KINK_DELTA of 0 may flip a ReLU mask: their rows are held to the loose bar."""
    vol = golden
    g = torch.Generator().manual_seed(5)
    valid = vol.active_coordinates.cpu()[(vol.weights[:, 0] >= 8).cpu()]
    n = 4000
    q = (valid[torch.randint(len(valid), (n,), generator=g)].float()
         + (torch.rand(n, 3, generator=g) - 0.5) * 1.6).reshape(1, n, 1, 3)
    gs = torch.rand(n, generator=g) * 2 - 1
    # float64 gradient
    ovol = _oracle64(orc, vol, np.load(os.path.join(GOLDEN, "sequence_64.npz"))["dims"])
    ovol.features.requires_grad_(True)
    out = ovol.decode_pts(q, sd64, None, is_coords=True, query_tensor=True)
    (out.reshape(-1) * gs.double()).sum().backward()
    ref = ovol.features.grad.detach()
    live = out.detach().reshape(-1) != vol.voxel_size
    # ReLU-kink flags: the float64 pre-activations of every corner evaluation of every live query
    nb = orc.get_neighbors(q)[0, :, :, 0]                                    # [8, n, 3] float corners
    local = (q[0, :, 0][None] - nb).reshape(-1, 3)
    rows = torch.tensor(ovol._rows(nb, ovol._tensor_map)).reshape(8, n)
    feats = ovol.features.detach()[rows.clamp(min=0)].reshape(-1, 8)
    pre = []
    P.mlp(P.sdf_layers(sd), P.sdf_inputs(local.numpy(), feats.numpy()), "f64", preacts=pre)
    near = np.zeros(8 * n, bool)
    for z in pre:
        near |= (np.abs(z) < KINK_DELTA).any(1)
    flagged = torch.from_numpy(near.reshape(8, n).any(0)) & live
    assert float(flagged.sum()) <= 0.25 * float(live.sum()), (int(flagged.sum()), int(live.sum()))
    assert int(live.sum()) > 500
    touched_flagged = torch.zeros(len(ref), dtype=torch.bool)
    touched_flagged[rows[:, flagged].reshape(-1).clamp(min=0)] = True
    # GPU gradient
    grad = torch.zeros_like(vol.features)
    with Modes(model)(mode):
        vol.decode_pts_backward(q.to(DEV), model.nerf, gs.to(DEV), grad, is_coords=True)
    got = grad.cpu().double()
    gmax = float(ref.abs().max())
    row_mag = ref.abs().amax(-1).clamp(min=1e-3 * gmax)
    rel = (got - ref).abs().amax(-1) / row_mag
    clean = ~touched_flagged & (ref.abs().amax(-1) > 0)
    assert int(clean.sum()) > 100
    assert float(rel[clean].max()) <= BWD_BAR, float(rel[clean].max())
    assert float((got - ref).abs().max()) <= BWD_FLAGGED_BAR * gmax
    print(f"backward mode {mode}: clean-row rel err {float(rel[clean].max()):.3e} over {int(clean.sum())} rows, "
          f"worst {float((got - ref).abs().max()) / gmax:.3e}; flagged queries {int(flagged.sum())} / {int(live.sum())}")


# ---------------------------------------------------------------------------------------------------------------
# tile geometry of k_lattice_table_x
# ---------------------------------------------------------------------------------------------------------------
_BLOCK = 18                     # live block of 18^3 voxels: up to ~150k table entries (> 2.25 rounds of 256 tiles)


def _table_reference(orc, sd64, vol, origins, min_pts):
    """Float64 lattice decode of ``origins`` [m, 3] on the volume's snapshot rows: the float64 MLP once per (row,
    lattice offset) -- the network input is exactly decode_pts's (fp32 local offset, its sin / cos, the features) --
    then the 8-corner blend of decode_pts in float64 (cross-checked against bnv_oracle.decode_pts by the caller)."""
    keys = vol.active_coordinates.cpu()
    feats = vol.features.detach().cpu()
    wts = vol.weights.cpu()[:, 0]
    n_rows = len(keys)
    offs = torch.tensor([[x, y, z] for x in (-.5, 0, .5) for y in (-.5, 0, .5) for z in (-.5, 0, .5)])
    x = torch.cat([orc.xyz_encoding(offs)[None].expand(n_rows, 27, 9), feats[:, None].expand(n_rows, 27, 8)], -1)
    table = orc.geo_forward(sd64, x)[..., 0] * vol.voxel_size                            # [rows, 27] float64
    dense = torch.full((64, 64, 64), -1, dtype=torch.long)
    dense[keys[:, 0], keys[:, 1], keys[:, 2]] = torch.arange(n_rows)
    pts = orc.lattice_coords(origins.cpu().numpy())[0]                                 # [m, 27, 3] fp32
    corners = orc.get_neighbors(pts[None])[0].long()                                   # [8, m, 27, 3]
    local = pts[None] - corners.float()
    w = torch.prod(1 - local.abs(), -1)
    w = (w / w.sum(0, keepdim=True)).double()
    rows = dense[corners[..., 0], corners[..., 1], corners[..., 2]]
    ok = (rows >= 0) & (wts[rows.clamp(min=0)] >= min_pts)
    li = ((local * 2).round().long() + 1)
    li = li[..., 0] * 9 + li[..., 1] * 3 + li[..., 2]
    val = (table[rows.clamp(min=0), li] * w).sum(0)
    return torch.where(ok.all(0), val, torch.full_like(val, vol.voxel_size))


def test_lattice_table_tile_geometry_vs_float64(bnv, model, orc, sd64):
    """The tile hand-out of k_lattice_table_x (full tiles of 128 evaluations, the half-tile tail when the last round
    holds at most grid / 2 tiles, two static tiles per workgroup then dynamic draws from a counter the last draw
    resets) against float64 at the mode-1 bar.  A synthetic volume (an 18^3 block of live voxels carrying feature
    rows of the golden sequence) is decoded with prefixes of its voxels as origins, plus 2 x CUs dead origins (no
    live lattice point: they keep the launch grid at CUs - reserve_cus without adding work); the prefix length is
    searched so that the device-side evaluation count (last_lattice_evals) lands in each branch.  Every case runs
    with half_tail 1 and 0 and with reserve_cus 0 and CUs / 8; then large -> small -> large on one workspace."""
    from bnv_fusion_amd import _lib
    lib = _lib.load()
    cus = int(lib.bnv_num_compute_units())
    assert cus >= 16
    z = np.load(os.path.join(GOLDEN, "sequence_64.npz"))
    dims = z["dims"]
    live_rows = torch.from_numpy(z["features_sorted"][z["weights_sorted"][:, 0] >= 8])
    r = torch.arange(20, 20 + _BLOCK)
    block = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    g = torch.Generator().manual_seed(11)
    feats = live_rows[torch.randint(len(live_rows), (len(block),), generator=g)]
    vol = bnv.SparseVolume(8, VOXEL, dims, 8, device=DEV)
    vol.insert(block.to(DEV), feats.to(DEV), torch.full((len(block), 1), 10.0, device=DEV),
               torch.zeros(len(block), 1, device=DEV))
    vol.to_tensor()
    i = torch.arange(2 * cus)
    dead = torch.stack([50 + i % 10, 2 + (i // 10) % 60, 2 + i // 600], -1)
    assert int(dead[:, 2].max()) < 62
    ref = _table_reference(orc, sd64, vol, block, 8)
    ovol = _oracle64(orc, vol, dims)
    chk = ovol.decode_pts(orc.lattice_coords(block[:40].numpy()), sd64, None, is_coords=True)[0, :, :, 0]
    assert float((chk - ref[:40]).abs().max()) < 1e-12
    live_all = block.to(DEV)
    dead = dead.to(DEV)

    def decode(m):
        with Modes(model)(1):
            out = vol.decode_lattice(torch.cat([live_all[:m], dead]).contiguous(), model.nerf, None, query_tensor=True)
        return out, int(vol.last_lattice_evals().item())

    def search(target_tiles):
        lo, hi = 1, len(block)
        assert (decode(hi)[1] + 127) // 128 >= target_tiles
        while lo < hi:
            mid = (lo + hi) // 2
            if (decode(mid)[1] + 127) // 128 >= target_tiles:
                hi = mid
            else:
                lo = mid + 1
        return lo

    def check(out, m, what):
        assert _same_mask(out[:m], ref[:m]), what
        assert bool((out[m:] == np.float32(VOXEL)).all()), what
        e = _alpha_err(out[:m], ref[:m])
        assert e <= FWD_BAR, (what, e)
        return e

    cases = [("T < G/2", lambda G: G // 4, lambda T, G: 0 < 2 * T < G),
             ("G/2 < T < G", lambda G: (3 * G) // 4, lambda T, G: G < 2 * T and T < G),
             ("T = G + r, r <= G/2", lambda G: G + G // 4, lambda T, G: T // G == 1 and 0 < 2 * (T % G) <= G),
             ("T = G + r, r > G/2", lambda G: G + (3 * G) // 4, lambda T, G: T // G == 1 and 2 * (T % G) > G),
             ("T >= 2G + r (dynamic)", lambda G: 2 * G + G // 4, lambda T, G: T // G >= 2 and 0 < 2 * (T % G) <= G),
             ("T = k G", lambda G: G, lambda T, G: T % G == 0)]
    record = []
    sizes = {}
    try:
        assert lib.bnv_set_option(b"lattice_pipe", 1) == 0
        for reserve in (0, cus // 8):
            assert lib.bnv_set_option(b"reserve_cus", reserve) == 0
            G = cus - reserve
            for name, target, ok in cases:
                m = search(target(G))
                sizes[(reserve, name)] = m
                for half_tail in (1, 0):
                    assert lib.bnv_set_option(b"half_tail", half_tail) == 0
                    out, E = decode(m)
                    T = (E + 127) // 128
                    assert ok(T, G), (name, reserve, E, T, G)
                    e = check(out, m, (name, reserve, half_tail))
                    record.append((name, G, reserve, half_tail, E, T, e))
                assert lib.bnv_set_option(b"half_tail", 1) == 0
        # large -> small -> large on one workspace: the tile counter must come back reset
        assert lib.bnv_set_option(b"reserve_cus", 0) == 0
        big, small = sizes[(0, cases[4][0])], sizes[(0, cases[0][0])]
        a, _ = decode(big)
        a = a.clone()
        b, _ = decode(small)
        check(b, small, "small after large")
        c, _ = decode(big)
        check(c, big, "large after small")
        assert torch.equal(a, c)
    finally:
        lib.bnv_set_option(b"half_tail", 1)
        lib.bnv_set_option(b"reserve_cus", 0)
        lib.bnv_set_option(b"lattice_pipe", 1)
    for rec in record:
        print("tile geometry %-24s G=%d reserve=%d half_tail=%d evals=%d tiles=%d alpha err %.3e" % rec)
