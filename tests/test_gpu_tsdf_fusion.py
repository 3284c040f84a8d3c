"""The HIP TSDF fusion kernels (csrc/tsdf.hip: k_tsdf_integrate, k_tsdf_integrate_batch; TSDFVolume._fold_color)
against the oracle's restatement of the reference's inline CUDA kernel (third_parties/fusion.py:68-141), bit for bit:
weight, tsdf and the folded colour volume, over the options of both entries.  The restatement is anchored to the
reference by tests/golden/tsdf_color.npz (tests/test_tsdf_fusion_cpu.py), whose geometry every test here uses: a
15 x 17 x 20 volume (19 blocks of 256 threads and a partial one) with the camera inside it, 24 x 32 frames.

Every operation of the kernel is one correctly rounded fp32 operation (add, mul, IEEE divide, floorf, roundf, fminf;
the library is built with -ffp-contract=off), and numpy float32 performs the same operations one ufunc at a time, so
the bar is equality of bits for all three volumes.  Needs a real MI355X: run with  -m gpu."""
import contextlib
import functools
import os
from unittest import mock

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PASSES = 2          # the golden's six frames, integrated twice in order: weights reach 4 even at obs_weight 0.5
MAX_DEPTH = 0.36    # a sample of the fixture equals it (360 mm): cut, as every sample beyond it


@pytest.fixture(scope="module")
def tsdf_mod():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    from bnv_fusion_amd import tsdf
    return tsdf


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(os.path.join(GOLDEN, "tsdf_color.npz"))
    return {k: z[k] for k in z.files}


def _metres(mm):
    """The uint16 conversion as restated: one correctly rounded float32 division."""
    return mm.astype(np.float32) / np.float32(1000)


def _oracle_fuse(frames, obs_weight, max_depth, half_to_even=False):
    """``frames``: (depth_mm, rgb or None, pose) in order, through the oracle's default (CUDA kernel) flavour ->
    (tsdf, weight, color, stats).  ``half_to_even``: the colour channels rounded like np.round / rintf instead."""
    from oracle import bnv_oracle as orc
    z = _golden()
    dims, vs = z["tsdf"].shape, float(z["voxel_size"])
    tsdf = np.full(dims, -5 * vs, dtype=np.float32)
    weight, color, stats = np.zeros(dims, dtype=np.float32), np.zeros(dims, dtype=np.float32), {}
    with mock.patch.object(orc, "_roundf", np.round) if half_to_even else contextlib.nullcontext():
        for mm, rgb, T in frames:
            orc.tsdf_integrate(tsdf, weight, z["origin"], vs, _metres(mm), z["intr"], T, obs_weight=obs_weight,
                               color=color, color_im=rgb, max_depth=max_depth, stats=stats)
    return tsdf, weight, color, stats


def _frames(n, with_color=True):
    z = _golden()
    k = len(z["poses"])
    return [(z["depths_mm"][t % k], z["colors"][t % k] if with_color else None, z["poses"][t % k]) for t in range(n)]


@functools.lru_cache(maxsize=None)
def _reference(obs_weight, with_color, max_depth):
    """The oracle's volumes for one parametrisation, computed once (read-only), and what the inputs exercise."""
    frames = _frames(PASSES * 6, with_color)
    tsdf, weight, color, stats = _oracle_fuse(frames, obs_weight, max_depth)
    stats["observed"] = int((weight > 0).sum())
    if with_color:
        stats["rounding_sensitive"] = int((_oracle_fuse(frames, obs_weight, max_depth, True)[2] != color).sum())
    for a in (tsdf, weight, color):
        a.setflags(write=False)
    return tsdf, weight, color, stats


def _volume(tsdf_mod):
    z = _golden()
    vol = tsdf_mod.TSDFVolume(z["bounds"].copy(), float(z["voxel_size"]), device=DEV)
    assert tuple(vol.tsdf.shape) == z["tsdf"].shape and np.array_equal(vol._vol_origin, z["origin"])
    return vol


def _host(vol):
    return vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.color.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_bit_equal(vol, ref, what=""):
    """weight, colour and tsdf against the oracle's, as float32 bit patterns (array_equal of the values would let
    -0.0 pass for 0.0)."""
    tsdf, weight, color = _host(vol)
    print(what, "tsdf bits differing:", int((_bits(tsdf) != _bits(ref[0])).sum()),
          "weight:", int((_bits(weight) != _bits(ref[1])).sum()), "colour:", int((_bits(color) != _bits(ref[2])).sum()))
    assert np.array_equal(_bits(weight), _bits(ref[1]))
    assert np.array_equal(_bits(color), _bits(ref[2]))
    assert np.array_equal(_bits(tsdf), _bits(ref[0]))


@pytest.mark.parametrize("max_depth", [None, MAX_DEPTH], ids=["no_cut", "max_depth"])
@pytest.mark.parametrize("with_color", [True, False], ids=["rgb", "no_rgb"])
@pytest.mark.parametrize("obs_weight", [1.0, 0.5, 2.5])
@pytest.mark.parametrize("depth_kind", ["uint16_mm", "float32_m"])
def test_integrate_equals_restated_cuda_kernel(tsdf_mod, depth_kind, obs_weight, with_color, max_depth):
    """TSDFVolume.integrate, frame by frame, against the oracle's default flavour: all three volumes bit-equal after
    the last frame (measured on the MI355X: 0 tsdf bits differ in every parametrisation).

    The test first checks, on counts taken from the oracle, that its inputs exercise what it claims: voxels behind
    the camera, voxels beyond the truncation band, voxels projecting onto zero depth and onto samples ``max_depth``
    cuts, weights of 4 and more, and colour averages ending in .5 in at least a quarter of the observed voxels (so
    rintf for roundf cannot pass).  No voxel has camera z == 0 exactly: the pixel coordinate is then not finite and
    its conversion to an integer is outside what is pinned here."""
    z = _golden()
    ref = _reference(obs_weight, with_color, max_depth)
    stats = ref[3]
    print(depth_kind, obs_weight, with_color, max_depth, stats)
    assert stats["cam_z_zero"] == 0
    assert stats["behind"] > 1000 and stats["truncated"] > 500 and stats["zero_depth"] > 100
    assert stats["observed"] > 800 and float(ref[1].max()) >= 4
    if max_depth is not None:
        assert stats["max_depth"] > 1000 and (z["depths_mm"] == int(round(max_depth * 1000))).any()
        cut = (z["depths_mm"] >= int(round(max_depth * 1000))).mean()
        assert 0.1 < cut < 0.9                                  # a visible share of the pixels, not all of them
    else:
        assert stats["max_depth"] == 0
    if with_color:
        assert stats["rounding_sensitive"] >= 0.25 * stats["observed"]
    vol = _volume(tsdf_mod)
    for mm, rgb, T in _frames(PASSES * 6, with_color):
        depth = mm if depth_kind == "uint16_mm" else _metres(mm)
        vol.integrate(rgb, torch.from_numpy(depth).to(DEV), z["intr"], T, obs_weight=obs_weight, max_depth=max_depth)
    _assert_bit_equal(vol, ref, depth_kind)
    if not with_color:
        assert not _bits(_host(vol)[2]).any()


def _float_frames():
    """Frames whose colour images are float32 and not integers, blue reaching beyond 255: the first frame's blue is
    300 .. 510 everywhere, so the ``min(..., 255)`` of the blue channel binds in every voxel it reaches (red and green
    are 8-bit by construction of the fold, blue is whatever floor(folded / 65536) gives)."""
    z = _golden()
    rng = np.random.default_rng(11)
    frames = []
    for t, (mm, _, T) in enumerate(_frames(6)):
        rgb = rng.uniform(0, 255, size=mm.shape + (3,)).astype(np.float32)
        if t == 0:
            rgb[..., 2] = rng.uniform(300, 510, size=mm.shape).astype(np.float32)
        elif t == 3:
            rgb[4:20, 6:26, 2] += np.float32(256)
        frames.append((mm, rgb, T))
    return frames


def test_float_colour_images_and_the_blue_clamp(tsdf_mod):
    """Non-integer float32 colour through TSDFVolume._fold_color (floor of a float32 sum that is not an integer,
    folded values beyond 2^24) and blue above 255 through the kernel's fminf: bit-equal to the oracle."""
    from oracle import bnv_oracle as orc
    z = _golden()
    frames = _float_frames()
    vol = _volume(tsdf_mod)
    for mm, rgb, _ in frames:
        got = vol._fold_color(torch.from_numpy(rgb)).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(orc.tsdf_fold_color(rgb)))
    assert orc.tsdf_fold_color(frames[0][1]).min() >= 2 ** 24
    first = _oracle_fuse(frames[:1], 2.5, None)
    blue = orc.tsdf_unfold_color(first[2])[0][first[1] > 0]
    assert blue.size > 300 and (blue == 255).all()              # the clamp bound in every voxel of the first frame
    ref = _oracle_fuse(frames, 2.5, None)
    for mm, rgb, T in frames:
        vol.integrate(rgb, torch.from_numpy(mm).to(DEV), z["intr"], T, obs_weight=2.5)
    _assert_bit_equal(vol, ref, "float colour")
    b, g, r = orc.tsdf_unfold_color(_host(vol)[2])
    for ch in (b, g, r):
        assert np.array_equal(ch, np.floor(ch)) and ch.min() >= 0 and ch.max() <= 255


def test_gate_zero_does_nothing_and_gate_one_is_the_ungated_call(tsdf_mod):
    z = _golden()
    frames = _frames(4)
    vols = {name: _volume(tsdf_mod) for name in ("ungated", "open", "shut")}
    gates = {"ungated": None, "open": torch.ones(1, dtype=torch.int32, device=DEV),
             "shut": torch.zeros(1, dtype=torch.int32, device=DEV)}
    for mm, rgb, T in frames[:3]:
        for vol in vols.values():
            vol.integrate(rgb, torch.from_numpy(mm).to(DEV), z["intr"], T, obs_weight=2.5, max_depth=MAX_DEPTH)
    before = _host(vols["shut"])
    mm, rgb, T = frames[3]
    for name, vol in vols.items():
        vol.integrate(rgb, torch.from_numpy(mm).to(DEV), z["intr"], T, obs_weight=2.5, max_depth=MAX_DEPTH,
                      gate=gates[name])
    after = {name: _host(vol) for name, vol in vols.items()}
    for a, b, c in zip(after["shut"], before, after["open"]):
        assert np.array_equal(_bits(a), _bits(b))
        assert not np.array_equal(_bits(a), _bits(c))                     # the fourth frame does change all three
    for a, b in zip(after["open"], after["ungated"]):
        assert np.array_equal(_bits(a), _bits(b))
    ref = _oracle_fuse(frames, 2.5, MAX_DEPTH)
    _assert_bit_equal(vols["open"], ref, "gate open")


def _batch_frames():
    """11 uint16 frames (two launches of the batch kernel), colour missing for frames 0, 4 and 8."""
    return [(mm, None if t % 4 == 0 else rgb, T) for t, (mm, rgb, T) in enumerate(_frames(11))]


def test_integrate_batch_equals_restated_cuda_kernel(tsdf_mod):
    """TSDFVolume.integrate_batch against the oracle frame by frame (not against ``integrate``): 11 frames, which is
    two launches, obs_weight 2.5, max_depth set, colour present for some frames only."""
    z = _golden()
    frames = _batch_frames()
    assert len(frames) > tsdf_mod.TSDFVolume.BATCH_MAX and any(f[1] is None for f in frames[:8])
    ref = _oracle_fuse(frames, 2.5, MAX_DEPTH)
    assert ref[3]["max_depth"] > 1000 and ref[3]["behind"] > 1000 and float(ref[1].max()) >= 4 * 2.5
    vol = _volume(tsdf_mod)
    vol.integrate_batch([torch.from_numpy(f[0]).to(DEV) for f in frames], [z["intr"]] * len(frames),
                        [f[2] for f in frames], obs_weight=2.5, max_depth=MAX_DEPTH, color_ims=[f[1] for f in frames])
    _assert_bit_equal(vol, ref, "batch")
    # without any colour image the colour volume is not touched
    vol = _volume(tsdf_mod)
    vol.integrate_batch([torch.from_numpy(f[0]).to(DEV) for f in frames], [z["intr"]] * len(frames),
                        [f[2] for f in frames], obs_weight=2.5, max_depth=MAX_DEPTH)
    _assert_bit_equal(vol, _oracle_fuse([(f[0], None, f[2]) for f in frames], 2.5, MAX_DEPTH), "batch, no colour")


def test_two_identical_runs_give_identical_bits(tsdf_mod):
    z = _golden()
    frames = _batch_frames()
    runs = []
    for _ in range(2):
        one, many = _volume(tsdf_mod), _volume(tsdf_mod)
        for mm, rgb, T in frames:
            one.integrate(rgb, torch.from_numpy(mm).to(DEV), z["intr"], T, obs_weight=0.5, max_depth=MAX_DEPTH)
        many.integrate_batch([torch.from_numpy(f[0]).to(DEV) for f in frames], [z["intr"]] * len(frames),
                             [f[2] for f in frames], obs_weight=0.5, max_depth=MAX_DEPTH,
                             color_ims=[f[1] for f in frames])
        runs.append(_host(one) + _host(many))
    for a, b in zip(*runs):
        assert np.array_equal(_bits(a), _bits(b))
    assert (runs[0][1] > 0).sum() > 800 and runs[0][2].max() > 65536
