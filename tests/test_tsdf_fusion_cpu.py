"""Pins the oracle's restatement of TSDFVolume.integrate -- weight, tsdf and the folded colour volume -- to
tests/golden/tsdf_color.npz, captured from the reference's own CPU fallback (tests/golden/make_golden_tsdf.py), and
checks that the fixture separates the fallback's half-to-even colour rounding from the CUDA kernel's ``roundf``.
CPU only; tests/test_gpu_tsdf_fusion.py holds the HIP kernels to the same restatement."""
import os

import numpy as np
import pytest

from oracle import bnv_oracle as orc
from conftest import GOLDEN


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "tsdf_color.npz"))


def _fuse(z, cpu_path):
    dims, vs = z["tsdf"].shape, float(z["voxel_size"])
    tsdf = np.full(dims, -5 * vs, dtype=np.float32)
    weight, color = np.zeros(dims, dtype=np.float32), np.zeros(dims, dtype=np.float32)
    for mm, rgb, T in zip(z["depths_mm"], z["colors"], z["poses"]):
        depth = mm.astype(np.float32) / np.float32(1000)
        orc.tsdf_integrate(tsdf, weight, z["origin"], vs, depth, z["intr"], T, obs_weight=float(z["obs_weight"]),
                           cpu_path=cpu_path, color=color, color_im=rgb)
    return tsdf, weight, color


@pytest.fixture(scope="module")
def fused(z):
    return {cpu_path: _fuse(z, cpu_path) for cpu_path in (True, False)}


def _channels_are_bytes(color):
    """Every unfolded channel is an integer in [0, 255] and the three refold to the stored value."""
    b, g, r = orc.tsdf_unfold_color(color)
    for ch in (b, g, r):
        assert np.array_equal(ch, np.floor(ch)) and ch.min() >= 0 and ch.max() <= 255
    assert np.array_equal(color.astype(np.float64), b.astype(np.float64) * 65536 + g.astype(np.float64) * 256 + r)


def test_fixture_is_what_the_tests_assume(z):
    assert z["tsdf"].shape == (15, 17, 20) and z["depths_mm"].shape == (6, 24, 32)
    assert z["depths_mm"].dtype == np.uint16 and z["colors"].dtype == np.uint8
    assert float(z["obs_weight"]) == 2.5 and z["color"].dtype == np.float32
    assert (z["depths_mm"] == 0).any(axis=(1, 2)).all()                 # the invalid patch of every frame
    centre = z["poses"][:, :3, 3]
    assert ((centre > z["bounds"][:, 0]) & (centre < z["bounds"][:, 1])).all()      # the camera is inside the volume
    assert int((z["weight"] > 0).sum()) > 1000 and float(z["weight"].max()) >= 4 * 2.5
    _channels_are_bytes(z["color"])


def test_cpu_flavour_reproduces_the_reference_fallback(z, fused):
    tsdf, weight, color = fused[True]
    assert np.array_equal(weight, z["weight"])
    assert np.array_equal(color, z["color"])
    assert np.abs(tsdf - z["tsdf"]).max() <= 1e-6
    assert not ((color != 0) & (weight == 0)).any()
    _channels_are_bytes(color)


def test_cuda_flavour_differs_from_the_fallback_only_by_colour_rounding(z, fused):
    """The default flavour fuses the same voxels (no projection of this fixture ties between two pixels), so weight
    and tsdf agree with the fallback's; its ``roundf`` moves the colour of a large share of the observed voxels --
    the share that lets the GPU test tell ``roundf`` from ``rint``."""
    tsdf, weight, color = fused[False]
    assert np.array_equal(weight, z["weight"])
    assert np.abs(tsdf - z["tsdf"]).max() <= 1e-6
    observed = z["weight"] > 0
    differs = color != z["color"]
    print("observed voxels", int(observed.sum()), "colour differs in", int(differs.sum()))
    assert not differs[~observed].any()
    assert differs.sum() >= 0.25 * observed.sum()
    # half away from zero never lands below half to even, and every later operation is monotone in the old channel
    got, ref = orc.tsdf_unfold_color(color), orc.tsdf_unfold_color(z["color"])
    for a, b in zip(got, ref):
        assert (a >= b).all()
    _channels_are_bytes(color)


def test_colour_is_left_alone_without_an_image(z):
    dims, vs = z["tsdf"].shape, float(z["voxel_size"])
    for cpu_path in (True, False):
        base = [np.full(dims, -5 * vs, dtype=np.float32), np.zeros(dims, dtype=np.float32)]
        with_col = [a.copy() for a in base]
        color = np.full(dims, 7.0, dtype=np.float32)
        depth = z["depths_mm"][0].astype(np.float32) / np.float32(1000)
        orc.tsdf_integrate(*base, z["origin"], vs, depth, z["intr"], z["poses"][0], cpu_path=cpu_path)
        orc.tsdf_integrate(*with_col, z["origin"], vs, depth, z["intr"], z["poses"][0], cpu_path=cpu_path,
                           color=color, color_im=None)
        assert np.array_equal(base[0], with_col[0]) and np.array_equal(base[1], with_col[1])
        assert (color == 7.0).all()


@pytest.mark.parametrize("cpu_path", [True, False])
def test_max_depth_zeroes_samples_at_or_beyond_it(z, cpu_path):
    """``max_depth`` is the loader's mask (depth * (depth < max_depth)): the same volumes as integrating the image
    masked by hand, with the sample equal to the bound cut as well."""
    dims, vs = z["tsdf"].shape, float(z["voxel_size"])
    depth = z["depths_mm"][2].astype(np.float32) / np.float32(1000)
    bound = float(np.float32(0.36))
    assert (z["depths_mm"][2] == 360).any() and (depth > bound).any() and ((depth > 0) & (depth < bound)).any()
    res = []
    for d, md in ((depth, bound), (np.where(depth >= np.float32(bound), np.float32(0), depth), None)):
        vols = [np.full(dims, -5 * vs, dtype=np.float32), np.zeros(dims, dtype=np.float32)]
        color = np.zeros(dims, dtype=np.float32)
        orc.tsdf_integrate(*vols, z["origin"], vs, d, z["intr"], z["poses"][2], obs_weight=2.5, cpu_path=cpu_path,
                           color=color, color_im=z["colors"][2], max_depth=md)
        res.append(vols + [color])
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    assert (res[0][1] > 0).sum() > 50


def test_fold_colour_formula():
    """TSDFVolume._fold_color's expression, floor(b * 65536 + g * 256 + r) in float32 left to right, against the
    oracle's fold of fusion.py:222-223: integer images, and float images whose folded value is not an integer before
    the floor."""
    f = np.float32
    rng = np.random.default_rng(5)

    def fold(c):
        c = np.asarray(c).astype(f)
        return np.floor(c[..., 2] * f(256 * 256) + c[..., 1] * f(256) + c[..., 0])

    u8 = rng.integers(0, 256, size=(24, 32, 3), dtype=np.uint8)
    u8[0, 0], u8[0, 1], u8[0, 2] = (255, 255, 255), (0, 0, 0), (255, 0, 1)
    got = orc.tsdf_fold_color(u8)
    assert got.dtype == f and np.array_equal(got, fold(u8))
    exact = u8[..., 2].astype(np.int64) * 65536 + u8[..., 1].astype(np.int64) * 256 + u8[..., 0]
    assert np.array_equal(got.astype(np.int64), exact)
    b, g, r = orc.tsdf_unfold_color(got)
    assert np.array_equal(np.stack([r, g, b], -1), u8.astype(f))
    fl = rng.uniform(0, 255, size=(24, 32, 3))
    fl[0, 0], fl[0, 1] = (255.0, 255.0, 255.0), (0.25, 0.5, 0.75)
    for img in (fl, fl.astype(f)):
        got = orc.tsdf_fold_color(img)
        assert got.dtype == f and np.array_equal(got, fold(img))
        assert np.array_equal(got, np.floor(got)) and got.max() < 2 ** 24
