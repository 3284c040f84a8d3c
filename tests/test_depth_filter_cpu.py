"""The depth filter without a GPU: bnv_depth_filter's argument validation, the properties of its numpy restatement
(tests/depth_filter_restatement.py, which tests/test_gpu_depth_filter.py holds the kernel to bit for bit), and the
reason the filter exists: the front end's Sobel normals of a disparity-quantised depth image."""
import ctypes as C

import numpy as np
import pytest

import depth_filter_restatement as dfr

INVALID = -1
SIGMA = dfr.DEFAULT_SIGMA_DEPTH


def test_argument_validation_without_a_gpu():
    """Every invalid call is refused before any HIP call, so this runs on the CPU."""
    from bnv_fusion_amd import _lib
    lib = _lib.load()
    depth, out, conf = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28)
    nan, inf = float("nan"), float("inf")

    def call(depth=depth, dtype=0, H=48, W=64, max_depth=3.0, radius=3, sigma=SIGMA, cut=3.0, conf=None, level=0,
             out=out):
        return lib.bnv_depth_filter(depth, dtype, H, W, max_depth, radius, sigma, cut, conf, level, out, None)

    assert call(depth=None) == INVALID
    assert call(out=None) == INVALID
    assert call(out=depth) == INVALID                                   # in place
    assert call(out=C.c_void_p((1 << 20) + 48 * 64 * 2 - 4)) == INVALID   # overlapping the image's last bytes
    assert call(dtype=1, out=C.c_void_p((1 << 20) - 48 * 64 * 4 + 4)) == INVALID
    for H, W in ((0, 64), (48, 0), (-1, 64), (48, -5)):
        assert call(H=H, W=W) == INVALID
    for dtype in (-1, 3):
        assert call(dtype=dtype) == INVALID
    for radius in (0, -1, 9, 100):
        assert call(radius=radius) == INVALID
    for bad in (0.0, -1.0, nan, inf, -inf):
        assert call(sigma=bad) == INVALID
        assert call(cut=bad) == INVALID
        assert call(max_depth=bad) == INVALID
    assert call(conf=None, level=1) == INVALID                          # a level without a map
    assert call(conf=conf, level=-1) == INVALID


def test_isolated_pixel_returns_itself_and_invalid_pixels_zero():
    d = np.zeros((9, 11), np.float32)
    d[4, 5] = np.float32(1.2345)
    for radius in (1, 3, 8):
        out = dfr.filter_depth(d, radius=radius)
        assert out.dtype == np.float32 and out.shape == d.shape
        assert out[4, 5] == d[4, 5]
        out[4, 5] = 0
        assert not out.any()
    u = np.zeros((5, 4), np.uint16)
    u[0, 0] = 1999                                                      # a corner: most of its window is outside
    assert dfr.filter_depth(u)[0, 0] == np.float32(1999 / 1000.0)


def test_bad_pixels_are_neither_output_nor_taps():
    """NaN, inf, negative and >= max_depth pixels give 0 and change no neighbour: the result equals that of the image
    with those pixels set to 0, bit for bit."""
    rng = np.random.default_rng(0)
    base = (1.0 + 0.002 * rng.standard_normal((12, 14))).astype(np.float32)
    bad = base.copy()
    spots = {(2, 3): np.nan, (5, 5): np.inf, (6, 9): -np.inf, (8, 2): 3.0, (9, 9): 7.5, (3, 10): -0.5}
    zeroed = base.copy()
    for (y, x), v in spots.items():
        bad[y, x] = v
        zeroed[y, x] = 0.0
    got, ref = dfr.filter_depth(bad, max_depth=3.0), dfr.filter_depth(zeroed, max_depth=3.0)
    assert got.tobytes() == ref.tobytes()
    assert np.isfinite(got).all()
    for y, x in spots:
        assert got[y, x] == 0.0
    assert (got[zeroed > 0] > 0).all()
    # a confidence gate does the same
    conf = np.full(base.shape, 2, np.uint8)
    for y, x in spots:
        conf[y, x] = 1
    assert dfr.filter_depth(base, conf=conf, conf_level=2).tobytes() == ref.tobytes()
    assert dfr.filter_depth(base, conf=conf, conf_level=1).tobytes() == dfr.filter_depth(base).tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_depth_step_is_kept(dtype):
    """1.0 m | 1.125 m at radius 3: the range kernel's cut (3 x 7.1 mm x z^2) is far below the 125 mm step, so no
    value lies strictly between the levels and every value is within 1e-6 m of its own side."""
    d = np.full((16, 20), 1.0, np.float64)
    d[:, 10:] = 1.125
    img = np.rint(d * 1000).astype(np.uint16) if dtype == np.uint16 else d.astype(np.float32)
    out = dfr.filter_depth(img, radius=3).astype(np.float64)
    assert not ((out > 1.0) & (out < 1.125)).any()
    assert np.abs(out - d).max() <= 1e-6


def test_smooths_within_the_range_cut_only():
    """A one-disparity-step staircase at 1 m (3.6 mm) is smoothed; the output stays inside the input's range."""
    step = 1.0 / (8 * 35.130)
    d = (1.0 + step * (np.arange(24) // 6))[None, :].repeat(10, 0).astype(np.float32)
    out = dfr.filter_depth(d, radius=3)
    assert out.min() >= d.min() and out.max() <= d.max()
    assert np.abs(np.diff(out[5].astype(np.float64))).max() < 0.5 * step


def test_normals_of_a_sensor_frame_improve_by_half():
    """Sweep frame 250 of the half-scale room at 480 x 640 through the restated Kinect model (seed 0): mean angle
    between the front end's Sobel normals and those of the clean depth, over pixels whose 7 x 7 clean neighbourhood
    lies within 3 cm.  Measured 22.1 degrees raw and 6.3 degrees after the filter at its defaults; the bar is half."""
    clean, mm, K = dfr.room_frame(250, 480, 640)
    raw = dfr.mean_normal_error_deg(mm, clean, K)
    filtered = dfr.mean_normal_error_deg(dfr.filter_depth(mm), clean, K)
    print(f"mean normal error: raw {raw:.2f} deg, filtered {filtered:.2f} deg")
    assert filtered <= 0.5 * raw
