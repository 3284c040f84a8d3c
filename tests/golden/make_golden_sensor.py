"""Records tests/golden/sensor_60x80.npz: the reference's own depth sensor model (src/utils/geometry.py:
Simulator.simulate) on a small clean depth image, with the normal draws given.

    python tests/golden/make_golden_sensor.py          (needs the reference tree; see ref_shims.py)

``Simulator.__init__`` reads a file that exists on its author's machine only, so the object is made without it and
``model`` set to ones (an undistortion factor of (1 - a) + a).  ``np.random.normal`` is substituted for the run: the
k-th call with the shuffle's sigma returns sigma * draws[pixel k // 2, k % 2], a call with the disparity's sigma
returns sigma * draws[the current pixel, 2] -- the order simulate() makes them in.  Stored: ``clean`` float32 [60, 80]
(metres, with holes), ``draws`` float64 [60, 80, 3] (standard normals), ``depth`` float64 [60, 80] (what simulate()
returned).  tests/test_mesh_ray_cpu.py replays it with tests/mesh_ray_restatement.sensor, bit for bit.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
H, W = 60, 80


def main():
    import ref_shims
    ref_shims.install()
    for name in ("scipy", "scipy.spatial", "scipy.spatial.transform"):
        try:
            __import__(name)
        except ImportError:
            ref_shims._mod(name, Rotation=object)
    from src.utils import geometry

    rng = np.random.default_rng(2024)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    clean = (1.2 + 0.9 * np.sin(c / 11.0) * np.cos(r / 7.0) + 0.02 * rng.standard_normal((H, W))).astype(np.float32)
    clean[(r // 6 + c // 9) % 7 == 0] = 0.0                       # holes, as a scan has
    clean[40:, 60:] = np.float32(7.5)                             # far: a few disparity steps only
    draws = rng.standard_normal((H, W, 3))
    draws[::5, ::7, :2] *= 3.0                                    # some shuffles of more than one pixel, and past the border

    sim = geometry.Simulator.__new__(geometry.Simulator)
    sim.model = np.ones((80, 80, 5))
    state = {"shuffles": 0}

    def normal(loc, scale):
        if scale == 0.25:
            k = state["shuffles"]
            state["shuffles"] += 1
            return loc + scale * draws.reshape(-1, 3)[k // 2, k % 2]
        assert scale == 0.027778
        return loc + scale * draws.reshape(-1, 3)[(state["shuffles"] - 1) // 2, 2]

    real = np.random.normal
    np.random.normal = normal
    try:
        depth = sim.simulate(clean.astype(np.float64))
    finally:
        np.random.normal = real
    assert state["shuffles"] == 2 * H * W
    out = os.path.join(HERE, "sensor_60x80.npz")
    np.savez_compressed(out, clean=clean, draws=draws, depth=np.asarray(depth, np.float64))
    print(out, os.path.getsize(out), "bytes; zeros", int((depth == 0).sum()))


if __name__ == "__main__":
    main()
