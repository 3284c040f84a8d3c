"""The smallest shapes at which the scans shared through csrc/scan.hpp can still go wrong and that no other test pins:
the front end's three-launch scan when its top level (k_scan_top<256>) needs a second round, and the float64 area
prefix of the surface sampler across a tile boundary, bit for bit in the kernel's own summation tree.
(The TSDF mesh's multi-block int64 scan is pinned by tests/test_gpu_tsdf_mesh.py: its 48 x 40 x 71 sphere is 2,130
tiles in three scan blocks, with the surface crossing both block boundaries.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_front_end_scan_top_second_round():
    """520 x 512 pixels = 260 tiles of 1,024: the 256-thread top kernel carries into a second round.  Invalid pixels in
    the first and the last tile.  Compacted rows == the padded call's valid rows == the oracle (test_gpu_parity.py's
    expected values and bars for the front end)."""
    from oracle import bnv_oracle as orc
    from bnv_fusion_amd import synthetic
    from bnv_fusion_amd.frontend import depth_to_input_pts
    H, W = 520, 512
    mm = synthetic.depth_u16(5, H, W)
    idx = np.arange(H * W).reshape(H, W)
    mm[idx % 7 == 3] = 0                 # holes in every tile
    mm[0, :9] = 0                        # the first tile
    mm[-1, -11:] = 12000                 # the last tile: beyond max_depth
    mm[200:203, :] = 0                   # a tile is two rows: tile 100 holds no valid pixel, tile 101 half of its own
    intr, T = synthetic.intrinsics(H, W), synthetic.pose(5)
    ref = orc.depth_to_input_pts(mm.astype(np.float64) / 1000.0, intr, T, max_depth=10.0).astype(np.float32)
    src = torch.from_numpy(mm).to(DEV)
    got = depth_to_input_pts(src, intr, T, max_depth=10.0)[0]
    full, n = depth_to_input_pts(src, intr, T, max_depth=10.0, compact=False)
    n_valid = int(((mm > 0) & (mm < 10000)).sum())
    assert int(n) == n_valid == ref.shape[0] == got.shape[0]
    assert torch.equal(full[0, :n_valid].view(torch.int32), got.view(torch.int32))     # same rows, same order, same bits
    assert torch.isnan(full[0, n_valid:]).all()
    g = got.cpu().numpy()
    exact = np.mean(g == ref)
    ulp = np.abs(g.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)).max()
    assert exact > 0.9999 and ulp <= 1, (exact, ulp)


def area_prefix_restated(V, F):
    """k_face_area_prefix's float64 prefix in its own order: 8 faces per thread in sequence, a Hillis-Steele scan over
    the 64 lanes of a wave, the 4 wave totals in wave order, tile after tile; prefix = (excl + wbase) + (incl - acc) +
    run."""
    V = V.astype(np.float32)
    e1 = V[F[:, 1]] - V[F[:, 0]]
    e2 = V[F[:, 2]] - V[F[:, 0]]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    ln = np.sqrt(((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).astype(np.float64)).astype(np.float32)
    af = np.float32(0.5) * ln
    a = np.where((af > 0) & (af <= np.finfo(np.float32).max), af.astype(np.float64), 0.0)
    n = len(F)
    tiles = (n + 2047) // 2048
    a = np.concatenate([a, np.zeros(tiles * 2048 - n)]).reshape(tiles, 256, 8)
    prefix = np.zeros((tiles, 256, 8))
    excl = 0.0
    for t in range(tiles):
        run = np.zeros((256, 8))
        acc = np.zeros(256)
        for e in range(8):
            acc = acc + a[t, :, e]
            run[:, e] = acc
        incl = acc.reshape(4, 64).copy()
        d = 1
        while d < 64:
            nxt = incl.copy()
            nxt[:, d:] = incl[:, d:] + incl[:, :-d]
            incl = nxt
            d *= 2
        wbase, tile_sum = np.zeros(4), 0.0
        for w in range(4):
            wbase[w] = tile_sum
            tile_sum = tile_sum + incl[w, 63]
        pre = (excl + np.repeat(wbase, 64)) + (incl.reshape(256) - acc)
        prefix[t] = pre[:, None] + run
        excl = excl + tile_sum
    return prefix.reshape(-1)[:n]


def test_area_prefix_across_a_tile_bit_for_bit():
    """2,049 faces: one more than a tile of 2,048, so the float64 prefix crosses a tile.  Prefix, total and the sampled
    faces equal the restatement bit for bit."""
    from bnv_fusion_amd import _lib
    lib = _lib.require_device(0)
    rng = np.random.default_rng(5)
    nv, nf, n = 700, 2049, 20000
    V = (rng.uniform(-1, 1, size=(nv, 3)) * np.array([1.0, 3.0, 0.01])).astype(np.float32)   # areas over many binades
    F = rng.integers(0, nv, size=(nf, 3)).astype(np.int32)
    F[100:140] = F[100:140, [0, 0, 1]]          # zero-area faces: a repeated vertex
    F[-1] = [3, 400, 77]                         # the face alone in the second tile has area
    U = rng.random((n, 3)).astype(np.float32)
    want = area_prefix_restated(V, F.astype(np.int64))
    assert want[-1] > want[2047] > 0
    ws_bytes = C.c_int64()
    assert lib.bnv_mesh_sample_surface_workspace(nf, C.byref(ws_bytes)) == 0
    v, f, u = (torch.from_numpy(x).to(DEV) for x in (V, F, U))
    ws = torch.zeros(int(ws_bytes.value), dtype=torch.uint8, device=DEV)
    pts = torch.empty((n, 3), dtype=torch.float32, device=DEV)
    ids = torch.empty(n, dtype=torch.int32, device=DEV)
    _lib.check(lib.bnv_mesh_sample_surface(_lib.ptr(v), nv, _lib.ptr(f), nf, _lib.ptr(u), n, _lib.ptr(ws),
                                           int(ws_bytes.value), _lib.ptr(pts), _lib.ptr(ids), None, _lib.stream_ptr()),
               "bnv_mesh_sample_surface")
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    al = lambda b: (b + 255) // 256 * 256      # noqa: E731
    got = raw[: nf * 8].view(np.float64)
    total = raw[al(nf * 8) + al(2 * 8):][:8].view(np.float64)[0]      # SampleStatus.total behind prefix and 2 tile words
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), int((got != want).sum())
    assert total == want[-1]
    key = U[:, 0].astype(np.float64) * want[-1]
    assert np.array_equal(ids.cpu().numpy(), np.searchsorted(want, key, side="right").astype(np.int32))
