"""The cloud-registration entries (include/bnv_fusion.h, "Cloud registration") refuse bad arguments before any HIP
call: no GPU needed."""
import ctypes as C

import numpy as np

INVALID, TOO_SMALL = -1, -2
P8 = C.c_void_p(8)                                         # a non-null pointer no refused call dereferences


def lib():
    from bnv_fusion_amd import _lib
    return _lib.load()


def levels(rows):
    a = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))
    return len(a), a.ctypes.data_as(C.POINTER(C.c_int32)), a


def index_bytes(n):
    b = C.c_int64(-1)
    rc = lib().bnv_cloud_index_bytes(n, C.byref(b))
    return rc, int(b.value)


def test_index_entries_refuse_bad_arguments():
    L = lib()
    rc, one = index_bytes(1)
    assert rc == 0 and one > 0 and one % 256 == 0
    rc, many = index_bytes(3000)
    assert rc == 0 and many > one + 3000 * (24 + 2 * (8 + 16))          # positions, normals, two grids of float4
    assert index_bytes(3000) == (0, many)                               # a function of the count alone
    for n in (0, -1, 2 ** 31 - 2, 2 ** 40):
        assert index_bytes(n)[0] == INVALID, n
    assert L.bnv_cloud_index_bytes(10, None) == INVALID
    for args in ((None, 10, P8, many), (P8, 10, None, many), (P8, 0, P8, many), (P8, -3, P8, many),
                 (P8, 2 ** 31 - 2, P8, 1 << 40)):
        assert L.bnv_cloud_index_build(*args, None) == INVALID, args
    assert L.bnv_cloud_index_build(P8, 3000, P8, many - 1, None) == TOO_SMALL
    assert L.bnv_cloud_index_build(P8, 3000, P8, 0, None) == TOO_SMALL
    for args in ((None, many, P8, 5, P8, P8), (P8, many, None, 5, P8, P8), (P8, many, P8, 5, None, P8),
                 (P8, many, P8, 5, P8, None), (P8, many, P8, 0, P8, P8), (P8, many, P8, 2 ** 31, P8, P8),
                 (P8, one - 1, P8, 5, P8, P8), (P8, 0, P8, 5, P8, P8)):        # bytes no index fits into
        assert L.bnv_cloud_index_nearest(*args, None) == INVALID, args


def test_register_entry_refuses_bad_arguments():
    L = lib()
    n, p, keep = levels([(4, 10), (2, 6), (1, 4)])
    assert int(L.bnv_cloud_register_bytes(n, p)) == int(L.bnv_mesh_register_bytes(n, p)) == (256 * 29 + 20 * 36) * 8
    assert int(L.bnv_cloud_register_bytes(n, None)) == 0
    for bad in ([(1, 1)] * 9, [(0, 3)], [(2, -1)], [(1, 0)]):
        nb, pb, kb = levels(bad)
        assert int(L.bnv_cloud_register_bytes(nb, pb)) == 0, bad
    eye = np.eye(4).reshape(-1)
    one = index_bytes(1)[1]

    def dp(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a.ctypes.data_as(C.POINTER(C.c_double)), a

    def call(**over):
        a = dict(index=P8, index_bytes=1 << 30, points=P8, n=1000, normals=None, T0=eye,
                 levels=[(4, 10), (2, 6), (1, 4)], dist=[0.2, 0.05, 0.02], cos=0.0, oriented=0, share=0.05,
                 spread=1e-3, max_w=0.1, max_v=0.2, ws=P8, ws_bytes=1 << 20, pose=P8, poses=None, stats=P8, status=P8)
        a.update(over)
        nl, pl, kl = levels(a["levels"])
        T0 = None if a["T0"] is None else dp(a["T0"])
        dist = None if a["dist"] is None else dp(a["dist"])
        return L.bnv_cloud_register(a["index"], a["index_bytes"], a["points"], a["n"], a["normals"], T0 and T0[0], nl,
                                    pl, dist and dist[0], a["cos"], a["oriented"], a["share"], a["spread"], a["max_w"],
                                    a["max_v"], a["ws"], a["ws_bytes"], a["pose"], a["poses"], a["stats"], a["status"],
                                    None, None, None)

    nan_T = eye.copy()
    nan_T[3] = np.nan
    for over in (dict(index=None), dict(points=None), dict(T0=None), dict(dist=None), dict(ws=None), dict(pose=None),
                 dict(stats=None), dict(status=None), dict(n=0), dict(n=-5), dict(n=1 << 31),
                 dict(index_bytes=one - 1), dict(index_bytes=0),                # no index fits: the header check the
                 dict(levels=[(1, 1)] * 9, dist=[0.1] * 9),                     # host can make without a read
                 dict(levels=[(0, 1)], dist=[0.1]), dict(levels=[(1, 0)], dist=[0.1]), dict(T0=nan_T),
                 dict(dist=[0.2, 0.0, 0.02]), dict(dist=[0.2, 0.05, float("inf")]),
                 dict(dist=[float("nan"), 0.05, 0.02]), dict(dist=[0.2, -1.0, 0.02]), dict(share=-0.1),
                 dict(share=float("nan")), dict(spread=float("nan")), dict(spread=-1.0), dict(max_w=0.0),
                 dict(max_v=float("inf")), dict(max_w=float("nan")), dict(normals=P8, cos=1.5),
                 dict(normals=P8, cos=float("nan")), dict(normals=P8, cos=-1.01)):
        assert call(**over) == INVALID, over
    assert call(ws_bytes=1024) == TOO_SMALL
