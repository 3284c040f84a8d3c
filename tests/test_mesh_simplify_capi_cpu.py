"""Mesh simplification: the C entries refuse invalid arguments before any HIP call (status codes of
include/bnv_fusion.h), so this runs without a GPU."""
import ctypes as C

import pytest

from conftest import ROOT  # noqa: F401

INVALID, TOO_SMALL = -1, -2


@pytest.fixture(scope="module")
def lib():
    import os
    from bnv_fusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_size_query(lib):
    n = C.c_int64(-1)
    assert lib.bnv_mesh_simplify_bytes(0, 0, C.byref(n)) == 0 and n.value > 0 and n.value % 256 == 0
    small = n.value
    assert lib.bnv_mesh_simplify_bytes(1000, 2000, C.byref(n)) == 0 and n.value > small and n.value % 256 == 0
    assert lib.bnv_mesh_simplify_bytes(1000, 2000, None) == INVALID
    for V, T in ((-1, 0), (0, -1), (2 ** 31 - 1, 0), (0, 2 ** 30 + 1)):
        assert lib.bnv_mesh_simplify_bytes(V, T, C.byref(n)) == INVALID
    assert lib.bnv_mesh_simplify_bytes(2 ** 31 - 2, 2 ** 30, C.byref(n)) == 0 and n.value > 2 ** 36


def test_arguments_are_refused_before_any_launch(lib):
    p8 = C.c_void_p(8)                                    # a non-null pointer no refused call dereferences
    n = C.c_int64()
    assert lib.bnv_mesh_simplify_bytes(4, 4, C.byref(n)) == 0

    def call(V=4, T=4, cell=0.1, placement=0, min_det=1e-3, ws=p8, ws_bytes=None, v=p8, f=p8, vo=p8, fo=p8, counts=p8):
        return lib.bnv_mesh_simplify(v, V, f, T, C.c_double(cell), placement, C.c_double(min_det), ws,
                                     n.value if ws_bytes is None else ws_bytes, vo, fo, counts, None)

    for cell in (0.0, -1.0, float("nan"), float("inf")):
        assert call(cell=cell) == INVALID
    for md in (-1e-9, float("nan"), float("inf")):
        assert call(min_det=md) == INVALID
    for placement in (-1, 2):
        assert call(placement=placement) == INVALID
    for V, T in ((-1, 4), (4, -1), (2 ** 31 - 1, 4), (4, 2 ** 30 + 1)):
        assert call(V=V, T=T) == INVALID
    for kw in ({"counts": None}, {"v": None}, {"vo": None}, {"f": None}, {"fo": None}):
        assert call(**kw) == INVALID
    assert call(ws=None) == TOO_SMALL
    assert call(ws_bytes=n.value - 1) == TOO_SMALL
