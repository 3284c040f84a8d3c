"""Workspace layouts are contracts: every size entry (bnv_*_workspace_bytes / bnv_*_workspace / bnv_shard_state_bytes)
and every exported *_offset entry returns, for a table of shapes, exactly the value recorded in
tests/golden/workspace_layouts.json.  The values were recorded once from the build BEFORE the layouts were rewritten on
csrc/workspace.hpp's carver; they are data, not something to regenerate from the code under test -- a difference is a
bug in a layout.  CPU only: the size functions are pure host code (as in tests/test_capi_symbols.py).

Shapes per entry: 0 and 1 where accepted, counts just below / at / above a multiple of 256 bytes of the entry's element
size, counts just below / at / above the entry's tile size, and one realistic size."""
import ctypes as C
import json
import os

import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_layouts.json")

GRID_DIMS = [(1, 1, 1), (7, 9, 11), (64, 64, 64), (200, 150, 100)]
# 4-byte pieces fill 256 bytes at 64 elements, 8-byte pieces at 32, 16-byte pieces at 16, 32-byte pieces at 8
AROUND_256B = [7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]


def _by_out(fn, *args):
    """An entry that returns a status and writes the size through its last argument: [status, bytes]."""
    out = C.c_int64(-1)
    rc = int(fn(*args, C.byref(out)))
    return [rc, int(out.value)]


def _i32x3(d):
    return (C.c_int32 * 3)(*d)


def _plan_grids(lib_mod, dims):
    grids = (lib_mod.Grid * len(dims))()
    for g, d in zip(grids, dims):
        g.n_xyz[:] = d
        g.voxel_size = 0.02
        for a in range(3):
            g.bound_min[a], g.bound_lo[a], g.bound_hi[a] = -1.0, -0.98, 1.0
    return grids


def measure():
    """{"entry(args)": value} for every case of the table, from the loaded library."""
    from bnv_fusion_amd import _lib
    lib = _lib.load()
    got = {}

    def put(name, args, value):
        got[f"{name}({', '.join(str(a) for a in args)})"] = value

    for name in ("bnv_encode_shard_counts_offset", "bnv_shard_state_loads_offset", "bnv_shard_state_table_offset"):
        put(name, (), int(getattr(lib, name)()))

    # depth front end: tiles of 1024 pixels
    for hw in [(1, 1), (1, 1023), (1, 1024), (1, 1025), (255, 257), (480, 640), (520, 512)]:
        put("bnv_depth_workspace_bytes", hw, int(lib.bnv_depth_workspace_bytes(*hw)))

    # encoder: 256 points per mark workgroup, 1024 slots (8 per point) and 1024 chunks of 64 voxels per scan tile
    for pts in [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 307200]:
        for d in GRID_DIMS:
            put("bnv_encode_workspace_bytes", (pts, d), int(lib.bnv_encode_workspace_bytes(pts, _i32x3(d))))

    # volume upsert: tiles of 2048 keys, 256-key blocks
    for n in [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 100000]:
        put("bnv_volume_workspace_bytes", (n,), int(lib.bnv_volume_workspace_bytes(n)))

    # TSDF marching cubes: tiles of 64 grid points, scan blocks of 1024 tiles
    for d in [(1, 1, 1), (2, 2, 2), (3, 3, 7), (4, 4, 4), (5, 13, 1), (32, 32, 64), (65537, 1, 1), (48, 40, 40),
              (256, 256, 128)]:
        put("bnv_tsdf_mesh_workspace_bytes", (d,), _by_out(lib.bnv_tsdf_mesh_workspace_bytes, _i32x3(d)))

    # lattice decode: n origins, 27 neighbours each; the persistent part depends on row_capacity only
    caps = [1, 63, 64, 65, 1000, 200000]
    for rc in caps:
        put("bnv_decode_lattice_count_offset", (rc,), int(lib.bnv_decode_lattice_count_offset(rc)))
        put("bnv_decode_lattice_table_offset", (rc,), int(lib.bnv_decode_lattice_table_offset(rc)))
        for n in [0, 1, 2, 3, 63, 64, 65, 2371]:
            put("bnv_decode_lattice_workspace_bytes", (n, rc), int(lib.bnv_decode_lattice_workspace_bytes(n, rc)))
            put("bnv_decode_lattice_list_offset", (n, rc), int(lib.bnv_decode_lattice_list_offset(n, rc)))

    # surface sampling: float64 prefix, tiles of 2048 faces
    for nf in [0, 1, 31, 32, 33, 2047, 2048, 2049, 100000]:
        put("bnv_mesh_sample_surface_workspace", (nf,), _by_out(lib.bnv_mesh_sample_surface_workspace, nf))

    # nearest neighbour: n_ref + 2 bins, scan tiles of 1024 bins
    for nr, nq in [(0, 1), (1, 1), (15, 17), (16, 16), (17, 15), (61, 63), (62, 64), (63, 65), (1021, 5), (1022, 5),
                   (1023, 5), (100000, 50000)]:
        put("bnv_nn_workspace_bytes", (nr, nq), _by_out(lib.bnv_nn_workspace_bytes, nr, nq))

    # mesh SDF / mesh rays: 8 F + 66 bins, scan tiles of 1024 bins; the edge table is a power of two >= 4 F
    for nv, nf in [(0, 0), (1, 1), (3, 1), (16, 16), (17, 15), (63, 21), (64, 64), (65, 65), (200, 119), (200, 120),
                   (200, 121), (50000, 100000)]:
        put("bnv_mesh_sdf_workspace_bytes", (nv, nf), _by_out(lib.bnv_mesh_sdf_workspace_bytes, nv, nf))
        put("bnv_mesh_ray_workspace_bytes", (nv, nf), _by_out(lib.bnv_mesh_ray_workspace_bytes, nv, nf))

    # renderer: n rays, k samples per round
    for n in [0, 1, 63, 64, 65, 307200]:
        for k in [0, 1, 5, 8, 32, 33]:
            put("bnv_render_workspace_bytes", (n, k), int(lib.bnv_render_workspace_bytes(n, k)))

    # mesh post-processing and components (the tail of both is rocPRIM's temporary storage for these sizes)
    for v, t in [(0, 0), (1, 1), (31, 33), (32, 32), (33, 31), (63, 21), (64, 64), (65, 130), (10000, 20000)]:
        put("bnv_mesh_post_workspace_bytes", (v, t), _by_out(lib.bnv_mesh_post_workspace_bytes, v, t))
        put("bnv_mesh_components_workspace_bytes", (v, t), _by_out(lib.bnv_mesh_components_workspace_bytes, v, t))

    # embedding training: B patches of n points, M query points each
    for b, n, m in [(0, 1, 1), (1, 1, 1), (1, 2, 1), (1, 64, 1), (2, 32, 3), (3, 21, 5), (4, 16, 16), (5, 13, 13),
                    (16, 64, 128), (1, 65, 1)]:
        put("bnv_train_workspace_bytes", (b, n, m), int(lib.bnv_train_workspace_bytes(b, n, m)))
        put("bnv_train_tcnn_workspace_bytes", (b, n, m), int(lib.bnv_train_tcnn_workspace_bytes(b, n, m)))

    # ICP: (stride, iterations) per level
    for levels in [(), (1, 1), (4, 0, 1, 1), (4, 7, 2, 8, 1, 9), (4, 3, 2, 5, 1, 10), (1, 4096), (1, 4097)]:
        arr = (C.c_int32 * max(len(levels), 1))(*levels)
        put("bnv_icp_workspace_bytes", levels, int(lib.bnv_icp_workspace_bytes(len(levels) // 2, arr)))

    # mesh colouring: 24-byte and 32-byte rows per vertex
    for v in [0, 1] + AROUND_256B + [100000]:
        put("bnv_mesh_normals_workspace_bytes", (v,), _by_out(lib.bnv_mesh_normals_workspace_bytes, v))
        put("bnv_mesh_color_workspace_bytes", (v,), _by_out(lib.bnv_mesh_color_workspace_bytes, v))

    # volume planning: per candidate grid a table and one word per 256 pixels
    for h, w in [(0, 1), (1, 1), (1, 255), (16, 16), (1, 257), (127, 129), (128, 128), (129, 127), (480, 640)]:
        for dims in [GRID_DIMS[:1], GRID_DIMS[1:3], GRID_DIMS]:
            for slots in [0, 64, 1024, 100]:
                grids = _plan_grids(_lib, dims)
                put("bnv_plan_workspace_bytes", (h, w, len(dims), slots),
                    int(lib.bnv_plan_workspace_bytes(h, w, grids, len(dims), slots)))

    # first-touch ownership state: blocks of 2^s voxels per axis
    for d in GRID_DIMS + [(255, 1, 1), (256, 1, 1), (257, 1, 1), (512, 512, 256)]:
        for s in [0, 2, 4, 8, 9]:
            put("bnv_shard_state_bytes", (d, s), int(lib.bnv_shard_state_bytes(_i32x3(d), s)))
    return got


@pytest.fixture(scope="module")
def layouts():
    from bnv_fusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    with open(GOLDEN) as fh:
        want = json.load(fh)
    return measure(), want


def test_every_size_and_offset_entry_is_covered(layouts):
    """The table calls every exported size / offset entry of the binding."""
    from bnv_fusion_amd import _lib
    got, _ = layouts
    called = {k.split("(")[0] for k in got}
    sizes = {s for s in _lib.SYMBOLS
             if s.endswith(("_workspace_bytes", "_offset")) or s in ("bnv_mesh_sample_surface_workspace",
                                                                      "bnv_shard_state_bytes")}
    assert sizes == called


def test_layouts_match_the_recorded_values(layouts):
    got, want = layouts
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} of {len(want)} differ, e.g. {list(wrong.items())[:5]}"


def test_valid_sizes_are_multiples_of_256_where_every_piece_is_carved(layouts):
    """Entries whose pieces all come from the carver: the total is a whole number of 256-byte pieces."""
    got, _ = layouts
    carved = ("bnv_encode_workspace_bytes", "bnv_decode_lattice_workspace_bytes", "bnv_render_workspace_bytes",
              "bnv_train_workspace_bytes", "bnv_train_tcnn_workspace_bytes", "bnv_plan_workspace_bytes",
              "bnv_mesh_post_workspace_bytes", "bnv_mesh_components_workspace_bytes", "bnv_nn_workspace_bytes",
              "bnv_mesh_sdf_workspace_bytes", "bnv_mesh_normals_workspace_bytes", "bnv_mesh_color_workspace_bytes",
              "bnv_mesh_sample_surface_workspace")
    for k, v in got.items():
        if k.split("(")[0] in carved:
            size = v[1] if isinstance(v, list) else v
            if size > 0:
                assert size % 256 == 0, (k, v)


def test_carver_stand_alone_under_host_sanitizers(tmp_path):
    """tests/workspace_carver_main.cpp (its own main, no HIP call): null base, alignment and typed take() against a
    hand-computed layout, built with the host AddressSanitizer and UndefinedBehaviorSanitizer and run once."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "carver_check")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "workspace_carver_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "carver ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
