"""Mesh normals and colours without a GPU: the host function against the restatement, analytic normals of a cube, the
restated colouring against ground truth and an independent visibility test, the PLY attributes, the colour field and
the C entries' argument validation.  (The kernels against the same restatement, bit for bit:
tests/test_gpu_mesh_color.py.)"""
import ctypes as C
import inspect

import numpy as np
import pytest

import mesh_color_restatement as M
from bnv_fusion_amd import mesh, synthetic
from mesh_color_restatement import MEAN_ERR, P99_ERR, bits, soup      # (the bars are measured on this file's scene)

H, W = 30, 40
K = np.array([[35.0, 0.0, 19.5], [0.0, 35.0, 14.5], [0.0, 0.0, 1.0]])
# six views face on and two from opposite corners: every face is seen flat once and slanted once
EYES = [(1.5, 0, 0), (-1.5, 0, 0), (0, 1.5, 0), (0, -1.5, 0), (0, 0, 1.5), (0, 0, -1.5), (1.0, 1.0, 1.0),
        (-1.0, -1.0, -1.0)]
DEPTH_TOL = 0.02


@pytest.fixture(scope="module")
def cube():
    return M.cube_mesh(8)


@pytest.fixture(scope="module")
def scene(cube):
    """The cube scanned by the restated ray caster and coloured by the restatement, once for every test."""
    v, f = cube
    poses = [M.look_at(e, (0.0, 0.0, 0.0)) for e in EYES]
    frames = M.scan(v, f, poses, K, H, W, synthetic.surface_color)
    colors, observed, state, traces = M.color_vertices(v, f, frames, depth_tol=DEPTH_TOL)
    return {"poses": poses, "frames": frames, "colors": colors, "observed": observed, "traces": traces}


def test_host_normals_equal_the_restatement(cube):
    rng = np.random.default_rng(5)
    for v, f in (cube, soup(), (rng.normal(size=(300, 3)).astype(np.float32), rng.integers(0, 300, (2000, 3)))):
        got = mesh.vertex_normals(mesh.TriMesh(v, f))
        assert got.dtype == np.float32 and got.shape == (len(v), 3)
        assert (bits(got) == bits(M.vertex_normals(v, f))).all()


def test_cube_normals_are_analytic(cube):
    """Face-interior vertices carry the face normal; edge and corner vertices the normalised sum of the adjacent face
    normals (the cube's cells are cut so that every adjacent face has the same triangle area at such a vertex)."""
    v, f = cube
    n = mesh.vertex_normals(mesh.TriMesh(v, f)).astype(np.float64)
    on = np.abs(np.abs(v.astype(np.float64)) - 0.4) < 1e-6              # [V, 3]: the vertex lies on that pair of faces
    assert sorted(np.bincount(on.sum(1)).tolist()) == [0, 8, 12 * 7, 6 * 49]
    want = np.sign(v.astype(np.float64)) * on
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.abs(n - want).max() <= 1e-6
    # outwards: the winding, not only the axis
    assert ((n * v).sum(1) > 0).all()


def test_face_order_changes_no_bit(cube):
    v, f = cube
    base = mesh.vertex_normals(mesh.TriMesh(v, f))
    perm = np.random.default_rng(1).permutation(len(f))
    assert (bits(mesh.vertex_normals(mesh.TriMesh(v, f[perm]))) == bits(base)).all()
    assert (bits(M.vertex_normals(v, f[perm])) == bits(base)).all()


def test_zero_normals_without_refusal():
    v, f = soup()
    n = mesh.vertex_normals(mesh.TriMesh(v, f))
    assert (n[[4, 5, 6, 7, 8, 9]] == 0).all()
    assert np.abs(np.linalg.norm(n[:4], axis=1) - 1.0).max() < 1e-6
    assert (bits(n) == bits(M.vertex_normals(v, f))).all()


def test_refusals():
    v, f = soup()
    bad = v.copy()
    bad[4, 1] = np.nan                                                  # (an unreferenced vertex counts too)
    with pytest.raises(ValueError, match="finite"):
        mesh.vertex_normals(mesh.TriMesh(bad, f))
    for idx in (-1, len(v)):
        g = f.copy()
        g[1, 2] = idx
        with pytest.raises(ValueError, match="outside"):
            mesh.vertex_normals(mesh.TriMesh(v, g))
    big = np.array([[0, 0, 0], [128, 0, 0], [0, 128, 0]], np.float32)  # 2^13 square units in one face
    with pytest.raises(ValueError, match="2\\^12"):
        mesh.vertex_normals(mesh.TriMesh(big, np.array([[0, 1, 2]])))
    many = np.array([[0, 0, 0], [64, 0, 0], [0, 64, 0]], np.float32)   # 2^11 each: two of them reach the total
    assert mesh.vertex_normals(mesh.TriMesh(many, np.array([[0, 1, 2]]))).shape == (3, 3)
    with pytest.raises(ValueError, match="2\\^12"):
        mesh.vertex_normals(mesh.TriMesh(many, np.array([[0, 1, 2], [0, 1, 2]])))
    assert [M.refused(bad, f), M.refused(v, f), M.refused(big, [[0, 1, 2]]), M.refused(many, [[0, 1, 2]] * 2)] == \
        ["finite", None, "area", "area"]


@pytest.mark.parametrize("case", list(M.area_limit_cases()))
def test_host_and_restatement_agree_at_the_total_area_limit(case):
    """The inputs of test_gpu_mesh_color.py::test_normals_total_area_limit: the host function refuses exactly those the
    restatement refuses, and gives the restatement's bits, (0, 0, 1), one face short of the limit."""
    v, f, accepted = M.area_limit_cases()[case]
    assert M.refused(v, f) == (None if accepted else "area")
    if not accepted:
        with pytest.raises(ValueError, match="2\\^12"):
            mesh.vertex_normals(mesh.TriMesh(v, f))
        return
    got = mesh.vertex_normals(mesh.TriMesh(v, f))
    assert (bits(got) == bits(M.vertex_normals(v, f))).all() and (got == np.array([0, 0, 1], np.float32)).all()


def test_colors_against_ground_truth(cube, scene):
    """The restated colouring of the cube (386 vertices, 8 poses at 40 x 30, depth in uint16 millimetres, the default
    parameters) against ``synthetic.surface_color`` at the vertices.  Measured with this restatement on this scene:
    8 of 386 vertices unobserved (2.07 %), mean absolute error 3.0884 levels, 99th percentile 13.2501 levels; a
    channel swap gives a mean of 39.9 and a transposed image 61.2.  The GPU result is bit-equal to this restatement
    (tests/test_gpu_mesh_color.py), so the 1.25x margin below only leaves room for a deliberate change of defaults."""
    v, f = cube
    assert len(v) == 386
    observed, colors = scene["observed"], scene["colors"]
    assert 1.0 - observed.mean() <= 0.05
    truth = synthetic.surface_color(v.astype(np.float64))
    err = np.abs(colors.astype(np.float64) - truth)[observed]
    print(f"unobserved {1.0 - observed.mean():.4f}, mean {err.mean():.4f}, p99 {np.percentile(err, 99):.4f}")
    assert err.mean() <= 1.25 * MEAN_ERR
    assert np.percentile(err, 99) <= 1.25 * P99_ERR
    assert (colors[~observed] == 128).all()


@pytest.mark.parametrize("mistake", ["channel swap", "transposed image"])
def test_a_wrong_image_fails_by_a_wide_factor(cube, scene, mistake):
    v, f = cube
    frames = []
    for fr in scene["frames"]:
        rgb = fr["rgb"][..., ::-1] if mistake == "channel swap" else fr["rgb"].transpose(1, 0, 2).reshape(H, W, 3)
        frames.append(dict(fr, rgb=np.ascontiguousarray(rgb)))
    colors, observed, _, _ = M.color_vertices(v, f, frames, depth_tol=DEPTH_TOL)
    err = np.abs(colors.astype(np.float64) - synthetic.surface_color(v.astype(np.float64)))[observed]
    assert err.mean() > 8 * 1.25 * MEAN_ERR


def test_no_colour_from_a_frame_that_does_not_see_the_vertex(cube, scene):
    """Visibility decided without a depth image: the segment from the vertex to the camera against every triangle.  A
    vertex whose occluder lies within depth_tol of it is within tolerance of a silhouette and set aside."""
    v, f = cube
    used_hidden = aside = any_hidden = 0
    for T, tr in zip(scene["poses"], scene["traces"]):
        dist = M.occluder_distance(T[:3, 3], v, f)
        used = tr["reason"] == M.USED
        hidden = np.isfinite(dist)
        near_silhouette = hidden & (dist <= DEPTH_TOL)
        used_hidden += int((used & hidden & ~near_silhouette).sum())
        aside += int((used & near_silhouette).sum())
        any_hidden += int(hidden.sum())
        assert (tr["reason"][hidden & ~near_silhouette] == M.NO_NEIGHBOUR).all()      # ... and the depth test says so
    assert any_hidden > len(v)                                          # the back of the cube, in every frame
    assert used_hidden == 0
    assert aside <= 0.02 * len(v) * len(scene["poses"])


def test_batching_and_resolve_in_the_restatement(cube, scene):
    v, f = cube
    n = M.vertex_normals(v, f)
    a, b = M.ColorState(len(v)), M.ColorState(len(v))
    M.accumulate(a, v, n, scene["frames"])
    M.accumulate(b, v, n, scene["frames"][:3])
    M.accumulate(b, v, n, scene["frames"][3:])
    assert (a.sums.view(np.uint64) == b.sums.view(np.uint64)).all() and (a.count == b.count).all()
    s = M.ColorState(4)
    s.sums[:] = [[0.5, 1.5, 2.5, 1.0], [300.0, -3.0, 254.5, 1.0], [7.0, 7.0, 7.0, 2.0], [0.0, 0.0, 0.0, 0.0]]
    s.count[:] = [1, 2, 1, 0]
    colors, observed = M.resolve(s, fill=(1, 2, 3))
    assert colors.tolist() == [[0, 2, 2], [255, 0, 254], [4, 4, 4], [1, 2, 3]]           # half to even, clamped, fill
    assert observed.tolist() == [True, True, True, False]


def test_export_without_attributes_writes_the_same_bytes(tmp_path):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32)
    f = np.array([[0, 1, 2]], np.int64)
    m = mesh.TriMesh(v, f)
    assert m.vertex_normals is None and m.vertex_colors is None
    literal = (b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\n"
               b"property float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
               + v.astype("<f4").tobytes() + b"\x03" + np.array([0, 1, 2], "<i4").tobytes())
    assert open(m.export(str(tmp_path / "plain.ply")), "rb").read() == literal


def test_attributes_round_trip_through_ply(tmp_path, cube):
    v, f = cube
    m = mesh.TriMesh(v, f)
    m.vertex_normals = mesh.vertex_normals(m)
    m.vertex_colors = np.clip(np.rint(synthetic.surface_color(v.astype(np.float64))), 0, 255).astype(np.uint8)
    path = m.export(str(tmp_path / "coloured.ply"))
    head = open(path, "rb").read(400)
    for prop in (b"property float nx", b"property float nz", b"property uchar red", b"property uchar blue"):
        assert prop in head
    back = mesh.load_ply(path)
    assert (back.vertices == v).all() and (back.faces == f).all()
    assert (bits(back.vertex_normals) == bits(m.vertex_normals)).all()
    assert back.vertex_colors.dtype == np.uint8 and (back.vertex_colors == m.vertex_colors).all()
    for only in ("vertex_normals", "vertex_colors"):                    # either attribute alone
        one = mesh.TriMesh(v, f)
        setattr(one, only, getattr(m, only))
        got = mesh.load_ply(one.export(str(tmp_path / (only + ".ply"))))
        assert (getattr(got, only) == getattr(m, only)).all()
        assert getattr(got, "vertex_colors" if only == "vertex_normals" else "vertex_normals") is None
    plain = mesh.load_ply(mesh.TriMesh(v, f).export(str(tmp_path / "plain.ply")))
    assert plain.vertex_normals is None and plain.vertex_colors is None
    with pytest.raises(ValueError, match="merge_vertices"):
        m.merge_vertices()
    assert len(mesh.TriMesh(v, f).merge_vertices().vertices) == len(v)
    short = mesh.TriMesh(v, f)
    short.vertex_colors = m.vertex_colors[:5]
    with pytest.raises(ValueError, match="vertex_colors"):
        short.export(str(tmp_path / "short.ply"))


def test_surface_color_is_the_same_in_numpy_and_torch():
    import torch
    p = np.random.default_rng(2).uniform(-3.0, 3.0, (5000, 3))
    a = synthetic.surface_color(p)
    b = synthetic.surface_color(torch.from_numpy(p)).numpy()
    assert a.shape == (5000, 3) and a.min() >= 0.0 and a.max() <= 255.0
    assert (a.view(np.uint64) == b.view(np.uint64)).all()
    assert a.max(0).min() > 200 and a.min(0).max() < 55                # every channel uses its range
    # channels differ, and each depends on its own two axes only
    assert np.abs(a[:, 0] - a[:, 1]).mean() > 20 and np.abs(a[:, 1] - a[:, 2]).mean() > 20
    q = p.copy()
    q[:, 2] += 0.123
    assert (synthetic.surface_color(q)[:, 0] == a[:, 0]).all() and (synthetic.surface_color(q)[:, 1] != a[:, 1]).any()


def test_scan_frames_keeps_its_keys_and_back_projects_pixel_centres():
    from bnv_fusion_amd import scan
    sig = inspect.signature(scan.scan_frames)
    assert sig.parameters["color"].default is None
    assert list(sig.parameters)[:5] == ["scanner", "poses", "K", "H", "W"]
    src = inspect.getsource(scan.scan_frames)
    assert '{"frame_id": i, "depth": d, "intr_mat": K.copy(), "T_wc": poses[i].copy()}' in src
    with pytest.raises(ValueError, match="color"):
        next(scan.scan_frames(None, np.eye(4)[None], K, H, W, color="plaid"))
    # the back-projection of scan.render_color on numpy: a plane z = 1.2 seen face on from the origin
    T = M.look_at((0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    d = np.full((H, W), 1.2)
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y = (c - K[0, 2]) / K[0, 0] * d, (r - K[1, 2]) / K[1, 1] * d
    world = np.stack([((x * T[a, 0] + y * T[a, 1]) + d * T[a, 2]) + T[a, 3] for a in range(3)], -1)
    o, rays = M.R.camera_rays(K, T, H, W)
    assert np.abs(world.reshape(-1, 3) - (o[None] + 1.2 * rays)).max() < 1e-12


def test_c_entries_validate_arguments_without_a_gpu():
    from bnv_fusion_amd import _lib
    lib = _lib.load()
    INVALID, TOO_SMALL = -1, -2
    p = C.c_void_p(8)
    n = C.c_int64()
    assert lib.bnv_mesh_normals_workspace_bytes(0, C.byref(n)) == INVALID
    assert lib.bnv_mesh_normals_workspace_bytes(10, None) == INVALID
    assert lib.bnv_mesh_normals_workspace_bytes(10, C.byref(n)) == 0 and n.value >= 240
    assert lib.bnv_mesh_vertex_normals(None, 3, p, 1, p, 1 << 20, p, p, None) == INVALID
    assert lib.bnv_mesh_vertex_normals(p, 0, p, 1, p, 1 << 20, p, p, None) == INVALID
    assert lib.bnv_mesh_vertex_normals(p, 3, None, 1, p, 1 << 20, p, p, None) == INVALID
    assert lib.bnv_mesh_vertex_normals(p, 3, p, -1, p, 1 << 20, p, p, None) == INVALID
    assert lib.bnv_mesh_vertex_normals(p, 3, p, 1, p, 1 << 20, None, p, None) == INVALID
    assert lib.bnv_mesh_vertex_normals(p, 3, p, 1, p, 1 << 20, p, None, None) == INVALID
    assert lib.bnv_mesh_vertex_normals(p, 3, p, 1, p, 8, p, p, None) == TOO_SMALL
    assert lib.bnv_mesh_color_workspace_bytes(-1, C.byref(n)) == INVALID
    assert lib.bnv_mesh_color_workspace_bytes(10, C.byref(n)) == 0 and n.value >= 360
    assert lib.bnv_mesh_color_begin(p, 1 << 20, 0, None) == INVALID
    assert lib.bnv_mesh_color_begin(None, 1 << 20, 10, None) == TOO_SMALL
    assert lib.bnv_mesh_color_begin(p, 8, 10, None) == TOO_SMALL

    def frame(**kw):
        f = _lib.MeshColorFrame()
        f.depth, f.conf, f.rgb, f.depth_dtype, f.conf_level = 8, None, 8, 0, 0
        f.height, f.width, f.color_height, f.color_width = 4, 5, 4, 5
        f.K[:] = f.K_color[:] = [5.0, 5.0, 2.0, 1.5]
        f.T_cw[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
        for k, val in kw.items():
            if isinstance(val, tuple):
                getattr(f, k)[val[0]] = val[1]
            else:
                setattr(f, k, val)
        return f

    def accumulate(frames, v=p, nrm=p, V=10, tol=0.02, cos_min=0.2, near=0.0, far=3.0, ws=p, ws_bytes=1 << 20, count=None):
        arr = (_lib.MeshColorFrame * max(len(frames), 1))(*frames)
        return lib.bnv_mesh_color_accumulate(v, nrm, V, arr if frames is not None else None,
                                             len(frames) if count is None else count, tol, cos_min, near, far, ws,
                                             ws_bytes, None)

    assert accumulate([frame()], v=None) == INVALID
    assert accumulate([frame()], nrm=None) == INVALID
    assert accumulate([frame()], V=0) == INVALID
    assert accumulate([], count=0) == INVALID
    assert accumulate([frame()] * 9) == INVALID                                         # > 8 frames
    assert lib.bnv_mesh_color_accumulate(p, p, 10, None, 1, 0.02, 0.2, 0.0, 3.0, p, 1 << 20, None) == INVALID
    for bad in (dict(depth=None), dict(rgb=None), dict(height=0), dict(width=0), dict(color_height=0),
                dict(color_width=0), dict(width=40000), dict(depth_dtype=2), dict(conf_level=1),
                dict(K=(0, np.nan)), dict(K=(3, np.inf)), dict(K_color=(1, np.nan)), dict(T_cw=(7, np.inf)),
                dict(center=(2, np.nan))):
        assert accumulate([frame(), frame(**bad)]) == INVALID, bad
    for bad in (dict(tol=-0.01), dict(tol=np.nan), dict(cos_min=-0.1), dict(cos_min=1.0), dict(cos_min=np.nan),
                dict(near=-1.0), dict(far=np.inf), dict(far=0.0)):
        assert accumulate([frame()], **bad) == INVALID, bad
    assert accumulate([frame()], ws=None) == TOO_SMALL
    assert accumulate([frame()], ws_bytes=8) == TOO_SMALL
    fill = (C.c_uint8 * 3)(128, 128, 128)
    assert lib.bnv_mesh_color_resolve(p, 1 << 20, 0, fill, p, p, None, None, None) == INVALID
    assert lib.bnv_mesh_color_resolve(p, 1 << 20, 10, None, p, p, None, None, None) == INVALID
    assert lib.bnv_mesh_color_resolve(p, 1 << 20, 10, fill, None, p, None, None, None) == INVALID
    assert lib.bnv_mesh_color_resolve(p, 1 << 20, 10, fill, p, None, None, None, None) == INVALID
    assert lib.bnv_mesh_color_resolve(None, 1 << 20, 10, fill, p, p, None, None, None) == TOO_SMALL
    assert lib.bnv_mesh_color_resolve(p, 8, 10, fill, p, p, None, None, None) == TOO_SMALL


def test_wrappers_refuse_cpu_tensors_and_bad_parameters():
    import torch
    v, f = M.cube_mesh(2)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(ValueError, match="GPU tensor"):
        mesh.vertex_normals_tensors(tv, tf)
    with pytest.raises(ValueError, match="GPU tensor"):
        mesh.VertexColorer(tv, tf)


def test_datasets_decode_colour_only_on_request(tmp_path):
    from PIL import Image
    from bnv_fusion_amd import datasets
    rng = np.random.default_rng(4)
    depth = [rng.integers(500, 2000, (6, 8)).astype(np.uint16) for _ in range(2)]
    root = datasets.write_sequence(str(tmp_path), "s/a", depth, K, [np.eye(4)] * 2, [1.0, 1.0, 1.0])
    import os
    os.makedirs(os.path.join(root, "image"), exist_ok=True)
    same, large = rng.integers(0, 256, (6, 8, 3)).astype(np.uint8), rng.integers(0, 256, (12, 16, 3)).astype(np.uint8)
    Image.fromarray(same).save(os.path.join(root, "image", "0.jpg"), format="PNG")        # (lossless, whatever its name)
    Image.fromarray(large).save(os.path.join(root, "image", "1.jpg"), format="PNG")
    plain = datasets.FusionInferenceDataset(str(tmp_path), "s/a", device="cpu")[0]
    assert "rgb" not in plain and "rgb_intr_mat" not in plain
    data = datasets.FusionInferenceDataset(str(tmp_path), "s/a", device="cpu", load_rgb=True)
    a, b = data[0], data[1]
    assert {k for k in a if k != "rgb"} == set(plain) and all(np.array_equal(a[k], plain[k]) for k in plain)
    assert a["rgb"].dtype == np.uint8 and (a["rgb"] == same).all() and "rgb_intr_mat" not in a
    assert (b["rgb"] == large).all()
    # twice the size, pixel centres at integers: u' = (u + 0.5) 2 - 0.5
    assert np.allclose(b["rgb_intr_mat"], [[70.0, 0, 39.5], [0, 70.0, 29.5], [0, 0, 1]])
    os.remove(os.path.join(root, "image", "1.jpg"))
    with pytest.raises(FileNotFoundError, match="colour image"):
        data[1]


def test_run_e2e_color_refuses_sequences_without_colour(tmp_path):
    import os
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_e2e.py"), "--synthetic", "2", "--color",
                        "--out", str(tmp_path / "out")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode != 0 and "no colour image" in r.stderr.replace("\n", " ")
    assert not os.path.exists(tmp_path / "out" / "final.ply")
