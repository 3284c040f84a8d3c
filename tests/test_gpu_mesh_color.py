"""Mesh normals and colours on the GPU (csrc/meshcolor.hip; include/bnv_fusion.h, "Mesh normals and colours") against
the numpy restatement of tests/mesh_color_restatement.py, bit for bit; occlusion; and the stage through the product:
NeuralMap.extract_mesh(color=...) against the colour field the frames were rendered from and against the only colour
the project had before, the TSDF volume's nearest-voxel colour."""
import numpy as np
import pytest
import torch

import mesh_color_restatement as M
from mesh_color_restatement import MEAN_ERR, bits, soup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_DEPTH = 3.0
# image size -> (focal length, cx): the cube (edge 0.75 m, seen face on from 1.5 m by frame 0) covers the image's last
# column and leaves background to its left, above and below, so that frame 0 has silhouette corners; powers of two
# keep the planted projections exact
CAMERAS = {(5, 7): (4.0, 5.0), (13, 17): (16.0, 11.0), (37, 70): (32.0, 60.0)}
EYE0 = (0.0, 0.0, -1.5)


def up(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.astype(np.int32)).to(DEV).to(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def down(frames):
    return [{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in fr.items()} for fr in frames]


def intr(H, W):
    f, cx = CAMERAS[(H, W)]
    return np.array([[f, 0.0, cx], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]])


# ---- normals -----------------------------------------------------------------------------------------------------------
def random_mesh(V, T, seed):
    rng = np.random.default_rng(seed)
    return (0.25 * rng.normal(size=(V, 3))).astype(np.float32), rng.integers(0, V, (T, 3)).astype(np.int64)


def planted_soup():
    """Random faces plus degenerate, duplicate and cancelling ones, and unreferenced vertices."""
    v, f = random_mesh(300, 600, 11)
    f = f[(f < 290).all(1)]                                             # 290 .. 299: unreferenced
    extra = np.array([[5, 5, 9], [7, 7, 7], [10, 11, 12], [10, 11, 12], [20, 21, 22], [20, 22, 21]], np.int64)
    v[280:283] = [[4, 4, 4], [5, 4, 4], [4, 5, 4]]                      # 280 .. 282: one face and its mirror image only
    f = f[(f < 280).all(1)]
    return v, np.concatenate([f, extra, [[280, 281, 282], [282, 281, 280]]])


NORMAL_CASES = {"one face": lambda: (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]])),
                "7 vertices": lambda: random_mesh(7, 9, 1), "255": lambda: random_mesh(255, 500, 2),
                "256": lambda: random_mesh(256, 500, 3), "257": lambda: random_mesh(257, 513, 4),
                "thousands of faces": lambda: random_mesh(1500, 4000, 5), "cube": lambda: M.cube_mesh(8),
                "small soup": soup, "planted soup": planted_soup}


@pytest.mark.parametrize("case", list(NORMAL_CASES))
def test_normals_match_restatement(case):
    from bnv_fusion_amd import mesh
    v, f = NORMAL_CASES[case]()
    f = np.asarray(f, np.int64)
    want = M.vertex_normals(v, f)
    got = mesh.vertex_normals_tensors(up(v), up(f)).cpu().numpy()
    assert got.dtype == np.float32 and (bits(got) == bits(want)).all()
    again = mesh.vertex_normals_tensors(up(v), up(f)).cpu().numpy()
    assert (bits(again) == bits(got)).all()
    perm = np.random.default_rng(0).permutation(len(f))
    assert (bits(mesh.vertex_normals_tensors(up(v), up(f[perm])).cpu().numpy()) == bits(got)).all()
    if case in ("small soup", "planted soup"):
        zero = [4, 5, 6, 7, 8, 9] if case == "small soup" else list(range(280, 300))
        assert (got[zero] == 0).all() and (np.abs(got).sum(1) > 0).sum() >= 4


def test_normals_refusals():
    from bnv_fusion_amd import mesh
    v, f = soup()
    bad = v.copy()
    bad[4, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        mesh.vertex_normals_tensors(up(bad), up(f))
    g = f.copy()
    g[1, 2] = len(v)
    with pytest.raises(ValueError, match="outside"):
        mesh.vertex_normals_tensors(up(v), up(g))
    many = np.array([[0, 0, 0], [64, 0, 0], [0, 64, 0]], np.float32)
    with pytest.raises(ValueError, match="2\\^12"):
        mesh.vertex_normals_tensors(up(many), up(np.array([[0, 1, 2], [0, 1, 2]])))


@pytest.mark.parametrize("case", list(M.area_limit_cases()))
def test_normals_total_area_limit(case):
    """The total-area step over many waves and every total slot: refused exactly when the total reaches 2^12, although
    no single face does (but in the last case); one face short of it, the restatement's bits."""
    from bnv_fusion_amd import mesh
    v, f, accepted = M.area_limit_cases()[case]
    if not accepted:
        with pytest.raises(ValueError, match="2\\^12"):
            mesh.vertex_normals_tensors(up(v), up(f))
        return
    got = mesh.vertex_normals_tensors(up(v), up(f)).cpu().numpy()
    assert got.dtype == np.float32 and (bits(got) == bits(M.vertex_normals(v, f))).all()
    assert (got == np.array([0, 0, 1], np.float32)).all()


# ---- colours -----------------------------------------------------------------------------------------------------------
def poses(n):
    from bnv_fusion_amd import scan
    ring = np.concatenate([scan.orbit_poses((0.0, 0.0, 0.0), 1.5, 8, height=0.5),
                           scan.orbit_poses((0.0, 0.0, 0.0), 1.4, 8, height=-0.7)])
    return np.concatenate([M.look_at(EYE0, (0.0, 0.0, 0.0))[None], ring])[:n]


class Scene:
    """The cube and 17 frames of it at one image size, generated on the GPU and downloaded, with planted vertices
    appended (unreferenced; their normals are given).  Frame 0 looks along +z from EYE0 with the identity rotation."""

    def __init__(self, H, W):
        from bnv_fusion_amd import mesh, scan
        self.H, self.W, self.K = H, W, intr(H, W)
        cube_v, self.f = M.cube_mesh(8, edge=0.75)
        scanner = scan.MeshScanner(mesh.TriMesh(cube_v, self.f), device=DEV)
        self.dev_frames = list(scan.scan_frames(scanner, poses(17), self.K, H, W, rounding="nearest",
                                                max_depth=MAX_DEPTH, color="procedural"))
        self.frames = down(self.dev_frames)
        f_, cx, cy = self.K[0, 0], self.K[0, 2], self.K[1, 2]
        d0 = self.frames[0]["depth"].astype(np.float64) / 1000.0
        assert (np.asarray(self.frames[0]["T_wc"]) == M.look_at(EYE0, (0, 0, 0))).all()
        assert (self.frames[0]["T_wc"][:3, :3] == np.eye(3)).all()

        def at(u, v, z):                                                # the world point frame 0 sees at (u, v, z)
            return [(u - cx) / f_ * z, (v - cy) / f_ * z, z + EYE0[2]]

        def block(n_valid):                                             # a 2 x 2 pixel block of frame 0 by its depths
            valid = (d0 > 0).astype(int)
            s = valid[:-1, :-1] + valid[:-1, 1:] + valid[1:, :-1] + valid[1:, 1:]
            ys, xs = np.nonzero(s == n_valid)
            assert len(ys), f"frame 0 has no 2 x 2 block with {n_valid} valid depths"
            return ys[0], xs[0], d0[ys[0]:ys[0] + 2, xs[0]:xs[0] + 2].max()

        z_face = 1.5 - 0.375
        y1, x1, z1 = block(1)
        y0, x0, _ = block(0)
        edge = z_face * (W - 1 - cx) / f_                               # projects exactly onto u = W - 1
        self.planted = {
            "behind": [0.1, 0.0, -2.5],
            "at max_depth": [0.0, 0.0, 1.5],                            # z + 1.5 == MAX_DEPTH exactly
            "last column": [edge, 0.0, -0.375],
            "just outside": [float(np.nextafter(np.float32(edge), np.float32(9))), 0.0, -0.375],
            "no depth": at(x0 + 0.5, y0 + 0.5, 1.0),
            "three background": at(x1 + 0.5, y1 + 0.5, z1),
            "zero normal": [0.0, 0.0, -0.375]}
        extra = np.array(list(self.planted.values()), np.float32)
        self.v = np.concatenate([cube_v, extra])
        self.index = {k: len(cube_v) + i for i, k in enumerate(self.planted)}
        self.normals = M.vertex_normals(self.v, self.f)
        assert (self.normals[len(cube_v):] == 0).all()                  # unreferenced
        for k, i in self.index.items():
            if k != "zero normal":
                self.normals[i] = (0.0, 0.0, -1.0)                      # towards frame 0's camera
        self.tv, self.tf, self.tn = up(self.v), up(self.f), up(self.normals)


@pytest.fixture(scope="module")
def scenes():
    return {size: Scene(*size) for size in CAMERAS}


def run_gpu(scene, frames, normals="given", **kw):
    from bnv_fusion_amd import mesh
    colorer = mesh.VertexColorer(scene.tv, scene.tf, normals=scene.tn if normals == "given" else None,
                                 max_depth=MAX_DEPTH, **kw)
    calls = frames if isinstance(frames, tuple) else (frames,)
    for part in calls:
        colorer.add(part)
    return [t.cpu().numpy() for t in colorer.result(return_weights=True)]


def check(scene, got, frames, normals="given", **kw):
    """The GPU's colours, observed flags, weights and counts equal the restatement's, bit for bit."""
    colors, observed, state, traces = M.color_vertices(scene.v, scene.f, frames, max_depth=MAX_DEPTH,
                                                       normals=scene.normals if normals == "given" else None, **kw)
    assert got[0].dtype == np.uint8 and got[0].shape == (len(scene.v), 3)
    assert (got[3] == state.count).all()
    assert (got[2].view(np.uint64) == state.sums[:, 3].view(np.uint64)).all()
    assert (got[1] == observed).all() and (got[0] == colors).all()
    return traces, observed


@pytest.mark.parametrize("n", [1, 3, 8, 9, 17])
def test_colors_match_restatement_for_every_frame_count(scenes, n):
    s = scenes[(13, 17)]
    traces, observed = check(s, run_gpu(s, s.dev_frames[:n]), s.frames[:n])
    assert observed.sum() > 50
    if n == 9:                                                          # 4 + 5 equals one call of 9
        whole = run_gpu(s, s.dev_frames[:9])
        split = run_gpu(s, (s.dev_frames[:4], s.dev_frames[4:9]))
        for a, b in zip(whole, split):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("size", list(CAMERAS))
@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_colors_match_restatement_and_planted_cases_occur(scenes, size, dtype):
    s = scenes[size]
    dev_frames, frames = s.dev_frames[:3], s.frames[:3]
    if dtype == "f32":
        dev_frames = [dict(fr, depth=fr["depth"].to(torch.float32) / 1000.0) for fr in dev_frames]
        frames = down(dev_frames)
        assert frames[0]["depth"].dtype == np.float32
    traces, observed = check(s, run_gpu(s, dev_frames), frames)
    t0, i = traces[0], s.index
    # every planted case is what the restatement saw in frame 0: none is vacuous
    assert t0["reason"][i["behind"]] == M.Z_RANGE and t0["z"][i["behind"]] < 0
    assert t0["reason"][i["at max_depth"]] == M.Z_RANGE and t0["z"][i["at max_depth"]] == MAX_DEPTH
    assert t0["u"][i["last column"]] == s.W - 1 and t0["reason"][i["last column"]] == M.USED
    assert s.W - 1 < t0["u"][i["just outside"]] < s.W - 1 + 1e-4
    assert t0["reason"][i["just outside"]] == M.OUT_OF_IMAGE
    assert t0["reason"][i["no depth"]] == M.NO_NEIGHBOUR and t0["n_zero"][i["no depth"]] == 4
    assert t0["reason"][i["three background"]] == M.USED
    assert t0["n_pass"][i["three background"]] == 1 and t0["n_zero"][i["three background"]] == 3
    assert all(t["reason"][i["zero normal"]] == M.ZERO_NORMAL for t in traces)
    assert observed[i["last column"]] and observed[i["three background"]]


def test_default_normals_and_the_one_call_form(scenes):
    from bnv_fusion_amd import mesh
    s = scenes[(13, 17)]
    check(s, run_gpu(s, s.dev_frames[:3], normals=None), s.frames[:3], normals=None)
    colors, observed = mesh.color_vertices((s.tv, s.tf), s.dev_frames[:3], max_depth=MAX_DEPTH)
    want, want_obs, _, _ = M.color_vertices(s.v, s.f, s.frames[:3], max_depth=MAX_DEPTH)
    assert observed.dtype == torch.bool and (colors.cpu().numpy() == want).all()
    assert (observed.cpu().numpy() == want_obs).all()
    host = mesh.TriMesh(s.v, s.f)
    out, obs = mesh.color_vertices(host, s.frames[:3], max_depth=MAX_DEPTH, device=DEV)   # host frames are uploaded
    assert out is host and (host.vertex_colors == want).all() and (obs == want_obs).all()
    assert (bits(host.vertex_normals) == bits(M.vertex_normals(s.v, s.f))).all()
    with pytest.raises(ValueError, match="frame 7 has no 'rgb'"):
        mesh.VertexColorer(s.tv, s.tf).add([{k: v for k, v in dict(s.dev_frames[0], frame_id=7).items() if k != "rgb"}])


def test_color_image_of_its_own_size(scenes):
    """Depth 13 x 17 beside colour 37 x 70 with its own intrinsics (the same poses)."""
    small, large = scenes[(13, 17)], scenes[(37, 70)]
    dev_frames = [dict(a, rgb=b["rgb"], rgb_intr_mat=large.K) for a, b in zip(small.dev_frames[:3], large.dev_frames)]
    traces, observed = check(small, run_gpu(small, dev_frames), down(dev_frames))
    reasons = np.concatenate([t["reason"] for t in traces])
    assert observed.sum() > 50 and (reasons == M.OUT_OF_COLOR).any()    # the colour camera sees less to the right
    from bnv_fusion_amd import mesh
    with pytest.raises(ValueError, match="rgb_intr_mat"):
        mesh.VertexColorer(small.tv, small.tf).add([dict(small.dev_frames[0], rgb=large.dev_frames[0]["rgb"])])


def test_confidence_gate(scenes):
    s = scenes[(13, 17)]
    rng = np.random.default_rng(3)
    dev_frames = [dict(fr, conf=up(rng.integers(0, 3, (s.H, s.W)).astype(np.uint8)), conf_level=2)
                  for fr in s.dev_frames[:3]]
    gated = run_gpu(s, dev_frames)
    check(s, gated, down(dev_frames))
    plain = run_gpu(s, s.dev_frames[:3])
    assert (gated[2] != plain[2]).any() and gated[3].sum() <= plain[3].sum()


# ---- occlusion ---------------------------------------------------------------------------------------------------------
def quad(half, n, z):
    """A square of half-size ``half`` in the plane ``z``, n x n cells, facing -z."""
    g = np.linspace(-half, half, n + 1)
    x, y = np.meshgrid(g, g)
    v = np.stack([x.reshape(-1), y.reshape(-1), np.full(x.size, z)], 1).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).reshape(-1)
    f = np.concatenate([np.stack([a, a + n + 1, a + 1], 1), np.stack([a + 1, a + n + 1, a + n + 2], 1)])
    return v, f.astype(np.int64)


def test_occlusion():
    """A 0.4 m quad at z = 0 in front of a 1 m quad at z = 1, both facing the first camera at z = -1: the front quad
    shadows |x|, |y| < 0.4 of the rear one.  The second camera stands between the quads."""
    from bnv_fusion_amd import mesh, scan, synthetic
    fv, ff = quad(0.2, 4, 0.0)
    rv, rf = quad(0.5, 10, 1.0)
    v, f = np.concatenate([fv, rv]), np.concatenate([ff, rf + len(fv)])
    n = M.vertex_normals(v, f)
    assert (n[:, 2] == -1).all()
    rear = np.arange(len(v)) >= len(fv)
    reach = np.abs(v[:, :2]).max(1)
    inside, outside = rear & (reach < 0.35), rear & (reach > 0.45)
    assert inside.sum() == 49 and outside.sum() == 40
    K = np.array([[48.0, 0.0, 31.5], [0.0, 48.0, 31.5], [0.0, 0.0, 1.0]])
    cams = np.stack([M.look_at((0, 0, -1.0), (0, 0, 1.0)), M.look_at((0, 0, 0.1), (0, 0, 1.0))])
    scanner = scan.MeshScanner(mesh.TriMesh(v, f), device=DEV)
    frames = list(scan.scan_frames(scanner, cams, K, 64, 64, rounding="nearest", color="procedural"))
    tv, tf = up(v), up(f)

    def run(frs, **kw):
        return [t.cpu().numpy() for t in mesh.VertexColorer(tv, tf, **kw).add(frs).result(return_weights=True)]

    colors, observed, _, count = run(frames[:1])
    assert not observed[inside].any() and observed[outside].all() and observed[~rear].all()
    colors, observed, _, count = run(frames)
    assert (count[inside] == 1).all() and (count[outside] == 2).all()   # the shadow: the second camera only
    err = np.abs(colors[inside].astype(np.float64) - synthetic.surface_color(v[inside].astype(np.float64)))
    print(f"occlusion: rear quad in the shadow, mean colour error {err.mean():.3f} levels")
    assert err.mean() <= 1.25 * MEAN_ERR
    # ... and it is the depth test that keeps the first frame out: a tolerance beyond the 1 m gap lets it in
    _, _, _, count = run(frames, depth_tol=1.5)
    assert (count[inside] == 2).all()
    got = run(frames)
    want = M.color_vertices(v, f, down(frames))
    assert (got[0] == want[0]).all() and (got[3] == want[2].count).all()


# ---- through the product -----------------------------------------------------------------------------------------------
SCALE, VOXEL = 0.5, 0.02
FRAMES = range(96, 141, 4)
# A 160 x 120 frame puts about 7 points into a 2 cm voxel one metre away: with the default min_pts_in_grid of 8 the map
# of these frames has no voxel to mesh (extract_mesh returns None; tests/test_gpu_track.py fuses 640 x 480 frames).
MIN_PTS = 2


@pytest.fixture(scope="module")
def product():
    """Twelve 160 x 120 frames of the half-size room mesh with the procedural colour, fused into a 128^3 map at 2 cm
    with its TSDF volume (tests/test_gpu_track.py's map, with MIN_PTS), extracted without and with colour."""
    import bnv_fusion_amd as bnv
    from bnv_fusion_amd import scan, sequence
    scanner = scan.MeshScanner(sequence.gt_mesh(SCALE), device=DEV)
    cams = np.stack([sequence.sweep_pose(t, SCALE) for t in FRAMES])
    frames = list(scan.scan_frames(scanner, cams, sequence.intrinsics(120, 160), 120, 160, max_depth=MAX_DEPTH,
                                   color="procedural"))
    assert len(frames) == 12 and frames[0]["rgb"].shape == (120, 160, 3)
    model = bnv.load_pretrained(device=DEV, voxel_size=VOXEL, min_pts_in_grid=MIN_PTS)
    nm = bnv.NeuralMap(np.array([2.54] * 3), VOXEL, model, min_pts_in_grid=MIN_PTS, device=DEV, tsdf=True)
    for fr in frames:
        nm.integrate(fr)
    torch.cuda.synchronize()
    plain = nm.extract_mesh(post_process=VOXEL / 4)
    coloured = nm.extract_mesh(post_process=VOXEL / 4, color=frames)
    return {"nm": nm, "frames": frames, "plain": plain, "coloured": coloured}


def test_extract_mesh_with_color(product):
    from bnv_fusion_amd import mesh, synthetic
    plain, m, frames = product["plain"], product["coloured"], product["frames"]
    assert plain.vertex_normals is None and plain.vertex_colors is None
    assert m.vertices.tobytes() == plain.vertices.tobytes() and m.faces.tobytes() == plain.faces.tobytes()
    V = len(m.vertices)
    assert m.vertex_colors.dtype == np.uint8 and m.vertex_colors.shape == (V, 3)
    assert m.vertex_normals.dtype == np.float32 and m.vertex_normals.shape == (V, 3)
    length = np.linalg.norm(m.vertex_normals.astype(np.float64), axis=1)
    assert (np.abs(length[length > 0] - 1.0) < 1e-6).all() and (length > 0).any()
    only = product["nm"].extract_mesh(post_process=VOXEL / 4, normals=True)
    assert only.vertex_colors is None and only.vertex_normals.tobytes() == m.vertex_normals.tobytes()
    # the normals point to the side of the cameras that observed the vertex
    tv, tf = up(m.vertices), up(m.faces)
    observed = np.zeros(V, bool)
    x, n = m.vertices.astype(np.float64), m.vertex_normals.astype(np.float64)
    for fr in frames:
        seen = mesh.VertexColorer(tv, tf, max_depth=MAX_DEPTH).add([fr]).result()[1].cpu().numpy()
        assert (((fr["T_wc"][:3, 3][None] - x[seen]) * n[seen]).sum(1) > 0).all()
        observed |= seen
    colors, obs = mesh.color_vertices((tv, tf), frames, max_depth=MAX_DEPTH)
    assert (colors.cpu().numpy() == m.vertex_colors).all() and (obs.cpu().numpy() == observed).all()
    # the acceptance figure: closer to the field than the TSDF volume's nearest-voxel colour on ITS mesh
    err = np.abs(m.vertex_colors.astype(np.float64) - synthetic.surface_color(x))[observed].mean()
    tv_, _, _, tc = product["nm"].tsdf_vol.get_mesh()
    tsdf_err = np.abs(tc.astype(np.float64) - synthetic.surface_color(tv_.astype(np.float64))).mean()
    print(f"extract_mesh(color=frames): {V} vertices, observed {observed.mean():.4f}, mean colour error {err:.3f} "
          f"levels; TSDF mesh ({len(tv_)} vertices): {tsdf_err:.3f} levels")
    assert observed.mean() > 0.1            # (the cameras saw the surface the map was fused from: the stage does something)
    assert err < tsdf_err


def test_extract_mesh_color_options(product):
    nm, frames = product["nm"], product["frames"]
    assert not any("rgb" in fr for fr in nm.frames)
    with pytest.raises(ValueError, match="rgb"):
        nm.extract_mesh(post_process=VOXEL / 4, color=True)
    kept = nm.frames
    try:
        nm.frames = frames[:2]
        m = nm.extract_mesh(post_process=VOXEL / 4, color=True)
        assert m.vertex_colors is not None and (m.vertex_colors != 128).any()
    finally:
        nm.frames = kept
    small = nm.extract_mesh(post_process=VOXEL / 4, min_component_area=0.01, color=frames)
    same = nm.extract_mesh(post_process=VOXEL / 4, min_component_area=0.01)
    assert small.vertices.tobytes() == same.vertices.tobytes() and small.faces.tobytes() == same.faces.tobytes()
    assert small.vertex_colors.shape == (len(small.vertices), 3) and small.vertex_normals.shape == small.vertices.shape
