"""Restatement the mesh normals and colours (csrc/meshcolor.hip; include/bnv_fusion.h, "Mesh normals and colours") are
pinned to, in numpy float64 in the kernels' operation order: every line below is one IEEE rounding per operation.

``vertex_normals``: the integer normal sums in Python integers.  ``ColorState`` / ``accumulate`` / ``resolve``: the
per-frame loop and the resolve; ``accumulate`` also returns, per frame, why every vertex was used or skipped
(``USED`` ...), so that a test can show its planted cases occur.  ``occluder_distance``: an INDEPENDENT visibility test --
per vertex a ray to the camera against every triangle (``brute_force`` of tests/mesh_ray_restatement.py), no depth
image involved.  ``cube_mesh`` / ``scan``: a closed subdivided cube and a ray-cast RGB-D scan of a mesh to test with.
"""
import numpy as np

import mesh_ray_restatement as R

NORMAL_SCALE = 2 ** 48
AREA_LIMIT = 2.0 ** 12
# why a vertex took nothing from a frame (the first test that failed), or USED
USED, ZERO_NORMAL, Z_RANGE, OUT_OF_IMAGE, NO_NEIGHBOUR, VIEW, OUT_OF_COLOR = range(7)
# the restated colouring of tests/test_mesh_color_cpu.py's scene against the colour field, in levels, as measured there
# (test_colors_against_ground_truth): the bar of every test that compares colours with the field
MEAN_ERR, P99_ERR = 3.0884, 13.2501


def bits(a):
    """An array's bytes as integers, to compare floats bit for bit."""
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def soup():
    """A small mesh with a degenerate face, an unreferenced vertex and a pair of cancelling faces."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1],          # a tetrahedron corner: faces 0, 1
                  [2, 2, 2],                                            # 4: unreferenced
                  [3, 0, 0], [4, 0, 0], [3, 1, 0],                      # 5..7: a face and its mirror image cancel
                  [5, 5, 5], [6, 6, 6]], np.float32)                    # 8, 9: only a degenerate face touches them
    f = np.array([[0, 1, 2], [0, 2, 3], [5, 6, 7], [5, 7, 6], [8, 9, 9]], np.int64)
    return v, f


def area_limit_cases():
    """name -> (v, f, accepted): one face tiled up to the total area of 2^12 and one short of it.  4096 faces of area 1
    are 64 waves of the normals kernel, 8192 of area 0.5 are 128: every one of its 64 total slots is added to twice.
    In exact arithmetic (2^50 or 2^49 units per face) the total reaches 2^62 at 4096 and at 8192 faces, not before."""
    unit = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0]], np.float32)      # area 1
    half = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)      # area 0.5
    whole = np.array([[0, 0, 0], [128, 0, 0], [0, 64, 0]], np.float32)  # area 2^12 in one face
    tile = lambda n: np.tile(np.array([[0, 1, 2]], np.int64), (n, 1))
    return {"4095 of area 1": (unit, tile(4095), True), "4096 of area 1": (unit, tile(4096), False),
            "8191 of area 0.5": (half, tile(8191), True), "8192 of area 0.5": (half, tile(8192), False),
            "one face of area 2^12": (whole, tile(1), False)}


def _cross(v, f):
    p = np.asarray(v, np.float32).astype(np.float64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    e1, e2 = b - a, c - a
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return cx, cy, cz


def refused(v, f):
    """None, or why the input is refused: "finite", "index" or "area"."""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    if not np.isfinite(v).all():
        return "finite"
    if len(f) and (len(v) == 0 or f.min() < 0 or f.max() >= len(v)):
        return "index"
    if len(f):
        cx, cy, cz = _cross(v, f)
        area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
        if (area >= AREA_LIMIT).any() or sum(int(q) for q in np.rint(area * 2.0 ** 50)) >= 2 ** 62:
            return "area"
    return None


def normal_sums(v, f):
    """Python-integer sums [V][3] of rint(cross * 2^48) over the faces at each of their corners."""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    sums = [[0, 0, 0] for _ in range(len(v))]
    if len(f):
        q = [np.rint(c * float(NORMAL_SCALE)) for c in _cross(v, f)]
        for t in range(len(f)):
            qt = (int(q[0][t]), int(q[1][t]), int(q[2][t]))
            for k in range(3):
                s = sums[int(f[t, k])]
                s[0] += qt[0]
                s[1] += qt[1]
                s[2] += qt[2]
    return sums


def vertex_normals(v, f):
    """float32 [V, 3]: the sums as float64 (to nearest even), divided by their length; a zero sum stays (0, 0, 0)."""
    assert refused(v, f) is None
    sums = normal_sums(v, f)
    out = np.zeros((len(sums), 3), np.float32)
    for i, s in enumerate(sums):
        if s[0] == 0 and s[1] == 0 and s[2] == 0:
            continue
        assert max(abs(c) for c in s) < 2 ** 62
        x, y, z = np.float64(s[0]), np.float64(s[1]), np.float64(s[2])       # int -> float64: to nearest even
        length = np.sqrt((x * x + y * y) + z * z)
        out[i] = (np.float32(x / length), np.float32(y / length), np.float32(z / length))
    return out


class ColorState:
    def __init__(self, n):
        self.sums = np.zeros((n, 4), np.float64)      # sum_r, sum_g, sum_b, sum_w
        self.count = np.zeros(n, np.int32)


def _depth_metres(depth):
    depth = np.asarray(depth)
    depth = depth.reshape(depth.shape[-2], depth.shape[-1])
    if depth.dtype in (np.uint16, np.int16):
        return depth.view(np.uint16).astype(np.float64) / 1000.0
    assert depth.dtype == np.float32, depth.dtype
    return depth.astype(np.float64)


def _project(f, c, x, z, n, ok):
    """u = (f x) / z + c; in bounds: 0 <= u <= n - 1.  -> (inside, x0, x1, fu, u); indices are 0 where not ``ok``."""
    with np.errstate(all="ignore"):
        u = (f * x) / z + c
    inside = ok & (u >= 0.0) & (u <= float(n - 1))
    us = np.where(inside, u, 0.0)
    fl = np.floor(us)
    x0 = fl.astype(np.int64)
    x1 = np.minimum(x0 + 1, n - 1)
    return inside, x0, x1, us - fl, u


def accumulate(state, verts, normals, frames, depth_tol=0.02, cos_min=0.2, near=0.0, max_depth=3.0):
    """Adds ``frames`` (dicts: ``depth`` uint16 millimetres or float32 metres [H, W], ``rgb`` uint8 [Hc, Wc, 3],
    ``intr_mat``, ``T_wc``; optional ``rgb_intr_mat``, ``conf``, ``conf_level``) to ``state`` in the order given ->
    a list with one dict per frame: ``reason`` [V] (USED ...), ``u``, ``v``, ``z`` [V], ``n_pass`` [V] (passing
    neighbours), ``n_zero`` [V] (neighbours whose depth is 0)."""
    x = np.asarray(verts, np.float32).astype(np.float64)
    n = np.asarray(normals, np.float32).astype(np.float64)
    has_normal = (n != 0.0).any(axis=1)
    traces = []
    for fr in frames:
        D = _depth_metres(fr["depth"])
        H, W = D.shape
        rgb = np.asarray(fr["rgb"])
        assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
        Hc, Wc = rgb.shape[:2]
        K = np.asarray(fr["intr_mat"], np.float64).reshape(3, 3)
        Kc = np.asarray(fr["rgb_intr_mat"], np.float64).reshape(3, 3) if fr.get("rgb_intr_mat") is not None else K
        shared = (Hc, Wc) == (H, W) and all(Kc[i, j] == K[i, j] for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
        T_wc = np.asarray(fr["T_wc"], np.float64).reshape(4, 4)
        T = np.linalg.inv(T_wc)                          # the host's world-to-camera matrix (mesh.world_to_camera)
        centre = T_wc[:3, 3]
        conf = None if fr.get("conf") is None else np.asarray(fr["conf"]).reshape(H, W)
        level = int(fr.get("conf_level", 0))
        reason = np.full(len(x), -1, np.int64)

        def fail(ok, code):
            reason[(reason < 0) & ~ok] = code

        fail(has_normal, ZERO_NORMAL)
        # 1. camera point
        p = [((T[a, 0] * x[:, 0] + T[a, 1] * x[:, 1]) + T[a, 2] * x[:, 2]) + T[a, 3] for a in range(3)]
        ok = has_normal & (p[2] > near) & (p[2] < max_depth)
        fail(ok, Z_RANGE)
        # 2. depth projection
        in_u, xa, xb, fu, u = _project(K[0, 0], K[0, 2], p[0], p[2], W, ok)
        in_v, ya, yb, fv, v = _project(K[1, 1], K[1, 2], p[1], p[2], H, ok)
        ok = in_u & in_v
        fail(ok, OUT_OF_IMAGE)
        # 3. occlusion test
        gu, gv = 1.0 - fu, 1.0 - fv
        bw = [gu * gv, fu * gv, gu * fv, fu * fv]
        corners = [(ya, xa), (ya, xb), (yb, xa), (yb, xb)]
        n_pass, n_zero = np.zeros(len(x), np.int64), np.zeros(len(x), np.int64)
        for c, (yy, xx) in enumerate(corners):
            yy, xx = np.where(ok, yy, 0), np.where(ok, xx, 0)
            d = D[yy, xx]
            with np.errstate(invalid="ignore"):
                passed = np.isfinite(d) & (d > 0.0) & (d < max_depth) & (np.abs(d - p[2]) <= depth_tol)
            if conf is not None:
                passed &= conf[yy, xx].astype(np.int64) >= level
            bw[c] = np.where(passed, bw[c], 0.0)
            n_pass += passed & ok
            n_zero += (d == 0.0) & ok
        wsum = ((bw[0] + bw[1]) + bw[2]) + bw[3]
        ok = ok & (wsum > 0.0)
        fail(ok, NO_NEIGHBOUR)
        # 4. view weight
        d0, d1, d2 = centre[0] - x[:, 0], centre[1] - x[:, 1], centre[2] - x[:, 2]
        with np.errstate(all="ignore"):
            length = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
            cosv = ((n[:, 0] * d0 + n[:, 1] * d1) + n[:, 2] * d2) / length
            ok = ok & (cosv > cos_min)
            fail(ok, VIEW)
            wt = cosv / (p[2] * p[2])
            # 5. colour sample
            if shared:
                bw = [b / wsum for b in bw]
            else:
                in_u, xa, xb, fu, _ = _project(Kc[0, 0], Kc[0, 2], p[0], p[2], Wc, ok)
                in_v, ya, yb, fv, _ = _project(Kc[1, 1], Kc[1, 2], p[1], p[2], Hc, ok)
                ok = in_u & in_v
                fail(ok, OUT_OF_COLOR)
                gu, gv = 1.0 - fu, 1.0 - fv
                bw = [gu * gv, fu * gv, gu * fv, fu * fv]
                corners = [(ya, xa), (ya, xb), (yb, xa), (yb, xb)]
        reason[reason < 0] = USED
        assert ((reason == USED) == ok).all()
        idx = np.nonzero(ok)[0]
        px = [rgb[yy[idx], xx[idx]].astype(np.float64) for yy, xx in corners]            # [k, 3] each
        b = [w[idx] for w in bw]
        for ch in range(3):
            col = ((b[0] * px[0][:, ch] + b[1] * px[1][:, ch]) + b[2] * px[2][:, ch]) + b[3] * px[3][:, ch]
            state.sums[idx, ch] = state.sums[idx, ch] + wt[idx] * col
        state.sums[idx, 3] = state.sums[idx, 3] + wt[idx]
        state.count[idx] += 1
        traces.append({"reason": reason, "u": u, "v": v, "z": p[2], "n_pass": n_pass, "n_zero": n_zero})
    return traces


def resolve(state, fill=(128, 128, 128)):
    """-> (colors uint8 [V, 3] = rint(sum / sum_w), half to even, clamped; observed bool [V]); unobserved: ``fill``."""
    observed = state.count > 0
    colors = np.empty((len(observed), 3), np.uint8)
    colors[:] = np.asarray(fill, np.uint8)
    s = state.sums[observed]
    colors[observed] = np.clip(np.rint(s[:, :3] / s[:, 3:4]), 0.0, 255.0).astype(np.uint8)
    return colors, observed


def color_vertices(verts, faces, frames, normals=None, fill=(128, 128, 128), **kw):
    """The whole stage -> (colors, observed, state, traces)."""
    normals = vertex_normals(verts, faces) if normals is None else normals
    state = ColorState(len(verts))
    traces = accumulate(state, verts, normals, frames, **kw)
    colors, observed = resolve(state, fill)
    return colors, observed, state, traces


# ---- an independent visibility test and a scene to test with -----------------------------------------------------------
def occluder_distance(centre, verts, faces, t_min=1e-6, t_max=1.0 - 1e-9):
    """float64 [V]: the distance in metres from each vertex to the first triangle that the segment from the vertex to
    the camera centre meets strictly between its ends (the vertex's own triangles meet it at t = 0 and do not count);
    inf when nothing is in the way: the vertex is visible.  Brute force over every triangle, float64, no depth image."""
    o = np.asarray(verts, np.float32).astype(np.float64)
    d = np.asarray(centre, np.float64)[None] - o
    return R.brute_force(o, d, verts, faces, t_min=t_min, t_max=t_max)["t"] * np.linalg.norm(d, axis=1)


def cube_mesh(n=8, edge=0.8, centre=(0.0, 0.0, 0.0)):
    """A closed cube of ``edge`` metres, every face an n x n grid of two-triangle cells whose diagonals alternate (for an
    even n every edge vertex then has as much triangle area on one of its faces as on the other, and every corner on
    all three), vertices shared along the edges, faces wound outwards -> (vertices float32 [6 n^2 + 2, 3], faces int64
    [12 n^2, 3])."""
    index, verts, faces = {}, [], []

    def vid(key):
        if key not in index:
            index[key] = len(verts)
            verts.append(key)
        return index[key]

    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):             # b x c = +axis: wound towards +axis
                        k = [0, 0, 0]
                        k[axis], k[b], k[c] = side, i + di, j + dj
                        q.append(vid(tuple(k)))
                    tris = [(q[0], q[1], q[2]), (q[0], q[2], q[3])] if (i + j) % 2 == 0 else \
                        [(q[1], q[2], q[3]), (q[1], q[3], q[0])]
                    faces += tris if side == n else [(t[0], t[2], t[1]) for t in tris]
    v = (np.asarray(verts, np.float64) / n - 0.5) * edge + np.asarray(centre, np.float64)
    return v.astype(np.float32), np.asarray(faces, np.int64)


def look_at(eye, target, down=(0.0, 1.0, 0.0)):
    """Camera-to-world pose at ``eye`` looking at ``target`` (+z forward, +y along ``down`` as far as the view allows)."""
    eye, target, down = (np.asarray(a, np.float64) for a in (eye, target, down))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(down, z)
    if np.linalg.norm(x) < 1e-9:
        x = np.cross(np.roll(down, 1), z)
    x = x / np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def scan(verts, faces, poses, K, H, W, color_fn, depth_dtype=np.uint16):
    """Ray-cast RGB-D frames of a mesh in float64 (``camera_rays`` / ``brute_force``): z-depth as uint16 millimetres
    (rounded to nearest) or float32 metres, 0 where nothing is hit; ``rgb`` = rint(color_fn(hit point)), 0 there."""
    frames = []
    for i, T in enumerate(poses):
        o, d = R.camera_rays(K, T, H, W)                       # d has camera z = 1: t IS the z-depth
        t = R.brute_force(o, d, verts, faces)["t"]
        hit = np.isfinite(t)
        z = np.where(hit, t, 0.0)
        pts = o[None] + z[:, None] * d
        rgb = np.where(hit[:, None], np.clip(np.rint(color_fn(pts)), 0, 255), 0.0).astype(np.uint8).reshape(H, W, 3)
        depth = np.rint(z * 1000.0).astype(np.uint16) if depth_dtype == np.uint16 else z.astype(np.float32)
        frames.append({"frame_id": i, "depth": depth.reshape(H, W), "rgb": rgb,
                       "intr_mat": np.asarray(K, np.float64).copy(), "T_wc": np.asarray(T, np.float64).copy()})
    return frames
