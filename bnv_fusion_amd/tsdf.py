"""TSDFVolume -- drop-in for the reference's third_parties/fusion.py:19-341 on MI355X
(SURVEY.md section 8 f-1).  Same constructor and ``integrate`` / ``get_volume`` / ``get_mesh`` / ``get_point_cloud``
surface; the volumes live on the GPU (``get_volume`` copies to host arrays like the reference's GPU mode does), and
marching cubes runs there too (csrc/mesh.hip, ``bnv_tsdf_mesh_*``).  ``meshwrite`` / ``pcwrite`` are the module
functions of fusion.py:366-426."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .mesh import _table, to_host


class TSDFVolume:
    def __init__(self, vol_bnds, voxel_size, use_gpu=True, device="cuda:0"):
        vol_bnds = np.asarray(vol_bnds, dtype=np.float64).copy()
        assert vol_bnds.shape == (3, 2), "[!] `vol_bnds` should be of shape (3, 2)."
        self._dev = torch.device(device)
        self._lib = _lib.require_device(self._dev.index or 0)
        self._vol_bnds = vol_bnds
        self._voxel_size = float(voxel_size)
        self._trunc_margin = 5 * self._voxel_size                      # fusion.py:36
        self._color_const = 256 * 256
        self._vol_dim = np.ceil((vol_bnds[:, 1] - vol_bnds[:, 0]) / self._voxel_size).copy(order="C").astype(int)
        self._vol_bnds[:, 1] = self._vol_bnds[:, 0] + self._vol_dim * self._voxel_size
        self._vol_origin = self._vol_bnds[:, 0].copy(order="C").astype(np.float32)
        dims = tuple(int(v) for v in self._vol_dim)
        # fusion.py:51-55: tsdf initialised to -trunc_margin (ones * 0 - margin), weights and colour to 0
        self.tsdf = torch.full(dims, -self._trunc_margin, dtype=torch.float32, device=self._dev)
        self.weight = torch.zeros(dims, dtype=torch.float32, device=self._dev)
        self.color = torch.zeros(dims, dtype=torch.float32, device=self._dev)
        self.gpu_mode = True

    def integrate(self, color_im, depth_im, cam_intr, cam_pose, obs_weight=1., max_depth=None, gate=None):
        """fusion.py:208-250.  depth_im [H, W] metres (numpy or tensor); color_im [H, W, 3] in [0, 255] or None.
        ``max_depth``: samples at or beyond it are invalid -- the reference's loader has already zeroed them when
        the frame reaches this call (common.py:110-113); here the raw image is passed and masked in the kernel.
        ``gate``: device int32 tensor; the launch does nothing when it holds 0 (pipelined NeuralMap: the frame's
        in-bounds point count, which the reference tests on the host before this call, run_e2e.py:91-92)."""
        depth = torch.as_tensor(depth_im)
        u16 = depth.dtype in (torch.uint16, torch.int16)     # the dataset's millimetres: converted in the kernel
        depth = depth.to(self._dev).contiguous() if u16 else depth.to(self._dev, torch.float32).contiguous()
        im_h, im_w = int(depth.shape[0]), int(depth.shape[1])
        col = self._fold_color(color_im)
        dim = (C.c_int32 * 3)(*[int(v) for v in self._vol_dim])
        org = (C.c_float * 3)(*self._vol_origin.tolist())
        intr = (C.c_float * 9)(*np.asarray(cam_intr, dtype=np.float64)[:3, :3].reshape(-1).astype(np.float32).tolist())
        pose = (C.c_float * 16)(*np.asarray(cam_pose, dtype=np.float64).reshape(-1).astype(np.float32).tolist())
        _lib.check(self._lib.bnv_tsdf_integrate(
            _lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.color if col is not None else None), dim, org,
            np.float32(self._voxel_size), np.float32(self._trunc_margin), _lib.ptr(depth), 0 if u16 else 1,
            _lib.ptr(col), im_h, im_w, intr, pose, float(obs_weight), float(max_depth or 0.0), _lib.ptr(gate),
            _lib.stream_ptr()), "bnv_tsdf_integrate")

    def _fold_color(self, color_im):
        """[H, W, 3] colour in [0, 255] -> the folded b*65536 + g*256 + r image of fusion.py:223-224 (or None)."""
        if color_im is None:
            return None
        c = torch.as_tensor(color_im).to(self._dev, torch.float32)
        return torch.floor(c[..., 2] * self._color_const + c[..., 1] * 256 + c[..., 0]).contiguous()

    BATCH_MAX = 8     # BNV_TSDF_BATCH_MAX

    def integrate_batch(self, depth_ims, cam_intrs, cam_poses, obs_weight=1., max_depth=None, color_ims=None):
        """``integrate`` for several consecutive uint16-millimetre depth frames of one size (``color_ims``: their colour
        images or None, per frame), one launch per BATCH_MAX frames; results identical to one call per frame in order."""
        ims = [torch.as_tensor(d) for d in depth_ims]
        if not ims:
            return
        cols = list(color_ims) if color_ims is not None else [None] * len(ims)
        if any(d.dtype not in (torch.uint16, torch.int16) or d.shape != ims[0].shape for d in ims):
            for d, k, p, c in zip(ims, cam_intrs, cam_poses, cols):
                self.integrate(c, d, k, p, obs_weight, max_depth)
            return
        cols = [self._fold_color(c) for c in cols]
        have_col = any(c is not None for c in cols)
        ims = [d.to(self._dev).contiguous() for d in ims]
        im_h, im_w = int(ims[0].shape[0]), int(ims[0].shape[1])
        dim = (C.c_int32 * 3)(*[int(v) for v in self._vol_dim])
        org = (C.c_float * 3)(*self._vol_origin.tolist())
        for g0 in range(0, len(ims), self.BATCH_MAX):
            grp = ims[g0: g0 + self.BATCH_MAX]
            k = len(grp)
            intr = np.stack([np.asarray(c, dtype=np.float64)[:3, :3].reshape(-1).astype(np.float32)
                             for c in cam_intrs[g0: g0 + k]]).reshape(-1)
            pose = np.stack([np.asarray(p, dtype=np.float64).reshape(-1).astype(np.float32)
                             for p in cam_poses[g0: g0 + k]]).reshape(-1)
            cg = cols[g0: g0 + k]
            _lib.check(self._lib.bnv_tsdf_integrate_batch_u16(
                _lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.color if have_col else None), dim, org,
                np.float32(self._voxel_size), np.float32(self._trunc_margin), k,
                (C.c_void_p * k)(*[d.data_ptr() for d in grp]),
                (C.c_void_p * k)(*[(c.data_ptr() if c is not None else 0) for c in cg]) if have_col else None,
                im_h, im_w,
                (C.c_float * (9 * k))(*intr.tolist()), (C.c_float * (16 * k))(*pose.tolist()), float(obs_weight),
                float(max_depth or 0.0), _lib.stream_ptr()), "bnv_tsdf_integrate_batch_u16")

    def render_depth(self, T_wc, K, H, W, near=0.1, max_depth=3.0, step=0.5, normals=True):
        """Depth (and normal) image of the TSDF volume from camera pose ``T_wc`` with pinhole ``K``: the same rays,
        schedule (``step`` in TSDF voxels) and hit rule as SparseVolume.render_depth, on the trilinear TSDF of the
        observed voxels (weight > 0) -> (depth [H, W] f32, normals [H, W, 3] f32 or None).  Runs on the current
        stream: frames a NeuralMap still has in its pipeline update this volume on side streams, so render a map's
        TSDF volume through NeuralMap.render_tsdf, which waits for them."""
        from .render import camera_args
        t, km = camera_args(T_wc, K, H, W, near, max_depth, step)
        H, W = int(H), int(W)
        depth = torch.empty((H, W), dtype=torch.float32, device=self._dev)
        nrm = torch.empty((H, W, 3), dtype=torch.float32, device=self._dev) if normals else None
        dim = (C.c_int32 * 3)(*[int(v) for v in self._vol_dim])
        org = (C.c_float * 3)(*self._vol_origin.tolist())
        _lib.check(self._lib.bnv_tsdf_render_depth(
            _lib.ptr(self.tsdf), _lib.ptr(self.weight), dim, org, np.float32(self._voxel_size), t, km, H, W,
            float(near), float(max_depth), float(step), _lib.ptr(depth), _lib.ptr(nrm), _lib.stream_ptr()),
            "bnv_tsdf_render_depth")
        return depth, nrm

    def get_volume(self):
        return self.tsdf.cpu().numpy(), self.color.cpu().numpy()

    def _mesh(self, level, observed_only, faces=True, normals=True):
        """count -> the one host read of the totals -> emit.  -> (vertices, faces or None, normals or None, colors)."""
        dev, lib = self._dev, self._lib
        table = _table(dev)
        dim = (C.c_int32 * 3)(*[int(v) for v in self._vol_dim])
        nbytes = C.c_int64()
        _lib.check(lib.bnv_tsdf_mesh_workspace_bytes(dim, C.byref(nbytes)), "bnv_tsdf_mesh_workspace_bytes")
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        tsdf, weight, color = self.tsdf.contiguous(), self.weight.contiguous(), self.color.contiguous()
        _lib.check(lib.bnv_tsdf_mesh_count(_lib.ptr(tsdf), _lib.ptr(weight), dim, float(level), int(bool(observed_only)),
                                           _lib.ptr(table), _lib.ptr(ws), nbytes.value, _lib.ptr(totals),
                                           _lib.stream_ptr()), "bnv_tsdf_mesh_count")
        V, T = totals.tolist()                  # the one host read: the outputs have to be allocated
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        tris = torch.empty((T, 3), dtype=torch.int64, device=dev) if faces else None
        norms = torch.empty((V, 3), dtype=torch.float32, device=dev) if normals else None
        cols = torch.empty((V, 3), dtype=torch.uint8, device=dev)
        if V:
            org = (C.c_float * 3)(*self._vol_origin.tolist())
            _lib.check(lib.bnv_tsdf_mesh_emit(
                _lib.ptr(tsdf), _lib.ptr(weight), _lib.ptr(color), dim, org, np.float32(self._voxel_size),
                float(level), int(bool(observed_only)), _lib.ptr(table), _lib.ptr(ws), nbytes.value, V, T,
                _lib.ptr(verts), _lib.ptr(tris), _lib.ptr(norms), _lib.ptr(cols), _lib.stream_ptr()),
                "bnv_tsdf_mesh_emit")
        return verts, tris, norms, cols

    def mesh_tensors(self, level=0.0, observed_only=False):
        """Marching cubes over the TSDF on the GPU -> device tensors (vertices f32 [V, 3] world coordinates, faces i64
        [T, 3], normals f32 [V, 3], colors u8 [V, 3] r, g, b); the one host copy is the count read that sizes them.

        The mesh is welded: one vertex per grid edge whose end values straddle ``level``, shared by the cells around
        it, ordered by the linear index of the edge's lower grid point, then axis x, y, z; faces by the linear index of
        the cell's base, then table order -- the same on every run.  The triangulation inside ambiguous cells is that
        of mc_tables.TRI_TABLE, not Lewiner's (skimage's marching_cubes_lewiner, fusion.py:327); the vertex set is the
        same for both.  Normals are the np.gradient of the volume at the edge's ends, interpolated along the edge and
        normalised (a zero gradient gives a zero normal); they point toward increasing TSDF, the free-space side, as the
        face winding does.  scikit-image is not available here, so whether its normals have the same sign is not
        checked.  Colours: the colour volume at the rounded (half to even) index-space position, unfolded as
        fusion.py:331-337.

        observed_only (not in the reference): a cell emits triangles only when its 8 corners have weight > 0, and a
        vertex exists only when such a cell uses it.  The volume starts at -trunc_margin (fusion.py:50-51), so
        unobserved space reads as inside, and by default a surface appears wherever observed free space meets it; this
        option leaves that surface out.  A volume with a dimension below 2 gives an empty mesh."""
        return self._mesh(level, observed_only)

    def get_mesh(self, observed_only=False):
        """fusion.py:323-341 -> numpy (verts f32 [V, 3], faces i64 [T, 3], norms f32 [V, 3], colors u8 [V, 3]) at
        level 0; see ``mesh_tensors``."""
        return tuple(to_host(*self._mesh(0.0, observed_only)))

    def get_point_cloud(self, observed_only=False):
        """fusion.py:302-321 -> float32 [V, 6]: the mesh vertices (xyz) followed by their colours (rgb)."""
        verts, _, _, cols = self._mesh(0.0, observed_only, faces=False, normals=False)
        verts, cols = to_host(verts, cols)
        return np.hstack([verts, cols])

    def sdf_delta(self, truncated_dist, sdf_delta_weight=1.0):
        """NeuralMap.prepare_tsdf_volume (run_e2e.py:169-186) without leaving the GPU:
        tsdf * (voxel * 5), clipped to +-truncated_dist, times sdf_delta_weight -> [1, 1, X, Y, Z]."""
        v = self.tsdf * (self._voxel_size * 5)
        v = torch.clip(v[None, None], min=-truncated_dist, max=truncated_dist)
        return v * sdf_delta_weight


_CHUNK = 1 << 16           # rows formatted per write


def _write_rows(fh, line, rows):
    """``line % row`` for every row of the float64 array ``rows``, one formatting call per chunk of rows."""
    for s in range(0, len(rows), _CHUNK):
        part = rows[s: s + _CHUNK]
        fh.write((line * len(part)) % tuple(part.reshape(-1).tolist()))


def meshwrite(filename, verts, faces, norms, colors):
    """fusion.py:366-399: an ASCII PLY with x, y, z, nx, ny, nz (``%f``), red, green, blue (``%d``) per vertex and
    ``3 i j k`` per face."""
    verts, norms = np.asarray(verts).reshape(-1, 3), np.asarray(norms).reshape(-1, 3)
    colors, faces = np.asarray(colors).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    with open(filename, "w") as fh:
        fh.write("ply\nformat ascii 1.0\n")
        fh.write("element vertex %d\n" % verts.shape[0])
        fh.write("property float x\nproperty float y\nproperty float z\n")
        fh.write("property float nx\nproperty float ny\nproperty float nz\n")
        fh.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
        fh.write("element face %d\n" % faces.shape[0])
        fh.write("property list uchar int vertex_index\n")
        fh.write("end_header\n")
        # %d of an integral float64 prints the integer, as %d of the uint8 does
        _write_rows(fh, "%f %f %f %f %f %f %d %d %d\n",
                    np.hstack([verts.astype(np.float64), norms.astype(np.float64), colors.astype(np.float64)]))
        _write_rows(fh, "3 %d %d %d\n", faces.astype(np.int64))


def pcwrite(filename, xyzrgb):
    """fusion.py:402-426: an ASCII PLY with x, y, z (``%f``) and red, green, blue (``%d`` of the uint8 cast)."""
    xyzrgb = np.asarray(xyzrgb).reshape(-1, 6)
    xyz, rgb = xyzrgb[:, :3], xyzrgb[:, 3:].astype(np.uint8)
    with open(filename, "w") as fh:
        fh.write("ply\nformat ascii 1.0\n")
        fh.write("element vertex %d\n" % xyz.shape[0])
        fh.write("property float x\nproperty float y\nproperty float z\n")
        fh.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
        fh.write("end_header\n")
        _write_rows(fh, "%f %f %f %d %d %d\n", np.hstack([xyz.astype(np.float64), rgb.astype(np.float64)]))
