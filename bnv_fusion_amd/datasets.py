"""The on-disk sequence layout the reference's ``fusion_inference_dataset`` reads
(src/datasets/fusion_inference_dataset.py:105-146; SURVEY.md section 8 f: data formats on the input side):

    <data_dir>/<scan_id>/depth/<i>.png          16-bit greyscale, millimetres (cv2.imread(path, -1) / 1000., common.py:93)
    <data_dir>/<scan_id>/pose/T_wc_<i>.txt      16 numbers on one line: camera-to-world, row-major
    <data_dir>/<scan_id>/pose/intr_mat_<i>.txt  9 (or 16) numbers on one line
    <data_dir>/<scan_id>/pose/dimensions.txt    3 numbers: the metric extent of the volume
    <data_dir>/<scan_id>/image/<i>.jpg          colour (decoded only on request: ``load_rgb=True``, for mesh colouring)

``ARKitDataset`` reads the other layout the reference offers (``FusionInferenceDatasetARKit``,
fusion_inference_dataset.py:242-306): an iPhone / iPad LiDAR capture exported by the *3D Scanner* app ("All Data"),

    <data_dir>/<scan_id>/depth_<n>.png    16-bit greyscale, millimetres (256x192 on current devices)
    <data_dir>/<scan_id>/conf_<n>.png     8-bit greyscale, ARKit depth confidence 0 / 1 / 2
    <data_dir>/<scan_id>/frame_<n>.jpg    colour, 1920x1440 (decoded only on request: ``load_rgb=True``)
    <data_dir>/<scan_id>/frame_<n>.json   cameraPoseARFrame (4x4, row-major, ARKit camera axes), intrinsics (3x3,
                                          row-major, of the 1920x1440 colour image)
    <data_dir>/<scan_id>/export.obj       the app's rough mesh: its bounds place the volume

and ``write_arkit_capture`` writes it.

``FusionInferenceDataset`` yields the frame dicts ``NeuralMap.integrate`` / ``fuse_and_decode_async`` take
(``depth`` as a uint16 tensor on the device: the GPU front end replaces the dataset's numpy unprojection).
OpenCV is not a dependency: the PNG container is parsed here (chunks + zlib), the scanline filters are reversed by
``bnv_png_unfilter`` in the shared library.  ``write_sequence`` produces the same layout (used by the tests and
``examples/run_e2e.py`` for a synthetic scene).
"""
import ctypes as C
import json
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib

_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def read_png16(path):
    """16-bit (or 8-bit) greyscale PNG -> numpy [H, W] uint16, like cv2.imread(path, -1)."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:8] != _PNG_SIG:
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos: pos + 8])
        body = data[pos + 8: pos + 8 + n]
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        pos += 12 + n
    if hdr is None:
        raise ValueError(f"{path}: no IHDR chunk")
    w, h, depth, colour, _, _, interlace = hdr
    if colour != 0 or depth not in (8, 16) or interlace != 0:
        raise ValueError(f"{path}: expected a non-interlaced 8/16-bit greyscale PNG (colour type {colour}, "
                         f"bit depth {depth}, interlace {interlace})")
    bpp = depth // 8
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    row = w * bpp
    if raw.size != h * (row + 1):
        raise ValueError(f"{path}: truncated image data")
    out = np.empty(h * row, dtype=np.uint8)
    lib = _lib.load()
    _lib.check(lib.bnv_png_unfilter(raw.ctypes.data_as(C.c_void_p), h, row, bpp, out.ctypes.data_as(C.c_void_p)),
               "bnv_png_unfilter")
    if bpp == 2:
        return out.view(">u2").reshape(h, w).astype(np.uint16)
    return out.reshape(h, w).astype(np.uint16)


def write_png16(path, image, filter_type=0, level=6):
    """numpy [H, W] uint16 -> 16-bit greyscale PNG.  ``filter_type`` 0..4 selects the scanline filter of every
    row (the tests write all five); ``level``: zlib compression level."""
    img = np.ascontiguousarray(np.asarray(image, dtype=np.uint16))
    h, w = img.shape
    if filter_type == 0:      # (fast path: no predictor arithmetic)
        raw = np.concatenate([np.zeros((h, 1), np.uint8), img.astype(">u2").view(np.uint8).reshape(h, 2 * w)],
                             axis=1).tobytes()
        return _write_png(path, w, h, raw, level)
    rows = img.astype(">u2").view(np.uint8).reshape(h, 2 * w).astype(np.int32)
    bpp = 2
    left = np.zeros_like(rows)
    left[:, bpp:] = rows[:, :-bpp]
    up = np.zeros_like(rows)
    up[1:] = rows[:-1]
    ul = np.zeros_like(rows)
    ul[1:, bpp:] = rows[:-1, :-bpp]
    if filter_type == 0:
        pred = 0
    elif filter_type == 1:
        pred = left
    elif filter_type == 2:
        pred = up
    elif filter_type == 3:
        pred = (left + up) >> 1
    elif filter_type == 4:
        p = left + up - ul
        pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    else:
        raise ValueError("filter_type must be 0..4")
    filt = ((rows - pred) & 0xFF).astype(np.uint8)
    raw = np.concatenate([np.full((h, 1), filter_type, np.uint8), filt], axis=1).tobytes()
    return _write_png(path, w, h, raw, level)


def write_png8(path, image, level=6):
    """numpy [H, W] uint8 -> 8-bit greyscale PNG (no scanline filter): an ARKit confidence map."""
    img = np.ascontiguousarray(np.asarray(image, dtype=np.uint8))
    h, w = img.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), img], axis=1).tobytes()
    return _write_png(path, w, h, raw, level, bit_depth=8)


def _write_png(path, w, h, raw, level, bit_depth=16):
    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    with open(path, "wb") as fh:
        fh.write(_PNG_SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bit_depth, 0, 0, 0, 0))
                 + chunk(b"IDAT", zlib.compress(raw, level)) + chunk(b"IEND", b""))
    return path


def _read_matrix(path):
    """read_pose (fusion_inference_dataset.py:123-128): one line of numbers -> square float32 matrix."""
    with open(path, "r") as fh:
        vals = np.asarray([float(t) for t in fh.read().splitlines()[0].split()])
    n = int(np.sqrt(len(vals)))
    return vals.reshape(n, n).astype(np.float32)


def read_rgb(path):
    """A colour image file -> uint8 [H, W, 3] (red, green, blue) on the host, decoded by Pillow, which is imported here
    and only here: nothing else in the package needs it."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError(f"load_rgb=True needs Pillow to decode {path} (import PIL failed: {e}); the depth path "
                          "does not") from None
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: missing -- the colour image of the frame (load_rgb=True)")
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def _scaled_intrinsics(intr, sy, sx):
    """Intrinsics of the same view resampled by (sy, sx), integer pixel coordinates being pixel centres:
    u' = (u + 0.5) s - 0.5."""
    out = np.asarray(intr, dtype=np.float64).copy()
    out[0, 0], out[0, 2] = out[0, 0] * sx, (out[0, 2] + 0.5) * sx - 0.5
    out[1, 1], out[1, 2] = out[1, 1] * sy, (out[1, 2] + 0.5) * sy - 0.5
    return out


def _plan_extent(dataset, plan_options):
    """``volume="plan"``: pass 1 of the volume planner (plan.VolumePlanner) over the dataset's own frames, served
    unaligned -> its Extent.  ``plan_options``: keyword arguments of VolumePlanner (trim, margin, align_yaw, up, ...);
    with ``align="manhattan"`` among them its pass 0 runs first and the frames are served in the scene's own axes."""
    from .plan import VolumePlanner
    planner = VolumePlanner(device=dataset.device, max_depth=dataset.max_depth, **(plan_options or {}))
    if planner.align == "manhattan":
        for k in range(len(dataset)):
            planner.add_normals(dataset[k])
        planner.manhattan()
    for k in range(len(dataset)):
        planner.add(dataset[k])
    return planner.extent()


def _volume_mode(volume):
    if volume not in ("file", "plan"):
        raise ValueError(f"volume {volume!r}: 'file' or 'plan'")
    return volume


class FusionInferenceDataset:
    """fusion_inference_dataset.py:105-146 for the per-frame path: ``dimensions`` and frames in order.  ``load_rgb``:
    every frame also carries ``rgb`` (uint8 [Hc, Wc, 3] on the host, ``image/<i>.jpg``) for
    mesh.VertexColorer, and ``rgb_intr_mat`` when the colour image is not of the depth image's size (the same view is
    assumed: the depth intrinsics rescaled).  ``volume="file"``: ``dimensions`` from ``pose/dimensions.txt``, poses as
    written (an origin-centred scene).  ``volume="plan"``: the file is not needed; ``dimensions`` and
    ``axis_align_mat`` are planned from the sequence's own frames (``plan_options``: keyword arguments of
    plan.VolumePlanner; ``extent``: its result) and every frame's ``T_wc`` is ``axis_align_mat @`` the written pose."""

    def __init__(self, data_dir, scan_id, skip_images=1, downsample_scale=1.0, max_depth=3.0, device="cuda:0",
                 num_images=None, load_rgb=False, volume="file", plan_options=None):
        self.load_rgb = bool(load_rgb)
        self.volume = _volume_mode(volume)
        self.axis_align_mat = None      # volume="plan": set below
        self.extent = None
        # max_depth: cfg.model.ray_tracer.ray_max_dist (fusion_inference_dataset.py:28; 3 m in
        # fusion_pointnet_model.yaml:43).  The frames carry the raw depth image; the cut-off is applied by the
        # kernels (NeuralMap(max_depth=dataset.max_depth)), where the reference's load_depth zeroes the image.
        self.root = os.path.join(data_dir, scan_id)
        self.scan_id = scan_id
        self.device = device
        self.max_depth = max_depth
        self.downsample_scale = float(downsample_scale)
        self.dimensions = None
        if self.volume == "file":
            with open(os.path.join(self.root, "pose", "dimensions.txt"), "r") as fh:
                self.dimensions = np.asarray([float(v) for v in fh.read().splitlines()[0].split()])
        n = len([f for f in os.listdir(os.path.join(self.root, "depth")) if f.endswith(".png")])
        if num_images is not None:
            n = min(n, int(num_images))
        self.indices = list(range(0, n, max(int(skip_images), 1)))
        if self.volume == "plan":
            self.extent = _plan_extent(self, plan_options)
            self.dimensions, self.axis_align_mat = self.extent.dimensions, self.extent.axis_align_mat

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, k):
        i = self.indices[k]
        depth = read_png16(os.path.join(self.root, "depth", f"{i}.png"))
        intr = _read_matrix(os.path.join(self.root, "pose", f"intr_mat_{i}.txt"))[:3, :3].copy()
        if self.downsample_scale != 1.0:
            # load_depth's dense mode (common.py:96-103): nearest-neighbour resize, intrinsics scaled (:135)
            depth = _resize_nearest(depth, self.downsample_scale)
            intr[:2, :3] *= self.downsample_scale
        frame = {
            "frame_id": i, "scene_id": self.scan_id, "max_depth": self.max_depth,
            "depth": torch.from_numpy(depth).to(self.device),
            "depth_path": os.path.join(self.root, "depth", f"{i}.png"),
            "intr_mat": intr.astype(np.float64),
            "T_wc": _read_matrix(os.path.join(self.root, "pose", f"T_wc_{i}.txt")).astype(np.float64),
        }
        if self.axis_align_mat is not None:
            frame["T_wc"] = self.axis_align_mat @ frame["T_wc"]
        if self.load_rgb:
            frame["rgb"] = read_rgb(os.path.join(self.root, "image", f"{i}.jpg"))
            if frame["rgb"].shape[:2] != depth.shape:
                frame["rgb_intr_mat"] = _scaled_intrinsics(intr, frame["rgb"].shape[0] / depth.shape[0],
                                                           frame["rgb"].shape[1] / depth.shape[1])
        return frame

    def __iter__(self):
        for k in range(len(self)):
            yield self[k]


def _resize_nearest(img, scale):
    """cv2.resize(img, (int(w * scale), int(h * scale)), interpolation=cv2.INTER_NEAREST): floor(dst * src / dst)."""
    h, w = img.shape
    rh, rw = int(h * scale), int(w * scale)
    ys = np.minimum((np.arange(rh) * (h / rh)).astype(np.int64), h - 1)
    xs = np.minimum((np.arange(rw) * (w / rw)).astype(np.int64), w - 1)
    return img[ys][:, xs]


# ARKit's camera looks down -z with y up; the reference's frames look down +z with y down (fusion_inference_dataset.py:
# 290-294).  Its own inverse.
_ARKIT_FLIP = np.diag([1.0, -1.0, -1.0, 1.0])
ARKIT_INTR_SCALE = 1 / 7.5      # colour intrinsics (1920x1440) -> depth intrinsics (256x192), hard-coded by the reference


def read_obj_vertices(path):
    """The ``v`` lines of a Wavefront OBJ file -> float64 [N, 3] (all the volume placement needs of the mesh)."""
    verts = []
    with open(path, "r") as fh:
        for line in fh:
            if line.startswith("v ") or line.startswith("v\t"):
                verts.append([float(t) for t in line.split()[1:4]])
    if not verts:
        raise ValueError(f"{path}: no vertices")
    return np.asarray(verts, dtype=np.float64)


class ARKitDataset:
    """FusionInferenceDatasetARKit (fusion_inference_dataset.py:242-306): an iPhone / iPad LiDAR capture, frames in the
    numeric order of their names (depth_10 after depth_9).  ``dimensions`` and ``axis_align_mat`` come from the
    bounds of ``export.obj`` (the volume is centred on them); poses are ``axis_align_mat @ cameraPoseARFrame @
    diag(1, -1, -1, 1)`` in float64; the colour intrinsics are scaled by ``intr_scale * downsample_scale``.

    Each frame dict is shaped like FusionInferenceDataset's (``depth`` uint16 on the device, ``intr_mat``, ``T_wc``,
    ...) and also carries the confidence map (``conf`` uint8 on the device) and ``conf_level``: NeuralMap keeps the
    pixels with ``0 < depth < max_depth`` and ``conf >= conf_level`` as points and as training rays; the normals and the
    TSDF side fusion see the range-masked depth, as in the reference.  ``skip_images`` (the reference ignores it for
    this layout) keeps every k-th frame; the default keeps all.  ``load_rgb``: every frame also carries ``rgb``
    (``frame_<n>.jpg``, uint8 [1440, 1920, 3] on the host) and ``rgb_intr_mat``, the file's own intrinsics.
    ``volume="plan"``: ``export.obj`` is not needed; ``dimensions`` and ``axis_align_mat`` are planned from the capture's
    own confidence-gated frames (``plan_options``: keyword arguments of plan.VolumePlanner, e.g. ``align_yaw=18``;
    ``extent``: its result)."""

    def __init__(self, data_dir, scan_id, confidence_level=2, max_depth=3.0, downsample_scale=1.0,
                 intr_scale=ARKIT_INTR_SCALE, skip_images=1, device="cuda:0", load_rgb=False, volume="file",
                 plan_options=None):
        self.load_rgb = bool(load_rgb)
        self.volume = _volume_mode(volume)
        self.extent = None
        self.root = os.path.join(data_dir, scan_id)
        self.scan_id = scan_id
        self.device = device
        self.confidence_level = int(confidence_level)
        self.max_depth = max_depth
        self.downsample_scale = float(downsample_scale)
        self.intr_scale = float(intr_scale)
        self.axis_align_mat = np.eye(4)
        self.dimensions = None
        if self.volume == "file":
            obj = os.path.join(self.root, "export.obj")
            if not os.path.exists(obj):
                raise FileNotFoundError(f"{obj}: missing -- the capture's rough mesh, whose bounds place the volume "
                                        "(volume=\"plan\" places it from the frames instead)")
            v = read_obj_vertices(obj)
            lo, hi = v.min(axis=0), v.max(axis=0)
            self.dimensions = hi - lo
            self.axis_align_mat[:3, 3] = -(lo + hi) / 2
        names = [f.split("_")[1].split(".")[0] for f in os.listdir(self.root) if f.startswith("depth_")]
        self.names = sorted(names, key=int)[:: max(int(skip_images), 1)]
        if self.volume == "plan":       # (the frames are served with the identity until the plan is there)
            self.extent = _plan_extent(self, plan_options)
            self.dimensions, self.axis_align_mat = self.extent.dimensions, self.extent.axis_align_mat

    def __len__(self):
        return len(self.names)

    def __getitem__(self, k):
        n = self.names[k]
        depth_path = os.path.join(self.root, f"depth_{n}.png")
        conf_path = os.path.join(self.root, f"conf_{n}.png")
        if not os.path.exists(conf_path):
            raise FileNotFoundError(f"{conf_path}: missing -- the depth confidence map of frame {n}")
        depth = read_png16(depth_path)
        conf = read_png16(conf_path).astype(np.uint8)
        with open(os.path.join(self.root, f"frame_{n}.json"), "r") as fh:
            cam = json.load(fh)
        T_wc = self.axis_align_mat @ np.asarray(cam["cameraPoseARFrame"], dtype=np.float64).reshape(4, 4) @ _ARKIT_FLIP
        intr = np.asarray(cam["intrinsics"], dtype=np.float64).reshape(3, 3)      # (a fresh array: scaled in place)
        color_intr = intr.copy()
        intr[:2, :3] *= self.intr_scale * self.downsample_scale
        if self.downsample_scale != 1.0:
            depth = _resize_nearest(depth, self.downsample_scale)
            conf = _resize_nearest(conf, self.downsample_scale)
        frame = {
            "frame_id": k, "scene_id": self.scan_id, "max_depth": self.max_depth,
            "depth": torch.from_numpy(depth).to(self.device),
            "conf": torch.from_numpy(conf).to(self.device), "conf_level": self.confidence_level,
            "depth_path": depth_path, "conf_path": conf_path,
            "intr_mat": intr, "T_wc": T_wc,
        }
        if self.load_rgb:
            frame["rgb"] = read_rgb(os.path.join(self.root, f"frame_{n}.jpg"))
            frame["rgb_intr_mat"] = color_intr
        return frame

    def __iter__(self):
        for k in range(len(self)):
            yield self[k]


def write_arkit_capture(data_dir, scan_id, depths_u16, confs_u8, intrinsics, poses, dimensions, center=(0.0, 0.0, 0.0),
                        intr_scale=ARKIT_INTR_SCALE, names=None, filter_type=0, level=6):
    """Writes a capture in the layout ARKitDataset reads: the inverse of the loader.  ``poses``: T_wc in the loader's
    frame (centred volume, +z forward); written as cameraPoseARFrame = translate(center) @ T_wc @ diag(1, -1, -1, 1).
    ``intrinsics`` (one 3x3, or one per frame) at depth resolution; written at colour resolution (rows 0-1 divided by
    ``intr_scale``).  ``export.obj`` is the box ``center +- dimensions / 2`` (8 vertices, 12 triangles): the loader
    recovers ``dimensions`` and ``axis_align_mat = translate(-center)`` from it.  ``names``: the frames' <n> (default
    0, 1, ...)."""
    root = os.path.join(data_dir, scan_id)
    os.makedirs(root, exist_ok=True)
    center = np.asarray(center, dtype=np.float64).reshape(3)
    half = np.asarray(dimensions, dtype=np.float64).reshape(3) / 2
    with open(os.path.join(root, "export.obj"), "w") as fh:
        for c in range(8):
            sgn = np.array([1.0 if c & 1 else -1.0, 1.0 if c & 2 else -1.0, 1.0 if c & 4 else -1.0])
            fh.write("v " + " ".join(repr(float(x)) for x in center + sgn * half) + "\n")
        quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
        for a, b, c, d in quads:
            fh.write(f"f {a + 1} {b + 1} {c + 1}\nf {a + 1} {c + 1} {d + 1}\n")
    unalign = np.eye(4)
    unalign[:3, 3] = center
    for i, (d, cf, T) in enumerate(zip(depths_u16, confs_u8, poses)):
        n = str(names[i]) if names is not None else str(i)
        write_png16(os.path.join(root, f"depth_{n}.png"), d, filter_type, level)
        write_png8(os.path.join(root, f"conf_{n}.png"), cf, level)
        K = np.array(intrinsics[i] if np.ndim(intrinsics) == 3 else intrinsics, dtype=np.float64).reshape(3, 3)
        K[:2, :3] /= intr_scale
        pose = unalign @ np.asarray(T, dtype=np.float64).reshape(4, 4) @ _ARKIT_FLIP
        with open(os.path.join(root, f"frame_{n}.json"), "w") as fh:
            json.dump({"cameraPoseARFrame": [float(x) for x in pose.reshape(-1)],
                       "intrinsics": [float(x) for x in K.reshape(-1)]}, fh)
    return root


def write_sequence(data_dir, scan_id, depths_u16, intrinsics, poses, dimensions, filter_type=4, level=6):
    """Writes a sequence in the reference's layout (depth PNGs, pose / intrinsics / dimensions text files; one empty
    placeholder per colour image so that the reference's frame count -- len(os.listdir("image")) -- agrees).
    ``depths_u16`` / ``poses`` may be generators (a 2,000-frame sequence is never held in memory)."""
    root = os.path.join(data_dir, scan_id)
    for sub in ("depth", "pose", "image"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    with open(os.path.join(root, "pose", "dimensions.txt"), "w") as fh:
        fh.write(" ".join(repr(float(v)) for v in dimensions) + "\n")
    for i, (d, T) in enumerate(zip(depths_u16, poses)):
        write_png16(os.path.join(root, "depth", f"{i}.png"), d, filter_type, level)
        K = np.asarray(intrinsics[i] if np.ndim(intrinsics) == 3 else intrinsics, dtype=np.float64)
        with open(os.path.join(root, "pose", f"intr_mat_{i}.txt"), "w") as fh:
            fh.write(" ".join(repr(float(v)) for v in K.reshape(-1)) + "\n")
        with open(os.path.join(root, "pose", f"T_wc_{i}.txt"), "w") as fh:
            fh.write(" ".join(repr(float(v)) for v in np.asarray(T, dtype=np.float64).reshape(-1)) + "\n")
        open(os.path.join(root, "image", f"{i}.jpg"), "wb").close()
    return root


# --------------------------------------------------------------------------- #
# local shape patches for training the embedding (the reference's fusion_pointnet_dataset)
# --------------------------------------------------------------------------- #
PATCH_CATEGORIES = ("03001627_noise", "03636649_noise")
N_LOCAL_SAMPLES = 64


class _PatchUnpickler:
    """pickle.Unpickler that admits only dicts, lists, tuples, scalars and numpy arrays: a patch file cannot name
    any other class or function."""
    _ALLOWED = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
                ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
                ("numpy", "ndarray"), ("numpy", "dtype")}

    @classmethod
    def load(cls, fh):
        import importlib
        import pickle

        class U(pickle.Unpickler):
            def find_class(self, module, name):
                if (module, name) not in cls._ALLOWED:
                    raise pickle.UnpicklingError(f"patch files may not reference {module}.{name}")
                return getattr(importlib.import_module(module), name)
        return U(fh).load()


def read_local_patch(path):
    """One reference patch pickle: {input_pts [k, 6], center [1, 3], training_pts [M, 3], gt_sdf [M]}."""
    with open(path, "rb") as fh:
        data = _PatchUnpickler.load(fh)
    if not isinstance(data, dict) or not {"input_pts", "center", "training_pts", "gt_sdf"} <= set(data):
        raise ValueError(f"{path}: not a local patch (input_pts, center, training_pts, gt_sdf)")
    return data


def write_local_patches(data_dir, category, seq, patches):
    """Writes ``patches`` (dicts with input_pts [k, 6], center [1, 3], training_pts [M, 3], gt_sdf [M]) as
    <data_dir>/local_shapes/<category>/<seq>/<i>.pkl, the layout the reference's fusion_pointnet_dataset reads."""
    import pickle
    d = os.path.join(data_dir, "local_shapes", category, seq)
    os.makedirs(d, exist_ok=True)
    paths = []
    for i, p in enumerate(patches):
        path = os.path.join(d, f"{i:06d}.pkl")
        with open(path, "wb") as fh:
            pickle.dump({k: np.asarray(p[k]) for k in ("input_pts", "center", "training_pts", "gt_sdf")}, fh,
                        protocol=4)
        paths.append(path)
    return paths


class LocalPatchDataset:
    """The reference's FusionPointNetDataset (src/datasets/fusion_pointnet_dataset.py) for stage "train" / "val":
    <data_dir>/local_shapes/{03001627,03636649}_noise/<seq>/*.pkl; train = sorted(seqs)[10:] (one item per patch),
    val = sorted(seqs)[:10] (one item per sequence: up to 500 of its patches in random order, patches of fewer than
    16 points skipped).  ``input_pts`` is resized to 64 points as ``_resize_input_pts`` does: drawn with replacement
    to 64 when there are fewer, then the first 64 of a random permutation.  ``seed`` seeds the draws (the reference
    uses the global numpy / torch RNGs)."""

    def __init__(self, data_dir, stage, seed=0, n_local_samples=N_LOCAL_SAMPLES):
        if stage not in ("train", "val"):
            raise ValueError(f"stage {stage!r}: 'train' or 'val'")
        self.stage, self.n_local_samples = stage, n_local_samples
        self.rng = np.random.default_rng(seed)
        root = os.path.join(data_dir, "local_shapes")
        self.file_paths = []
        for cat in PATCH_CATEGORIES:
            seq_dir = os.path.join(root, cat)
            if not os.path.isdir(seq_dir):
                continue
            seqs = sorted(os.listdir(seq_dir))
            seqs = seqs[:10] if stage == "val" else seqs[10:]
            for seq in seqs:
                files = [os.path.join(seq_dir, seq, f) for f in sorted(os.listdir(os.path.join(seq_dir, seq)))]
                if stage == "val":
                    self.file_paths.append(files)
                else:
                    self.file_paths.extend(files)

    def __len__(self):
        return len(self.file_paths)

    def resize_input_pts(self, pts):
        pts = np.asarray(pts, np.float32)
        if len(pts) < self.n_local_samples:
            pts = pts[self.rng.integers(0, len(pts), self.n_local_samples)]
        return self.rng.permutation(pts)[: self.n_local_samples]

    def _item(self, data):
        return {"input_pts": self.resize_input_pts(data["input_pts"]),
                "sample_center": np.asarray(data["center"], np.float32)[0],
                "training_pts": np.asarray(data["training_pts"], np.float32),
                "gt": np.asarray(data["gt_sdf"], np.float32)}

    def __getitem__(self, idx):
        if self.stage == "train":
            return self._item(read_local_patch(self.file_paths[idx]))
        items = []
        for p in self.rng.permutation(np.array(self.file_paths[idx], dtype=object))[:500]:
            data = read_local_patch(p)
            if len(data["input_pts"]) < 16:
                continue
            items.append(self._item(data))
        return {k: np.stack([it[k] for it in items]) for k in ("input_pts", "sample_center", "training_pts", "gt")}

    def batches(self, batch_size, shuffle=True, drop_last=False):
        """Stacked batches of training items (train stage)."""
        order = self.rng.permutation(len(self)) if shuffle else np.arange(len(self))
        for s in range(0, len(order), batch_size):
            ids = order[s: s + batch_size]
            if drop_last and len(ids) < batch_size:
                break
            items = [self[int(i)] for i in ids]
            yield {k: np.stack([it[k] for it in items]) for k in ("input_pts", "training_pts", "gt")}
