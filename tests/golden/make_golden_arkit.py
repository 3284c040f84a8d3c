"""Golden vectors for the ARKit capture loader and its confidence gate, captured from the reference's own
FusionInferenceDatasetARKit (src/datasets/fusion_inference_dataset.py:242-306) and
IterableInferenceDataset._sample_key_frame (:365-420).

Build-container only (needs /root/reference):  python tests/golden/make_golden_arkit.py
A tiny capture (3 frames, 256x192, confidence 0 / 1 / 2 mixed, some depth beyond max_depth, a non-cubic export.obj)
is written with datasets.write_arkit_capture; the reference's __init__, read_extr_pose, read_intr_pose, read_mask and
read_depth then read it.  cv2.imread / cv2.resize and trimesh.load are absent from this image: the generation-time
stand-ins below decode the unfiltered PNGs the writer produces, resize by nearest neighbour (an identity at
downsample_scale 1) and collect an OBJ's ``v`` lines.  They live here and nowhere else.  World points go through
``geometry.depth2xyz`` / ``get_homogeneous`` as __getitem__ calls them (fusion_inference_dataset.py:67-68), with the
intrinsics handed over as float32 for the reason make_golden_frontend.py gives (numpy 1.x value-based casting).

Only DATA is written (tests/golden/arkit_capture.npz: the capture's files, byte for byte, and the expected values).
"""
import os
import sys
import tempfile
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import ref_shims  # noqa: E402

H, W = 192, 256
MAX_DEPTH = 3.0
CONF_LEVEL = 2
NAMES = [0, 7, 12]                 # depth_12 after depth_7: the numeric order
DIMS = np.array([2.7, 1.9, 1.3])   # non-cubic export.obj
CENTER = np.array([0.35, -0.2, 1.1])
SEED = 5
SAMPLING = 2000
PTS_FRAME = 1                      # the frame whose masked world points are recorded


def _imread(path, flags=-1):
    """cv2.imread(path, -1) for the non-interlaced, unfiltered greyscale PNGs datasets.write_png16 / write_png8 write."""
    data = open(path, "rb").read()
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n = int.from_bytes(data[pos: pos + 4], "big")
        kind, body = data[pos + 4: pos + 8], data[pos + 8: pos + 8 + n]
        if kind == b"IHDR":
            hdr = (int.from_bytes(body[0:4], "big"), int.from_bytes(body[4:8], "big"), body[8])
        elif kind == b"IDAT":
            idat.append(body)
        pos += 12 + n
    w, h, bits = hdr
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, -1)
    assert (raw[:, 0] == 0).all(), "stand-in decodes filter type 0 only"
    px = raw[:, 1:]
    return px.copy() if bits == 8 else px.reshape(h, w, 2).astype(np.uint16) @ np.array([256, 1], np.uint16)


def _resize(img, dsize, interpolation=None):
    w, h = dsize
    ih, iw = img.shape
    ys = np.minimum((np.arange(h) * (ih / h)).astype(np.int64), ih - 1)
    xs = np.minimum((np.arange(w) * (iw / w)).astype(np.int64), iw - 1)
    return img[ys][:, xs]


def _trimesh_load(path):
    v = [[float(t) for t in ln.split()[1:4]] for ln in open(path) if ln.startswith("v ")]
    return types.SimpleNamespace(vertices=np.asarray(v))


def _capture(root):
    from bnv_fusion_amd import datasets, synthetic
    rng = np.random.default_rng(3)
    depths, confs, poses = [], [], []
    for k, t in enumerate((0, 3, 6)):
        d = synthetic.depth_u16(t, H, W)
        d[20:40, 30:60] = 3200 + 10 * k                   # beyond max_depth
        d[100:104, 200:220] = 0                            # no depth
        c = rng.choice(np.array([0, 1, 2], np.uint8), size=(H, W), p=[0.1, 0.15, 0.75])
        T = synthetic.pose(t).copy()
        T[:3, 3] += [0.05 * k, -0.02 * k, 0.03]
        depths.append(d)
        confs.append(c)
        poses.append(T)
    datasets.write_arkit_capture(root, "scan", depths, confs, synthetic.intrinsics(H, W), poses, DIMS, center=CENTER,
                                 names=NAMES)
    return os.path.join(root, "scan")


def main():
    ref_shims.install()
    ref_shims.install_run_e2e()
    sys.modules["cv2"].imread = _imread
    sys.modules["cv2"].resize = _resize
    sys.modules["cv2"].INTER_NEAREST = 0
    sys.modules["trimesh"].load = _trimesh_load
    if not hasattr(np, "bool"):
        np.bool = bool                                     # the reference's numpy 1.x alias
    from src.datasets.fusion_inference_dataset import FusionInferenceDatasetARKit, IterableInferenceDataset
    from src.utils import geometry
    cfg = ref_shims.AttrDict(
        dataset=dict(scan_id="scan", skip_images=1, sample_shift=0, downsample_scale=1.0, img_res=[H, W],
                     num_pixels=5000, depth_scale=1000.0, confidence_level=CONF_LEVEL),
        model=dict(feature_vector_size=8, voxel_size=0.01, ray_tracer=dict(ray_max_dist=MAX_DEPTH)),
        trainer=dict(dense_volume=False))
    with tempfile.TemporaryDirectory() as tmp:
        root = _capture(tmp)
        cfg["dataset"]["data_dir"] = tmp
        ds = FusionInferenceDatasetARKit(cfg, "test")
        files = sorted(os.listdir(root))
        out = {"files": np.array(files), "conf_level": CONF_LEVEL, "max_depth": MAX_DEPTH,
               "dimensions": np.asarray(ds.dimensions, np.float64),
               "axis_align_mat": np.asarray(ds.axis_align_mat, np.float64),
               "order": np.array([int(os.path.basename(p)[len("depth_"):-len(".png")]) for p in ds.depth_paths])}
        for f in files:
            out["file:" + f] = np.frombuffer(open(os.path.join(root, f), "rb").read(), np.uint8)
        Ts, Ks, masks, pts, counts = [], [], [], [], []
        for i in range(len(ds.depth_paths)):
            T_wc = ds.read_extr_pose(ds.T_wc_paths[i])                                   # :287-295
            K = ds.read_intr_pose(ds.intr_mat_paths[i])[:3, :3]                          # :297-302
            depth, mask = ds.read_depth(ds.depth_paths[i])                               # :62
            mask = mask * ds.read_mask(ds.mask_paths[i])                                 # :63-64
            mask = mask.astype(bool)
            pts_c = geometry.depth2xyz(depth, K.astype(np.float32)).reshape(-1, 3)       # :67
            pts_w = (T_wc @ geometry.get_homogeneous(pts_c).T)[:3, :].T                  # :68
            Ts.append(T_wc)
            Ks.append(K)
            masks.append(mask)
            pts.append(pts_w[mask.reshape(-1)])
            counts.append(int(mask.sum()))
        # (the world points of one frame, rounded to float32 as run_e2e.py:249 does: the fixture stays small)
        out.update(T_wc=np.stack(Ts), intr_mat=np.stack(Ks), mask=np.stack(masks), counts=np.array(counts),
                   pts_frame=PTS_FRAME, pts_w=pts[PTS_FRAME].astype(np.float32))
        # the optimiser's key frame sampling of frame 0 under a fixed seed (:373-420)
        it = IterableInferenceDataset([], MAX_DEPTH, None, None, None, SAMPLING, confidence_level=CONF_LEVEL)
        meta = {"depth_path": ds.depth_paths[0], "mask_path": ds.mask_paths[0],
                "intr_mat": torch.from_numpy(Ks[0]).unsqueeze(0), "T_wc": torch.from_numpy(Ts[0]).unsqueeze(0)}
        torch.manual_seed(SEED)
        rays = it._sample_key_frame(meta)
        out.update(key_seed=SEED, key_sampling=SAMPLING, key_uv=rays["uv"][0].numpy(),
                   key_mask=rays["mask"][0].numpy(), key_neighbor_masks=rays["neighbor_masks"][0].numpy())
    np.savez_compressed(os.path.join(HERE, "arkit_capture.npz"), **out)
    print("arkit_capture:", files, "valid", counts, "order", out["order"],
          "key mask mean", float(out["key_mask"].mean()))


if __name__ == "__main__":
    main()
