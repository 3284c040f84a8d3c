"""Cuts embedding-training patches from a triangle mesh on the GPU and writes them in the reference's local-patch
layout, <out>/local_shapes/<category>/<seq>/*.pkl, which the reference's own train.py and
examples/train_embedding.py --data-dir read.

    python examples/cut_patches.py chair.obj --out DATA --category 03001627_noise --seq chair_0001 --voxel-size 0.02

MESH: OBJ or PLY.  The reference's dataset reads the categories 03001627_noise and 03636649_noise and takes the first
ten sequences (sorted) of each as its validation set.  --noise S: Gaussian position noise of the surface samples, in
voxels (the reference's "_noise" data).  Patches whose ground truth has no trustworthy sign (an open mesh: a training
point closest to the mesh boundary) are dropped unless --keep-open.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh")
    ap.add_argument("--out", required=True, metavar="DATA_DIR")
    ap.add_argument("--category", required=True)
    ap.add_argument("--seq", required=True)
    ap.add_argument("--voxel-size", type=float, default=0.02)
    ap.add_argument("--n-samples", type=int, default=200000)
    ap.add_argument("--M", type=int, default=256, help="training points per patch")
    ap.add_argument("--noise", type=float, default=0.0)
    ap.add_argument("--min-pts", type=int, default=16)
    ap.add_argument("--max-pts", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--keep-open", action="store_true")
    args = ap.parse_args()

    import bnv_fusion_amd as bnv
    bnv.configure_runtime()
    import torch
    from bnv_fusion_amd import datasets, mesh as mesh_io, patches

    m = mesh_io.load_obj(args.mesh) if args.mesh.lower().endswith(".obj") else mesh_io.load_ply(args.mesh)
    t0 = time.perf_counter()
    p = patches.cut_local_patches(m, args.voxel_size, args.n_samples, M=args.M, noise=args.noise, min_pts=args.min_pts,
                                  max_pts=args.max_pts, generator=torch.Generator(device="cuda:0").manual_seed(args.seed),
                                  device="cuda:0", drop_open=not args.keep_open)
    torch.cuda.synchronize()
    cut_s = time.perf_counter() - t0
    if args.category not in datasets.PATCH_CATEGORIES:
        print(f"note: the reference's dataset reads only the categories {datasets.PATCH_CATEGORIES}", file=sys.stderr)
    paths = datasets.write_local_patches(args.out, args.category, args.seq, p.to_patch_dicts())
    print(f"{args.mesh}: {len(m.vertices)} vertices, {len(m.faces)} faces -> {p.stats} (cut in {cut_s:.2f}s); "
          f"wrote {len(paths)} patches under {os.path.join(args.out, 'local_shapes', args.category, args.seq)}")


if __name__ == "__main__":
    main()
