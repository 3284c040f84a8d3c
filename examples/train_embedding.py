"""Trains the local shape embedding (point encoder + SDF decoder) on the GPU: the reference's src/train.py with the
fusion_pointnet model (training_global=False), batch 100, Adam lr 1e-3, StepLR(20000, 0.5) per epoch.

    python examples/train_embedding.py --data-dir DATA --epochs 10 --out runs/emb
    python examples/train_embedding.py --synthetic 20000 --epochs 2 --out /tmp/emb
    python examples/train_embedding.py --mesh chair.obj room.ply --voxel-size 0.02 --epochs 5 --out runs/emb

--data-dir: the reference's local-patch layout (<DATA>/local_shapes/{03001627,03636649}_noise/<seq>/*.pkl);
--synthetic N: N patches of analytic shapes with exact SDF (synthetic.local_patches), a tenth more held out for
validation; --mesh PATH [PATH ...] --voxel-size V [--noise S] [--n-samples N]: patches cut from the user's own meshes
(OBJ / PLY) on the GPU (patches.cut_local_patches: N surface samples per mesh, Gaussian position noise of S voxels,
exact mesh SDF as ground truth), every tenth patch held out for validation.  Prints the train and val loss per epoch; writes <out>/last.npz (load_pretrained(path=...),
run_e2e.py --weights) and <out>/last.ckpt (the reference's checkpoint layout).  --tiny-cuda: the reference's default
tiny-cuda-nn networks (tiny_cuda: True); the files are then in the pointnet_tcnn layout (run_e2e.py --tiny-cuda
--weights <out>/last.npz).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--data-dir")
    src.add_argument("--synthetic", type=int, metavar="N")
    src.add_argument("--mesh", nargs="+", metavar="PATH", help="OBJ / PLY meshes to cut patches from (needs --voxel-size)")
    ap.add_argument("--voxel-size", type=float, help="--mesh: lattice spacing of the patches, in the mesh's units")
    ap.add_argument("--noise", type=float, default=0.0, help="--mesh: position noise of the surface samples, in voxels")
    ap.add_argument("--n-samples", type=int, default=200000, help="--mesh: surface samples per mesh")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=100)
    ap.add_argument("--init", default="scratch", help="scratch | pretrained | PATH (.npz)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--M", type=int, default=256, help="--synthetic / --mesh: training points per patch")
    ap.add_argument("--tiny-cuda", action="store_true",
                    help="the reference's default tiny-cuda-nn networks (TcnnEmbeddingTrainer, pointnet_tcnn layout)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import bnv_fusion_amd as bnv
    bnv.configure_runtime()
    import numpy as np
    import torch
    from bnv_fusion_amd import datasets, synthetic, train, weights

    if args.init == "scratch":
        init = None
    elif args.init == "pretrained":
        init = weights.load_npz(weights.DEFAULT_TCNN if args.tiny_cuda else weights.DEFAULT_FP32)
    else:
        init = weights.load_npz(args.init)
    cls = train.TcnnEmbeddingTrainer if args.tiny_cuda else train.EmbeddingTrainer
    trainer = cls(init, seed=args.seed, lr=args.lr, device="cuda:0")
    rng = np.random.default_rng(args.seed)

    if args.synthetic:
        d = synthetic.local_patches(args.synthetic, args.M, seed=args.seed, noise=0.02)
        v = synthetic.local_patches(max(1, args.synthetic // 10), args.M, seed=args.seed + 1, noise=0.02)
        keys = ("input_pts", "training_pts", "gt")
        data = {k: d[k] for k in keys}
        val = [{k: v[k] for k in keys}]

        def train_batches():
            order = rng.permutation(args.synthetic)
            for s in range(0, len(order), args.batch_size):
                ids = np.sort(order[s: s + args.batch_size])
                yield {k: data[k][ids] for k in keys}
    elif args.mesh:
        if not args.voxel_size or args.voxel_size <= 0:
            sys.exit("--mesh needs --voxel-size V (> 0)")
        from bnv_fusion_amd import mesh as mesh_io, patches
        gen = torch.Generator(device="cuda:0").manual_seed(args.seed)
        sets = []
        for path in args.mesh:
            t0 = time.perf_counter()
            m = mesh_io.load_obj(path) if path.lower().endswith(".obj") else mesh_io.load_ply(path)
            p = patches.cut_local_patches(m, args.voxel_size, args.n_samples, M=args.M, noise=args.noise,
                                          generator=gen, device="cuda:0")
            torch.cuda.synchronize()
            print(f"{path}: {len(m.faces)} faces -> {p.stats} in {time.perf_counter() - t0:.2f}s", flush=True)
            sets.append(p)
        # (set, patch) of every patch; every tenth is held out
        index = np.concatenate([np.stack([np.full(len(p), k), np.arange(len(p))], 1) for k, p in enumerate(sets)])
        held = np.arange(len(index)) % 10 == 9
        train_ids, val_ids = index[~held], index[held]
        if len(train_ids) == 0:
            sys.exit("the meshes gave no training patches: more samples or a larger --voxel-size")

        def gather(ids):
            parts = [sets[k].batch(torch.from_numpy(ids[ids[:, 0] == k, 1]), generator=gen)
                     for k in range(len(sets)) if np.any(ids[:, 0] == k)]
            return {key: torch.cat([b[key] for b in parts]) for key in ("input_pts", "training_pts", "gt")}

        val = [gather(val_ids[s: s + 500]) for s in range(0, len(val_ids), 500)]

        def train_batches():
            order = rng.permutation(len(train_ids))
            for s in range(0, len(order), args.batch_size):
                yield gather(train_ids[order[s: s + args.batch_size]])
    else:
        ds = datasets.LocalPatchDataset(args.data_dir, "train", seed=args.seed)
        vs = datasets.LocalPatchDataset(args.data_dir, "val", seed=args.seed)
        if len(ds) == 0:
            sys.exit(f"no training patches under {args.data_dir}/local_shapes")
        val = [vs[i] for i in range(len(vs))]

        def train_batches():
            return ds.batches(args.batch_size)

    os.makedirs(args.out, exist_ok=True)
    for epoch in range(args.epochs):
        t0 = time.perf_counter()
        losses = []
        for b in train_batches():
            if b["input_pts"].shape[0] * train.MIN_PTS_IN_GRID // 2 < 2:
                continue
            losses.append(trainer.step(**b)["loss"])
        train_loss = float(torch.stack(losses).mean()) if losses else float("nan")
        val_loss = float(np.mean([float(trainer.eval_loss(b)) for b in val])) if val else float("nan")
        trainer.end_epoch()
        print(f"epoch {epoch}: train_loss {train_loss:.5f}  val_loss {val_loss:.5f}  steps {len(losses)}  "
              f"lr {trainer.lr:.2e}  {time.perf_counter() - t0:.1f}s", flush=True)
    trainer.save_npz(os.path.join(args.out, "last.npz"))
    trainer.save_ckpt(os.path.join(args.out, "last.ckpt"))
    print(f"wrote {os.path.join(args.out, 'last.npz')} and last.ckpt")


if __name__ == "__main__":
    main()
