"""Scores reconstructed meshes against ground-truth meshes on the GPU: the reference's metric (pred -> gt mean
distance, precision, gt -> pred mean distance, recall, F1 at 2.5 cm; bnv_fusion_amd/evaluate.py).

    python examples/evaluate_mesh.py --pred a.ply --gt b.ply [--vertices-only] [--normals]     # compute_chamfer.py
    python examples/evaluate_mesh.py --pred-dir PRED --gt-dir GT --file-name final.ply          # evaluate_bnvf.py
    python examples/evaluate_mesh.py --pred a.ply --gt b.ply --align [--align-guess POSE.txt]   # register, then score

Single-pair mode mirrors src/scripts/compute_chamfer.py; directory mode mirrors src/scripts/evaluate_bnvf.py: every
sequence directory of PRED with exactly one file whose name contains --file-name is scored against
GT/<sequence>/gt_mesh.ply, with the sequence's figures and the running averages.  Both print the reference's summary
line "pred_gt/accuracy/gt_pred/recall/F1".
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bnv_fusion_amd as bnv                                    # noqa: E402

bnv.configure_runtime()
from bnv_fusion_amd import evaluate                             # noqa: E402
from bnv_fusion_amd.mesh import load_ply                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pred")
    ap.add_argument("--gt")
    ap.add_argument("--vertices-only", action="store_true", help="ground truth = a random subset of its vertices")
    ap.add_argument("--normals", action="store_true", help="also the normal consistency (single-pair mode)")
    ap.add_argument("--pred-dir")
    ap.add_argument("--gt-dir")
    ap.add_argument("--file-name")
    ap.add_argument("--threshold", type=float, default=0.025)
    ap.add_argument("--n-samples", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", help="write the figures to this file")
    ap.add_argument("--align", action="store_true",
                    help="register the prediction to the ground-truth mesh first (point-to-mesh ICP)")
    ap.add_argument("--align-guess", metavar="POSE.txt",
                    help="with --align: a 4 x 4 text matrix, prediction -> ground truth, to start from (default identity)")
    args = ap.parse_args()
    if args.align_guess and not args.align:
        ap.error("--align-guess goes with --align")
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    kw = dict(n_samples=args.n_samples, threshold=args.threshold, vertices_only=args.vertices_only, generator=gen,
              device=dev)
    if args.align:
        kw["align"] = {"T_guess": np.loadtxt(args.align_guess).reshape(4, 4)} if args.align_guess else True

    def report_alignment(res):
        """Prints what --align did and makes the result JSON-ready."""
        from bnv_fusion_amd import register
        print(f"alignment: {register.STATUS_NAMES[res['align_status']]}; unaligned "
              f"{evaluate.summary_line(res['unaligned'])}")
        print(np.array2string(res["T_align"], precision=6, suppress_small=True))
        res["T_align"] = res["T_align"].tolist()

    if args.pred and args.gt:
        res = evaluate.evaluate_meshes(load_ply(args.pred), load_ply(args.gt), normals=args.normals, **kw)
        if args.align:
            report_alignment(res)
        print("pred -> gt: ", res["pred_gt"])
        print(f"precision @ {args.threshold}:", res["accuracy"])
        print("gt -> pred: ", res["gt_pred"])
        print(f"recall @ {args.threshold}:", res["recall"])
        print("F1: ", res["F1"])
        print(evaluate.summary_line(res))
        if args.normals:
            print(res["normal_consistency"])
        out = res
    elif args.pred_dir and args.gt_dir and args.file_name:
        if args.normals:
            ap.error("--normals is a single-pair option")
        out = {"sequences": {}, "average": {}}
        acc = {k: [] for k in evaluate.KEYS}
        for seq in sorted(os.listdir(args.pred_dir)):
            seq_dir = os.path.join(args.pred_dir, seq)
            if not os.path.isdir(seq_dir):
                continue
            files = [f for f in os.listdir(seq_dir) if args.file_name in f]
            if len(files) != 1:
                continue
            print(f"{seq}:")
            res = evaluate.evaluate_meshes(load_ply(os.path.join(seq_dir, files[0])),
                                           load_ply(os.path.join(args.gt_dir, seq, "gt_mesh.ply")), **kw)
            if args.align:
                report_alignment(res)
            for k in evaluate.KEYS:
                acc[k].append(res[k])
            out["sequences"][seq] = res
            out["average"] = {k: float(np.mean(v)) for k, v in acc.items()}
            print(evaluate.summary_line(res))
            print("sequence result:")
            print(*[res[k] for k in evaluate.KEYS])
            print("average result:")
            print(*[out["average"][k] for k in evaluate.KEYS])
        if not out["sequences"]:
            sys.exit(f"no sequence of {args.pred_dir} has exactly one file matching {args.file_name!r}")
    else:
        ap.error("give --pred and --gt, or --pred-dir, --gt-dir and --file-name")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
