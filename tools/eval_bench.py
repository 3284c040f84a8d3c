"""Timings and figures of the mesh evaluation (bnv_fusion_amd/evaluate.py) on one GPU -> one JSON document.

    python tools/eval_bench.py [--quick] [--json OUT]

speed: evaluate_meshes at 100k / 100k samples (end to end and per stage, HIP events after warm-up), the NN query
alone at 1M x 1M, vertices-only against the room-sweep mesh (512^3, --sweep-frames frames of sequence.py), and the
grid build's share of each (the same call with one query point).  quality: F1 at 2.5 cm on the pan scene
(40 frames of synthetic.depth_u16 at 256^3, gt_mesh("union") for precision, gt_mesh("common") for recall) for MLP
modes 0 / 1 / 3, the tiny-cuda-nn checkpoint, and before / after NeuralMap.optimize(200).  --quick: small sizes, for a
kernel trace (rocprofv3 --kernel-trace --stats -- python tools/eval_bench.py --quick)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bnv_fusion_amd as bnv  # noqa: E402

bnv.configure_runtime()
from bnv_fusion_amd import evaluate, sequence, synthetic  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def pan_map(model, n_frames=40, H=480, W=640):
    dims, voxel = synthetic.GRID_DIMS[256]
    nm = bnv.NeuralMap(np.array([dims] * 3), voxel, model, capacity=400000, device=DEV)
    for t in range(n_frames):
        fr = {"depth": torch.from_numpy(synthetic.depth_u16(t, H, W)).to(DEV), "intr_mat": synthetic.intrinsics(H, W),
              "T_wc": synthetic.pose(t)}
        nm.integrate(fr)
        nm.frames.append(fr)
    return nm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--sweep-frames", type=int, default=600)
    args = ap.parse_args()
    out = {"speed": {}, "quality": {}}
    gen = lambda: torch.Generator(device=DEV).manual_seed(0)   # noqa: E731
    gt_u, gt_c = synthetic.gt_mesh("union"), synthetic.gt_mesh("common")
    voxel = synthetic.GRID_DIMS[256][1]

    # ---- speed: evaluate_meshes 100k / 100k on the pan-scene mesh
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel)
    nm = pan_map(model, 8 if args.quick else 40)
    mesh = nm.extract_mesh()
    n = 20000 if args.quick else 100000
    pv = torch.from_numpy(mesh.vertices).to(DEV)
    pf = torch.from_numpy(mesh.faces.astype(np.int32)).to(DEV)
    gv = torch.from_numpy(gt_u.vertices).to(DEV)
    gf = torch.from_numpy(gt_u.faces.astype(np.int32)).to(DEV)
    sp = {"pred_mesh": [len(mesh.vertices), len(mesh.faces)], "gt_mesh": [len(gt_u.vertices), len(gt_u.faces)]}
    sp["evaluate_meshes_ms"] = timed(lambda: evaluate.evaluate_meshes((pv, pf), (gv, gf), n_samples=n, generator=gen()))
    P = evaluate.sample_surface(pv, pf, n, generator=gen())[0]
    G = evaluate.sample_surface(gv, gf, n, generator=gen())[0]
    sp["sample_pred_ms"] = timed(lambda: evaluate.sample_surface(pv, pf, n, generator=gen()))
    sp["sample_gt_ms"] = timed(lambda: evaluate.sample_surface(gv, gf, n, generator=gen()))
    sp["nn_pred_gt_ms"] = timed(lambda: evaluate.nn_d2(P, G))
    sp["nn_gt_pred_ms"] = timed(lambda: evaluate.nn_d2(G, P))
    sp["nn_build_only_ms"] = timed(lambda: evaluate.nn_d2(P[:1], G))
    out["speed"]["evaluate_100k"] = sp
    if not args.quick:
        # ---- NN alone at 1M x 1M (surface samples of the gt mesh against those of the pred mesh)
        P1 = evaluate.sample_surface(pv, pf, 1000000, generator=gen())[0]
        G1 = evaluate.sample_surface(gv, gf, 1000000, generator=gen())[0]
        big = {"nn_1m_ms": timed(lambda: evaluate.nn_d2(G1, P1), reps=3),
               "nn_1m_build_only_ms": timed(lambda: evaluate.nn_d2(G1[:1], P1), reps=3)}
        out["speed"]["nn_1m"] = big
        del P1, G1
        # ---- vertices-only against the room-sweep mesh
        dims, vx, scale = sequence.DIMS[512]
        snm = bnv.NeuralMap(np.array([dims] * 3), vx, model, capacity=100000, device=DEV, tsdf=True)
        snm.inputs_resident = True
        sequence.run(snm, sequence.sweep_frames(range(args.sweep_frames), scale=scale, device=DEV), pipelined=True,
                     checksums=False)
        smesh = snm.extract_mesh()
        sv = torch.from_numpy(smesh.vertices).to(DEV)
        sf = torch.from_numpy(smesh.faces.astype(np.int32)).to(DEV)
        sgt = sequence.gt_mesh(scale)
        sw = {"sweep_mesh": [len(smesh.vertices), len(smesh.faces)]}
        # vertices-only, the sweep mesh as the ground truth side (compute_chamfer.py --vertice_only) and as pred
        sw["vertices_only_ms"] = timed(lambda: evaluate.evaluate_meshes(sgt, (sv, sf), vertices_only=True,
                                                                        generator=gen()), reps=3)
        SV = sv
        Ps = evaluate.sample_surface(torch.from_numpy(sgt.vertices).to(DEV),
                                     torch.from_numpy(sgt.faces.astype(np.int32)).to(DEV), 100000, generator=gen())[0]
        sw["nn_all_vertices_vs_100k_ms"] = timed(lambda: evaluate.nn_d2(SV, Ps), reps=3)
        sw["nn_100k_vs_all_vertices_ms"] = timed(lambda: evaluate.nn_d2(Ps, SV), reps=3)
        sw["nn_100k_vs_all_vertices_build_only_ms"] = timed(lambda: evaluate.nn_d2(Ps[:1], SV), reps=3)
        res = evaluate.evaluate_meshes((sv, sf), sgt, generator=gen())
        sw["precision_vs_room_gt"] = res["accuracy"]
        out["speed"]["sweep"] = sw
        del snm, smesh, sv, sf

    # ---- quality on the pan scene
    def score(m):
        res = evaluate.evaluate_meshes(m, gt_u, gt_recall=gt_c, generator=gen())
        return dict(res, summary=evaluate.summary_line(res))

    q = out["quality"]
    q["pan_points_mode1_40f"] = None
    for mode in ((1,) if args.quick else (0, 1, 3)):
        mdl = bnv.load_pretrained(device=DEV, voxel_size=voxel).set_mlp_mode(mode)
        q[f"mlp_mode_{mode}"] = score(pan_map(mdl, 8 if args.quick else 40).extract_mesh())
    nmp = bnv.NeuralMap(np.array([synthetic.GRID_DIMS[256][0]] * 3), voxel, model, device=DEV)
    for t in range(8 if args.quick else 40):
        nmp.integrate({"input_pts": torch.from_numpy(synthetic.frame(t)).to(DEV)})
    q["pan_points_mode1_40f"] = score(nmp.extract_mesh())
    if not args.quick:
        tc = bnv.load_pretrained(device=DEV, voxel_size=voxel, tiny_cuda=True)
        q["tcnn"] = score(pan_map(tc).extract_mesh())
        nmo = pan_map(model)
        q["before_optimize"] = score(nmo.extract_mesh())
        t0 = time.perf_counter()
        nmo.optimize(200, last_frame=-1, ray_max_dist=3, generator=torch.Generator().manual_seed(1))
        torch.cuda.synchronize()
        q["optimize_200_s"] = time.perf_counter() - t0
        q["after_optimize_200"] = score(nmo.extract_mesh())
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(txt)


if __name__ == "__main__":
    main()
