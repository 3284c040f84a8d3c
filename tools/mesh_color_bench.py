"""Timings of the appearance stage of an extracted mesh (mesh.vertex_normals_tensors, mesh.VertexColorer) next to
the device post-process of the same mesh (mesh.post_process_mesh_tensors) -> one JSON document.

    python tools/mesh_color_bench.py [--sweep-frames N] [--grids 256] [--json OUT]

Mesh: the room sweep (sequence.py, its first N frames) extracted at each grid and post-processed on the device with
the vertex threshold voxel / 4, as run_e2e.py does.  Colour frames: 8 sweep frames at 480 x 640 whose colour image is
the procedural field of synthetic.surface_color at the depth image's points (scan.render_color).  Per mesh: V / T, and
in ms per call (HIP events, median of 5 after 2 warm-up calls; device tensors in and out) the post-process, the
normals, one accumulate launch of 8 frames (the launch alone: frames resident, structs built) and the resolve; the
observed share after those 8 frames.  For a kernel breakdown: rocprofv3 --kernel-trace --stats -- python
tools/mesh_color_bench.py"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bnv_fusion_amd as bnv  # noqa: E402

bnv.configure_runtime()
from bnv_fusion_amd import mesh as M, scan, sequence  # noqa: E402
from mesh_post_bench import DEV, sweep_mesh, timed  # noqa: E402


def color_frames(indices, scale):
    frames = []
    for fr in sequence.sweep_frames(indices, scale=scale, device=DEV):
        metres = fr["depth"].to(torch.float32) / 1000.0
        frames.append(dict(fr, rgb=scan.render_color(metres, fr["intr_mat"], fr["T_wc"], "procedural")))
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep-frames", type=int, default=600)
    ap.add_argument("--grids", default="256")
    ap.add_argument("--json")
    args = ap.parse_args()
    out = {}
    for grid in [int(g) for g in args.grids.split(",")]:
        raw, voxel = sweep_mesh(grid, args.sweep_frames)
        eps = voxel / 4
        v_in, f_in = torch.from_numpy(raw.vertices).to(DEV), torch.from_numpy(raw.faces).to(DEV)
        post_ms = timed(lambda: M.post_process_mesh_tensors(v_in, f_in, eps))
        v, f = M.post_process_mesh_tensors(v_in, f_in, eps)
        normals_ms = timed(lambda: M.vertex_normals_tensors(v, f))
        step = max(1, args.sweep_frames // M.COLOR_MAX_FRAMES)
        frames = color_frames(range(0, step * M.COLOR_MAX_FRAMES, step), sequence.DIMS[grid][2])
        colorer = M.VertexColorer(v, f)
        batch = [colorer._frame(fr) for fr in frames]
        accumulate_ms = timed(lambda: colorer._launch(batch))
        resolve_ms = timed(lambda: colorer.result())
        observed = M.VertexColorer(v, f, normals=colorer.normals).add(frames).result()[1]
        out[f"sweep_{grid}"] = {"frames": args.sweep_frames, "V": int(v.shape[0]), "T": int(f.shape[0]),
                                "post_process_ms": round(post_ms, 3), "normals_ms": round(normals_ms, 3),
                                "accumulate_8_frames_ms": round(accumulate_ms, 3), "resolve_ms": round(resolve_ms, 3),
                                "color_frames": len(frames), "image": list(frames[0]["rgb"].shape[:2]),
                                "observed_share": round(float(observed.float().mean()), 4)}
        print(json.dumps({f"sweep_{grid}": out[f"sweep_{grid}"]}), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
