"""Both multi-GPU modes of bnv_fusion_amd.distributed as REAL process groups on the GPU: world = 2 to MAX_WORLD
processes that share the one GPU of the test box (gloo transport; RCCL needs one GPU per rank -- the 8-GPU RCCL run
is the bench's), every rank on the HIP path.  The outputs of all ranks together must be bit-identical (torch.equal)
to the single-GPU NeuralMap on the same frames.  Needs a real MI355X: run with  -m gpu."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# the largest world that shares the test GPU: no more than six processes may hold it at once, and a launch of ``world``
# ranks from this (GPU-holding) process puts world + 2 of them on it
MAX_WORLD = 4


def _launch(world, mode, grid, frames, out, hw, checkpoint="fp32", ownership=None, _tries=3, extra=(), env_extra=None):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, BNV_DIST_BACKEND="gloo", OMP_NUM_THREADS="4", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.update(env_extra or {})
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    # children, not an exec of this (GPU-initialised) process
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_gpu_worker.py"),
           "--mode", mode, "--grid", str(grid), "--frames", str(frames), "--height", str(hw[0]), "--width", str(hw[1]),
           "--checkpoint", checkpoint, "--out", str(out)] + (["--ownership", ownership] if ownership else []) + list(extra)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0 and _tries > 1 and "EADDRINUSE" in (r.stdout + r.stderr):
        # the free port found above was taken before the rendezvous store listened on it: once more with another
        return _launch(world, mode, grid, frames, out, hw, checkpoint, ownership, _tries - 1, extra, env_extra)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [torch.load(os.path.join(out, f"rank{k}.pt"), weights_only=False) for k in range(world)]


def _single(grid, frames, hw, checkpoint="fp32"):
    import bnv_fusion_amd as bnv
    from bnv_fusion_amd import synthetic
    bnv.set_mlp_mode(1)
    dims, voxel = synthetic.GRID_DIMS[grid]
    model = bnv.load_pretrained(device=DEV, voxel_size=voxel, tiny_cuda=checkpoint == "tcnn")
    nm = bnv.NeuralMap(np.array([dims] * 3), voxel, model, device=DEV, tsdf=True)
    outs = []
    for t in range(frames):
        fr = {"depth": torch.from_numpy(synthetic.depth_u16(t, *hw)).to(DEV), "intr_mat": synthetic.intrinsics(*hw),
              "T_wc": synthetic.pose(t)}
        c, s = nm.fuse_and_decode(fr)
        outs.append((c.cpu(), s.cpu()))
    return outs, nm.volume.num_rows(), nm.tsdf_vol.tsdf.cpu(), voxel


@pytest.fixture(scope="module")
def single_512():
    return _single(512, 10, (480, 640))


@pytest.fixture(scope="module")
def single_256():
    return _single(256, 12, (240, 320))


def _model_of_run(world, ownership, grid, n_frames, hw, block_log2, axis):
    """tools/shard_model.py's CPU model of the same run: the owner table after ``n_frames`` frames and the SDF-MLP
    evaluations every rank does for the last frame."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("shard_model", os.path.join(ROOT, "tools", "shard_model.py"))
    sm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sm)
    from bnv_fusion_amd import distributed as D, synthetic
    dim, voxel = synthetic.GRID_DIMS[grid]
    mn, mx, n = sm.world_range(dim, voxel)
    rule = D.OwnershipModel(ownership, world, n, block_log2, axis=axis)
    weight = np.zeros(int(n.prod()), dtype=np.float32)
    for t in range(n_frames):
        ids, cnt = D.touched_voxels(synthetic.frame(t, *hw)[0], mn, mx, voxel, n)
        coords = D.unflatten(ids, n)
        rule.frame(coords)
        emit = cnt >= 8
        weight[ids[emit]] += np.minimum(cnt[emit] / np.float32(32.0), np.float32(1.0)).astype(np.float32)
    ev = coords[emit]
    own = rule.owner(ev)
    ok = weight >= 8.0
    per = [len(np.unique(sm.lattice_entries(ev[own == r], ok, n)[0])) for r in range(world)]
    return rule, per


@pytest.mark.parametrize("world,ownership", [(2, "first_touch"), (4, "first_touch"), (4, "hash"), (4, "region"),
                                             (2, "region")])
def test_spatial_sharding_processes_equal_single_gpu(tmp_path, single_512, world, ownership):
    """BASELINE config 3 in miniature: 512^3 grid, full 640x480 frames, the active-voxel set sharded by blocks
    over ``world`` processes (all ownership rules), one all-gather of boundary records per frame."""
    ref, rows, tsdf, voxel = single_512
    ranks = _launch(world, "spatial", 512, len(ref), tmp_path, (480, 640), ownership=ownership)
    assert all(r["meta"]["ownership"] == ownership for r in ranks)
    if ownership != "hash":      # the same table on every rank, and it levels the load
        t0, l0 = ranks[0]["meta"]["owner_table"], ranks[0]["meta"]["owner_loads"]
        assert all(np.array_equal(r["meta"]["owner_table"], t0) and np.array_equal(r["meta"]["owner_loads"], l0)
                   for r in ranks)
        assert l0.max() <= (1.05 if ownership == "first_touch" else 1.15) * l0.mean(), l0
    if world == 4:
        # the CPU model that prices ownership rules (tools/shard_model.py) describes THIS run: same owner table, and
        # the SDF-MLP evaluations of every rank for the last frame -- real ghost rows, real exchange -- are the model's
        m0 = ranks[0]["meta"]
        rule, per = _model_of_run(world, ownership, 512, len(ref), (480, 640), m0["block_log2"], m0["axis"])
        if ownership != "hash":
            assert np.array_equal(m0["owner_table"], rule.table)
        got = [r["meta"]["mlp_evals"][len(ref) - 1] for r in ranks]
        assert all(abs(g - p) <= 0.005 * p + 16 for g, p in zip(got, per)), (got, per)
    for t, (rc, rs) in enumerate(ref):
        parts = [r["out"][t] for r in ranks]
        assert all(p[0] is not None and len(p[0]) > 0 for p in parts)              # every rank owns part of every frame
        coords = torch.cat([p[0] for p in parts])
        sdf = torch.cat([p[1] for p in parts])
        flat = (coords[:, 0] * 512 + coords[:, 1]) * 512 + coords[:, 2]
        order = torch.argsort(flat)
        assert torch.equal(coords[order], rc), t                                    # the shards partition the frame
        assert torch.equal(sdf[order], rs), t                                       # bit-identical SDF
    assert float((ref[-1][1] != voxel).float().mean()) > 0.05                       # and the decode is live
    sizes = [len(r["out"][len(ref) - 1][0]) for r in ranks]
    assert max(sizes) < {"first_touch": 1.10, "region": 1.20}.get(ownership, 1.35) * (sum(sizes) / world)   # the load is level
    for r in ranks:
        m = r["meta"]
        assert m["host_waits"] == len(ref)                                          # ONE host wait per frame
        assert torch.equal(m["tsdf"], tsdf)
        assert rows / world < m["rows"] < rows                                      # own rows + ghost rows
        per_frame = m["exchanged_bytes"] / len(ref)
        assert per_frame < 48 * 1.6 * len(ref[-1][0])                               # boundary records only, 48 B each


def test_spatial_sharding_with_frames_announced_ahead(tmp_path, single_512):
    """ShardedNeuralMap.fuse_and_decode_async(next_frame=...): every frame's encode is enqueued a frame ahead; the last
    frame announces one that never comes and abandon() drops it (bnv_frame_cancel) -- the outputs are the single
    GPU's, no slot stays busy."""
    ref, rows, tsdf, voxel = single_512
    ranks = _launch(2, "spatial", 512, len(ref), tmp_path, (480, 640), extra=["--ahead"])
    for t, (rc, rs) in enumerate(ref):
        coords = torch.cat([r["out"][t][0] for r in ranks])
        sdf = torch.cat([r["out"][t][1] for r in ranks])
        order = torch.argsort((coords[:, 0] * 512 + coords[:, 1]) * 512 + coords[:, 2])
        assert torch.equal(coords[order], rc) and torch.equal(sdf[order], rs), t
    assert all(r["meta"]["host_waits"] == len(ref) for r in ranks)


def test_spatial_sharding_max_world_512_full_frames(tmp_path, single_512):
    """BASELINE config 3's shape: 512^3 grid, 640x480 frames, the active-voxel set sharded over MAX_WORLD processes (they
    share this box's GPU over gloo; the 8-GPU RCCL run is the driver's), one all-gather of boundary records and one
    host wait per frame -- bit-identical to the single-GPU run."""
    ref, rows, tsdf, voxel = single_512
    world = MAX_WORLD
    ranks = _launch(world, "spatial", 512, len(ref), tmp_path, (480, 640))
    for t, (rc, rs) in enumerate(ref):
        parts = [r["out"][t] for r in ranks]
        assert all(p[0] is not None and len(p[0]) > 0 for p in parts)
        coords = torch.cat([p[0] for p in parts])
        sdf = torch.cat([p[1] for p in parts])
        order = torch.argsort((coords[:, 0] * 512 + coords[:, 1]) * 512 + coords[:, 2])
        assert torch.equal(coords[order], rc), t
        assert torch.equal(sdf[order], rs), t
    sizes = [len(r["out"][len(ref) - 1][0]) for r in ranks]
    assert max(sizes) < 1.35 * (sum(sizes) / world)
    for r in ranks:
        m = r["meta"]
        assert m["host_waits"] == len(ref) and torch.equal(m["tsdf"], tsdf)
        assert rows / world < m["rows"] < rows
        assert m["exchanged_bytes"] / len(ref) < 48 * 1.6 * len(ref[-1][0])


@pytest.mark.parametrize("world", [2, 4])
def test_frame_parallel_processes_equal_single_gpu(tmp_path, single_256, world):
    """Frame-parallel mode: ranks encode / decode different frames of a batch, replicated volume."""
    ref, rows, tsdf, voxel = single_256
    ranks = _launch(world, "frame", 256, len(ref), tmp_path, (240, 320))
    for t, (rc, rs) in enumerate(ref):
        c, s = ranks[t % world]["out"][t]
        assert torch.equal(c, rc) and torch.equal(s, rs), t
    for r in ranks:
        assert r["meta"]["rows"] == rows and torch.equal(r["meta"]["tsdf"], tsdf)


@pytest.mark.parametrize("world", [2, MAX_WORLD])
def test_tcnn_checkpoint_sharded_over_processes(tmp_path, world):
    """BASELINE config 4 in miniature: the reference's default tiny-cuda-nn (fp16) networks, 512^3 grid, the volume
    sharded over 2 and over MAX_WORLD processes -- bit-identical to the single-GPU run in the same arithmetic (the single GPU
    runs the block encoder with its per-wave LDS tables, the shards the per-tile encoder on their owned-pair lists:
    the integer sums make them agree bit for bit)."""
    ref, rows, tsdf, voxel = _single(512, 9, (240, 320), checkpoint="tcnn")
    ranks = _launch(world, "spatial", 512, len(ref), tmp_path, (240, 320), checkpoint="tcnn")
    for t, (rc, rs) in enumerate(ref):
        parts = [r["out"][t] for r in ranks if r["out"][t][0] is not None]
        coords = torch.cat([p[0] for p in parts])
        sdf = torch.cat([p[1] for p in parts])
        order = torch.argsort((coords[:, 0] * 512 + coords[:, 1]) * 512 + coords[:, 2])
        assert torch.equal(coords[order], rc) and torch.equal(sdf[order], rs), t
    import bnv_fusion_amd as bnv
    bnv.set_mlp_mode(1)


def test_max_world_ranks_both_modes(tmp_path, single_256):
    """The driver's scaling run uses 8 ranks; both modes as MAX_WORLD processes (sharing this box's GPU), 256^3, 320x240
    frames -- frame-parallel batches of MAX_WORLD frames plus a ragged last batch, and the MAX_WORLD-way sharded
    volume -- bit-identical to the single-GPU run."""
    world = MAX_WORLD
    ref, rows, tsdf, voxel = single_256 if len(single_256[0]) % world else _single(256, 10, (240, 320))
    assert len(ref) % world                                                     # a ragged last batch
    (tmp_path / "fp").mkdir()
    (tmp_path / "sp").mkdir()
    ranks = _launch(world, "frame", 256, len(ref), tmp_path / "fp", (240, 320))
    for t, (rc, rs) in enumerate(ref):
        c, s = ranks[t % world]["out"][t]
        assert torch.equal(c, rc) and torch.equal(s, rs), t
    assert all(r["meta"]["rows"] == rows and torch.equal(r["meta"]["tsdf"], tsdf) for r in ranks)
    ranks = _launch(world, "spatial", 256, len(ref), tmp_path / "sp", (240, 320))
    for t, (rc, rs) in enumerate(ref):
        parts = [r["out"][t] for r in ranks if r["out"][t][0] is not None]
        coords = torch.cat([p[0] for p in parts])
        sdf = torch.cat([p[1] for p in parts])
        order = torch.argsort((coords[:, 0] * 256 + coords[:, 1]) * 256 + coords[:, 2])
        assert torch.equal(coords[order], rc) and torch.equal(sdf[order], rs), t
    assert all(r["meta"]["host_waits"] == len(ref) and torch.equal(r["meta"]["tsdf"], tsdf) for r in ranks)
