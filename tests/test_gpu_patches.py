"""The patch cutter (bnv_fusion_amd/patches.py) on the GPU: against an analytic box, the 2/4/8-fold pairing of samples
in lattice planes, open meshes, and the whole chain mesh -> patches -> trained embedding / pickles.

The distance tolerance is the one of tests/test_gpu_mesh_sdf.py: TOL_REL * 2^-23 * L."""
import numpy as np
import pytest
import torch

import mesh_sdf_restatement as R
from test_gpu_mesh_sdf import TOL_REL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _mesh(V, F):
    from bnv_fusion_amd.mesh import TriMesh
    return TriMesh(V, F)


def _box():
    return R.box_mesh((1.0, -0.5, 2.0), R.rotation(3), (0.31, 0.22, 0.17), n=6)


def test_cutter_against_an_analytic_box():
    from bnv_fusion_amd import patches, synthetic
    V, F, shape = _box()
    voxel, M = 0.02, 64
    kw = dict(voxel_size=voxel, n_samples=100000, M=M, noise=0.0, min_pts=16, max_pts=128, device=DEV)
    p = patches.cut_local_patches(_mesh(V, F), generator=_gen(7), **kw)
    P = len(p)
    off = p.offsets.cpu().numpy()
    cnt = np.diff(off)
    inp = p.input_pts.cpu().numpy().astype(np.float64)
    ctr = p.centers.cpu().numpy()
    q = p.training_pts.cpu().numpy().astype(np.float64)
    gt = p.gt.cpu().numpy().astype(np.float64)
    L = max(np.abs(V).max(), np.abs(ctr).max() + voxel)
    tol = TOL_REL * R.ULP32 * L
    print(f"\nbox: {p.stats}, {cnt.min()} .. {cnt.max()} points per patch, tolerance {tol:.3e}")
    # shapes, ranges, stats
    assert P > 1000 and off[0] == 0 and off[-1] == len(inp) and q.shape == (P, M, 3) and gt.shape == (P, M)
    assert cnt.min() >= 16 and cnt.max() <= 128
    assert np.abs(inp[:, :3]).max() <= 1.0 and np.abs(q).max() <= 1.0
    s = p.stats
    assert s["samples"] == 100000 and s["pairs"] == 8 * s["samples"]
    assert s["vertices_seen"] >= s["vertices_kept"] == s["patches"] + s["dropped_open"] and s["patches"] == P
    assert s["dropped_open"] == 0 and not bool(p.open.any())
    # the ground truth is the analytic box distance at centre + q * voxel, for every training point of every patch
    world = ctr[:, None, :] + q * voxel
    exact = synthetic.shape_sdf(shape, world.reshape(-1, 3)).reshape(P, M)
    err = np.abs(gt * voxel - exact)
    print(f"max |gt * voxel - analytic| = {err.max():.3e} = {err.max() / (R.ULP32 * L):.3f} x 2^-23 L")
    assert (err <= tol).all()
    assert (gt < 0).any() and (gt > 0).any()
    # every input point lies on the box, its normal is the normal of the face it lies on
    centre_of = np.repeat(ctr, cnt, axis=0)
    pos = centre_of + inp[:, :3] * voxel
    assert (np.abs(synthetic.shape_sdf(shape, pos)) <= tol).all()
    loc = (pos - shape["center"]) @ shape["rotation"]
    n_loc = inp[:, 3:] @ shape["rotation"]
    axis = np.abs(n_loc).argmax(1)
    k = np.arange(len(inp))
    assert (np.abs(np.abs(n_loc[k, axis]) - 1.0) <= 1e-6).all()
    assert (np.abs(loc[k, axis] - np.sign(n_loc[k, axis]) * shape["half"][axis]) <= tol).all()
    # the same generator seed gives the same bits; another seed does not
    again = patches.cut_local_patches(_mesh(V, F), generator=_gen(7), **kw)
    for name in ("offsets", "input_pts", "centers", "training_pts", "gt"):
        assert torch.equal(getattr(p, name), getattr(again, name)), name
    other = patches.cut_local_patches(_mesh(V, F), generator=_gen(8), **kw)
    assert other.input_pts.shape != p.input_pts.shape or not torch.equal(other.input_pts, p.input_pts)
    # batches: the shapes the trainers take, points of the right patch, the resize rule
    ids = torch.arange(0, P, max(P // 50, 1))
    b = p.batch(ids, generator=_gen(1))
    assert b["input_pts"].shape == (len(ids), 64, 6) and b["training_pts"].shape == (len(ids), M, 3)
    assert torch.equal(b["gt"], p.gt[ids.to(DEV)])
    for row, pid in enumerate(ids.tolist()):
        own = {tuple(r) for r in p.input_pts[off[pid]:off[pid + 1]].cpu().numpy().tolist()}
        got = [tuple(r) for r in b["input_pts"][row].cpu().numpy().tolist()]
        assert set(got) <= own
        if cnt[pid] >= 64:
            assert len(set(got)) == 64            # a permutation: no point twice
    assert torch.equal(p.batch(ids, generator=_gen(1))["input_pts"], b["input_pts"])


def test_samples_in_lattice_planes_count_2_4_8_fold():
    """An axis-aligned box whose faces lie in lattice planes (voxel and corners are powers of two: exact in fp32):
    every sample has an integer coordinate, so it pairs at least twice with each of its vertices."""
    from bnv_fusion_amd import evaluate, patches
    voxel, n, min_pts, max_pts = 0.0625, 20000, 16, 40
    V, F, _ = R.box_mesh((0.25, 0.25, 0.25), np.eye(3), (0.125, 0.125, 0.125), n=2)
    v = torch.from_numpy(V).to(DEV)
    f = torch.from_numpy(F.astype(np.int32)).to(DEV)
    p = patches.cut_local_patches(v, voxel, n, M=8, min_pts=min_pts, max_pts=max_pts, generator=_gen(3), faces=f)
    # the cutter's first draw is sample_surface's: the same generator state gives the same samples
    pts = evaluate.sample_surface(v, f, n, generator=_gen(3))[0].cpu().numpy().astype(np.float64)
    xn = pts / voxel
    lo, hi = np.floor(xn), np.ceil(xn)
    assert ((lo == hi).sum(1) >= 1).all()
    corners = np.stack([np.where(np.array(c, bool), hi, lo) for c in patches._CORNERS], 1).astype(np.int64)   # [n, 8, 3]
    verts, inv, with_mult = np.unique(corners.reshape(-1, 3), axis=0, return_inverse=True, return_counts=True)
    pairs = np.unique(np.stack([inv.reshape(-1), np.repeat(np.arange(n), 8)], 1), axis=0)
    distinct = np.bincount(pairs[:, 0], minlength=len(verts))
    assert with_mult.sum() == 8 * n and distinct.sum() <= 4 * n and (with_mult >= 2 * distinct).all()
    kept = with_mult >= min_pts
    assert p.stats["vertices_seen"] == len(verts) and p.stats["vertices_kept"] == kept.sum() == len(p)
    # np.unique sorts the vertices as the cutter's keys do: (x, y, z) lexicographic
    assert np.array_equal(p.centers.cpu().numpy(), verts[kept] * voxel)
    assert np.array_equal(p.counts().cpu().numpy(), np.minimum(distinct[kept], max_pts))
    assert (distinct[kept] < with_mult[kept]).all()
    # no point twice in a patch
    off = p.offsets.cpu().numpy()
    inp = p.input_pts.cpu().numpy()
    for k in range(0, len(p), max(len(p) // 40, 1)):
        rows = inp[off[k]:off[k + 1]]
        assert len(np.unique(rows, axis=0)) == len(rows)


def test_open_mesh_patches_are_dropped_and_counted():
    from bnv_fusion_amd import patches, synthetic
    m = synthetic.gt_mesh(step_px=8)
    kw = dict(voxel_size=0.04, n_samples=60000, M=32, device=DEV)
    p = patches.cut_local_patches(m, generator=_gen(5), **kw)
    k = patches.cut_local_patches(m, generator=_gen(5), drop_open=False, **kw)
    print(f"\nopen mesh: {p.stats}; kept and flagged: {k.stats}")
    assert p.stats["dropped_open"] > 0 and p.stats["patches"] == len(p) == p.stats["vertices_kept"] - p.stats["dropped_open"]
    assert not bool(p.open.any())
    assert k.stats["dropped_open"] == 0 and len(k) == k.stats["vertices_kept"] == p.stats["vertices_kept"]
    assert int(k.open.sum()) == p.stats["dropped_open"]
    keep = ~k.open
    assert torch.equal(k.gt[keep], p.gt) and torch.equal(k.centers[keep], p.centers)
    assert torch.equal(k.counts()[keep], p.counts())
    # a flagged patch holds a training point whose closest feature is on the rim of the mesh
    from bnv_fusion_amd import evaluate
    world = (k.centers[:, None, :] + k.training_pts.double() * 0.04).float()
    feature = evaluate.MeshSDF(m, device=DEV).query(world)[3]
    assert torch.equal(((feature & evaluate.FEATURE_BOUNDARY) != 0).any(1), k.open)


def _torus_and_box_patches(seed, n_samples):
    from bnv_fusion_amd import patches
    Vt, Ft = R.torus_mesh()
    Vb, Fb, _ = _box()
    return [patches.cut_local_patches(_mesh(Vt, Ft), 0.03, n_samples, M=128, generator=_gen(seed), device=DEV),
            patches.cut_local_patches(_mesh(Vb, Fb), 0.02, n_samples, M=128, generator=_gen(seed + 1), device=DEV)]


def _cat(batches):
    return {k: torch.cat([b[k] for b in batches]) for k in ("input_pts", "training_pts", "gt")}


@pytest.mark.parametrize("kind", ["fp32", "tcnn"])
def test_embedding_learns_from_cut_patches(kind):
    """200 steps from scratch on patches cut from the torus and the box: the loss on held-out patches of the same
    meshes (other samples, other training points) must be strictly below its value before training."""
    from bnv_fusion_amd import train
    sets = _torus_and_box_patches(21, 150000)
    held_sets = _torus_and_box_patches(99, 60000)
    g = _gen(0)
    held = _cat([s.batch(torch.arange(0, len(s), max(len(s) // 200, 1)), generator=g) for s in held_sets])
    t = (train.EmbeddingTrainer if kind == "fp32" else train.TcnnEmbeddingTrainer)(seed=0, device=DEV)
    before = float(t.eval_loss(held))
    rng = np.random.default_rng(0)
    for _ in range(200):
        parts = [s.batch(torch.from_numpy(rng.integers(0, len(s), 50)), generator=g) for s in sets]
        t.step(**_cat(parts))
    after = float(t.eval_loss(held))
    print(f"\n{kind}: {[len(s) for s in sets]} patches, held-out loss {before:.4f} -> {after:.4f} after 200 steps")
    assert np.isfinite(after) and after < before


def test_patch_dicts_round_trip_through_the_pickle_layout(tmp_path):
    from bnv_fusion_amd import datasets, patches
    V, F, _ = _box()
    p = patches.cut_local_patches(_mesh(V, F), 0.04, 20000, M=16, generator=_gen(2), device=DEV)
    dicts = p.to_patch_dicts()
    assert len(dicts) == len(p) > 20
    paths = datasets.write_local_patches(str(tmp_path), datasets.PATCH_CATEGORIES[0], "seq_a", dicts[:30])
    off = p.offsets.cpu().numpy()
    for k, path in enumerate(paths):
        d = datasets.read_local_patch(path)
        assert np.array_equal(d["input_pts"], p.input_pts[off[k]:off[k + 1]].cpu().numpy())
        assert d["center"].shape == (1, 3) and np.array_equal(d["center"][0], p.centers[k].cpu().numpy().astype(np.float32))
        assert np.array_equal(d["training_pts"], p.training_pts[k].cpu().numpy())
        assert np.array_equal(d["gt_sdf"], p.gt[k].cpu().numpy())
    # the reference's layout: the first ten sequences of a category are its validation set
    ds = datasets.LocalPatchDataset(str(tmp_path), "val", seed=0)
    item = ds[0]
    assert item["input_pts"].shape == (30, 64, 6) and item["training_pts"].shape == (30, 16, 3)
    assert item["gt"].shape == (30, 16)
