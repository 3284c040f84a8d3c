"""Inputs shared by tests/test_cloud_cpu.py and tests/test_gpu_cloud.py: name -> (points fp32 [N, 3], origins fp32
[M, 3], origin_index or None, keyword arguments)."""
import numpy as np

CAMERA0 = np.array([[0.0, 0.0, -1.5]], dtype=np.float32)      # synthetic.pose(t)'s optical centre
ORIGINS3 = np.array([[0.0, 0.0, -1.5], [2.0, -1.0, 0.5], [-3.0, 0.5, 4.0]], dtype=np.float32)


def lattice(n=5):
    """n^3 integer points: every distance is exact in fp32 and most are shared by many pairs (ties)."""
    return np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def random_cloud(n, seed, flat=0.05):
    """A noisy slab: planes can be fitted everywhere."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, (n, 3))
    p[:, 2] = flat * rng.normal(size=n) + 0.3 * np.sin(2.0 * p[:, 0])
    return p.astype(np.float32)


def frame_points(H, W):
    from bnv_fusion_amd import synthetic
    return np.ascontiguousarray(synthetic.frame(0, H, W)[0])


def cluster_and_far(n_cluster=600, seed=5):
    """A tight cluster plus 20 points about a hundred cell edges away: for those 20 the k-th neighbour (k > 20) lies
    in the cluster, many rings out -- the stop test has to keep going and the search moves to the coarse grid."""
    rng = np.random.default_rng(seed)
    a = random_cloud(n_cluster, seed) * np.float32(0.05)
    b = (rng.normal(size=(20, 3)) * 0.002 + np.array([3.0, 2.0, 1.0])).astype(np.float32)
    p = np.concatenate([a, b]).astype(np.float32)
    return p[rng.permutation(len(p))]


def degenerate_cases():
    rng = np.random.default_rng(9)
    cases = {}
    for n in (1, 2, 5):
        cases[f"N={n}"] = (random_cloud(n, n), CAMERA0, None, dict(k=16))
    cases["coincident"] = (np.tile(np.array([[0.25, -0.5, 1.0]], np.float32), (40, 1)), CAMERA0, None, dict(k=16))
    t = np.arange(50, dtype=np.float32)
    cases["collinear"] = (np.stack([t, 2 * t, -t], 1).astype(np.float32), CAMERA0, None, dict(k=16))
    p = random_cloud(200, 3)
    p[[0, 17, 63, 64, 199]] = np.nan
    p[5, 1] = np.inf
    p[100, 0] = -np.inf
    cases["nan rows"] = (p, CAMERA0, None, dict(k=16))
    cases["all nan"] = (np.full((9, 3), np.nan, np.float32), CAMERA0, None, dict(k=8))
    cases["radius below spacing"] = (lattice(4), CAMERA0, None, dict(k=8, max_radius=0.5))
    cases["radius one spacing"] = (lattice(4), CAMERA0, None, dict(k=8, max_radius=1.0, min_neighbors=4))
    oi = rng.integers(0, 3, 150).astype(np.int32)
    oi[[3, 77]] = 3
    oi[10] = -1
    cases["bad origin index"] = (random_cloud(150, 4), ORIGINS3, oi, dict(k=10))
    big = random_cloud(300, 6) * np.float32(0.2)
    small = (random_cloud(4, 7) * np.float32(0.01) + np.float32(50.0)).astype(np.float32)
    cases["two clusters"] = (np.concatenate([big, small]), CAMERA0, None, dict(k=16, max_radius=1.0, min_neighbors=6))
    cases["two clusters, no radius"] = (np.concatenate([big, small]), CAMERA0, None, dict(k=16))
    return cases
