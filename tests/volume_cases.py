"""Key sets on which a subtly wrong sparse-volume index cannot give the right answer (plain module, CPU only).

The volume finds a voxel's row through an open-addressing table: packed 64-bit key, home slot ``mix64(key) & mask``,
linear probing (csrc/volume.hip, csrc/volume_keys.hpp).  Random keys at <= 50 % load almost never probe more than a
few slots, so the generators here SEARCH a fixed cube of coordinates for keys with a chosen home slot: one family forms
one probe chain, and a family whose home is the table's last slot forms a chain that wraps to slot 0.  Everything is
deterministic: the cube is walked in lexicographic (x, y, z) order and the keys come back in that order.

``pack_key`` and ``home`` restate csrc/volume_keys.hpp in numpy; ``mix64`` is the package's own host restatement.
tests/test_volume_cases_cpu.py checks what the GPU tests (tests/test_gpu_volume_index.py) rely on.
"""
import numpy as np

from bnv_fusion_amd.distributed import mix64

KEY_OFFSET = 1 << 20        # kKeyOffset
KEY_LIMIT = 1 << 21         # an axis is valid when 0 <= x + KEY_OFFSET < KEY_LIMIT
CUBE = 128                  # the generators search [0, CUBE)^3
RANGE_EDGE_VALUES = (-(1 << 20), -(1 << 20) + 1, -1, 0, (1 << 20) - 2, (1 << 20) - 1)


def pack_key(coords):
    """coords [n, 3] int64 -> (keys [n] uint64, valid [n] bool): offset 2^20, then a << 42 | b << 21 | c.  The key of
    an invalid coordinate is meaningless (the kernels never form it)."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    valid = ((c >= -KEY_OFFSET) & (c < KEY_LIMIT - KEY_OFFSET)).all(1)
    s = np.where(valid[:, None], c + KEY_OFFSET, 0).astype(np.uint64)
    return (s[:, 0] << np.uint64(42)) | (s[:, 1] << np.uint64(21)) | s[:, 2], valid


def home(coords, n_slots):
    """Home slot of every coordinate in a table of ``n_slots`` (a power of two)."""
    assert n_slots > 0 and n_slots & (n_slots - 1) == 0
    keys, valid = pack_key(coords)
    assert valid.all()
    return (mix64(keys) & np.uint64(n_slots - 1)).astype(np.int64)


def cube_coords(cube=CUBE):
    """Every coordinate of [0, cube)^3, lexicographic in (x, y, z)."""
    r = np.arange(cube, dtype=np.int64)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)


def top_slot_family(n_slots_small, n_slots_big, cube=CUBE):
    """Keys of the cube whose home is the LAST slot of the big table; it is then the last slot of every smaller
    power-of-two table too, n_slots_small included: one chain that wraps to slot 0, before and after growth."""
    assert n_slots_small <= n_slots_big
    c = cube_coords(cube)
    c = c[home(c, n_slots_big) == n_slots_big - 1]
    assert (home(c, n_slots_small) == n_slots_small - 1).all()
    return c


def near_top_family(n_slots, last_k=8, cube=CUBE):
    """Keys of the cube whose home is one of the last ``last_k`` slots."""
    c = cube_coords(cube)
    return c[home(c, n_slots) >= n_slots - last_k]


def range_edge_keys():
    """All 6^3 combinations of the first / last valid values and the values around zero, per axis."""
    v = np.asarray(RANGE_EDGE_VALUES, dtype=np.int64)
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)


def range_outside_keys():
    """One key per axis and sign with that axis one step outside the range and the other two at valid edge values,
    then one key with an axis at 2^40 and one at -2^40."""
    lo, hi = -(1 << 20), (1 << 20) - 1
    out = []
    for axis in range(3):
        for bad, others in ((lo - 1, (hi, lo)), (hi + 1, (lo, hi))):
            k = list(others)
            k.insert(axis, bad)
            out.append(k)
    out.append([0, 1 << 40, -1])
    out.append([hi, lo, -(1 << 40)])
    return np.asarray(out, dtype=np.int64)


# ---- the chain of the GPU tests: SparseVolume(capacity=1024) has 2048 slots, one doubling of the rows gives 4096 ----
CHAIN_SLOTS = (2048, 4096)
N_CHAIN, N_ABSENT, N_NEW, N_SPILL = 450, 300, 300, 700


def chain_sets():
    """(chain, absent, new, spill) coordinates:
    chain   N_CHAIN keys with home 4095 at 4096 slots (hence 2047 at 2048): the wrapping chain, before and after growth;
    rest    the other keys with home 2047 at 2048 slots (557: the two sets overlap) -- ``absent`` is its last N_ABSENT
            (looked up while absent: the probe must cross the whole chain), ``new`` N_NEW a little before the end
            (upserted by the integrate cases, after the absent look-ups); the end of ``rest`` holds the keys that
            keep colliding with the chain at 4096 slots;
    spill   N_SPILL keys whose home at 2048 slots is one of the 7 slots in front of the last: they run into the chain
            and walk all of it."""
    small, big = CHAIN_SLOTS
    fam_big = top_slot_family(small, big)
    fam_small = top_slot_family(small, small)
    chain = fam_big[:N_CHAIN]
    in_chain = {tuple(k) for k in chain.tolist()}
    rest = np.asarray([k for k in fam_small.tolist() if tuple(k) not in in_chain], dtype=np.int64).reshape(-1, 3)
    near = near_top_family(small)
    spill = near[home(near, small) != small - 1][:: 9][:N_SPILL]
    return chain, rest[-N_ABSENT:], rest[-N_NEW - 43: -43], spill


# ---- the small non-cubic grid of the brick and grid-face cases ----
FACE_DIMS, FACE_VOXEL, FACE_N_XYZ = [0.12, 0.14, 0.18], 0.02, [8, 9, 11]
FACE_SEED, FACE_DROP = 5, 0.125
FACE_WEIGHTS = (2.0, 8.0, 20.0)
# A lattice point is live when all of its up to 8 corner voxels exist with weight >= min_pts.  With a voxel present and
# heavy enough with probability p, the 27 points of an origin are live with (p + 6 p^2 + 12 p^4 + 8 p^8) / 27: equal
# odds of the three weights (p = 0.58) would leave 15 % live; one weight in ten below the bar (p = 0.79) leaves ~38 %.
FACE_WEIGHT_P = (0.1, 0.45, 0.45)
FACE_MIN_PTS = 8


def shell_coords(n_xyz=FACE_N_XYZ, pad=2):
    """Every voxel of [-pad, n + pad - 1] per axis: the grid and ``pad`` layers outside each face."""
    ax = [np.arange(-pad, n + pad, dtype=np.int64) for n in n_xyz]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


def grid_coords(n_xyz=FACE_N_XYZ):
    return shell_coords(n_xyz, pad=0)


def face_case(features_pool):
    """Rows of the grid-face decode: the voxels of ``shell_coords()`` with about one in eight left out (fixed seed),
    features drawn from ``features_pool`` [m, 8] (real rows, so that the decoder stays in its certified range),
    weights from FACE_WEIGHTS (so that the >= min_pts decision varies) -> (coords, feats, weights [n, 1])."""
    rng = np.random.default_rng(FACE_SEED)
    c = shell_coords()
    c = c[rng.random(len(c)) >= FACE_DROP]
    feats = np.asarray(features_pool, dtype=np.float32)[rng.integers(0, len(features_pool), len(c))]
    w = np.asarray(FACE_WEIGHTS, dtype=np.float32)[rng.choice(len(FACE_WEIGHTS), len(c), p=FACE_WEIGHT_P)]
    return c, feats, w[:, None]


def face_reference(orc, sd):
    """The oracle alone on the grid-face case -> (coords, feats, weights, origins [792, 3], ref [792, 27] float32 SDF of
    OracleSparseVolume.decode_pts on the 3x3x3 lattice of every in-grid voxel, live rows)."""
    import os

    import torch
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequence_64.npz"))
    c, f, w = face_case(z["features_sorted"])
    ovol = orc.OracleSparseVolume(8, FACE_VOXEL, np.asarray(FACE_DIMS), FACE_MIN_PTS)
    assert ovol.n_xyz.tolist() == FACE_N_XYZ
    ovol.insert(torch.from_numpy(c), torch.from_numpy(f), torch.from_numpy(w), torch.zeros(len(c), 1))
    origins = grid_coords()
    with torch.no_grad():
        ref = ovol.decode_pts(orc.lattice_coords(origins), sd, None, is_coords=True, query_tensor=False)[0, :, :, 0]
    return c, f, w, origins, ref


def on_a_face(origins, n_xyz=FACE_N_XYZ):
    """Origins with a coordinate equal to 0 or n - 1."""
    o = np.asarray(origins)
    return ((o == 0) | (o == np.asarray(n_xyz) - 1)).any(1)


# ---- duplicate keys in one insert call ----
DUP_KEYS, DUP_ROWS, DUP_EXISTING = 500, 2000, 100


def duplicate_case(seed=11):
    """-> (distinct [500, 3], occ [2000] index into ``distinct`` of every row of the call, shuffled): every key occurs
    2..8 times.  The first DUP_EXISTING keys of ``distinct`` are the ones a test puts into the volume beforehand."""
    rng = np.random.default_rng(seed)
    cube = cube_coords(64)
    distinct = cube[rng.permutation(len(cube))[:DUP_KEYS]]
    count = np.full(DUP_KEYS, 2)
    while count.sum() < DUP_ROWS:
        k = rng.integers(0, DUP_KEYS)
        if count[k] < 8:
            count[k] += 1
    occ = np.repeat(np.arange(DUP_KEYS), count)
    return distinct, occ[rng.permutation(len(occ))]


# ---- oracle.integrate, vectorised (the 70-workgroup frame: the dict loop would take minutes) ----
def integrate_rows(coords, feats, weights, hits, fr_coords, fr_feats, fr_pcounts):
    """bnv_oracle.integrate on row arrays (torch CPU, the same float32 ops in the same order): existing keys keep their
    rows, new keys follow in frame order; keys unique within the frame.  -> (coords, feats, weights [n, 1], hits [n, 1])."""
    import torch
    index = {tuple(k): r for r, k in enumerate(coords.tolist())}
    rows, n = [], len(index)
    for k in fr_coords.tolist():
        r = index.get(tuple(k))
        if r is None:
            r = index[tuple(k)] = n
            n += 1
        rows.append(r)
    rows = torch.tensor(rows, dtype=torch.int64)
    grow = n - len(coords)
    coords = torch.cat([coords, torch.zeros((grow, 3), dtype=coords.dtype)])
    feats = torch.cat([feats, torch.zeros((grow, feats.shape[1]))])
    weights = torch.cat([weights, torch.zeros((grow, 1))])
    hits = torch.cat([hits, torch.zeros((grow, 1))])
    w = torch.clip(fr_pcounts.reshape(-1, 1) / 32, max=1)
    old_f, old_w = feats[rows], weights[rows]
    new_w = old_w + w
    feats[rows] = (old_f * old_w + fr_feats * w) / new_w
    weights[rows] = new_w
    coords[rows] = fr_coords
    return coords, feats, weights, hits
