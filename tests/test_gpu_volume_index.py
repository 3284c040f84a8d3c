"""The sparse volume's index -- open-addressing table (packed 64-bit key, linear probing, CAS insert), growth by
re-hashing, and the dense row index of the grid (the "brick") -- at its edges, against the dict oracle
(oracle/bnv_oracle.py: OracleSparseVolume, integrate, decode_pts).  Needs a real MI355X: run with  -m gpu.

The inputs are the ones on which a subtly wrong table cannot give the oracle's answer (tests/volume_cases.py; that they
are what they claim is checked on the CPU by tests/test_volume_cases_cpu.py): one probe chain that wraps past the last
slot, built and extended by racing threads and carried through a growth; the first / last valid coordinate of every
axis and the first invalid ones; frames that end on, one before and one behind a workgroup boundary of the one-launch
upserts, and one longer than a look-back window; rows just outside the grid under a decode at its faces; keys given
several times in one insert.

Bars: those of test_integrate_sequence_vs_reference_golden for the same comparison -- row coordinates and row ORDER
identical, weights bit for bit, features within 2e-6, num_hits identical -- and the north-star SDF bar with identical
mask decisions for the decode.  Values that were only stored (insert) must come back bit for bit.

The reads of vol._slot_keys / _slot_rows / _brick / _n_slots are deliberate: they prove that the case happened."""
import ctypes as C

import numpy as np
import pytest
import torch

import volume_cases as VC
from conftest import WEIGHTS_FP32

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SDF_TOL = 1e-4      # north_star: SDF max-abs-err < 1e-4
FEAT_TOL = 2e-6     # integrated features against the oracle's ATen ops
DIMS64 = [1.24] * 3
POISON = 7_000_000  # a coordinate beyond a device-side count: would raise the key-range error if it were read


@pytest.fixture(scope="module")
def bnv():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    import bnv_fusion_amd
    return bnv_fusion_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import bnv_oracle
    return bnv_oracle


@pytest.fixture(scope="module")
def sets():
    return tuple(torch.from_numpy(s) for s in VC.chain_sets())


class Pair:
    """A HIP volume and the oracle's, fed the same calls."""

    def __init__(self, bnv, orc, dims=DIMS64, capacity=1024, brick=None):
        self.orc = orc
        self.vol = bnv.SparseVolume(8, 0.02, np.array(dims), 8, capacity=capacity, device=DEV, brick=brick)
        self.ovol = orc.OracleSparseVolume(8, 0.02, np.array(dims), 8)

    def insert(self, keys, f, w, h):
        self.vol.insert(keys.to(DEV), f.to(DEV), w.to(DEV), h.to(DEV))
        self.ovol.insert(keys, f, w, h)

    def integrate(self, keys, f, pc, n_dev=None):
        """``n_dev``: an int -- the tensors are buffers, the count is read on the device."""
        nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
        self.vol.integrate(keys.to(DEV), f.to(DEV), pc.to(DEV), n_dev=nd)
        n = len(keys) if n_dev is None else n_dev
        self.orc.integrate(self.ovol, keys[:n], f[:n], pc[:n].reshape(-1, 1))

    def integrate_batch(self, frames, device_counts=False):
        """frames: (keys, feats, pcounts, n) with n <= len(keys)."""
        dev = []
        for k, f, p, n in frames:
            nd = torch.tensor([n], dtype=torch.int32, device=DEV) if device_counts else None
            m = len(k) if device_counts else n
            dev.append((k[:m].to(DEV), f[:m].to(DEV), p[:m].to(DEV), nd))
        self.vol.integrate_batch(dev)
        for k, f, p, n in frames:
            self.orc.integrate(self.ovol, k[:n], f[:n], p[:n].reshape(-1, 1))

    # ---- comparisons ----
    def assert_rows(self, feat_tol=FEAT_TOL):
        """Row arrays against the oracle's: coordinates and order identical, weights and num_hits bit for bit, features
        within ``feat_tol`` (0: bit for bit).  num_rows() raises on a sticky error."""
        n = self.vol.num_rows()
        assert n == len(self.ovol._keys)
        c, f, w, h = (t.cpu() for t in self.vol.to_tensor())
        oc, of, ow, oh = self.ovol.to_tensor()
        assert torch.equal(c, oc)
        assert torch.equal(w, ow) and torch.equal(h, oh)
        err = float((f - of).abs().max()) if n else 0.0
        print("rows", n, "feature err", err)
        assert err <= feat_tol and bool(torch.isfinite(f).all())

    def assert_query(self, keys, feat_tol=FEAT_TOL, snapshot=False):
        got = (self.vol._query_tensor if snapshot else self.vol.query)(keys.to(DEV))
        ref = (self.ovol._query_tensor if snapshot else self.ovol.query)(keys)
        assert torch.equal(got[1].cpu(), ref[1]) and torch.equal(got[2].cpu(), ref[2])
        assert float((got[0].cpu() - ref[0]).abs().max()) <= feat_tol
        return ref

    def rows_of(self, keys):
        """bnv_volume_query's out_rows for ``keys``, and the dict's."""
        return _rows_of(self.vol, keys), np.asarray(self.ovol._rows(keys, self.ovol._map))

    def assert_table(self):
        """The slot table IS the dict: as many occupied slots as keys, every one holding a key of the dict with its
        row; and the brick holds the same rows for the voxels inside the grid, -1 everywhere else."""
        slots, coords, rows = _table(self.vol)
        assert len(slots) == len(self.ovol._map) == len({tuple(k) for k in coords.tolist()})
        assert [self.ovol._map[tuple(k)] for k in coords.tolist()] == rows.tolist()
        if self.vol._brick is not None:
            nx, ny, nz = self.vol._n_xyz_host
            expect = np.full(nx * ny * nz, -1, dtype=np.int32)
            k = np.asarray(self.ovol._keys, dtype=np.int64).reshape(-1, 3)
            inside = ((k >= 0) & (k < np.array([nx, ny, nz]))).all(1)
            expect[(k[inside, 0] * ny + k[inside, 1]) * nz + k[inside, 2]] = np.nonzero(inside)[0]
            assert np.array_equal(self.vol._brick.cpu().numpy(), expect)
            return int(inside.sum()), int((~inside).sum())
        return None


def _rows_of(vol, keys):
    from bnv_fusion_amd import _lib
    k = keys.reshape(-1, 3).long().contiguous().to(DEV)
    out = torch.full((len(k),), -9, dtype=torch.int32, device=DEV)
    _lib.check(vol._lib.bnv_volume_query(C.byref(vol._struct()), _lib.ptr(k), len(k), _lib.ptr(vol._features),
                                         _lib.ptr(vol._weights), _lib.ptr(vol._num_hits), vol._row_capacity, None, None,
                                         None, _lib.ptr(out), _lib.stream_ptr()), "bnv_volume_query")
    return out.cpu().numpy()


def _table(vol):
    """(occupied slots, their keys unpacked to coordinates, their rows), slots ascending."""
    keys = vol._slot_keys.cpu().numpy().view(np.uint64)
    assert len(keys) == vol._n_slots
    slots = np.nonzero(keys != np.uint64(0xFFFFFFFFFFFFFFFF))[0]
    k = keys[slots]
    coords = np.stack([k >> np.uint64(42), (k >> np.uint64(21)) & np.uint64(0x1FFFFF), k & np.uint64(0x1FFFFF)], 1)
    return slots, coords.astype(np.int64) - VC.KEY_OFFSET, vol._slot_rows.cpu().numpy()[slots]


def _slots_of(vol, keys):
    """Slots that hold ``keys`` (a set of coordinate tuples), ascending."""
    slots, coords, _ = _table(vol)
    return slots[[tuple(k) in keys for k in coords.tolist()]]


class _no_growth:
    """integrate / integrate_batch set rows aside for a whole frame, new keys or not, and grow the tables when the
    frame might not fit.  Where a case needs the table to stay as it is and the rows it really creates do fit, the
    reservation is skipped for the call: the kernels themselves refuse a row beyond the capacity (error 3)."""

    def __init__(self, vol, new_rows):
        self.vol, self.new_rows = vol, new_rows

    def __enter__(self):
        assert self.vol.num_rows() + self.new_rows <= self.vol._row_capacity       # nothing has to grow
        self.vol._reserve = lambda n: None

    def __exit__(self, *exc):
        del self.vol._reserve
        return False


def _values(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 8, generator=g), torch.rand(n, 1, generator=g) + 0.25,
            torch.randint(0, 5, (n, 1), generator=g).float())


def _frame_values(n, seed):
    """feats randn, pcounts 1..80 (weights on both sides of the clip at 32)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 8, generator=g), torch.randint(1, 81, (n,), generator=g)


def _chain_pair(bnv, orc, sets, brick=None):
    """Case 1's state: the 450 chain keys inserted in three calls of 150 -- within a call every thread races down the
    one chain, which starts at the table's last slot."""
    chain = sets[0]
    p = Pair(bnv, orc, capacity=1024, brick=brick)
    assert p.vol._n_slots == 2048
    f, w, h = _values(len(chain), 1)
    for lo in range(0, len(chain), 150):
        s = slice(lo, lo + 150)
        p.insert(chain[s], f[s], w[s], h[s])
    return p


def _chain_frame(sets):
    """Case 2's frame: 300 keys of the chain and 300 new keys of the same home, interleaved (every wave holds both)."""
    chain, _, new, _ = sets
    keys = torch.stack([chain[:300], new], 1).reshape(-1, 3)
    return (keys,) + _frame_values(len(keys), 2)


# ---------------------------------------------------------------------------------------------
# case 1: one chain, built under contention, wrapping
# ---------------------------------------------------------------------------------------------
def test_one_wrapping_chain_built_under_contention(bnv, orc, sets):
    chain, absent, _, _ = sets
    p = _chain_pair(bnv, orc, sets)
    assert p.vol.num_rows() == 450 and p.vol._n_slots == 2048
    # the chain happened: slot 2047 and slots 0..448, nothing else
    slots, _, _ = _table(p.vol)
    assert slots.tolist() == list(range(449)) + [2047]
    p.assert_table()
    # every key is found, with the values and the row of its insertion; absent keys of the same home, whose probe
    # crosses all 450 slots and the wrap before it meets an empty one, read as zeros
    p.assert_query(chain, 0)
    ref = p.assert_query(absent, 0)
    assert all(float(t.abs().sum()) == 0 for t in ref)
    got, want = p.rows_of(torch.cat([chain, absent]))
    assert np.array_equal(got, want) and np.array_equal(got[:450], np.arange(450)) and (got[450:] == -1).all()
    p.assert_rows(0)
    p.assert_query(chain, 0, snapshot=True)
    assert all(float(t.abs().sum()) == 0 for t in p.assert_query(absent, 0, snapshot=True))


# ---------------------------------------------------------------------------------------------
# case 2: integrate down the same chain
# ---------------------------------------------------------------------------------------------
def test_integrate_down_the_chain(bnv, orc, sets):
    keys, f, pc = _chain_frame(sets)
    one = _chain_pair(bnv, orc, sets)
    with _no_growth(one.vol, 300):
        one.integrate(keys, f, pc)
    one.assert_rows()
    assert one.vol.num_rows() == 750 <= 1024 and one.vol._n_slots == 2048       # nothing grew: still the 2048-slot chain
    slots, _, _ = _table(one.vol)
    assert slots.tolist() == list(range(749)) + [2047]
    one.assert_table()
    one.assert_query(keys)
    # the same frame through the batched upsert: bit for bit the same volume
    one_b = _chain_pair(bnv, orc, sets)
    with _no_growth(one_b.vol, 300):
        one_b.integrate_batch([(keys, f, pc, len(keys))])
    for a, b in zip(one.vol.to_tensor(), one_b.vol.to_tensor()):
        assert torch.equal(a, b)
    # three frames that split and overlap the same keys: one integrate each against one integrate_batch
    g = torch.Generator().manual_seed(4)
    frames = []
    for lo, hi, seed in ((0, 300, 5), (200, 500, 6), (350, 600, 7)):
        sel = torch.cat([keys[lo:hi], keys[:50]]) if lo == 350 else keys[lo:hi]
        sel = sel[torch.randperm(len(sel), generator=g)]
        frames.append((sel,) + _frame_values(len(sel), seed) + (len(sel),))
    seq, bat = _chain_pair(bnv, orc, sets), _chain_pair(bnv, orc, sets)
    with _no_growth(seq.vol, 300):
        for k, ff, pp, _ in frames:
            seq.integrate(k, ff, pp)
    with _no_growth(bat.vol, 300):
        bat.integrate_batch(frames)
    for p in (seq, bat):
        p.assert_rows()
        assert p.vol.num_rows() == 750 and p.vol._n_slots == 2048
        p.assert_table()
    for a, b in zip(seq.vol.to_tensor(), bat.vol.to_tensor()):
        assert torch.equal(a, b)
    assert int(bat.vol._slot_mask.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------
# case 3: growth re-hashes a colliding set
# ---------------------------------------------------------------------------------------------
def test_growth_rehashes_a_colliding_set(bnv, orc, sets):
    chain, absent, _, spill = sets
    p = _chain_pair(bnv, orc, sets)
    assert p.vol._n_slots == 2048
    rows_before, _ = p.rows_of(chain)
    f, w, h = _values(len(spill), 3)
    p.insert(spill, f, w, h)                       # 450 + 700 rows > 1024: the tables double and every row is re-hashed
    assert p.vol.num_rows() == 1150 and p.vol._n_slots == 4096 and p.vol._row_capacity == 2048
    everything = torch.cat([chain, spill])
    got, want = p.rows_of(everything)
    assert np.array_equal(got, want) and np.array_equal(got, np.arange(1150))
    assert np.array_equal(got[:450], rows_before)                                # the same rows as before the growth
    # the chain still collides under the new mask: slot 4095 and a contiguous run from slot 0
    in_chain = {tuple(k) for k in chain.tolist()}
    assert _slots_of(p.vol, in_chain).tolist() == list(range(449)) + [4095]
    p.assert_table()
    p.assert_query(everything, 0)
    assert all(float(t.abs().sum()) == 0 for t in p.assert_query(absent, 0))
    assert (p.rows_of(absent)[0] == -1).all()
    p.assert_rows(0)
    # case 2's frame on the grown table
    keys, ff, pc = _chain_frame(sets)
    p.integrate(keys, ff, pc)
    p.assert_rows()
    assert p.vol.num_rows() == 1450 and p.vol._n_slots == 4096
    p.assert_table()
    p.assert_query(torch.cat([everything, keys]))


# ---------------------------------------------------------------------------------------------
# case 4: the brick equals the table
# ---------------------------------------------------------------------------------------------
def test_brick_equals_the_table_through_every_upsert(bnv, orc, sets):
    """After the states of cases 1-3 (keys of [0, 128)^3 in a 64^3 grid: inside and outside the brick), with and
    without the dense index: the same row arrays, and the brick word of every in-grid key is the dict's row."""
    chain, _, _, spill = sets
    keys, ff, pc = _chain_frame(sets)
    f, w, h = _values(len(spill), 3)
    twins = [_chain_pair(bnv, orc, sets, brick=b) for b in (True, False)]
    assert twins[0].vol._brick is not None and twins[1].vol._brick is None
    for step in range(3):
        for p in twins:
            if step == 1:
                p.integrate_batch([(keys[:400], ff[:400], pc[:400], 400)])
            elif step == 2:
                p.insert(spill, f, w, h)
                p.integrate(keys, ff, pc)
            counts = p.assert_table()
            if counts:
                print("in / outside the grid", counts)
                assert min(counts) > 20
            p.assert_rows()
        for a, b in zip(twins[0].vol.to_tensor(), twins[1].vol.to_tensor()):
            assert torch.equal(a, b)


def test_brick_on_a_non_cubic_grid_and_after_reset(bnv, orc):
    """Grid [8, 9, 11]; keys: every voxel of [-2, n + 1] per axis, through insert, integrate and integrate_batch with
    the tables growing on the way.  The brick allocation survives reset(): stale rows must be gone."""
    shell = torch.from_numpy(VC.shell_coords())
    shell = shell[torch.randperm(len(shell), generator=torch.Generator().manual_seed(8))]
    assert len(shell) == 12 * 13 * 15
    twins = [Pair(bnv, orc, dims=VC.FACE_DIMS, capacity=1024, brick=b) for b in (True, False)]
    for p in twins:
        assert p.vol._n_xyz_host == VC.FACE_N_XYZ
        f, w, h = _values(900, 9)
        p.insert(shell[:900], f, w, h)
        ff, pc = _frame_values(900, 10)
        p.integrate(shell[600:1500], ff, pc)
        fb, pb = _frame_values(len(shell), 11)
        p.integrate_batch([(shell[lo:hi], fb[lo:hi], pb[lo:hi], hi - lo) for lo, hi in ((1200, 1900), (1700, len(shell)))])
        assert p.vol.num_rows() == len(shell) and p.vol._n_slots > 2048
        counts = p.assert_table()
        assert counts is None or counts == (8 * 9 * 11, len(shell) - 8 * 9 * 11)
        p.assert_rows()
    for a, b in zip(twins[0].vol.to_tensor(), twins[1].vol.to_tensor()):
        assert torch.equal(a, b)
    brick = twins[0].vol._brick
    for p in twins:
        p.vol.reset(1024)
        p.ovol = orc.OracleSparseVolume(8, 0.02, np.array(VC.FACE_DIMS), 8)
        assert p.vol.num_rows() == 0
        ff, pc = _frame_values(len(shell[::3]), 12)
        p.integrate(shell[::3], ff, pc)
        counts = p.assert_table()
        assert counts is None or 200 < counts[0] < 8 * 9 * 11 // 2
        p.assert_rows()
    assert twins[0].vol._brick is brick                      # the same allocation, and no row of the first fill in it
    for a, b in zip(twins[0].vol.to_tensor(), twins[1].vol.to_tensor()):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------
# case 5: the ends of the key range
# ---------------------------------------------------------------------------------------------
def test_first_and_last_valid_coordinates(bnv, orc):
    edge = torch.from_numpy(VC.range_edge_keys())
    p = Pair(bnv, orc)
    f, w, h = _values(216, 13)
    p.insert(edge[:100], f[:100], w[:100], h[:100])
    ff, pc = _frame_values(216, 14)
    perm = torch.randperm(216, generator=torch.Generator().manual_seed(15))
    p.integrate(edge[perm], ff, pc)                               # 100 existing, 116 new
    p.integrate_batch([(edge, ff, pc, 216), (edge[perm][:77], ff[:77], pc[:77], 77)])
    assert p.vol.num_rows() == 216                                # 216 distinct rows, no error
    p.assert_rows()
    p.assert_table()
    p.assert_query(edge)
    got, want = p.rows_of(edge)
    assert np.array_equal(got, want) and sorted(got.tolist()) == list(range(216))


@pytest.mark.parametrize("path", ["integrate", "insert", "integrate_batch"])
def test_first_invalid_coordinates_are_refused(bnv, orc, path):
    """Each key one step (or far) outside the range, upserted between two valid keys: the sticky error is raised, and
    once acknowledged the volume holds exactly the two valid keys with the oracle's values."""
    from bnv_fusion_amd._lib import BnvError
    hi, lo = (1 << 20) - 1, -(1 << 20)
    good = torch.tensor([[hi, lo, 5], [lo, hi, hi]])
    for bad in VC.range_outside_keys().tolist():
        keys = torch.tensor([good[0].tolist(), bad, good[1].tolist()])
        p = Pair(bnv, orc)
        ff, pc = _frame_values(3, 16)
        f, w, h = _values(3, 17)
        ok = torch.tensor([0, 2])
        if path == "integrate":
            p.vol.integrate(keys.to(DEV), ff.to(DEV), pc.to(DEV))
            orc.integrate(p.ovol, keys[ok], ff[ok], pc[ok].reshape(-1, 1))
        elif path == "insert":
            p.vol.insert(keys.to(DEV), f.to(DEV), w.to(DEV), h.to(DEV))
            p.ovol.insert(keys[ok], f[ok], w[ok], h[ok])
        else:
            p.vol.integrate_batch([(keys[:2].to(DEV), ff[:2].to(DEV), pc[:2].to(DEV), None),
                                   (keys[1:].to(DEV), ff[1:].to(DEV), pc[1:].to(DEV), None)])
            orc.integrate(p.ovol, keys[:1], ff[:1], pc[:1].reshape(-1, 1))
            orc.integrate(p.ovol, keys[2:], ff[2:], pc[2:].reshape(-1, 1))
        with pytest.raises(BnvError, match="21-bit"):
            p.vol.num_rows()
        p.vol._status[1] = 0                                      # acknowledge
        assert p.vol.num_rows() == 2, bad
        p.assert_rows()
        p.assert_table()
        p.assert_query(good)
        assert _rows_of(p.vol, torch.tensor([bad]))[0] == -1


def test_lookups_of_invalid_coordinates_read_as_absent(bnv, orc):
    edge = torch.from_numpy(VC.range_edge_keys())
    out = torch.from_numpy(VC.range_outside_keys())
    p = Pair(bnv, orc)
    f, w, h = _values(216, 13)
    p.insert(edge, f, w, h)
    p.assert_rows(0)
    assert all(float(t.abs().sum()) == 0 for t in p.vol.query(out.to(DEV)))
    assert all(float(t.abs().sum()) == 0 for t in p.vol._query_tensor(out.to(DEV)))
    assert (_rows_of(p.vol, out) == -1).all()
    before = p.vol.weights.clone()
    p.vol.count_optim(out.to(DEV))
    assert torch.equal(p.vol.weights, before)
    p.vol.count_optim(torch.cat([out, edge[:50], edge[:50]]).to(DEV))             # mixed with valid keys: those count once
    p.ovol.count_optim(torch.cat([edge[:50], edge[:50]]))
    assert torch.equal(p.vol.weights.cpu(), p.ovol.weights)
    assert p.vol.num_rows() == 216                                                # no error, nothing changed
    p.assert_table()


# ---------------------------------------------------------------------------------------------
# case 6: workgroup boundaries of the one-launch upserts
# ---------------------------------------------------------------------------------------------
def _tile_keys():
    """Keys per workgroup of bnv_volume_integrate, from the library that is loaded."""
    from bnv_fusion_amd import _lib
    t = int(_lib.load().bnv_volume_integrate_tile_keys())
    assert t >= 64 and t % 64 == 0
    return t


def _boundary_pool(n, seed):
    """n distinct keys of [0, 128)^3 in a fixed random order."""
    cube = VC.cube_coords()
    return torch.from_numpy(cube[np.random.default_rng(seed).permutation(len(cube))[:n]])


def _held_before(n, seed):
    """Which keys of a frame the volume already holds: every second one (the odd indices: a one-key tail behind a
    workgroup boundary is a NEW key) and a random quarter of the others -- so that the number of created keys differs
    from wave to wave.  The frame's last key is always new."""
    held = torch.zeros(n, dtype=torch.bool)
    held[1::2] = True
    held |= torch.rand(n, generator=torch.Generator().manual_seed(seed)) < 0.25
    held[-1] = False
    return held


@pytest.mark.parametrize("count", ["host", "device"])
@pytest.mark.parametrize("size", ["1", "T-1", "T", "T+1", "2T", "2T+1"])
def test_integrate_at_workgroup_boundaries(bnv, orc, size, count):
    T = _tile_keys()
    n = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T": 2 * T, "2T+1": 2 * T + 1}[size]
    cap = 3 * T + 300
    keys = torch.full((cap, 3), POISON, dtype=torch.int64)
    keys[:n] = _boundary_pool(n, 20)
    ff, pc = _frame_values(cap, 21)
    held = _held_before(n, 22)
    if n >= 128:
        per_wave = (~held)[: n // 64 * 64].reshape(-1, 64).sum(1)
        assert len(set(per_wave.tolist())) > 1                     # created counts differ from wave to wave
    p = Pair(bnv, orc, capacity=8192)
    if held.any():
        f, w, h = _values(int(held.sum()), 23)
        p.insert(keys[:n][held], f, w, h)
    if count == "host":
        p.integrate(keys[:n], ff[:n], pc[:n])
    else:
        p.integrate(keys, ff, pc, n_dev=n)
    assert p.vol.num_rows() == n
    p.assert_rows()
    p.assert_table()
    # a device-side count of 0: nothing is read, nothing changes, no error
    before = [t.clone() for t in p.vol.to_tensor()]
    p.integrate(keys, ff, pc, n_dev=0)
    assert p.vol.num_rows() == n
    for a, b in zip(before, p.vol.to_tensor()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("count", ["host", "device"])
def test_integrate_batch_at_block_boundaries(bnv, orc, count):
    """Frames of 255, 256, 257, 0, 1 and 512 keys in one call (the batch numbers rows per 256 items, frames padded to
    whole blocks); the frames overlap, and the volume holds part of their keys beforehand."""
    sizes = [255, 256, 257, 0, 1, 512]
    pool = _boundary_pool(1100, 24)
    held = _held_before(1100, 25)
    p = Pair(bnv, orc, capacity=8192)
    f, w, h = _values(int(held.sum()), 26)
    p.insert(pool[held], f, w, h)
    frames, lo = [], 0
    for j, n in enumerate(sizes):
        assert lo + n <= len(pool)
        buf = torch.full((n + 300, 3), POISON, dtype=torch.int64)
        buf[:n] = pool[lo: lo + n]
        frames.append((buf,) + _frame_values(n + 300, 27 + j) + (n,))
        lo += n * 2 // 3                                           # a third of every frame returns in the next one
    p.integrate_batch(frames, device_counts=(count == "device"))
    p.assert_rows()
    p.assert_table()
    assert int(p.vol._slot_mask.abs().sum()) == 0
    # an empty device-side count alone
    before = [t.clone() for t in p.vol.to_tensor()]
    p.integrate_batch([(frames[3][0], frames[3][1], frames[3][2], 0)], device_counts=True)
    for a, b in zip(before, p.vol.to_tensor()):
        assert torch.equal(a, b)
    assert p.vol.num_rows() == len(before[0])


def test_integrate_across_more_than_one_lookback_window(bnv):
    """70 workgroups (a look-back window covers 64), half of the keys new.  Expected rows by the kernel's contract,
    restated in numpy -- existing rows keep theirs, new keys follow in batch order, which is what the dict gives --
    and values by bnv_oracle.integrate's ops vectorised on the CPU (volume_cases.integrate_rows, checked against the
    oracle itself in test_volume_cases_cpu.py)."""
    T = _tile_keys()
    n = 70 * T
    keys = _boundary_pool(n, 30)
    held = torch.rand(n, generator=torch.Generator().manual_seed(31)) < 0.5
    vol = bnv.SparseVolume(8, 0.02, np.array(DIMS64), 8, capacity=1 << 17, device=DEV)
    f, w, h = _values(int(held.sum()), 32)
    vol.insert(keys[held].to(DEV), f.to(DEV), w.to(DEV), h.to(DEV))
    ff, pc = _frame_values(n, 33)
    vol.integrate(keys.to(DEV), ff.to(DEV), pc.to(DEV))
    n_old = int(held.sum())
    rows = np.empty(n, dtype=np.int64)
    rows[held.numpy()] = np.arange(n_old)
    rows[~held.numpy()] = n_old + np.arange(n - n_old)
    assert vol.num_rows() == n
    assert np.array_equal(_rows_of(vol, keys), rows)
    ec, ef, ew, eh = VC.integrate_rows(keys[held], f, w, h, keys, ff, pc)
    c, gf, gw, gh = (t.cpu() for t in vol.to_tensor())
    assert torch.equal(c, ec) and torch.equal(gw, ew) and torch.equal(gh, eh)
    err = float((gf - ef).abs().max())
    print("feature err", err)
    assert err <= FEAT_TOL


# ---------------------------------------------------------------------------------------------
# case 7: decode at the grid's faces, with rows outside the grid
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def face(orc):
    return VC.face_reference(orc, orc.load_weights(WEIGHTS_FP32))


@pytest.mark.parametrize("mode", [1, 0])
def test_decode_at_the_grid_faces_with_rows_outside(bnv, orc, face, mode):
    """Every in-grid voxel of the [8, 9, 11] grid as an origin: its lattice reads neighbours at -1 and n, outside the
    brick, where the fused look-up must fall back to the hash.  Rows exist there (or are missing, or too light), so a
    look-up that treats off-grid voxels as absent changes mask decisions and values."""
    c, f, w, origins, ref = face
    voxel = np.float32(VC.FACE_VOXEL)
    ref = ref.numpy()
    on_face = VC.on_a_face(origins)
    live = ref != voxel
    assert live[on_face].mean() > 0.30 and (~live)[on_face].mean() > 0.10       # (the CPU suite proves it for the oracle)
    model = bnv.load_pretrained(device=DEV, voxel_size=VC.FACE_VOXEL)
    bnv.set_mlp_mode(mode)
    try:
        outs = {}
        for brick in (True, False):
            vol = bnv.SparseVolume(8, VC.FACE_VOXEL, np.array(VC.FACE_DIMS), VC.FACE_MIN_PTS, capacity=4096, device=DEV,
                                   brick=brick)
            assert (vol._brick is not None) == brick and vol._n_xyz_host == VC.FACE_N_XYZ
            vol.insert(torch.from_numpy(c).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(w).to(DEV),
                       torch.zeros(len(c), 1, device=DEV))
            o = torch.from_numpy(origins).to(DEV)
            lat = vol.decode_lattice(o, model.nerf, query_tensor=False).cpu().numpy()
            pts = vol.decode_pts(orc.lattice_coords(origins).to(DEV), model.nerf, None, is_coords=True,
                                 query_tensor=False).cpu().numpy()[0, :, :, 0]
            vol.num_rows()                                            # raises if a kernel flagged anything
            for name, out in (("decode_lattice", lat), ("decode_pts", pts)):
                err = float(np.abs(out - ref).max())
                print(name, "brick" if brick else "hash", "mode", mode, "err", err)
                assert out.shape == ref.shape
                assert np.array_equal(out == voxel, ref == voxel), name      # mask decisions identical
                assert err <= SDF_TOL, (name, err)
            outs[brick] = (lat, pts)
        assert np.array_equal(outs[True][0], outs[False][0]) and np.array_equal(outs[True][1], outs[False][1])
    finally:
        bnv.set_mlp_mode(1)


# ---------------------------------------------------------------------------------------------
# case 8: duplicate keys in one insert
# ---------------------------------------------------------------------------------------------
def test_duplicate_keys_in_one_insert(bnv, orc):
    """2000 rows drawn from 500 keys (2..8 times each, shuffled), 100 of the keys already in the volume.  One row per
    key, new rows in the order of first occurrence, and every stored row is WHOLE: its 8 features (all equal to the
    occurrence's index), weight and num_hits come from one occurrence.  bnv_volume_insert lets the LAST occurrence of a
    key write (what the reference's map gives when the occurrences are inserted one by one), so the volume must equal
    the oracle's bit for bit; the weaker property the issue asks for is asserted first, by itself."""
    distinct, occ = VC.duplicate_case()
    distinct, occ = torch.from_numpy(distinct), torch.from_numpy(occ)
    p = Pair(bnv, orc, capacity=1024)
    f, w, h = _values(VC.DUP_EXISTING, 40)
    p.insert(distinct[:VC.DUP_EXISTING], f, w, h)
    keys = distinct[occ]
    idx = torch.arange(len(occ), dtype=torch.float32)
    feats, weights, hits = idx[:, None].repeat(1, 8), idx[:, None] + 1, idx[:, None] + 3
    p.insert(keys, feats, weights, hits)
    assert p.vol.num_rows() == VC.DUP_KEYS
    c, gf, gw, gh = (t.cpu() for t in p.vol.to_tensor())
    seen, first_order = set(), []
    for k in occ.tolist():
        if k not in seen and k >= VC.DUP_EXISTING:
            first_order.append(k)
        seen.add(k)
    assert torch.equal(c[:VC.DUP_EXISTING], distinct[:VC.DUP_EXISTING])
    assert torch.equal(c[VC.DUP_EXISTING:], distinct[first_order])              # rows in order of first occurrence
    occurrences = {}
    for i, k in enumerate(occ.tolist()):
        occurrences.setdefault(tuple(distinct[k].tolist()), set()).add(float(i))
    for r, k in enumerate(c.tolist()):
        own = occurrences[tuple(k)]
        assert bool((gf[r] == gf[r, 0]).all()), (r, gf[r])                       # not torn
        assert float(gf[r, 0]) in own and float(gw[r]) - 1 in own and float(gh[r]) - 3 in own
        assert float(gf[r, 0]) == float(gw[r]) - 1 == float(gh[r]) - 3 == max(own)
    p.assert_rows(0)
    p.assert_table()
    p.assert_query(distinct, 0)
