"""The conditions that keep tests/test_gpu_volume_index.py from passing vacuously, checked on the CPU: every key family
of tests/volume_cases.py is large enough and has the claimed home slot at every table size the GPU tests pass through,
the restated key packing is injective at the ends of its range and rejects what lies outside, the vectorised
restatement of the oracle's integrate is the oracle's, and the grid-face decode has both live and masked lattice
values where it matters -- by the oracle alone."""
import numpy as np
import pytest
import torch

import volume_cases as VC
from conftest import WEIGHTS_FP32


@pytest.fixture(scope="module")
def orc():
    from oracle import bnv_oracle
    return bnv_oracle


def _as_set(c):
    return {tuple(k) for k in np.asarray(c).tolist()}


def test_top_slot_family_sizes_and_homes():
    """The figures the chain cases were sized by: cube [0, 128)^3, 1007 keys with home 2047 at 2048 slots, 516 of them
    with home 4095 at 4096, 254 of those with home 8191 at 8192 -- and a family of the big table is one of every
    smaller table."""
    f2, f4, f8 = (VC.top_slot_family(2048, n) for n in (2048, 4096, 8192))
    print(len(f2), len(f4), len(f8))
    assert (len(f2), len(f4), len(f8)) == (1007, 516, 254)
    assert _as_set(f8) <= _as_set(f4) <= _as_set(f2)
    for fam, sizes in ((f2, (2048,)), (f4, (2048, 4096)), (f8, (2048, 4096, 8192))):
        for n in sizes:
            assert (VC.home(fam, n) == n - 1).all()
        assert (fam >= 0).all() and (fam < VC.CUBE).all() and len(_as_set(fam)) == len(fam)
    near = VC.near_top_family(2048)
    print(len(near))
    assert 7000 < len(near) < 9000 and (VC.home(near, 2048) >= 2040).all()


def test_chain_sets_are_what_the_gpu_cases_take():
    chain, absent, new, spill = VC.chain_sets()
    assert (len(chain), len(absent), len(new), len(spill)) == (VC.N_CHAIN, VC.N_ABSENT, VC.N_NEW, VC.N_SPILL)
    small, big = VC.CHAIN_SLOTS
    # the chain keeps the last slot as its home through the growth; absent / new keys share it in the small table
    assert (VC.home(chain, small) == small - 1).all() and (VC.home(chain, big) == big - 1).all()
    assert (VC.home(absent, small) == small - 1).all() and (VC.home(new, small) == small - 1).all()
    # after the growth the absent and the new keys still collide with the chain or sit half a table away, both kinds
    for s in (absent, new):
        hb = VC.home(s, big)
        assert set(hb.tolist()) == {small - 1, big - 1} and (hb == big - 1).sum() > 30 and (hb == small - 1).sum() > 30
    # the spill keys start in the 7 slots in front of the chain's home, all 7 of them
    assert set(VC.home(spill, small).tolist()) == set(range(small - 8, small - 1))
    assert set(VC.home(spill, big).tolist()) <= set(range(small - 8, small - 1)) | set(range(big - 8, big - 1))
    sets = [_as_set(s) for s in (chain, absent, new, spill)]
    assert [len(s) for s in sets] == [VC.N_CHAIN, VC.N_ABSENT, VC.N_NEW, VC.N_SPILL]
    assert not sets[0] & (sets[1] | sets[2] | sets[3]) and not sets[3] & (sets[1] | sets[2])
    assert len(sets[1] - sets[2]) == 43            # (absent and new overlap: only 557 keys share the home)
    # nothing grows while the chain is built and integrated into: 450 + 300 rows in 1024
    assert VC.N_CHAIN + VC.N_NEW <= 1024 < VC.N_CHAIN + VC.N_SPILL <= 2048
    # the chain reaches both inside and outside a 64^3 grid (the brick covers only part of it)
    inside = (np.concatenate([chain, new, spill]) < 64).all(1)
    assert 50 < inside.sum() < len(inside) - 50


def test_pack_key_at_the_ends_of_the_range():
    edge = VC.range_edge_keys()
    assert edge.shape == (216, 3)
    keys, valid = VC.pack_key(edge)
    assert valid.all() and len(set(keys.tolist())) == 216
    assert all(k != 0xFFFFFFFFFFFFFFFF for k in keys.tolist())        # none is the empty-slot word
    # unpacking gives the coordinates back
    k = keys.astype(np.uint64)
    back = np.stack([k >> np.uint64(42), (k >> np.uint64(21)) & np.uint64(0x1FFFFF), k & np.uint64(0x1FFFFF)], 1)
    assert np.array_equal(back.astype(np.int64) - VC.KEY_OFFSET, edge)
    out = VC.range_outside_keys()
    assert out.shape == (8, 3)
    _, valid = VC.pack_key(out)
    assert not valid.any()
    # exactly one axis is outside, by one step (first six) or by far (last two); the other two are valid
    bad = (out < -VC.KEY_OFFSET) | (out >= VC.KEY_OFFSET)
    assert (bad.sum(1) == 1).all()
    assert sorted(map(tuple, np.argwhere(bad[:6]).tolist())) == [(i, i // 2) for i in range(6)]
    assert sorted(out[:6][bad[:6]].tolist()) == [-VC.KEY_OFFSET - 1] * 3 + [VC.KEY_OFFSET] * 3
    assert sorted(out[6:][bad[6:]].tolist()) == [-(1 << 40), 1 << 40]


def test_duplicate_case():
    distinct, occ = VC.duplicate_case()
    assert distinct.shape == (VC.DUP_KEYS, 3) and len(_as_set(distinct)) == VC.DUP_KEYS
    count = np.bincount(occ, minlength=VC.DUP_KEYS)
    assert len(occ) == VC.DUP_ROWS and count.min() >= 2 and count.max() <= 8 and len(set(count.tolist())) >= 5
    # shuffled: occurrences of a key lie far apart, in different workgroups of 256, for most keys
    first = np.full(VC.DUP_KEYS, -1)
    last = np.zeros(VC.DUP_KEYS, dtype=np.int64)
    for i, k in enumerate(occ.tolist()):
        if first[k] < 0:
            first[k] = i
        last[k] = i
    assert ((last // 256) != (first // 256)).mean() > 0.8
    # the order of first occurrence is not the order of the keys, nor that of the last occurrences
    assert not np.array_equal(np.argsort(first), np.arange(VC.DUP_KEYS))
    assert not np.array_equal(np.argsort(first), np.argsort(last))


def test_integrate_rows_is_the_oracles_integrate(orc):
    g = torch.Generator().manual_seed(2)
    pool = torch.from_numpy(VC.cube_coords(16))
    pool = pool[torch.randperm(len(pool), generator=g)]
    ovol = orc.OracleSparseVolume(8, 0.02, np.array([1.24] * 3), 8)
    ovol.insert(pool[:300], torch.randn(300, 8, generator=g), torch.rand(300, 1, generator=g) + 0.25,
                torch.randint(0, 5, (300, 1), generator=g).float())
    state = ovol.to_tensor()
    for lo, n in ((150, 400), (0, 1), (500, 333)):
        fc = pool[lo: lo + n]
        ff, pc = torch.randn(n, 8, generator=g), torch.randint(1, 80, (n,), generator=g)
        orc.integrate(ovol, fc, ff, pc.reshape(-1, 1))
        state = VC.integrate_rows(*state, fc, ff, pc)
        for a, b in zip(state, ovol.to_tensor()):
            assert a.shape == b.shape and torch.equal(a, b)


def test_grid_face_case_has_live_and_masked_values_at_the_faces(orc):
    """Case 7's condition, by the oracle alone: among the origins with a coordinate equal to 0 or n - 1, more than
    30 % of the lattice values are decoded and more than 10 % are masked; rows exist outside the grid next to every
    face, and some of them are missing or too light."""
    sd = orc.load_weights(WEIGHTS_FP32)
    c, f, w, origins, ref = VC.face_reference(orc, sd)
    assert len(origins) == 8 * 9 * 11 and ref.shape == (792, 27)
    face = VC.on_a_face(origins)
    assert face.sum() == 792 - 6 * 7 * 9                      # 414: most origins lie on a face, an edge or a corner
    live = (ref != VC.FACE_VOXEL)[torch.from_numpy(face)]
    print("live share on the faces", float(live.float().mean()))
    assert float(live.float().mean()) > 0.30 and float((~live).float().mean()) > 0.10
    n = np.asarray(VC.FACE_N_XYZ)
    outside = ((c < 0) | (c >= n)).any(1)
    have = _as_set(c)
    for axis in range(3):
        for layer in (-2, -1, int(n[axis]), int(n[axis]) + 1):
            sel = outside & (c[:, axis] == layer)
            assert sel.sum() > 50 and len(set(w[sel, 0].tolist())) == 3
    assert len(have) < len(VC.shell_coords()) * 0.92 and set(w[:, 0].tolist()) == set(VC.FACE_WEIGHTS)
    assert float(np.abs(f).max()) < 300.0                     # inside the decoder's certified feature range
