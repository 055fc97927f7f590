"""CPU: cabac_hip_sparse_pack_host / _unpack_host (csrc/cabac_sparse_host.cpp) against tests/sparse_model.py — every shape, both
element widths, the edges of a block's list, junk outside the coded region, odd offsets and gaps with sentinels, the capacity,
the int16 boundaries, every flag alone with first_bad, and the identities S1 and S2 of include/cabac_hip_sparse.h."""
import numpy as np
import pytest

import parse_corpus as PC
import sparse_model as M
from entropy_coding_amd import capi

SENT = {np.int16: 0x5A5A, np.int32: 0x5A5A5A5A}


def check_pack(tus, coeff, capacity=None, room=3):
    """pack_host against the model: firsts, entries, status; nothing written past the capacity."""
    w_first, w_ent, w_st = M.pack(tus, coeff, capacity)
    cap = w_st["n_entries"] if capacity is None else capacity
    entries = np.full(cap + room, 0xA5A5A5A5, np.uint32)
    first = np.full(len(tus) + 1 + room, 0xA5A5A5A5, np.uint32)
    before = coeff.copy()
    g_first, g_ent, st = capi.sparse_pack_host(tus, coeff, entry_capacity=cap, entries=entries, ent_first=first)
    assert M.status_dict(st) == w_st, (M.status_dict(st), w_st)
    assert np.array_equal(first[:len(tus) + 1], w_first) and np.all(first[len(tus) + 1:] == 0xA5A5A5A5)
    assert np.array_equal(entries[:min(cap, w_st["n_entries"])], w_ent)
    assert np.all(entries[cap:] == 0xA5A5A5A5)
    assert np.array_equal(coeff, before)
    for t in range(len(tus)):                                       # ascending pos inside every block
        e = w_ent[int(w_first[t]):min(int(w_first[t + 1]), len(w_ent))] & 0xFFFF
        assert np.all(np.diff(e.astype(np.int64)) > 0)
    return w_first, w_ent, w_st


def check_unpack(tus, first, entries, n_total, dtype, n_entries=None):
    """unpack_host against the model, both on an array of sentinels: equal everywhere, so nothing outside the good blocks moved."""
    want = np.full(n_total, SENT[dtype], dtype)
    got = want.copy()
    w_st = M.unpack(tus, first, entries, want, n_entries)
    st = capi.sparse_unpack_host(tus, first, entries, got, n_entries)
    assert M.status_dict(st) == w_st, (M.status_dict(st), w_st)
    assert np.array_equal(got, want)
    return got, w_st


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_every_shape_both_widths_round_trip(dtype):
    rng = np.random.default_rng(41)
    for density in (0.0, 0.1, 1.0):                                 # empty, sparse and full blocks
        tus, n_total = M.layout(M.ALL_SHAPES)
        coeff = M.fill(rng, tus, n_total, dtype, density=density)
        first, ent, st = check_pack(tus, coeff)
        assert st["flags"] == 0 and st["first_bad"] == M.NO_BAD
        if density == 0.0:
            assert st["n_entries"] == 0
        if density == 1.0:
            pass                                                    # (a level may still be drawn as 0)
        back, _ = check_unpack(tus, first, ent, n_total, dtype)
        for tu in tus:                                              # S2: the coded region reproduced, the rest of the block zero
            w, h, off = 1 << int(tu["log2_width"]), 1 << int(tu["log2_height"]), int(tu["coeff_offset"])
            a, b = coeff[off:off + w * h].reshape(h, w).copy(), back[off:off + w * h].reshape(h, w)
            a[32:, :] = 0
            a[:, 32:] = 0
            assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_single_entries_at_the_first_and_the_last_coded_position(dtype):
    tus, n_total = M.layout(M.ALL_SHAPES)
    for last in (False, True):
        coeff = np.zeros(n_total, dtype)
        want_pos = []
        for tu in tus:
            w, h, off = 1 << int(tu["log2_width"]), 1 << int(tu["log2_height"]), int(tu["coeff_offset"])
            pos = (min(h, 32) - 1) * w + min(w, 32) - 1 if last else 0
            coeff[off + pos] = -3
            want_pos.append(pos)
        first, ent, st = check_pack(tus, coeff)
        assert st["n_entries"] == len(tus) and np.array_equal(first, np.arange(len(tus) + 1))
        assert np.array_equal(ent & 0xFFFF, want_pos) and np.all(ent >> 16 == 0xFFFD)
        back, _ = check_unpack(tus, first, ent, n_total, dtype)
        assert np.array_equal(back, coeff)


def test_junk_outside_the_coded_region_is_ignored_by_pack_and_zeroed_by_unpack():
    rng = np.random.default_rng(42)
    tus, n_total = M.layout([(6, 6), (6, 2), (2, 6), (6, 0), (0, 6), (6, 5), (5, 6)])
    coeff = M.fill(rng, tus, n_total, np.int16, density=0.2, junk=True)
    first, ent, st = check_pack(tus, coeff)
    clean = coeff.copy()
    for tu in tus:
        w, h, off = 1 << int(tu["log2_width"]), 1 << int(tu["log2_height"]), int(tu["coeff_offset"])
        blk = clean[off:off + w * h].reshape(h, w)
        blk[32:, :] = 0
        blk[:, 32:] = 0
    assert not np.array_equal(clean, coeff)                         # there was junk
    f2, e2, _ = M.pack(tus, clean)
    assert np.array_equal(first, f2) and np.array_equal(ent, e2)
    back, _ = check_unpack(tus, first, ent, n_total, np.int16)
    assert np.array_equal(back, clean)


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_odd_offsets_gaps_and_sentinels(dtype):
    rng = np.random.default_rng(43)
    shapes = [(0, 1), (1, 1), (0, 0), (1, 0), (2, 2), (0, 1), (3, 1), (1, 1), (6, 6), (0, 1), (5, 5), (1, 1)] + M.mixed_shapes(rng, 40)
    tus, n_total = M.layout(shapes, rng, gaps=True, odd=True)
    assert any(int(t["coeff_offset"]) & 1 and 1 <= int(t["log2_width"]) + int(t["log2_height"]) <= 2 for t in tus)   # 1 x 2, 2 x 2 at odd offsets
    coeff = M.fill(rng, tus, n_total, dtype, density=0.4)
    first, ent, st = check_pack(tus, coeff)
    back, _ = check_unpack(tus, first, ent, n_total, dtype)         # (compared with the model on sentinels: the gaps stay)
    inside = np.zeros(n_total, bool)
    for tu in tus:
        inside[int(tu["coeff_offset"]):int(tu["coeff_offset"]) + (1 << (int(tu["log2_width"]) + int(tu["log2_height"])))] = True
    assert np.all(back[~inside] == SENT[dtype]) and (~inside).any()


def test_capacity_need_minus_one_and_zero():
    rng = np.random.default_rng(44)
    tus, n_total = M.layout(M.mixed_shapes(rng, 30), rng, gaps=True)
    coeff = M.fill(rng, tus, n_total, np.int16, density=0.5)
    need = M.pack(tus, coeff)[2]["n_entries"]
    assert need > 1
    for cap in (need - 1, 0):
        first, ent, st = check_pack(tus, coeff, capacity=cap)
        assert st["flags"] == M.OVERFLOW and st["n_entries"] == need and int(first[-1]) == need and st["first_bad"] == M.NO_BAD
    assert check_pack(tus, coeff, capacity=need)[2]["flags"] == 0


def test_int16_boundaries_and_a_wide_level_that_raises_range():
    tus, n_total = M.layout([(2, 2), (2, 2), (2, 2)])
    c16 = np.zeros(n_total, np.int16)
    c16[[0, 5, 16, 47]] = [-32768, 32767, -1, 1]
    first, ent, st = check_pack(tus, c16)
    assert st["flags"] == 0 and list(ent >> 16) == [0x8000, 0x7FFF, 0xFFFF, 1]
    assert np.array_equal(check_unpack(tus, first, ent, n_total, np.int16)[0], c16)
    c32 = c16.astype(np.int32)
    assert check_pack(tus, c32)[2]["flags"] == 0                    # the same levels from 32-bit blocks: in range
    assert np.array_equal(check_unpack(tus, first, ent, n_total, np.int32)[0], c32)   # sign-extended
    c32[20] = 40000
    first, ent, st = check_pack(tus, c32)
    assert st["flags"] == M.RANGE and st["first_bad"] == 1
    assert int(ent[int(first[1]) + 1]) == 4 | ((40000 & 0xFFFF) << 16)              # stored truncated
    c32[20] = -32769
    assert check_pack(tus, c32)[2]["flags"] == M.RANGE


def test_each_bad_flag_alone_with_first_bad():
    rng = np.random.default_rng(45)
    tus, n_total = M.layout([(2, 2)] * 6)
    coeff = M.fill(rng, tus, n_total, np.int16, density=0.6, sentinel=False)
    first, ent, _ = M.pack(tus, coeff)
    # BAD_POS: pos 16 in a 4 x 4 block
    e = ent.copy()
    k = int(first[3])
    assert int(first[4]) > k
    e[k] = (e[k] & 0xFFFF0000) | 16
    _, st = check_unpack(tus, first, e, n_total, np.int16)
    assert st["flags"] == M.BAD_POS and st["first_bad"] == 3
    # BAD_FIRST: descends / passes n_entries
    f = first.copy()
    f[2] = f[3] + 1
    _, st = check_unpack(tus, f, ent, n_total, np.int16)
    assert st["flags"] == M.BAD_FIRST and st["first_bad"] == 2
    _, st = check_unpack(tus, first, ent, n_total, np.int16, n_entries=int(first[5]) - 1)
    assert st["flags"] == M.BAD_FIRST and st["first_bad"] == 4 and st["n_entries"] == int(first[5]) - 1
    # BAD_BLOCK: log2 size 7, and a block that passes the end of the array
    for field, value in (("log2_width", 7), ("coeff_offset", n_total - 15)):
        bad = tus.copy()
        bad[1][field] = value
        _, st = check_unpack(bad, first, ent, n_total, np.int16)
        assert st["flags"] == M.BAD_BLOCK and st["first_bad"] == 1
        f2, e2, st = check_pack(bad, coeff)
        assert st["flags"] == M.BAD_BLOCK and st["first_bad"] == 1 and f2[1] == f2[2]


def test_refusals_of_the_host_forms():
    tus, n_total = M.layout([(2, 2)])
    L = capi.load_library()
    z = np.zeros(16, np.int16)
    f, e, s = np.zeros(2, np.uint32), np.zeros(16, np.uint32), np.zeros(1, capi.SPARSE_STATUS_DTYPE)
    args = (1, tus.ctypes.data, z.ctypes.data)
    assert L.cabac_hip_sparse_pack_host(*args, 3, 16, f.ctypes.data, e.ctypes.data, 16, s.ctypes.data) == -2        # coeff_bytes
    assert L.cabac_hip_sparse_pack_host(*args, 2, 1 << 32, f.ctypes.data, e.ctypes.data, 16, s.ctypes.data) == -2  # 32-bit firsts
    assert L.cabac_hip_sparse_pack_host(*args, 2, 16, f.ctypes.data, e.ctypes.data, 16, None) == -2
    assert L.cabac_hip_sparse_unpack_host(1, tus.ctypes.data, f.ctypes.data, e.ctypes.data, 0, z.ctypes.data, 2, 1 << 32, s.ctypes.data) == -2


def test_s1_and_s2_on_random_blocks_of_the_corpus():
    rng = np.random.default_rng(46)
    for case in range(200):
        blocks = [PC.random_tu(rng, PC.MIXED_STYLES[int(rng.integers(0, len(PC.MIXED_STYLES)))]) for _ in range(int(rng.integers(1, 5)))]
        shapes = [(int(np.log2(m[0])), int(np.log2(m[1]))) for m, _ in blocks]
        tus, n_total = M.layout(shapes, rng, gaps=True, odd=bool(case & 1))
        dtype = np.int16 if case % 3 else np.int32
        coeff = np.full(n_total, SENT[dtype], dtype)
        for tu, (m, c) in zip(tus, blocks):
            coeff[int(tu["coeff_offset"]):int(tu["coeff_offset"]) + c.size] = np.clip(c, -32768, 32767).ravel()
        first, ent, st = check_pack(tus, coeff)
        assert st["flags"] == 0
        back, _ = check_unpack(tus, first, ent, n_total, dtype)     # S2 (the corpus leaves nothing outside the coded region)
        assert np.array_equal(back, coeff)
        # S1: the entries of each block shuffled, expanded, compacted again
        shuffled = ent.copy()
        for t in range(len(tus)):
            lo, hi = int(first[t]), int(first[t + 1])
            shuffled[lo:hi] = rng.permutation(shuffled[lo:hi])
        again, _ = check_unpack(tus, first, shuffled, n_total, dtype)
        f2, e2, _ = check_pack(tus, again)
        assert np.array_equal(f2, first) and np.array_equal(e2, ent)
