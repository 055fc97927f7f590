"""CPU: tests/assemble_model.py against what it restates — its count against the oracle's orc_count_emulations (pinned to the
reference's OutputBitstream::countStartCodeEmulations in tests/test_oracle_vs_reference.py), its concatenation against
sharding.compact_payload — and the checks that keep the GPU cases of tests/test_gpu_assemble.py honest: that the crafted batches
reach the branches they are made for, computed from the model alone."""
import ctypes

import numpy as np

import assemble_model as M
import helpers as H


def oracle_count():
    orc = H.load_oracle()
    orc.lib.orc_count_emulations.argtypes = [H.u8p, ctypes.c_long]
    orc.lib.orc_count_emulations.restype = ctypes.c_int
    return lambda b: orc.lib.orc_count_emulations(H._ptr(np.ascontiguousarray(b, np.uint8), H.u8p), len(b))


def crafted_zero_runs():
    """The streams of test_gpu_assemble.test_count_emulations_on_crafted_zero_runs"""
    rng = np.random.default_rng(5)
    streams = [np.zeros(n, np.uint8) for n in (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 200, 1000)]
    for k in range(600):
        n = int(rng.integers(1, 400))
        p0 = float(rng.choice([0.3, 0.6, 0.9, 0.98]))
        streams.append(rng.choice(np.array([0, 1, 2, 3, 4, 255], np.uint8), size=n, p=[p0] + [(1 - p0) / 5] * 5).astype(np.uint8))
    for lead in range(0, 70, 3):
        for run in (2, 3, 4, 63, 64, 65, 130):
            streams.append(np.concatenate([np.full(lead, 9, np.uint8), np.zeros(run, np.uint8), np.array([1, 0, 0, 2, 0, 0, 0, 3, 7], np.uint8)]))
    return streams


def test_count_by_hand():
    for text, want in (("", 0), ("00", 0), ("00 00", 0), ("00 00 00", 1), ("00 00 01", 1), ("00 00 03", 1), ("00 00 04", 0),
                       ("00 00 00 00", 1), ("00 00 00 00 00", 2), ("00 00 00 00 01", 2), ("00 00 00 01", 1),
                       ("00 00 04 00 00 03", 1), ("01 00 00 02 00 00 02", 2), ("00 00 00 00 00 00 00", 3), ("ff 00 00", 0)):
        assert M.count_bytes(np.array(bytearray.fromhex(text), np.uint8)) == want, text


def test_count_is_the_oracles():
    orc_count = oracle_count()
    streams = crafted_zero_runs()
    for batch in [M.count_batch(n) for n in M.COUNT_N_SUBS] + [M.long_run_batch()]:
        d, r, slots = batch["desc"], batch["results"], batch["slots"]
        for partial in (False, True):                              # (with and without the last byte: more strings, both legitimate)
            n = M.fifo_bytes(d, r, partial=partial)
            streams += [slots[int(o): int(o) + int(k)] for o, k in zip(d["byte_offset"], n)]
    assert len(streams) > 4000
    got = [M.count_bytes(b) for b in streams]
    want = [orc_count(b) for b in streams]
    assert got == want and max(want) > 30000


def test_count_takes_whole_bytes_inside_the_slot():
    b = M.count_batch(5)
    d, r = b["desc"], b["results"]
    n = M.fifo_bytes(d, r)
    assert np.array_equal(n, np.minimum(r["n_bits"] // 8, d["byte_capacity"]))
    assert np.array_equal(M.counts_of(b), [M.count_bytes(b["slots"][int(o): int(o) + int(k)]) for o, k in zip(d["byte_offset"], n)])


def test_assemble_is_shardings_concatenation():
    from entropy_coding_amd import sharding
    for n_sub in (1, 5, 1025):
        b = M.shared_batch(n_sub)
        keep = b["kind"] != M.OVERFLOWED                           # (compact_payload knows no overflowed substreams)
        d, r = b["desc"][keep], b["results"][keep]
        want = sharding.compact_payload(d, b["slots"], r)
        offs = M.offsets(d, r)
        assert int(offs[-1]) == len(want) and np.array_equal(np.diff(offs.astype(np.int64)), (r["n_bits"].astype(np.int64) + 7) // 8)
        got = M.assemble(d, r, b["slots"], len(want) + 5, np.full(len(want) + 9, M.PAY_SENTINEL, np.uint8))
        assert np.array_equal(got[: len(want)], want) and (got[len(want):] == M.PAY_SENTINEL).all()
        short = M.assemble(d, r, b["slots"], len(want) - 3, np.full(len(want) + 9, M.PAY_SENTINEL, np.uint8))
        assert np.array_equal(short[: len(want) - 3], want[:-3]) and (short[len(want) - 3:] == M.PAY_SENTINEL).all()


def test_split_gather_pack_by_hand():
    d = np.zeros(3, H.DESC_DTYPE)
    d["byte_offset"], d["byte_capacity"] = [0, 16, 32], [5, 2, 16]
    pay = np.arange(1, 12, dtype=np.uint8)
    got = M.split(d, np.array([0, 3, 7, 11], np.uint64), pay, np.full(48, 0xEE, np.uint8))
    want = np.full(48, 0xEE, np.uint8)
    want[0:3], want[16:18], want[32:36] = [1, 2, 3], [4, 5], [8, 9, 10, 11]   # the second span is 4 bytes, its slot holds 2
    assert np.array_equal(got, want)
    src = np.arange(100, 120, dtype=np.uint16)
    got = M.gather([3, 0, 9], [1, 6, 8], [2, 0, 3], src, np.full(12, 7, np.uint16))
    assert got.tolist() == [7, 103, 104, 7, 7, 7, 7, 7, 109, 110, 111, 7]
    rng = np.random.default_rng(2)
    for n in (0, 1, 7, 8, 9, 2049):
        bins = rng.integers(0, 2, size=n, dtype=np.uint8)
        assert np.array_equal(M.pack_bins(bins | 0x80 * (n > 7)), np.packbits(bins, bitorder="little"))   # (only bit 0 of a bin counts)


# ------------------------------------------------------------------------------------------------ the GPU cases reach their branches
def test_partial_bytes_change_the_count():
    differs = 0
    for batch in [M.count_batch(n) for n in M.COUNT_N_SUBS] + [M.long_run_batch()]:
        d, r, slots = batch["desc"], batch["results"], batch["slots"]
        part = batch["kind"] == M.PARTIAL
        assert part.any() and ((r["n_bits"][part] & 7) != 0).all()
        assert np.array_equal(np.unique(r["n_bits"][part] & 7), np.arange(1, 8)) or len(d) < 30
        differs += int(np.count_nonzero(M.counts_of(batch)[part] != M.count(d, r, slots, partial=True)[part]))
    assert differs >= 20, differs


def test_bytes_behind_the_slot_would_add_matches():
    more = 0
    for batch in [M.count_batch(n) for n in M.COUNT_N_SUBS]:
        d, r, slots = batch["desc"], batch["results"], batch["slots"]
        over = batch["kind"] == M.OVERFLOWED
        assert (over.any() or len(d) == 1) and (r["n_bits"][over].astype(np.int64) > 8 * d["byte_capacity"][over].astype(np.int64)).all()
        more += int(np.count_nonzero(M.count(d, r, slots, clamp=False)[over] > M.counts_of(batch)[over]))
    assert more >= 20, more


def test_clipping_capacities_cut_at_every_byte_phase():
    for n_sub in M.N_SUBS:
        b = M.shared_batch(n_sub)
        offs = M.offsets(b["desc"], b["results"])
        total = int(offs[-1])
        caps = M.clip_capacities(offs)
        assert caps["total"] == total and caps["total+1"] > total and {"0", "1"} <= set(caps)
        if n_sub == 0:
            continue
        phases = set()
        for name, cap in caps.items():
            if name in ("total", "total+1") or cap >= total:
                assert name in ("total", "total+1") or (n_sub == 1 and name == "boundary"), (n_sub, name)
                continue
            s, left = M.cut_at(offs, cap)                           # a capacity below the total drops bytes
            full = M.assemble(b["desc"], b["results"], b["slots"], total, np.full(total, M.PAY_SENTINEL, np.uint8))
            assert 0 <= left < int(offs[s + 1]) - int(offs[s]) and (full[cap:] != M.PAY_SENTINEL).any()
            if left:
                phases.add(left % 4)
            if name == "boundary":
                assert left == 0 and s > 0
            if name == "tile_1":
                assert s >= 1024
        assert phases == {0, 1, 2, 3}, (n_sub, phases)
        assert ("tile_1" in caps) == (n_sub > 1024)


def test_overflowed_substreams_need_the_clamp():
    seen = 0
    for n_sub in M.N_SUBS:
        b = M.shared_batch(n_sub)
        d, r = b["desc"], b["results"]
        over = b["kind"] == M.OVERFLOWED
        assert (M.sizes(d, r, clamp=False)[over] > M.sizes(d, r)[over]).all() and (r["flags"][over] == H.RES_OVERFLOW).all()
        assert np.array_equal(M.sizes(d, r, clamp=False)[~over], M.sizes(d, r)[~over]) and not r["flags"][~over].any()
        assert np.array_equal(M.sizes(d, r), b["size"].astype(np.uint64))
        part = b["kind"] == M.PARTIAL
        assert ((r["n_bits"][part] & 7) != 0).all()
        # what lies right behind an overflowed slot differs from what the payload holds before the call
        for s in np.nonzero(over)[0]:
            end = int(d["byte_offset"][s]) + int(d["byte_capacity"][s])
            assert end == len(b["slots"]) or b["slots"][end] != M.PAY_SENTINEL
        seen += int(over.sum())
        assert n_sub < 3 or over.any()
    assert seen > 700


def test_wide_offsets_exceed_their_slots():
    b = M.shared_batch(1025)
    offs, pay = M.wide_offsets(b)
    span = np.diff(offs.astype(np.int64))
    assert np.count_nonzero(span > b["desc"]["byte_capacity"].astype(np.int64)) >= 500 and len(pay) == int(offs[-1])
