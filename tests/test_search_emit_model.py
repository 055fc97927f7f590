"""CPU: tests/search_emit_model.py, the model the GPU tests of the winner log (include/cabac_hip_search_emit.h) compare with.

1. Pinned to the compiled reference with what libcabac_ref already exports: six rounds over 3 chains with 1 .. 5 alternatives
   a group; the winners' expanded strings (search_unit_model.round_model's own) concatenated per chain must be the strings the
   log model emits, ref_encode_records of them must give the model's bytes, and the set every chain has committed after the
   last round must be advance() over its emitted string from ctx_init(qp, init_id).
2. Clipping, positions and rebasing of the log on hand-written cases.
3. All or nothing."""
import numpy as np
import pytest

import helpers as H
import search_emit_model as E
import search_unit_model as U
from test_gpu_residual import make_tus
from test_gpu_residual_estimate import advance


@pytest.mark.parametrize("seed", [0, 1])
def test_emitted_bytes_and_committed_sets_are_the_reference_s(seed):
    ref, orc = H.load_ref(), H.load_oracle()
    rng = np.random.default_rng(0xE317 + seed)
    K = 3
    qp, init = rng.integers(20, 40, K), rng.integers(0, 3, K)
    sets = [orc.ctx_init(int(qp[k]), int(init[k])) for k in range(K)]
    log = E.LogModel(K)
    want = [[] for _ in range(K)]
    sizes = set()
    for r in range(6):
        c, gf, which = E.search_round(rng, K, 5)
        sizes |= set(np.diff(gf).tolist())
        dist = rng.integers(0, 3000, c.n_cand).astype(np.uint64)
        out_set = np.arange(K, dtype=np.uint32)
        _, pick, _, sets, _, _, strings, fl = U.round_model(gf, c.cand_first, c.blocks, c.tus, sets, which, c.rec_first, c.records, c.tu_at,
                                                            out_set, dist, 3 << 15)
        assert not fl.any() and (pick != E.NONE).all()
        assert log.append(pick, np.arange(K, dtype=np.uint32), c.cand_first, c.tus, c.coeff, c.rec_first, c.records, c.tu_at)
        for k in range(K):
            want[k].append(strings[int(pick[k])])
    pick, cf, rf, recs = E.tail_round(K)
    assert log.append(pick, np.arange(K, dtype=np.uint32), cf, np.zeros(0, H.TU_DTYPE), np.zeros(0, np.int32), rf, recs, None)
    assert sizes >= {1, 5} and len(log.entries) == 7 * K
    payload, offsets, bits, info, counts, strings = log.emit(qp, init, 3)
    for k in range(K):
        whole = np.concatenate(want[k] + [recs[k:k + 1]])
        assert np.array_equal(strings[k], whole), k                        # the log expands to what the rounds costed
        b, nb = ref.encode_records(whole, int(qp[k]), int(init[k]), 3)
        assert np.array_equal(payload[int(offsets[k]):int(offsets[k + 1])], b) and nb == int(bits[k]), k
        s0, s1, rate = orc.ctx_init(int(qp[k]), int(init[k]))
        s0, s1 = s0.astype(np.int64), s1.astype(np.int64)
        advance(s0, s1, rate, strings[k])
        assert np.array_equal(s0.astype(np.uint16), sets[k][0]) and np.array_equal(s1.astype(np.uint16), sets[k][1]), k
        assert np.array_equal(rate, sets[k][2]) and np.array_equal(counts[k], E.counts_of(whole))
    assert not (info & (H.TU_INFO_EMPTY | H.TU_INFO_BAD_DESC)).any()


def _four_blocks():
    blocks = [np.full((4, 4), v, np.int32) for v in (1, 2, 3, 4)]
    tus, coeff = make_tus(blocks, [0, 0, 1, 1], [0, 0, 0, 0])
    return blocks, tus, coeff


def test_positions_clipping_and_rebasing_by_hand():
    blocks, tus, coeff = _four_blocks()
    records = np.arange(100, 110, dtype=np.uint16)
    # candidate 0: blocks 0..2 in records [0, 6); candidate 1: a run that goes backwards, block 3; candidate 2: no block, [4, 10)
    cand_first = np.array([0, 3, 4, 4], np.uint32)
    rec_first = np.array([0, 6, 4, 10], np.uint64)
    log = E.LogModel(4)
    # a tu_at going backwards stays, one past the run is clamped to its end
    assert log.append([0], [2], cand_first, tus, coeff, rec_first, records, np.array([4, 1, 99, 0], np.uint32))
    # NULL positions: every block behind the run
    assert log.append([0, E.NONE, 2], [3, 1, 0], cand_first, tus, coeff, rec_first, records, None)
    # a backwards rec_first is an empty run; its block sits at 0 whatever tu_at says; a pick >= n_cand and a chain >= n_chain append nothing
    assert log.append([1, 3, 0, 0], [1, 0, 4, E.NO_CHAIN], cand_first, tus, coeff, rec_first, records, np.array([0, 0, 0, 7], np.uint32))
    a = log.arrays()
    assert a["tu_at"].tolist() == [4, 4, 6, 6, 6, 6, 0]
    assert a["records"].tolist() == list(range(100, 106)) * 2 + list(range(104, 110))
    assert a["entries"].tolist() == [(0, 2, 6, 3, 0, 0, 0), (6, 3, 6, 3, 3, 0, 0), (12, 0, 6, 0, 6, 0, 0), (18, 1, 0, 1, 6, 0, 0)]
    assert a["tu"]["coeff_offset"].tolist() == [0, 16, 32, 48, 64, 80, 96] and a["tu"]["channel"].tolist() == [0, 0, 1, 0, 0, 1, 1]
    assert a["coeff"].tolist() == [v for v in (1, 2, 3, 1, 2, 3, 4) for _ in range(16)]
    assert (int(a["counters"]["n_entry"]), int(a["counters"]["n_record"]), int(a["counters"]["n_tu"]), int(a["counters"]["n_coeff"]),
            int(a["counters"]["flags"])) == (4, 18, 7, 112, 0)
    # a second entry of a chain starts behind the first: chain 2 gets candidate 2, then candidate 0
    assert log.append([2], [2], cand_first, tus, coeff, rec_first, records, None)
    assert log.append([0], [2], cand_first, tus, coeff, rec_first, records, np.array([0, 0, 0, 0], np.uint32))
    assert log.arrays()["entries"][-2:].tolist() == [(18, 2, 6, 0, 7, 6, 3), (24, 2, 6, 3, 7, 12, 3)]
    strings, _, spans = log.strings()
    assert spans[0][0] == 2 and spans[-1] == (2, spans[-2][2], len(strings[2])) and len(strings[1]) == len(E.block_records(blocks, tus, 3)[0])
    lens, recs, first, splices = log.host_form()
    assert lens.tolist() == [6, 0, 18, 6] and first.tolist() == [0, 0, 1, 7, 10]
    assert splices.tolist() == [(0, 6), (4, 0), (4, 1), (6, 2), (12, 7), (12, 8), (12, 9), (6, 3), (6, 4), (6, 5)]
    # a descriptor with a log2 size above 6 copies nothing and keeps the rest of itself
    bad = tus.copy()
    bad[1]["log2_width"] = 7
    log = E.LogModel(1, int16=True)
    assert log.append([0], [0], cand_first, bad, coeff, rec_first, records, None)
    a = log.arrays()
    assert a["tu"]["coeff_offset"].tolist() == [0, 16, 16] and a["tu"]["log2_width"].tolist() == [2, 7, 2] and len(a["coeff"]) == 32
    assert a["coeff"].dtype == np.int16 and log.strings()[1][1] == H.TU_INFO_BAD_DESC


def test_a_call_is_all_or_nothing():
    _, tus, coeff = _four_blocks()
    records = np.arange(100, 110, dtype=np.uint16)
    cand_first, rec_first = np.array([0, 3, 4], np.uint32), np.array([0, 6, 10], np.uint64)
    for caps, bit in (((2, 14, 5, 80), E.OVER_ENTRIES), ((3, 13, 5, 80), E.OVER_RECORDS), ((3, 14, 4, 80), E.OVER_BLOCKS),
                      ((3, 14, 5, 79), E.OVER_COEFFS), ((2, 13, 4, 79), 0xF0)):
        log = E.LogModel(2, *caps)
        assert log.append([1], [0], cand_first, tus, coeff, rec_first, records, None)
        before = log.arrays()
        assert not log.append([0, 1], [1, 0], cand_first, tus, coeff, rec_first, records, None)
        after = log.arrays()
        assert int(after["counters"]["flags"]) == E.OVERFLOW | bit
        after["counters"]["flags"] = 0
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        assert log.chain_rec == [4, 0] and log.chain_tu == [1, 0]
        log.reset()
        assert log.arrays()["counters"]["flags"] == 0 and not log.entries
    log = E.LogModel(2, 3, 14, 5, 80)
    assert log.append([1], [0], cand_first, tus, coeff, rec_first, records, None)
    assert log.append([0, 1], [1, 0], cand_first, tus, coeff, rec_first, records, None)                 # an exact fit
