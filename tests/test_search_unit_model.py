"""CPU: tests/search_unit_model.py, the model the GPU tests of the search rounds over candidates with side records compare with.

1. With no side records the model is tests/search_model.py's.
2. The model is pinned to the compiled reference as tests/test_search_model.py pins that one: a chain started from
   ctx_init(qp, init) is advanced for several rounds; the model's cost of EVERY candidate, started from the set the model
   committed, must equal ref.estimate_from_history(hist = the winners' expanded strings of the rounds before, rec = the
   candidate's expanded string, qp, init), and the set it started from must be the one the reference reached.
3. Clamping of tu_at and clipping of rec_first, against strings worked out by hand.
4. An align record behind a block rounds a total that includes the block."""
import numpy as np
import pytest

import helpers as H
import search_model as M0
import search_unit_model as M
from test_gpu_residual import make_tus
from test_search_model import _candidates, _ts_like

TS, TS_FLAG, SH = H.TU_TRANSFORM_SKIP, H.TU_TS_FLAG, H.TU_SIGN_HIDING


def _same_set(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_no_side_records_is_the_block_model():
    orc = H.load_oracle()
    rng = np.random.default_rng(0x51DE0)
    sets = [orc.ctx_init(30, 1), orc.ctx_init(22, 0)]
    blocks, chromas, flags = _candidates(rng, "regular")
    b2, c2, f2 = _candidates(rng, "ts")
    blocks, chromas, flags = blocks + b2, chromas + c2, flags + f2
    blocks[3] = np.zeros_like(blocks[3])                                   # an empty block
    tus, _ = make_tus(blocks, chromas, flags)
    tus[8]["channel"] = 2                                                  # a bad descriptor
    cand_first = np.array([0, 2, 4, 4, 7, 9, 12], np.uint32)                # one candidate without a block
    which = [0, 1, 0, 1, 0, 1]
    rec_first = np.zeros(7, np.uint64)
    none = np.zeros(0, np.uint16)
    for tu_at in (None, np.full(12, 5, np.uint32)):
        for c in range(6):
            a = M.walk_candidate(blocks, tus, int(cand_first[c]), int(cand_first[c + 1]), none, tu_at, sets[which[c]])
            b = M0.walk_candidate(blocks, tus, int(cand_first[c]), int(cand_first[c + 1]), sets[which[c]])
            assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and _same_set(a[3], b[3]) and np.array_equal(a[4], b[4]) and a[5] == 0
        dist = rng.integers(0, 1 << 16, 6).astype(np.uint64)
        got = M.round_model([0, 3, 6], cand_first, blocks, tus, sets, which, rec_first, none, tu_at, [0, 1], dist, 3 << 30)
        want = M0.round_model([0, 3, 6], cand_first, blocks, tus, sets, which, [0, 1], dist, 3 << 30)
        for k in (0, 1, 2, 4, 5):
            assert np.array_equal(got[k], want[k]), k
        assert all(_same_set(a, b) for a, b in zip(got[3], want[3])) and not got[7].any()
        assert all(np.array_equal(a, b) for a, b in zip(got[6], want[6]))


def _unit_candidates(rng, k):
    """One group of 4 alternatives: two blocks with a side run around them (a transform_skip_flag record in front of a
    transform-skip block), one block with side records on one side only, a side-only alternative, and a plain one."""
    blocks, chromas, flags, first, runs, at = [], [], [], [0], [], []
    kind = ["regular", "ts", "dq", "bdpcm", "regular", "ts"][k % 6]
    b, c, f = _candidates(rng, kind)
    # alternative 0: two blocks, 30 side records, one block in the middle and one at the end
    blocks += b[0:2]; chromas += c[0:2]; flags += f[0:2]
    runs.append(M.side_run(rng, 30, ts_flag=0, trm=(k % 2 == 0), align=(k % 3 == 0))); at += [int(rng.integers(0, 31)), 30]
    first.append(len(blocks))
    # alternative 1: a transform-skip luma block behind its transform_skip_flag (context 310), three records behind it
    blocks.append(_ts_like(rng, 8, 8)); chromas.append(0); flags.append(TS)
    run = M.side_run(rng, 12)
    run[8] = 310 | 0x8000
    runs.append(run); at.append(9)
    first.append(len(blocks))
    # alternative 2: side records only ("all cbf zero")
    runs.append(M.side_run(rng, 17, ts_flag=1))
    first.append(len(blocks))
    # alternative 3: one block, no side records
    blocks.append(b[2]); chromas.append(c[2]); flags.append(f[2])
    runs.append(np.zeros(0, np.uint16)); at.append(0)
    first.append(len(blocks))
    rec_first = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.uint64)
    return blocks, chromas, flags, np.asarray(first, np.uint32), rec_first, np.concatenate(runs), np.asarray(at, np.uint32)


@pytest.mark.parametrize("qp,init", [(22, 0), (32, 1), (37, 2)])
def test_costs_and_carried_contexts_are_the_reference_s(qp, init):
    ref, orc = H.load_ref(), H.load_oracle()
    rng = np.random.default_rng(0x5EA2C5 + qp)
    sets = [orc.ctx_init(qp, init)]
    hist = np.zeros(0, np.uint16)
    lam = (1 << 31) + 4321
    winners, touched = set(), set()
    for k in range(6):
        blocks, chromas, flags, cand_first, rec_first, records, tu_at = _unit_candidates(rng, k)
        tus, _ = make_tus(blocks, chromas, flags)
        dist = rng.integers(0, 1 << 25, 4).astype(np.uint64)         # about the spread of the rates
        if k == 1:
            dist[[0, 1, 3]] = M.U64_MAX                                    # the side-only alternative wins at least once
        bits, pick, cost, new_sets, _, _, strings, fl = M.round_model([0, 4], cand_first, blocks, tus, sets, [0] * 4, rec_first, records,
                                                                      tu_at, [0], dist, lam)
        assert not fl.any()
        for c in range(4):
            rc, want, s0, s1, rate = ref.estimate_from_history(hist, strings[c], qp, init)
            assert rc == 0 and int(bits[c]) == want, (k, c)
            assert _same_set((s0, s1, rate), sets[0]), (k, c)
            touched |= set(int(r) & 0x1FF for r in strings[c])
        w = int(pick[0])
        assert int(cost[0]) == M.cost_of(bits[w], dist[w], lam)
        winners.add(w)
        hist = np.concatenate([hist, strings[w]])
        sets = new_sets
    rc, _, s0, s1, rate = ref.estimate_from_history(hist, np.zeros(0, np.uint16), qp, init)
    assert rc == 0 and _same_set((s0, s1, rate), sets[0])
    assert 2 in winners and len(winners) >= 2
    assert {310, 311} <= touched and any(i < 86 for i in touched) and any(292 <= i < 357 for i in touched)


def test_positions_are_clamped_and_runs_are_clipped():
    S = np.arange(100, 106, dtype=np.uint16)                               # six side records, recognisable
    A, B, C = np.array([1, 2], np.uint16), np.array([3], np.uint16), np.array([4, 5], np.uint16)
    s, spans = M.expand(S, [2, 2, 4], [A, B, C])                           # two blocks at one position keep their order
    assert s.tolist() == [100, 101, 1, 2, 3, 102, 103, 4, 5, 104, 105] and spans == [(2, 4), (4, 5), (7, 9)]
    s, spans = M.expand(S, [4, 1, 99], [A, B, C])                          # a position going backwards stays; one past the end clamps
    assert s.tolist() == [100, 101, 102, 103, 1, 2, 3, 104, 105, 4, 5] and spans == [(4, 6), (6, 7), (9, 11)]
    s, spans = M.expand(S, [0, None, 3], [A, None, C])                     # None: behind the run; an empty block contributes nothing
    assert s.tolist() == [1, 2, 100, 101, 102, 103, 104, 105, 4, 5] and spans == [(0, 2), (8, 8), (8, 10)]
    s, spans = M.expand(S[:0], [7], [A])
    assert s.tolist() == [1, 2] and spans == [(0, 2)]
    s, spans = M.expand(S, [], [])
    assert s.tolist() == S.tolist() and spans == []
    assert M.positions([5, 3, 0xFFFFFFFF, 1], 9) == [5, 5, 9, 9]
    # rec_first: clipped to its last entry, a run that goes backwards is empty
    rf = [0, 9, 4, 6, 6]
    assert [M.clip_run(rf, c) for c in range(4)] == [(0, 6), (6, 0), (4, 2), (6, 0)]
    assert M.is_bad([0x1FC]) and M.is_bad([0x81FB, 5]) and M.is_bad([379]) and not M.is_bad([378, 0x1FD, 0x1FE, 0x81FF])


def test_align_behind_a_block_rounds_a_total_that_includes_the_block():
    orc = H.load_oracle()
    rng = np.random.default_rng(0xA11)
    start = orc.ctx_init(27, 2)
    found = 0
    for _ in range(8):
        blocks = [H.random_block(rng, 8, 8, density=0.5, big=0.1)]
        tus, _ = make_tus(blocks, [0], [SH])
        side = np.array([M.REC_EP, 20 | 0x8000, M.REC_ALIGN, 300, M.REC_EP | 0x8000], np.uint16)
        bits, shares, _, _, string, fl = M.walk_candidate(blocks, tus, 0, 1, side, [2], start)
        front = orc.estimate_records_from(side[:2], *start)[1]
        s0, s1, rate = start[0].astype(np.int64), start[1].astype(np.int64), start[2].copy()
        M.advance(s0, s1, rate, string[:-2])
        tail = orc.estimate_records_from(side[3:], s0.astype(np.uint16), s1.astype(np.uint16), rate)[1]
        assert fl == 0 and string[-3] == M.REC_ALIGN and bits == ((front + shares[0] + 0x7FFF) & ~0x7FFF) + tail
        moved = M.walk_candidate(blocks, tus, 0, 1, side, [5], start)[0]    # the block behind the align: it is not rounded
        found += bits != moved and (front + shares[0]) % 0x8000 != 0
    assert found
