"""CPU: tests/search_model.py, the model the GPU tests of the search rounds compare with.

1. The contexts the model carries from round to round are the compiled reference's: a chain started from ctx_init(qp, init) is
   advanced for several rounds by the model; the model's cost of EVERY candidate of round k, started from the set the model
   committed, must equal ref.estimate_from_history(hist = the winners' records of rounds 0 .. k-1, rec = the candidate's
   records, qp, init) — the reference codes the history with its own update() (contexts.cpp:903-913), assigns the contexts to a
   fresh estimator (Ctx::operator=, contexts.hpp:254) and costs the candidate.  The states it started from are compared too.
2. select: ties, an empty group, all candidates excluded, saturation, a NULL distortion — against numbers worked out by hand."""
import numpy as np
import pytest

import helpers as H
import search_model as M
from test_gpu_residual import make_tus

TS, BDPCM, TS_FLAG, DQ, SH = H.TU_TRANSFORM_SKIP, H.TU_BDPCM, H.TU_TS_FLAG, H.TU_DEP_QUANT, H.TU_SIGN_HIDING


def _ts_like(rng, w, h):
    c = rng.integers(-3, 4, (h, w)).astype(np.int32) * (rng.random((h, w)) < 0.6)
    if not c.any():
        c[0, 0] = 2
    return c.astype(np.int32)


def _candidates(rng, kind):
    """One group: 3 alternatives of 2 blocks each (a luma and a chroma block, or two of one kind)."""
    blocks, chromas, flags = [], [], []
    for _ in range(3):
        for ch in (0, 1):
            w, h = [(4, 4), (8, 8), (16, 16), (8, 4), (32, 32)][int(rng.integers(0, 5))]
            if kind == "regular":
                blocks.append(H.random_block(rng, w, h, density=0.6, big=0.1)); flags.append(SH)
            elif kind == "dq":
                blocks.append(H.random_block(rng, w, h, density=0.6, big=0.1)); flags.append(DQ)
            elif kind == "ts":
                blocks.append(_ts_like(rng, w, h)); flags.append(TS | TS_FLAG)
            else:
                blocks.append(_ts_like(rng, w, h)); flags.append(TS | BDPCM)
            chromas.append(ch)
    return blocks, chromas, flags


@pytest.mark.parametrize("qp,init", [(22, 0), (32, 1), (37, 2)])
def test_carried_contexts_are_the_reference_s(qp, init):
    ref, orc = H.load_ref(), H.load_oracle()
    rng = np.random.default_rng(0x5EA2C4 + qp)
    sets = [orc.ctx_init(qp, init)]
    hist = np.zeros(0, np.uint16)
    lam = (1 << 31) + 12345
    for k, kind in enumerate(["regular", "ts", "dq", "bdpcm", "regular", "dq", "ts", "bdpcm"]):
        blocks, chromas, flags = _candidates(rng, kind)
        tus, _ = make_tus(blocks, chromas, flags)
        cand_first = np.arange(0, 7, 2, dtype=np.uint32)
        dist = rng.integers(0, 1 << 20, 3).astype(np.uint64)
        bits, pick, cost, new_sets, _, _, recs = M.round_model([0, 3], cand_first, blocks, tus, sets, [0, 0, 0], [0], dist, lam)
        for c in range(3):
            rc, want, s0, s1, rate = ref.estimate_from_history(hist, recs[c], qp, init)
            assert rc == 0 and int(bits[c]) == want, (k, kind, c)
            assert np.array_equal(s0, sets[0][0]) and np.array_equal(s1, sets[0][1]) and np.array_equal(rate, sets[0][2]), (k, c)
        w = int(pick[0])
        assert w == min(range(3), key=lambda c: (M.cost_of(bits[c], dist[c], lam), c)) and int(cost[0]) == M.cost_of(bits[w], dist[w], lam)
        hist = np.concatenate([hist, recs[w]])
        sets = new_sets
    # and the set after the last round
    rc, _, s0, s1, rate = ref.estimate_from_history(hist, np.zeros(0, np.uint16), qp, init)
    assert rc == 0 and np.array_equal(s0, sets[0][0]) and np.array_equal(s1, sets[0][1]) and np.array_equal(rate, sets[0][2])


def test_select_edge_cases():
    U = M.U64_MAX
    one = 1 << 31                                   # lambda 1.0 against SCALE_BITS: cost = dist + frac_bits
    # ties go to the lowest index; an empty group; a group with every candidate excluded
    frac = [7, 5, 5, 9, 3, 3, 3, 1]
    pick, cost = M.select([0, 4, 4, 7, 8], frac, None, one)
    assert pick.tolist() == [1, M.NONE, 4, 7] and cost.tolist() == [5, U, 3, 1]
    dist = [0, 0, 0, 0, U, U, U, 2]
    pick, cost = M.select([0, 4, 4, 7, 8], frac, dist, one)
    assert pick.tolist() == [1, M.NONE, M.NONE, 7] and cost.tolist() == [5, U, U, 3]
    # an excluded candidate does not win a tie, a distortion breaks one
    pick, cost = M.select([0, 3], [5, 5, 5], [U, 1, 0], one)
    assert pick.tolist() == [2] and cost.tolist() == [5]
    # the product is floored after the full 128-bit multiplication
    assert M.cost_of(3, 10, 1 << 30) == 11 and M.cost_of((1 << 64) - 1, 0, 1 << 31) == (1 << 64) - 1 - 1   # saturates at 2^64 - 2
    assert M.cost_of((1 << 64) - 1, 0, (1 << 31) - 1) == (((1 << 64) - 1) * ((1 << 31) - 1)) >> 31
    assert M.cost_of(1 << 40, 0, 1 << 60) == U - 1 and M.cost_of(0, U - 1, 5) == U - 1 and M.cost_of(1, U - 1, one) == U - 1
    # saturated candidates still compare equal: the lowest index wins, and the cost is 2^64 - 2, not "none"
    pick, cost = M.select([0, 3], [1 << 63, 1 << 62, 5], [0, 0, U], 1 << 40)
    assert pick.tolist() == [0] and cost.tolist() == [U - 1]
    # runs are clipped to group_first[-1]; one that goes backwards is empty
    pick, cost = M.select([0, 9, 2, 3], [4, 3, 2, 1], None, one)
    assert pick.tolist() == [2, M.NONE, 2] and cost.tolist() == [2, U, 2]
    pick, cost = M.select([0, 2, 4], [4, 3, 2, 1], None, one, n_cand_max=3)
    assert pick.tolist() == [1, 2]
