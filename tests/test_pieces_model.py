"""CPU: tests/pieces_model.py pinned to itself and to the models it is composed of: any cut is the whole, a single piece is
emit_model.Replay, pend < 16 behind every piece, the state's words add up, and the oracle's prefixes chain through the sets."""
import numpy as np
import pytest

import ctx_sets_model as M
import emit_model as E
import helpers as H
import pieces_model as P


def _free_cases(step=7):
    return [(name, rec) for name, rec, n_head in E.all_families()[::step] if n_head == len(rec)]


def test_a_single_piece_is_the_replay_of_the_emission_tests():
    for name, rec in _free_cases(5):
        whole = E.Replay(rec)
        rp, states = P.replay_pieces(rec, [])
        assert not states and bytes(rp.out) == bytes(whole.out) and rp.n_bits == whole.n_bits, name
        probe = E.Replay(rec, finish=False)
        first = P.PieceReplay().feed(rec)
        assert (first.pos, first.buf, first.nbuf, first.pend, first.low) == (probe.pos, probe.buf, probe.nbuf, probe.pend, probe.low), name


def test_any_cut_is_the_whole_and_pend_stays_under_16():
    rng = np.random.default_rng(77)
    for name, rec in _free_cases():
        whole = E.Replay(rec)
        want, n_bits = E.finished_bytes(E.code(rec))
        assert bytes(whole.out) == want.tobytes() and whole.n_bits == n_bits
        cut_sets = [[k] for k in (0, 1, len(rec) // 2, len(rec) - 1, len(rec))] + [list(range(1, len(rec)))[:40]]
        cut_sets += [sorted(int(x) for x in rng.integers(0, len(rec) + 1, size=3)) for _ in range(3)]
        for cuts in cut_sets:
            rp, states = P.replay_pieces(rec, cuts)
            assert bytes(rp.out) == bytes(whole.out) and rp.n_bits == whole.n_bits, (name, cuts)
            for (first, end), st in zip(P.pieces_of(len(rec), cuts), states):
                low, rp_word, buf, nbuf = st["priv"]
                pend, rng_ = rp_word >> 16, rp_word & 0xFFFF
                assert pend < 16 and 256 <= rng_ <= 510 and low < 1 << (10 + pend), (name, cuts)
                assert st["bytes_final"] % 2 == 0 and st["bits"] == 8 * st["bytes_final"] + 16 * nbuf + pend
                assert st["bits"] == E.code(rec[:end]).S            # getNumWrittenBits(): the sum of the shifts
                assert bytes(whole.out[:st["bytes_final"]]) == bytes(rp.out[:st["bytes_final"]])


def test_the_cut_moves_bytes_final_but_not_the_bytes():
    """The same prefix behind different cuts: the same bits, not always the same bytes_final (a piece hands over every whole
    unit it has; the one-call form looks every fourth bin of ITS steps)."""
    seen = set()
    for name, rec in _free_cases(3):
        k = len(rec) // 2
        a = P.replay_pieces(rec, [k])[1][0]
        b = P.replay_pieces(rec, [max(k - 3, 0), k])[1][1]
        assert a["bits"] == b["bits"], name
        seen.add(a["bytes_final"] == b["bytes_final"])
    assert True in seen


def test_cross_census_sees_every_event_on_directed_cuts():
    fams = {name: rec for name, rec, n_head in E.all_families() if n_head == len(rec)}
    cases = [(fams["trm1/16/0"], [8, 12]), (fams["grid/K1/f0/e1"], [35]), (fams["grid/K1/f0/e0"], [6, 28, 34])]
    sib = fams["long-sibling/K8"]
    cases.append((sib, [len(sib)]))                      # the cut directly in front of the finish that resolves the run
    cen = P.cross_census(cases)
    for ev in P.CROSS_EVENTS + ("run3",):
        assert cen.get(ev), (ev, cen)


def test_overflow_is_the_one_call_forms():
    for name, rec in E.capacity_cases():
        if not E.is_free(rec):
            continue
        n = len(E.finished_bytes(E.code(rec))[0])
        for cap in (0, 1, n // 2, n - 1, n, n + 1):
            at = P.overflows_at(rec, [len(rec) // 3, 2 * len(rec) // 3], cap)
            assert (at is not None) == (n > cap), (name, cap, at)


def test_oracle_prefixes_chain_through_the_sets():
    """encode_from / decode_from on prefixes and advance_from between them: the composition the GPU tests compare with."""
    rng = np.random.default_rng(78)
    rec = H.random_records(rng, 69, ctx_frac=0.8, ctx_pool=np.arange(86, 292))
    ctx = M.init_set(30, 1)
    per, data = P.encode_pieces(rec, [20, 20, 55], ctx)
    rc, whole, nbits, left = M.encode_from(rec, ctx, 3)
    assert rc >= 0 and np.array_equal(data, whole) and per[-1][0] == nbits
    assert [p[0] for p in per[:-1]] == sorted(p[0] for p in per[:-1]) and per[0][0] == per[1][0]
    between = P.contexts_between(rec, [20, 20, 55], ctx)
    for k, (first, end) in enumerate(P.pieces_of(len(rec), [20, 20, 55])):
        want = M.advance_from(rec[:end], ctx)
        assert all(np.array_equal(a, b) for a, b in zip(per[k][2], want))
        assert all(np.array_equal(a, b) for a, b in zip(between[k], M.advance_from(rec[:first], ctx)))
    dper, bins = P.decode_pieces(rec, [20, 20, 55], ctx, whole)
    assert np.array_equal(bins, rec >> 15) and dper[-1][1] == 0
    assert all(np.array_equal(a, b) for a, b in zip(dper[-1][2], left))
