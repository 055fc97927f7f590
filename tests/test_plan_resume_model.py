"""CPU: tests/plan_resume_model.py pinned to tests/parse_plan_model.py — any cut is the whole, a single piece is want_walk, and a
piece of a unit whose references stay inside its pieces is a unit of its own."""
import functools

import numpy as np
import pytest

import ctx_sets_model as CS
import helpers as H
import parse_elements_model as E
import parse_plan_model as PM
import plan_resume_model as R
from test_parse_plan_model import TU_OUTCOMES


@functools.lru_cache(maxsize=None)
def mixed():
    """Transform units, lone blocks (a transform-skip one and a zero-out one among them) and block-free runs, the terminate bin last"""
    rng = np.random.default_rng(0x50A1)
    ts = ((8, 8, 0, H.TU_TRANSFORM_SKIP), H.random_block(rng, 8, 8, density=0.4))
    zo = ((32, 32, 0, H.TU_SBT_ZERO_OUT), np.pad(H.random_block(rng, 16, 16, density=0.3), ((0, 16), (0, 16))))
    segs = [("tu", PM.tu_case(rng, *TU_OUTCOMES[0])), ("block",) + ts] + R.random_segments(rng, [7]) + \
           [("block",) + zo, ("tu", PM.tu_case(rng, *TU_OUTCOMES[3 % len(TU_OUTCOMES)])), ("block",) + PM.chroma_block(rng)] + \
           R.random_segments(rng, [1]) + [R.flat_segment(rng, 70)]
    return R.join(rng, segs, qp=30)


def test_a_single_piece_is_want_walk():
    u, _ = mixed()
    (n_bits, flags, left), = R.expect(u, [])
    assert (n_bits, flags) == PM.want_walk(u) and flags == 0
    string = PM.expand(u["plan"], u["values"], u["metas"], u["blocks"], u["at"], u["guards"])[0]
    assert all(np.array_equal(a, b) for a, b in zip(left, CS.advance_from(string, CS.init_set(u["qp"], 2))))


def test_any_cut_is_the_whole():
    u, cuts = mixed()
    whole = PM.expand(u["plan"], u["values"], u["metas"], u["blocks"], u["at"], u["guards"])[0]
    n, nb = len(u["plan"]), len(u["metas"])
    # the cuts between the segments, with a piece of nothing, and every entry boundary of the unguarded tail
    tail = [c for c in R.entry_cuts(u) if c[0] > cuts[-2][0]]
    for cs in (cuts, [cuts[0], cuts[0]] + cuts[1:], cuts[:-2] + tail[:-1], []):
        spans = R.spans_of(u, cs)
        assert (spans[0][:2], spans[-1][2:]) == ((0, 0), (n, nb))
        parts = []
        for k, sp in enumerate(spans):
            p = R.piece_unit(u, sp, k == len(spans) - 1)
            parts.append(PM.expand(p["plan"], p["values"], p["metas"], p["blocks"], p["at"], p["guards"], p["infos"])[0])
            # the piece alone, walked by the writer's side, decides what the whole decided
            values, infos, coded, _ = PM.fill(p["plan"], p["values"], p["metas"], p["blocks"], p["at"], p["guards"])
            assert (values, infos, coded) == (p["values"], p["infos"], p["coded"]), (k, sp)
            assert np.array_equal(np.concatenate(parts + [np.zeros(0, np.uint16)]), R.prefix_string(u, sp[2], sp[3])), (k, sp)
        assert np.array_equal(np.concatenate(parts), whole)
        exp = R.expect(u, cs)
        assert exp[-1][:2] == PM.want_walk(u)
        bits = [e[0] for e in exp[:-1]]
        assert bits == sorted(bits) and all(e[1] == 0 for e in exp)
        for (_, _, e1, b1), (n_bits, _, _) in zip(spans[:-1], exp[:-1]):
            assert R.shifts_at(u, e1, b1) + 8 == n_bits
        assert all(np.array_equal(a, b) for a, b in zip(exp[-1][2], R.expect(u, [])[0][2]))
    # the kinds of piece the GPU tests need are there
    spans = R.spans_of(u, cuts)
    assert any(sp[0] == sp[2] and sp[3] == sp[1] + 1 for sp in spans), "a piece of one block and no entry"
    assert any(sp[2] == sp[0] + 1 and sp[1] == sp[3] for sp in spans), "a piece of one entry"


def test_what_is_no_cut_is_refused_and_a_reference_across_a_cut_is_seen():
    u, cuts = mixed()
    e = PM.TU_BLOCK_AT                                             # the first unit's three blocks stand in front of entry 10
    assert R.is_cut(u, e, 0) and R.is_cut(u, e, 3) and R.is_cut(u, e, 1)
    assert not R.is_cut(u, e + 1, 0) and not R.is_cut(u, e - 1, 3)
    with pytest.raises(AssertionError):
        R.spans_of(u, [(e + 1, 0)])
    assert R.references_stay_inside(u, cuts)
    assert not R.references_stay_inside(u, [(2, 0)])               # tu_cbf_cr's guard looks back at tu_cbf_cb
    assert not R.references_stay_inside(u, [(e, 3)])               # the BLOCK_INFO entries behind the blocks
