"""CPU: tests/plan_continue_model.py pinned to tests/write_plan_model.py and the oracle — the bytes behind the last piece are the
one plan write's for every way of cutting, the bits behind every piece are the oracle's written bits of the prefix, and a piece's
own walk finds what the header says it finds."""
import functools

import numpy as np

import helpers as H
import parse_elements_model as E
import parse_plan_model as PM
import plan_continue_model as C
import plan_resume_model as R
import write_plan_model as W
from test_parse_plan_model import TU_OUTCOMES
from test_plan_resume_model import mixed


@functools.lru_cache(maxsize=None)
def joined():
    """TU segments joined with flat runs and a lone block, the terminate bin in a piece of its own"""
    rng = np.random.default_rng(0xC0A1)
    segs = [R.flat_segment(rng, 5), ("tu", PM.tu_case(rng, *TU_OUTCOMES[7])), ("block",) + PM.chroma_block(rng), R.flat_segment(rng, 1),
            ("tu", PM.tu_case(rng, *TU_OUTCOMES[21])), R.flat_segment(rng, 12)]
    return R.join(rng, segs, qp=26)


def _written_bits(u, string):
    """What getNumWrittenBits() answers behind `string`: the oracle's probe"""
    return H.load_oracle().encode_records(string, u["qp"], C.INIT_ID, 4)[1]


def _cut_lists(u, cuts):
    tail = [c for c in R.entry_cuts(u) if c[0] > cuts[-2][0]]
    return (cuts, [cuts[0], cuts[0]] + cuts[1:] + [cuts[-1]], cuts[:-2] + tail[:-1], [])


def test_the_final_bytes_are_the_one_plan_write_s_for_every_way_of_cutting():
    for u, cuts in (mixed(), joined()):
        one = C.whole(u)
        assert one["flag"] == 0 and one["values"] == [v & 0xFFFFFFFF for v in u["values"]] and one["infos"] == u["infos"]
        assert np.array_equal(one["data"], u["data"])              # (the unit's bytes are the oracle's of the same string)
        for cs in _cut_lists(u, cuts):
            out, data = C.expect(u, cs)
            assert np.array_equal(data, one["data"]), cs
            assert out[-1][:2] == (one["n_bits"], 0), cs
            assert all(f == 0 for _, f, _ in out)


def test_the_bits_behind_every_piece_are_the_oracle_s_written_bits_of_the_prefix():
    for u, cuts in (mixed(), joined()):
        for cs in _cut_lists(u, cuts):
            out, _ = C.expect(u, cs)
            bits = [b for b, _, _ in out[:-1]]
            assert bits == sorted(bits)
            for (e, b), n_bits in zip(cs, bits):
                assert n_bits == _written_bits(u, R.prefix_string(u, e, b)), (e, b)
    u, _ = joined()
    assert C.expect(u, [(0, 0)])[0][0][0] == 0                     # a piece of nothing in front: start() has written nothing


def test_the_record_cuts_are_the_lengths_of_the_expanded_prefixes():
    u, cuts = joined()
    rc = C.record_cuts(u, cuts)
    string = C.whole_string(u)
    assert rc == sorted(rc) and rc[-1] == len(string) - 1          # the terminate bin is the last piece
    spans = R.spans_of(u, cuts)
    assert any(sp[0] == sp[2] and sp[3] == sp[1] + 1 for sp in spans), "a piece of one block and no entry"
    assert any(sp[2] == sp[0] + 1 and sp[1] == sp[3] for sp in spans), "a piece of one entry"
    assert spans[-1][2] - spans[-1][0] == 1 and int(u["plan"][-1, 0]) & 15 == E.TRM


def test_a_piece_s_own_walk_finds_the_stops():
    u, cuts = joined()
    spans = R.spans_of(u, cuts)
    assert all(C.piece_stop(u, sp) == 0 for sp in spans)
    # a reference across a piece boundary: tu_cbf_cr's guard looks back at tu_cbf_cb
    e0 = spans[1][0]
    assert not R.references_stay_inside(u, [(e0 + 2, spans[1][1])])
    assert C.piece_stop(u, (e0 + 2, spans[1][1], spans[1][2], spans[1][3])) == W.BAD_RECORD
    # a value outside its element's code, in the piece that holds it and in no other
    i = next(k for k in range(spans[0][0], spans[0][2]) if W.domain_top(int(u["plan"][k, 0])) not in (None, 0xFFFFFFFF))
    bad = dict(u, values=list(u["values"]))
    bad["values"][i] = W.domain_top(int(u["plan"][i, 0])) + 1
    assert [C.piece_stop(bad, sp) for sp in spans] == [W.BAD_VALUE] + [0] * (len(spans) - 1)
    # a coded block without a coefficient
    k = next(t for t, on in enumerate(u["coded"]) if on)
    empty = dict(u, blocks=[np.zeros_like(b) if t == k else b for t, b in enumerate(u["blocks"])])
    stops = [C.piece_stop(empty, sp) for sp in spans]
    assert stops.count(W.BAD_VALUE) == 1 and stops[[sp[1] <= k < sp[3] for sp in spans].index(True)] == W.BAD_VALUE
