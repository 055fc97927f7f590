"""The expectation of include/cabac_hip_plan_continue.h, on the CPU, composed from what the models already answer: a unit of
tests/parse_plan_model.py cut into pieces as tests/plan_resume_model.py cuts it (is_cut, spans_of, piece_unit); per piece
write_plan_model.stop_of on the piece alone (the stop), parse_plan_model.expand on the pieces (the expanded record string and the
record cuts the entry cuts map to), pieces_model.encode_pieces on that string under those cuts (n_bits behind every piece, the
bytes behind the last), ctx_sets_model.advance_from (the contexts behind every piece), and write_plan_model.write for the whole.
Nothing here encodes on its own."""
import numpy as np

import ctx_sets_model as CS
import parse_plan_model as PM
import pieces_model as P
import plan_resume_model as R
import write_plan_model as W

INIT_ID = R.INIT_ID


def whole_string(u):
    return PM.expand(u["plan"], u["values"], u["metas"], u["blocks"], u["at"], u["guards"])[0]


def record_cuts(u, cuts):
    """The cuts of the expanded record string that the entry cuts (e, b) map to"""
    return [len(R.prefix_string(u, e, b)) for e, b in cuts]


def piece_stop(u, span):
    """0, BAD_RECORD or BAD_VALUE: what the piece's own walk finds (write_plan_model.stop_of on the piece as a unit of its own;
    its values are the whole's filled values, which are the real values wherever a real element is active)"""
    p = R.piece_unit(u, span, False)
    return W.stop_of(p["plan"], p["values"], p["metas"], p["blocks"], p["at"] if p["metas"] else None, p["guards"] if p["metas"] else None)


def whole(u):
    """write_plan_model.write of the whole unit: what ONE plan write gives (flag, values, infos, coded, data, n_bits)"""
    return W.write(u["plan"], u["values"], u["metas"], u["blocks"], u["at"], u["guards"], u["qp"])


def expect(u, cuts, ctx=None, cap=None):
    """([(n_bits, flags, contexts behind the piece)] per piece, the bytes behind the last piece) of a VALID unit whose references
    stay inside its pieces, coded from the contexts `ctx` (None: the init set of the unit's qp)"""
    ctx = CS.init_set(u["qp"], INIT_ID) if ctx is None else ctx
    spans = R.spans_of(u, cuts)
    assert R.references_stay_inside(u, cuts) and all(piece_stop(u, sp) == 0 for sp in spans)
    string = whole_string(u)
    rc = record_cuts(u, cuts)
    parts = []
    for k, sp in enumerate(spans):                                 # the pieces, expanded one by one, are the whole cut at rc
        p = R.piece_unit(u, sp, k == len(spans) - 1)
        parts.append(PM.expand(p["plan"], p["values"], p["metas"], p["blocks"], p["at"], p["guards"], p["infos"])[0])
    assert np.array_equal(np.concatenate(parts + [np.zeros(0, np.uint16)]), string)
    assert [len(x) for x in parts] == [b - a for a, b in P.pieces_of(len(string), rc)]
    out, data = P.encode_pieces(string, rc, ctx, cap)
    for (_, _, left), end in zip(out, rc + [len(string)]):
        assert all(np.array_equal(a, b) for a, b in zip(left, CS.advance_from(string[:end], ctx)))
    return out, data
