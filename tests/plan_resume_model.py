"""The expectation of include/cabac_hip_plan_resume.h, on the CPU, composed from what the models already answer: a unit of
tests/parse_plan_model.py (build, tu_unit, random_cond_plan) cut into pieces; per piece the oracle's decode_records on the expanded
prefix without FINISH (n_bits), ctx_sets_model.advance_from over that prefix (the contexts behind the piece), and for the last
piece parse_plan_model.want_walk.  Nothing here decodes on its own.

A CUT is (e, b): in front of entry e and of block b.  The walk codes, for i = 0 .. n, first every block with at(t) == i, then entry
i; so a cut is one of the walk's when every block in front of b stands at or in front of e and every other block at or behind e.
Blocks at position e may lie on either side: (e, b) with b in front of them cuts in front of those blocks, with b behind them
behind the blocks and in front of entry e.  A PIECE is the span between two cuts: entries e0 .. e1 - 1, blocks b0 .. b1 - 1, with
positions relative to e0.

Units are built so that no reference crosses a cut (join: every segment's plan is generated on its own, references are relative):
what is inside a piece is then a unit of parse_plan_model of its own, with the whole's values, info words and coded flags."""
import numpy as np

import ctx_sets_model as CS
import helpers as H
import parse_elements_model as E
import parse_plan_model as PM

INIT_ID = 2                                                        # parse_unit_model.pack and parse_plan_model.build


# ------------------------------------------------------------------------------------------------ cuts and pieces
def positions(u):
    return PM.positions(len(u["metas"]), u["at"], len(u["plan"]))


def is_cut(u, e, b):
    pos = positions(u)
    return 0 <= e <= len(u["plan"]) and 0 <= b <= len(pos) and all(p <= e for p in pos[:b]) and all(p >= e for p in pos[b:])


def spans_of(u, cuts):
    """[(e0, b0, e1, b1)] of the pieces of `u` cut at `cuts` (ascending, repeats allowed: pieces of nothing)"""
    edges = [(0, 0)] + [(int(e), int(b)) for e, b in cuts] + [(len(u["plan"]), len(u["metas"]))]
    assert all(is_cut(u, e, b) for e, b in edges), "no cut of the walk"
    assert all(a[0] <= c[0] and a[1] <= c[1] for a, c in zip(edges, edges[1:]))
    return [(a[0], a[1], c[0], c[1]) for a, c in zip(edges[:-1], edges[1:])]


def entry_cuts(u):
    """Every cut in front of an entry and behind the blocks that stand there, the end included: (e, b(e)) for e = 0 .. n"""
    pos = positions(u)
    return [(e, sum(1 for p in pos if p <= e)) for e in range(len(u["plan"]) + 1)]


def piece_unit(u, span, last):
    """The piece as a unit of its own: the whole's bytes, qp, values, info words and coded flags, positions relative to the piece.
    Only the last piece carries FINISH."""
    e0, b0, e1, b1 = span
    pos = positions(u)
    return dict(plan=np.asarray(u["plan"], np.uint32).reshape(-1, 2)[e0:e1], values=list(u["values"][e0:e1]),
                metas=list(u["metas"][b0:b1]), blocks=list(u["blocks"][b0:b1]), infos=list(u["infos"][b0:b1]), coded=list(u["coded"][b0:b1]),
                at=[p - e0 for p in pos[b0:b1]], guards=None if u["guards"] is None else list(u["guards"][b0:b1]),
                qp=u["qp"], finish=bool(last and u["finish"]), data=u["data"])


def prefix_string(u, e, b):
    """The expanded record string in front of the cut (e, b)"""
    assert is_cut(u, e, b)
    pos = positions(u)
    return PM.expand(np.asarray(u["plan"], np.uint32).reshape(-1, 2)[:e], u["values"][:e], u["metas"][:b], u["blocks"][:b], pos[:b],
                     None if u["guards"] is None else u["guards"][:b], u["infos"][:b])[0]


def references_stay_inside(u, cuts):
    """No guard, CABAC_PE_COND back reference, CABAC_PE_BLOCK_INFO or block guard of `u` reaches in front of its piece"""
    plan = np.asarray(u["plan"], np.uint32).reshape(-1, 2)
    pos = positions(u)
    for e0, b0, e1, b1 in spans_of(u, cuts):
        for i in range(e0, e1):
            w0, w1 = int(plan[i, 0]), int(plan[i, 1])
            kind, f = PM.fields(w0)
            if (w1 & 0xFF) > i - e0:
                return False
            if kind == PM.COND and f["join"] != 0 and f["back2"] > i - e0:
                return False
            if kind == PM.BLOCK_INFO and f["which"] >= sum(1 for p in pos[b0:b1] if p <= i):
                return False
        if u["guards"] is not None:
            for t in range(b0, b1):
                if (int(u["guards"][t]) & 0xFF) > pos[t] - e0:
                    return False
    return True


# ------------------------------------------------------------------------------------------------ what every piece reports
def expect(u, cuts, ctx=None):
    """[(n_bits, flags, contexts behind the piece)] per piece of a VALID unit whose bytes hold it all.  Non-final pieces: what the
    plan parse reports for the prefix without FINISH; the last: want_walk of the whole."""
    orc = H.load_oracle()
    ctx = CS.init_set(u["qp"], INIT_ID) if ctx is None else ctx
    spans = spans_of(u, cuts)
    out = []
    for k, (_, _, e1, b1) in enumerate(spans):
        string = prefix_string(u, e1, b1)
        left = CS.advance_from(string, ctx)
        if k == len(spans) - 1:
            n_bits, flags = PM.want_walk(u)
        else:
            rc, bins, n_bits = orc.decode_records(string, u["qp"], INIT_ID, u["data"], flags=0)
            assert rc == 0 and np.array_equal(bins, string >> 15)
            flags = 0
        out.append((n_bits, flags, left))
    return out


def shifts_at(u, e, b):
    """S, the bits the decoder has shifted at the cut: the n_bits of the prefix without FINISH is S + 8"""
    string = prefix_string(u, e, b)
    rc, _, n_bits = H.load_oracle().decode_records(string, u["qp"], INIT_ID, u["data"], flags=0)
    assert rc == 0
    return n_bits - 8


# ------------------------------------------------------------------------------------------------ builders
def join(rng, segments, qp=None, close=True):
    """One unit out of segments, each generated on its own, and the cuts between them -> (unit, cuts).  A segment is
    ("plan", plan, real values) — a block-free run of entries; ("tu", parse_plan_model.tu_case(...)) — 24 entries with three blocks
    in front of entry 10; ("block", meta, coefficients) — one unguarded block and no entry.  close: the terminate bin behind the
    last segment, in a piece of its own."""
    plans, values, metas, blocks, at, guards, cuts = [], [], [], [], [], [], []
    n = 0
    for seg in segments:
        if seg[0] == "plan":
            p = np.asarray(seg[1], np.uint32).reshape(-1, 2)
            plans.append(p)
            values += list(seg[2])
            n += len(p)
        elif seg[0] == "tu":
            p, v, m, bl, a, g = seg[1]
            plans.append(p)
            values += list(v)
            metas += list(m)
            blocks += list(bl)
            at += [x + n for x in a]
            guards += list(g)
            n += len(p)
        else:
            assert seg[0] == "block"
            metas.append(seg[1])
            blocks.append(np.asarray(seg[2], np.int32))
            at.append(n)
            guards.append(0)
        cuts.append((n, len(metas)))
    plan = np.concatenate(plans + [np.zeros((0, 2), np.uint32)]).astype(np.uint32)
    if close:
        plan, values = E.close(plan, values)
    else:
        cuts = cuts[:-1]
    u = PM.build(rng, plan, values, metas, blocks, at if metas else None, guards if metas else None, qp=qp)
    assert references_stay_inside(u, cuts)
    return u, cuts


def random_segments(rng, sizes, kinds=None):
    return [("plan",) + tuple(PM.random_cond_plan(rng, n, kinds=kinds)) for n in sizes]


def flat_segment(rng, n, kinds=None, small=True):
    """n unguarded real elements: a run that may be cut in front of every entry"""
    plan = np.zeros((n, 2), np.uint32)
    plan[:, 0] = [E.random_element(rng, kinds) for _ in range(n)]
    return ("plan", plan, [E.random_value(rng, w0, small) for w0 in plan[:, 0]])
