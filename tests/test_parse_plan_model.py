"""CPU: tests/parse_plan_model.py, the model the GPU tests of the plan parse rest on, pinned to parse_elements_model and the oracle:
without computed entries it is that model; on block-free plans with CONDs its exact reader reads what the bin-by-bin decoder
reads; the P2 rewrite keeps its results; and the worked transform unit round-trips for every outcome."""
import itertools

import numpy as np
import pytest

import helpers as H
import parse_corpus as PC
import parse_elements_model as E
import parse_plan_model as PM
from entropy_coding_amd import capi


def _damage(rng, u):
    d = np.concatenate([u["data"], np.zeros(16 * len(u["plan"]) + 16, np.uint8)])
    for _ in range(int(rng.integers(1, 4))):
        d[int(rng.integers(0, len(u["data"])))] ^= 1 << int(rng.integers(0, 8))
    if d[0] == 0xFF:
        d[0] = 0x7F
    return d


def test_without_computed_entries_it_is_the_element_model():
    rng = np.random.default_rng(0xA1)
    for rep in range(12):
        plan, values = E.close(*E.random_plan(rng, int(rng.integers(1, 80)), guard_frac=0.5, small=True))
        u = E.make_unit(rng, plan, values)
        for data in (u["data"], _damage(rng, u)):
            assert PM.read_plan(plan, data, u["qp"], finish=True) == E.read_plan(plan, data, u["qp"], finish=True), rep
            assert PM.dec_walk(plan, data, u["qp"]) == E.first_out_of_range(plan, data, u["qp"]), rep
        assert PM.fill(plan, values)[0] == values
        assert np.array_equal(PM.expand(plan, values, [], [], None, None)[0], E.expand(plan, values, [], [], None, None)[0])
    # with blocks: the same string, the same verdicts
    m0, c0 = PC.random_tu(rng, "regular")
    m1, c1 = PC.random_tu(rng, "regular")
    plan, values = E.close(np.array([[capi.element(E.CTX_BIN, ctx=20), 0], [capi.element(E.CTX_BIN, ctx=21), 0]], np.uint32), [1, 0])
    guards = [capi.guard(2, capi.GUARD_EQ, 1), capi.guard(1, capi.GUARD_EQ, 1)]
    u = E.make_unit(rng, plan, values, [m0, m1], [c0, c1], at=[2, 2], guards=guards)
    b = PM.build(rng, plan, values, [m0, m1], [c0, c1], at=[2, 2], guards=guards, qp=u["qp"])
    assert np.array_equal(b["data"], u["data"]) and b["values"] == u["values"] and b["coded"] == u["coded"] == [True, False]
    assert b["infos"] == [PM.info_of(m0, c0), PM.NOT_CODED]
    n_bits = PM.want_walk(b)[0]
    args = (u["data"], u["qp"], plan, [m0, m1], [2, 2], guards)
    for vals, infos in ((values, b["infos"]), ([1, 1, 1], b["infos"]), (values, [PM.NOT_CODED] * 2)):
        assert PM.consistent(*args, vals, [c0, c1], infos, n_bits, finish=True) == E.consistent(*args, vals, [c0, c1], infos, n_bits, finish=True)
    # the bad entries of kinds 0 .. 8 are the element model's
    for w0, gw, i in ((15, 0, 3), (capi.element(E.CTX_BIN, ctx=379), 0, 3), (capi.element(E.CTX_BIN, ctx=1), 0x400, 3),
                      (capi.element(E.CTX_BIN, ctx=1), capi.guard(4), 3), (capi.element(E.CTX_BIN, ctx=1), capi.guard(3), 3)):
        assert PM.is_bad_entry(w0, gw, i, 2) == E.is_bad_entry(w0, gw, i)


def test_fields_bad_entries_and_values_of_the_computed_kinds():
    w0, w1 = capi.cond(3, capi.GUARD_GE, 7, capi.JOIN_AND, 200)
    assert PM.fields(w0) == (9, dict(back2=200, join=1)) and w1 == capi.guard(3, capi.GUARD_GE, 7)
    assert PM.fields(capi.block_info(15, 18, 1)) == (10, dict(which=15, shift=18, width=1))
    ok = lambda w0, w1, i, nb: not PM.is_bad_entry(w0, w1, i, nb)
    assert ok(*capi.cond(3, 0, 0), 3, 0) and not ok(*capi.cond(4, 0, 0), 3, 0)
    assert ok(*capi.cond(0, 0, 0, capi.JOIN_OR, 3), 3, 0) and not ok(*capi.cond(0, 0, 0, capi.JOIN_OR, 4), 3, 0)
    assert not ok(*capi.cond(0, 0, 0, capi.JOIN_AND, 0), 3, 0) and ok(*capi.cond(0, 0, 0, capi.JOIN_NONE, 0), 0, 0)
    assert not ok(9 | 3 << 12 | 1 << 4, 0, 3, 0) and not ok(9, 0x400, 3, 0) and ok(9 | 0xFFFFC000, 0, 0, 0)
    assert ok(capi.block_info(1, 0, 32), 0, 0, 2) and not ok(capi.block_info(2, 0, 32), 0, 0, 2)
    assert not ok(10, 0, 0, 1) and not ok(10 | 17 << 8 | 16 << 13, 0, 0, 1) and ok(10 | 16 << 8 | 16 << 13, 0, 0, 1)
    assert not ok(capi.block_info(0), capi.guard(1), 0, 1) and not ok(capi.block_info(0), 0x800, 5, 1)
    assert all(not ok(k, 0, 5, 5) for k in range(11, 16))
    vals = [5, 0, 1]
    for cmp, want in zip(range(4), (5 != 4, 5 == 4, 5 >= 4, 5 < 4)):
        w = capi.cond(3, cmp, 4)
        assert PM.computed_value(*w, vals, 3, []) == int(want)
        for join, back2, o in ((1, 2, 0), (1, 1, 1), (2, 2, 0), (2, 1, 1)):
            w = capi.cond(3, cmp, 4, join, back2)
            assert PM.computed_value(*w, vals, 3, []) == int((want and o) if join == 1 else (want or o))
    assert PM.computed_value(*capi.cond(0, capi.GUARD_EQ, 9), vals, 3, []) == 1
    infos = [0x00011, 0x20000, 0x10007]
    assert PM.computed_value(capi.block_info(0, 0, 16), 0, vals, 3, infos) == 7
    assert PM.computed_value(capi.block_info(0, 16, 1), 0, vals, 3, infos) == 1
    assert PM.computed_value(capi.block_info(1, 17, 1), 0, vals, 3, infos) == 1
    assert PM.computed_value(capi.block_info(2, 0, 32), 0, vals, 3, infos) == 0x11
    assert PM.computed_value(capi.block_info(2, 0, 32), capi.guard(2, capi.GUARD_NE, 0), vals, 3, infos) == 0      # guarded off
    assert PM.nb_of([0, 2, 2, 5], 5) == [1, 1, 3, 3, 3]


@pytest.mark.parametrize("damaged", [False, True])
def test_exact_reader_agrees_with_the_bin_decoder_on_block_free_plans_with_conds(damaged):
    rng = np.random.default_rng(0xA2 + damaged)
    conds = joins = changed = 0
    for rep in range(30):
        plan, real = PM.random_cond_plan(rng, int(rng.integers(5, 60)))
        plan, real = PM.close(plan, real)
        u = PM.build(rng, plan, real)
        conds += sum(PM.is_computed(w) for w in plan[:, 0])
        joins += sum(PM.fields(w)[1]["join"] != 0 for w in plan[:, 0] if PM.is_computed(w))
        data = _damage(rng, u) if damaged else u["data"]
        first, front = PM.dec_walk(plan, data, u["qp"])
        r = PM.read_plan(plan if first is None else plan[:first], data, u["qp"], finish=first is None)
        assert r["flags"] in (0, H.RES_BAD_STOP, E.RES_BAD_VALUE)
        assert r["values"] == front[:r["n_written"]] and (r["n_written"] == len(front) or r["flags"] == E.RES_BAD_VALUE), rep
        if not damaged:
            assert first is None and r["flags"] == 0 and r["values"] == u["values"], rep
            assert PM.consistent(data, u["qp"], plan, [], None, None, r["values"], [], [], r["n_bits"], finish=True) == (True, 0)
            k = next(i for i, w in enumerate(plan[:, 0]) if PM.is_computed(w))
            wrong = list(r["values"])
            wrong[k] ^= 1                                          # a computed value that its inputs do not give
            assert not PM.consistent(data, u["qp"], plan, [], None, None, wrong, [], [], r["n_bits"], finish=True)[0]
        changed += r["values"] != u["values"][:r["n_written"]]
    assert conds >= 60 and joins >= 20 and (changed > 0) == damaged


def test_p2_rewrite_preserves_the_model_s_results():
    rng = np.random.default_rng(0xA4)
    seen = 0
    for rep in range(30):
        plan, real = PM.random_cond_plan(rng, int(rng.integers(5, 60)), p2=True)
        plan, real = PM.close(plan, real)
        u = PM.build(rng, plan, real)
        rw = PM.p2_rewrite_unit(u)
        is_cond = np.array([PM.is_computed(w) for w in plan[:, 0]])
        seen += int(is_cond.sum())
        assert not any(PM.is_computed(w) for w in rw["plan"][:, 0])
        for data in (u["data"], _damage(rng, u)):
            first = PM.dec_walk(plan, data, u["qp"])[0]              # up to the first element met OUT OF RANGE, if there is one
            assert first == E.first_out_of_range(rw["plan"], data, u["qp"])[0]
            cut, fin = (len(plan), True) if first is None else (first, False)
            a, b = PM.read_plan(plan[:cut], data, u["qp"], finish=fin), E.read_plan(rw["plan"][:cut], data, u["qp"], finish=fin)
            assert (a["n_bits"], a["flags"], a["n_written"]) == (b["n_bits"], b["flags"], b["n_written"]), rep
            n = a["n_written"]
            assert np.array_equal(np.array(a["values"])[~is_cond[:n]], np.array(b["values"])[~is_cond[:n]]), rep
            assert not np.array(b["values"], np.int64)[is_cond[:n]].any()
    assert seen >= 40
    # with blocks behind a COND: the rewritten unit codes the same blocks, from the same bytes
    plan = np.array([[capi.element(E.EP_BINS, n=3), 0], capi.cond(1, capi.GUARD_GE, 4), [capi.element(E.CTX_BIN, ctx=9), capi.guard(1)]], np.uint32)
    (m, c) = PM.chroma_block(rng)
    for v0 in (3, 4):
        p, real = PM.close(plan, [v0, 0, 1])
        u = PM.build(rng, p, real, [m], [c], at=[3], guards=[capi.guard(2)])
        rw = PM.p2_rewrite_unit(u)
        assert rw["guards"] == [capi.guard(3, capi.GUARD_GE, 4)] and int(rw["plan"][2, 1]) == capi.guard(2, capi.GUARD_GE, 4)
        vals = [v if not PM.is_computed(w) else 0 for v, w in zip(u["values"], p[:, 0])]
        assert E.expand(rw["plan"], vals, [m], [c], [3], rw["guards"])[3] == u["coded"] == [v0 == 4]
        assert np.array_equal(E.expand(rw["plan"], vals, [m], [c], [3], rw["guards"])[0], PM.expand(p, u["values"], [m], [c], [3], u["guards"])[0])


TU_OUTCOMES = [o for o in itertools.product((0, 1), (0, 1), (0, 1), (False, True), (False, True), (False, True))
               if not (o[4] and o[5])]                              # a violating block has scanPosLast > 0


def test_tu_plan_round_trips_for_every_outcome():
    """cbf_cb x cbf_cr x cbf_y x ts x scanPosLast 0 / > 0 x violating / not: the unit decides what the syntax says, and its
    string decodes to itself with the decisions the model's own rule gives."""
    rng = np.random.default_rng(0xA5)
    orc = H.load_oracle()
    mts = lf = 0
    for o in TU_OUTCOMES:
        cb, cr, y, ts, last_zero, violating = o
        u = PM.tu_unit(rng, [PM.tu_case(rng, *o)])
        v, want = u["values"], PM.tu_expected(u, 0)
        assert u["coded"] == [bool(cb), bool(cr), bool(y)], o
        assert (v[3], v[6], v[17], v[22]) == (want["cbf_cr"], want["any"], want["mts_coded"], want["lfnst_coded"]), o
        assert want["cbf_cr"] == cr and want["any"] == int(bool(cb or cr or y))
        assert want["mts_coded"] == int(bool(y) and not ts and not last_zero and not violating), o
        if y and not ts:
            assert bool(v[11]) == violating and (v[10] == 0) == last_zero and v[12] == 0 and v[13] == 0, o
        if not y:
            assert v[13] == 1
        if not want["any"]:
            assert v[7:10] == [0, 0, 0]
        mts += want["mts_coded"]
        lf += want["lfnst_coded"]
        n_bits, flags = PM.want_walk(u)
        assert flags == 0
        assert PM.consistent(u["data"], u["qp"], u["plan"], u["metas"], u["at"], u["guards"], v, u["blocks"], u["infos"], n_bits, finish=True) == (True, 0)
        for k in (3, 6, 17, 22):                                     # one decision flipped: no longer consistent
            w = list(v)
            w[k] ^= 1
            assert not PM.consistent(u["data"], u["qp"], u["plan"], u["metas"], u["at"], u["guards"], w, u["blocks"], u["infos"], n_bits, finish=True)[0]
        # the oracle's block parser reads the coded blocks back from the same bytes: the records are those of the syntax
        string = PM.expand(u["plan"], v, u["metas"], u["blocks"], u["at"], u["guards"])[0]
        rc, bins, _ = orc.decode_records(string, u["qp"], 2, u["data"], flags=1)
        assert rc == 0 and np.array_equal(bins, string >> 15)
    assert 0 < mts < len(TU_OUTCOMES) and 0 < lf < len(TU_OUTCOMES)
    # several units in a row: the references are relative, the info words those of the unit's own blocks
    cases = [PM.tu_case(rng, *TU_OUTCOMES[k]) for k in (7, 40, 21, 47, 2)]
    u = PM.tu_unit(rng, cases)
    assert len(u["plan"]) == 5 * PM.TU_LEN + 1 and PM.want_walk(u)[1] == 0
    for k in range(5):
        want = PM.tu_expected(u, k)
        v = u["values"][PM.TU_LEN * k:]
        assert (v[3], v[6], v[17], v[22]) == (want["cbf_cr"], want["any"], want["mts_coded"], want["lfnst_coded"]), k
