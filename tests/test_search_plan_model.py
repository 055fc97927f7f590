"""CPU: tests/search_plan_model.py against itself and against the models it is composed of — the resolved form of a plan
candidate, with its coded blocks spliced in at the resolved positions, IS parse_plan_model.expand's string; the header's table of
the most bins per element kind holds wherever write_plan_model says a value is in its domain; stops and capacity give the empty
form."""
import numpy as np

import helpers as H
import parse_elements_model as E
import parse_plan_model as PM
import search_plan_model as S
import write_plan_model as W
from entropy_coding_amd import capi
from test_parse_plan_model import TU_OUTCOMES

el, gd = capi.element, capi.guard


def tu_cand(rng, outcome):
    p, v, m, b, a, g = PM.tu_case(rng, *outcome)
    return S.cand(p, v, m, [np.clip(x, -32767, 32767) for x in b], a, g)


def test_resolved_form_spliced_is_expand_s_string_for_the_worked_unit():
    """Every outcome of the worked transform unit: side records + blocks at the resolved positions == the walk's record string;
    mts_idx has records exactly when the unit's own rule says it is coded"""
    rng = np.random.default_rng(0x5EA1)
    mts = 0
    for o in TU_OUTCOMES:
        c = tu_cand(rng, o)
        r = S.resolve(c)
        assert r["flag"] == 0 and r["coded"] == [bool(o[0]), bool(o[1]), bool(o[2])], o
        want = PM.expand(c["plan"], r["values"], c["metas"], c["blocks"], c["at"], c["guards"])[0]
        assert np.array_equal(S.spliced(c, r), want), o
        assert r["at_out"] == sorted(r["at_out"]) and r["at_out"][-1] <= len(r["records"])
        u = dict(values=r["values"], infos=r["infos"])
        exp = PM.tu_expected(u, 0)
        assert r["values"][17] == exp["mts_coded"], o
        # the records of mts_idx (entry 18): present exactly when coded
        without = S.resolve(dict(c, plan=np.concatenate([c["plan"][:18], [list(capi.cond(0))], c["plan"][19:]]).astype(np.uint32)))
        assert (len(r["records"]) > len(without["records"])) == bool(exp["mts_coded"]), o
        mts += exp["mts_coded"]
    assert 0 < mts < len(TU_OUTCOMES)


def test_resolved_form_of_random_plans_and_the_block_free_identity():
    rng = np.random.default_rng(0x5EA2)
    for n in (0, 1, 5, 64, 65, 300):
        plan, real = PM.random_cond_plan(rng, n)
        c = S.cand(plan, real)
        r = S.resolve(c)
        assert r["flag"] == 0
        want = PM.expand(plan, r["values"], [], [], None, None)[0]
        assert np.array_equal(r["records"], want) and np.array_equal(S.spliced(c, r), want), n
        assert len(r["records"]) <= sum(S.bin_bound(w0) for w0 in plan[:, 0])
    # blocks at positions inside a random plan, no guards: positions count the records in front
    plan, real = PM.random_cond_plan(rng, 40)
    blocks = [H.random_block(rng, 4, 4, density=0.5) | 1 for _ in range(3)]
    c = S.cand(plan, real, [(4, 4, 0, 0)] * 3, blocks, at=[0, 17, 40])
    r = S.resolve(c)
    assert np.array_equal(S.spliced(c, r), PM.expand(plan, r["values"], c["metas"], c["blocks"], c["at"], None)[0])
    assert r["at_out"][0] == 0 and r["at_out"][2] == len(r["records"]) and all(r["coded"])


def test_bin_bound_holds_over_every_domain():
    """At domain_top and at every inside value of edge_values the binariser makes at most bin_bound(w0) records; the bound is
    reached for every kind; no entry makes more than 255"""
    rng = np.random.default_rng(0x5EA3)
    reached = set()
    words = [E.random_element(rng) for _ in range(400)] + [el(E.TRM), el(E.UNARY_MAX, ctx=1, ctx_n=2, max_symbol=255),
                                                           el(E.EXP_GOLOMB, count=0), el(E.EXP_GOLOMB, count=31), el(E.EP_BINS, n=32),
                                                           el(E.REM_ABS, rice=14, cutoff=0, max_log2=15), el(E.TRUNC_BIN, max_symbol=(1 << 28) - 1),
                                                           el(E.REM_ABS, rice=0, cutoff=12, max_log2=20)]
    for w0 in words:
        bound = S.bin_bound(w0)
        assert 0 <= bound <= 255
        tries = [v for v, inside in W.edge_values(w0) if inside]
        top = W.domain_top(w0)
        if top is not None and top >= 0:
            tries += [min(top, 0xFFFFFFFF)] + [int(v) for v in rng.integers(0, min(top, 0xFFFFFFFF) + 1, 6)]
        for v in tries:
            n = len(E.records_of([E.op_of(w0, v)]))
            assert n <= bound, (hex(w0), v, n, bound)
            if n == bound:
                reached.add(w0 & 15)
    assert reached == {E.CTX_BIN, E.EP_BINS, E.REM_ABS, E.TRM, E.UNARY_MAX, E.UNARY_EP, E.EXP_GOLOMB, E.TRUNC_BIN, E.ALIGN}
    assert S.bin_bound(capi.cond(1)[0]) == 0 and S.bin_bound(capi.block_info(0, 0, 16)) == 0


def test_stops_and_capacity_give_the_empty_form():
    rng = np.random.default_rng(0x5EA4)
    good = tu_cand(rng, (1, 1, 1, False, False, False))
    bad_value = dict(good, values=[5] + good["values"][1:])                      # tu_cbf_cb = 5
    bad_entry = dict(bad_value, plan=np.concatenate([good["plan"], [[15, gd(1, capi.GUARD_EQ, 77)]]]).astype(np.uint32),
                     values=bad_value["values"] + [0])                           # kind 15 behind a false guard, and the bad value
    cands = [good, bad_value, bad_entry, good]
    R = S.resolve_all(cands)
    assert R["flags"].tolist() == [0, S.BAD_VALUE, S.BAD_RECORD, 0]
    assert R["rec_first"][1] == R["rec_first"][2] == R["rec_first"][3] and R["total"] == 2 * len(S.resolve(good)["records"])
    assert (R["tus_out"]["log2_width"][3:9] == 7).all() and (R["tu_at_out"][3:9] == 0).all() and R["coded"][:3].all()
    assert np.array_equal(R["tus_out"]["coeff_offset"], S.pack(cands)["tus"]["coeff_offset"])
    over = S.resolve_all(cands, capacity=R["total"] - 1)
    assert over["flags"].tolist() == [S.OVERFLOW, S.BAD_VALUE, S.BAD_RECORD, S.OVERFLOW] and over["total"] == R["total"]
    assert not over["rec_first"].any() and len(over["records"]) == 0 and (over["tus_out"]["log2_height"] == 7).all()
    assert S.resolve_all(cands, capacity=R["total"])["flags"].tolist() == R["flags"].tolist()
    # in the round a flagged candidate costs UINT64_MAX and is picked only where its group has nothing else
    sets = [H.load_oracle().ctx_init(30, 2)]
    m = S.round_model(cands, [0, 2, 3, 4], sets, [0, 0, 0, 0], None, None, 1 << 16)
    assert m["bits"][1] == m["bits"][2] == S.U64_MAX and m["pick"].tolist() == [0, 2, 3]
