"""CPU: tests/parse_elements_model.py, the model the GPU tests of the element parse rest on, pinned to the oracle — the exact reader
returns the writer's input for valid streams of every kind with guards of every cmp and back, and the consistency check accepts
the writer's input and rejects a result with one value changed, one guard outcome flipped or one skipped block reported as coded."""
import numpy as np
import pytest

import helpers as H
import parse_corpus as PC
import parse_elements_model as E
from entropy_coding_amd import capi


def _coded(plan, values, qp, finish=True):
    rng = np.random.default_rng(1)
    return E.make_unit(rng, plan, values, qp=qp, finish=finish)


def test_exact_reader_returns_the_writer_s_values_for_every_kind():
    rng = np.random.default_rng(0xE1)
    seen = set()
    for rep in range(40):
        plan, values = E.close(*E.random_plan(rng, int(rng.integers(1, 140)), guard_frac=0.5))
        u = _coded(plan, values, int(rng.integers(0, 64)))
        r = E.read_plan(u["plan"], u["data"], u["qp"], finish=True)
        assert r["flags"] == 0 and r["values"] == u["values"], rep
        seen |= {int(w) & 15 for w, on in zip(plan[:, 0], r["active"]) if on}
    assert seen == set(range(9))


@pytest.mark.parametrize("back", [1, 63, 64, 255])
@pytest.mark.parametrize("cmp", [0, 1, 2, 3])
def test_guards_of_every_comparison_and_distance(back, cmp):
    """Element `back` is guarded by element 0, a 3-bit value, against operand 4: both outcomes, read back exactly."""
    rng = np.random.default_rng(0xE2 + back)
    outcomes = set()
    for v0 in (3, 4, 5):
        fill, fv = E.random_plan(rng, back - 1, kinds=[E.CTX_BIN, E.EP_BINS, E.UNARY_EP], guard_frac=0.0)
        plan = np.concatenate([[[capi.element(E.EP_BINS, n=3), 0]], fill,
                               [[capi.element(E.EXP_GOLOMB, count=1), capi.guard(back, cmp, 4)]]]).astype(np.uint32)
        holds = (v0 != 4, v0 == 4, v0 >= 4, v0 < 4)[cmp]
        plan, values = E.close(plan, [v0] + fv + [9 if holds else 0])
        u = _coded(plan, values, 30)
        r = E.read_plan(u["plan"], u["data"], 30, finish=True)
        assert r["flags"] == 0 and r["values"] == values and r["active"][back] == holds
        outcomes.add(holds)
    assert outcomes == {True, False}


def test_bad_entries_and_the_prefix_bound():
    orc = H.load_oracle()
    good = [[capi.element(E.CTX_BIN, ctx=7), 0], [capi.element(E.EP_BINS, n=2), 0]]
    data = orc.encode_records(np.array([7, H.REC_EP, H.REC_EP | 0x8000, 0x81FF], np.uint16), 30, 2, 3)[0]
    for w0, gw in ([9, 0], [capi.element(E.CTX_BIN, ctx=379), 0], [capi.element(E.UNARY_MAX, ctx=1, ctx_n=400, max_symbol=3), 0],
                   [capi.element(E.EP_BINS, n=33), 0], [capi.element(E.UNARY_EP, max_symbol=33), 0], [capi.element(E.TRUNC_BIN), 0],
                   [capi.element(E.REM_ABS, rice=15, max_log2=15), 0], [capi.element(E.REM_ABS, max_log2=14), 0],
                   [capi.element(E.REM_ABS, max_log2=21), 0], [capi.element(E.REM_ABS, cutoff=13, max_log2=20), 0],
                   [capi.element(E.CTX_BIN, ctx=1), 0x400], [capi.element(E.CTX_BIN, ctx=1), capi.guard(3)]):
        r = E.read_plan(np.array(good + [[w0, gw]] + good, np.uint32), data, 30, finish=True)
        assert r["flags"] == H.RES_BAD_RECORD and r["values"] == [0, 1] and r["n_written"] == 2, (w0, gw)
    # an all-ones bypass run: range 256 after align, value bits all one
    ones = np.array([H.REC_ALIGN] + [H.REC_EP | 0x8000] * 40 + [0x81FF], np.uint16)
    data = orc.encode_records(ones, 30, 2, 3)[0]
    for count in (0, 5, 31):
        plan = np.array([[capi.element(E.ALIGN), 0], [capi.element(E.EXP_GOLOMB, count=count), 0], good[0]], np.uint32)
        r = E.read_plan(plan, data, 30)
        rc, _, nread = orc.decode_records(ones[:1 + 32 - count], 30, 2, data)
        assert r["flags"] == E.RES_BAD_VALUE and r["values"] == [0] and r["n_bits"] == nread


def _block_unit(rng):
    """cbf(1) -> block 0; cbf(0) -> block 1 (skipped); a guarded transform_skip_flag; a unary prefix with escape and sign"""
    m0, c0 = PC.random_tu(rng, "regular")
    m1, c1 = PC.random_tu(rng, "regular")
    plan = np.array([[capi.element(E.CTX_BIN, ctx=20), 0], [capi.element(E.CTX_BIN, ctx=21), 0],
                     [capi.element(E.UNARY_MAX, ctx=30, ctx_n=31, max_symbol=5), 0],
                     [capi.element(E.EXP_GOLOMB, count=0), capi.guard(1, capi.GUARD_EQ, 5)],
                     [capi.element(E.EP_BINS, n=1), capi.guard(2, capi.GUARD_NE, 0)],
                     [capi.element(E.CTX_BIN, ctx=310), capi.guard(5, capi.GUARD_EQ, 1)]], np.uint32)
    plan, values = E.close(plan, [1, 0, 5, 6, 1, 0])
    guards = [capi.guard(6, capi.GUARD_EQ, 1), capi.guard(5, capi.GUARD_EQ, 1)]
    return E.make_unit(rng, plan, values, [m0, m1], [c0, c1], at=[6, 6], guards=guards, qp=31)


def test_consistency_check_accepts_the_input_and_rejects_a_changed_result():
    orc = H.load_oracle()
    rng = np.random.default_rng(0xE3)
    u = _block_unit(rng)
    assert u["coded"] == [True, False]
    string, _, _, _ = E.expand(u["plan"], u["values"], u["metas"], u["blocks"], u["at"], u["guards"])
    rc, _, n_bits = orc.decode_records(string, u["qp"], 2, u["data"], flags=1)
    assert rc == 0
    infos = [5, E.NOT_CODED]
    args = (u["data"], u["qp"], u["plan"], u["metas"], u["at"], u["guards"])
    assert E.consistent(*args, u["values"], u["blocks"], infos, n_bits, finish=True) == (True, 0)
    for i in (0, 2, 3, 4):                                         # one value changed
        v = list(u["values"])
        v[i] ^= 1
        assert not E.consistent(*args, v, u["blocks"], infos, n_bits, finish=True)[0], i
    v = list(u["values"])
    v[1] = 1                                                       # one guard outcome flipped: the second cbf, block 1 then coded
    assert not E.consistent(*args, v, u["blocks"], [5, 5], n_bits, finish=True)[0]
    assert not E.consistent(*args, u["values"], u["blocks"], [5, 5], n_bits, finish=True)[0]      # a skipped block reported as coded
    assert not E.consistent(*args, u["values"], u["blocks"], [E.NOT_CODED, E.NOT_CODED], n_bits, finish=True)[0]
    # a skipped element reported with a value
    plan, values = E.close(np.array([[capi.element(E.EP_BINS, n=1), 0], [capi.element(E.CTX_BIN, ctx=9), capi.guard(1, capi.GUARD_EQ, 1)]],
                                    np.uint32), [0, 0])
    s = _coded(plan, values, 25)
    r = E.read_plan(plan, s["data"], 25, finish=True)
    assert r["values"] == [0, 0, 1] and r["active"] == [True, False, True]
    assert E.consistent(s["data"], 25, plan, [], None, None, [0, 0, 1], [], [], r["n_bits"], finish=True) == (True, 0)
    assert not E.consistent(s["data"], 25, plan, [], None, None, [0, 1, 1], [], [], r["n_bits"], finish=True)[0]
    c = [u["blocks"][0].copy(), u["blocks"][1]]
    ys, xs = np.nonzero(c[0])
    c[0][ys[0], xs[0]] += 1                                        # one coefficient changed
    assert not E.consistent(*args, u["values"], c, infos, n_bits, finish=True)[0]
    assert not E.consistent(*args, u["values"], u["blocks"], infos, n_bits + 1, finish=True)[0]


def test_exact_reader_and_consistency_agree_on_damaged_block_free_streams():
    rng = np.random.default_rng(0xE4)
    flagged = 0
    for rep in range(30):
        plan, values = E.close(*E.random_plan(rng, int(rng.integers(5, 40)), guard_frac=0.5, small=True))
        u = _coded(plan, values, int(rng.integers(0, 64)))
        d = np.concatenate([u["data"], np.zeros(4 * len(plan) + 16, np.uint8)])
        d[int(rng.integers(0, len(u["data"])))] ^= 1 << int(rng.integers(0, 8))
        if d[0] == 0xFF:
            d[0] = 0x7F
        r = E.read_plan(plan, d, u["qp"], finish=True)
        assert r["flags"] in (0, H.RES_BAD_STOP, E.RES_BAD_VALUE)
        if r["flags"] != E.RES_BAD_VALUE:
            ok, rc = E.consistent(d, u["qp"], plan, [], None, None, r["values"], [], [], r["n_bits"], finish=True)
            assert ok and {0: 0, -5: H.RES_BAD_STOP}[rc] == r["flags"], rep
        flagged += r["flags"] != 0
    assert flagged


def test_the_state_tracker_reads_what_the_oracle_reads_and_finds_the_state():
    """first_out_of_range's own decoder returns the oracle's values on valid streams of every kind and never reports the state
    there; behind a terminate bin of 1 it always does; on damaged streams with ALIGN it does sometimes, and in front of the
    element it names the exact reader's values are its own."""
    rng = np.random.default_rng(0xE5)
    for rep in range(25):
        plan, values = E.close(*E.random_plan(rng, int(rng.integers(1, 100)), guard_frac=0.5))
        u = _coded(plan, values, int(rng.integers(0, 64)))
        assert E.first_out_of_range(plan, u["data"], u["qp"]) == (None, u["values"]), rep
        more = np.concatenate([plan, [[capi.element(E.EP_BINS, n=0), 0], [capi.element(E.EP_BINS, n=5), 0]]])
        idx, vals = E.first_out_of_range(more, np.concatenate([u["data"], np.zeros(4, np.uint8)]), u["qp"])
        assert idx == len(plan) + 1 and vals == u["values"] + [0], rep      # behind the terminate bin of 1: the first that reads
    met = 0
    for rep in range(60):
        plan, values = E.close(*E.random_plan(rng, int(rng.integers(5, 40)), guard_frac=0.5, small=True))
        u = _coded(plan, values, int(rng.integers(0, 64)))
        d = np.concatenate([u["data"], np.zeros(16 * len(plan) + 16, np.uint8)])
        d[int(rng.integers(0, len(u["data"])))] ^= 1 << int(rng.integers(0, 8))
        if d[0] == 0xFF:
            d[0] = 0x7F
        idx, vals = E.first_out_of_range(plan, d, u["qp"])
        met += idx is not None
        r = E.read_plan(plan if idx is None else plan[:idx], d, u["qp"])
        assert r["values"] == vals[:r["n_written"]] and (r["n_written"] == len(vals) or r["flags"] == E.RES_BAD_VALUE), rep
    assert met
