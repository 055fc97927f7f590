"""GPU: the plan write in pieces at batch scale (include/cabac_hip_plan_continue.h): cabac_hip_plan_continue_write_device on 1 030
substreams, where the two plan walks run hundreds of workgroups, the scan of the record counts runs over more than one block,
plan_stops_pieces_kernel runs five blocks and the encode leg under cabac_hip_piece_encoder_set(ctx, 7) takes sixteen substreams
per workgroup — and, as substreams finish at different pieces, later launches fall below 1 024 and below 256 substreams.

The units are those of tests/test_gpu_plan_continue.py (batch_case, shape_case, boundary_case, stop_case) with their cuts,
replicated; tests/plan_continue_model.py is evaluated once per distinct (unit, cuts).  Everything is bit-exact: == on integers;
guards and sentinels are looked at after every launch (test_gpu_plan_continue.Run does).  Every test leaves setting 4."""
import functools

import numpy as np
import pytest

import helpers as H
import plan_continue_model as C
import plan_resume_model as R
import write_plan_model as W
from entropy_coding_amd import capi
from test_gpu_plan_continue import (ENC_REFUSED, Run, _spoil, assert_c1, assert_closed, assert_open, assert_set, assert_written, batch_case,
                                    boundary_case, shape_case, stop_case)

pytestmark = pytest.mark.gpu

N = 1030
EDGES = (255, 256, 1023, 1024, N - 1)                              # either side of a block of 256 and of the encoder's threshold
SAMPLE = sorted(set(range(0, N, 8)) | set(EDGES))                  # the substreams compared with the model after every launch


@pytest.fixture(scope="module")
def ctx():
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    yield c
    c.close()


@pytest.fixture
def hip(ctx):
    ctx.piece_encoder_set(7)
    yield ctx
    ctx.piece_encoder_set(4)


def check_sample(run, units, spans, exp, sample):
    """test_gpu_plan_continue.check_against_model on the substreams of `sample`: results, states, sets, bytes, values and info
    words behind every piece are the model's"""
    def check(i, res, n_sub):
        st, sets = run.states(), run.sets()
        for s in sample:
            if s >= n_sub:
                continue
            out, data = exp[s]
            n_bits, flags, left = out[i]
            assert tuple(res[s]) == (n_bits, flags), (i, s)
            assert_set(sets, s, left, (i, s))
            assert_written(run, s, units[s], spans[s][i][2], spans[s][i][3], what=(i, s))
            if i < len(spans[s]) - 1:
                assert_open(run, st, s, n_bits, data, (i, s))
            else:
                assert_closed(run, st, s, n_bits, data, what=(i, s))
    return check


# ---------------------------------------------------------------------------------------------- 9. model, setting 4, the one call
@functools.lru_cache(maxsize=None)
def scale_case():
    """The distinct (unit, cuts) of batch_case(), shape_case() and boundary_case() — of the latter five cuts of the chain in
    one substream and six single cuts — replicated to 1 030 substreams, more pieces first, the ways of cutting with equally many
    pieces dealt in turn.  -> (units, cuts, model per substream, substreams per launch)"""
    distinct = [(u, c, e) for (u, c), e in zip(*batch_case())] + [(u, c, e) for (u, c), e in zip(*shape_case())]
    u, cuts, exp = boundary_case()
    few = cuts[0][3::7][:5]
    distinct.append((u, few, C.expect(u, few)))
    distinct += [(u, cuts[k], exp[k]) for k in range(1, len(cuts), max(1, (len(cuts) - 1) // 6))][:6]
    by_pieces = {}
    for d in distinct:
        by_pieces.setdefault(len(d[1]) + 1, []).append(d)
    assert set(by_pieces) == {12, 9, 6, 4, 2, 1} and len(by_pieces[2]) == 7, {k: len(v) for k, v in by_pieces.items()}
    copies = {12: 100, 9: 100, 6: 200, 4: 200, 2: 425, 1: 5}
    subs = []
    for pieces in sorted(by_pieces, reverse=True):
        subs += [by_pieces[pieces][j % len(by_pieces[pieces])] for j in range(copies[pieces])]
    assert len(subs) == N
    live = [sum(1 for d in subs if len(d[1]) + 1 > i) for i in range(12)]
    # every substream, then all but five (sixteen per workgroup, on states from memory), then below 1 024, then below 256
    assert live == [1030, 1025, 600, 600, 400, 400, 200, 200, 200, 100, 100, 100], live
    return [d[0] for d in subs], [d[1] for d in subs], [d[2] for d in subs], live


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_a_thousand_substreams_against_the_model_setting_4_and_the_one_call(hip, int16):
    units, cuts, exp, live = scale_case()
    run7, run4 = Run(hip, units, int16), Run(hip, units, int16)
    spans = [R.spans_of(u, c) for u, c in zip(units, cuts)]
    check = check_sample(run7, units, spans, exp, SAMPLE)
    assert set(EDGES) <= set(SAMPLE) and len(SAMPLE) <= N // 8 + 1 + len(EDGES)
    for i, n_sub in enumerate(live):
        assert n_sub == sum(1 for sp in spans if len(sp) > i)
        args = ([sp[i] for sp in spans[:n_sub]], [i == len(sp) - 1 for sp in spans[:n_sub]], n_sub)
        hip.piece_encoder_set(4)
        res4 = run4.launch(*args)
        hip.piece_encoder_set(7)
        res7 = run7.launch(*args)
        check(i, res7, n_sub)
        assert np.array_equal(res7, res4), i                        # every substream: the two settings write the same
        assert run7.states().tobytes() == run4.states().tobytes(), i
        assert np.array_equal(run7.bytes(), run4.bytes()), i
        assert np.array_equal(run7.values(), run4.values()) and np.array_equal(run7.info, run4.info), i
        assert np.array_equal(run7.last_info, run4.last_info), i
        for x, y in zip(run7.sets(), run4.sets()):
            assert np.array_equal(x, y), i
    assert all(w["kind"] == capi.CODER_CLOSED for w in run7.states())
    assert_c1(run7, Run(hip, units, int16), units, exp)


# ---------------------------------------------------------------------------------------------- 10. stops and refusals
AT = (3, 255, 256, 257, 1023, 1024, N - 1)
AT_LATER = (5, 259, 1021, 1026)                                    # spoiled one piece later


def _neighbours(special):
    """The 1-in-8 sample and the four substreams around every special one"""
    near = {s + d for s in special for d in (-2, -1, 1, 2) if 0 <= s + d < N}
    return sorted((set(SAMPLE) | near) - set(special))


def _snapshot(run, subs):
    return (run.states(), run.sets(), run.bytes(), {s: run.values(s) for s in subs}, {s: run.infos(s) for s in subs})


def _assert_nothing_written(run, s, st, sets, image, before, want_state, what):
    was_st, was_sets, was_image, was_val, was_info = before
    assert st[s].tobytes() == want_state.tobytes(), what
    assert np.array_equal(run.slot(s, image=image), run.slot(s, image=was_image)), ("a byte", what)
    assert np.array_equal(sets[0][s], was_sets[0][s]) and np.array_equal(sets[1][s], was_sets[1][s]), ("a set", what)
    assert np.array_equal(run.values(s), was_val[s]) and np.array_equal(run.infos(s), was_info[s]), ("a value or an info word", what)


def test_stops_at_high_indices_raise_their_flag_in_their_own_piece(hip):
    """The five stopping substreams of stop_case() — BAD_VALUE in piece 1 and in piece 0, BAD_RECORD from a bad entry and from a
    reference across a cut, a coded block without a coefficient — at indices on either side of a block of 256 substreams and of
    1 024, every other substream the good unit.  plan_stops_pieces_kernel gives a stop its result and its flag."""
    cases, good, (out, data) = stop_case()
    stopping = [c for c in cases if c[2] is not None]
    assert len(stopping) == 5
    special = {s: stopping[(j + 2) % 5] for j, s in enumerate(AT)}
    assert {c[3] for s, c in special.items() if s >= 1024} == {W.BAD_VALUE, W.BAD_RECORD} == {c[3] for s, c in special.items() if s < 256}
    units = [special[s][0] if s in special else good for s in range(N)]
    spans = [R.spans_of(good, special[s][1] if s in special else cases[0][1]) for s in range(N)]
    run = Run(hip, units)
    neighbours = check_sample(run, units, spans, [(out, data)] * N, _neighbours(special))
    before = _snapshot(run, special)
    for i in range(3):
        res = run.launch([sp[i] for sp in spans], [i == 2] * N)
        st, sets, image = run.states(), run.sets(), run.bytes()
        neighbours(i, res, N)
        for s, (u, c, k, flag) in special.items():
            e1, b1 = spans[s][i][2:]
            if i < k:                                               # in front of the stop: the prefix of the good unit
                n_bits = H.load_oracle().encode_records(R.prefix_string(good, e1, b1), good["qp"], C.INIT_ID, 4)[1]
                assert tuple(res[s]) == (n_bits, 0), (i, s)
                assert_open(run, st, s, n_bits, data, (i, s))
            else:                                                   # {0, flag}; the flag ORed into the state; then passed on
                assert tuple(res[s]) == (0, flag), (i, s, res[s])
                want = before[0][s].copy()
                if i == k and want["kind"] == capi.CODER_FRESH:     # a fresh in state comes out as the state of start()
                    want["kind"], want["priv"] = capi.CODER_ENC, [0, 510, 0, 0]
                want["flags"] |= flag
                assert want["kind"] == capi.CODER_ENC and want["flags"] == flag, (i, s)
                _assert_nothing_written(run, s, st, sets, image, before, want, (i, s))
        before = _snapshot(run, special)


def test_refused_and_flagged_states_at_high_indices_write_nothing(hip):
    """Every refused condition of cabac_hip_pieces.h and one state with a sticky flag, on valid states behind piece 0 (seven of them,
    at the indices of the test above, refused again by the last piece) and behind piece 1 (the other four).  These are states the
    header defines; no arbitrary garbage is fed."""
    cases, good, (out, data) = stop_case()
    kinds = ("sticky",) + ENC_REFUSED
    assert len(kinds) == len(AT) + len(AT_LATER)
    when = {s: (1, kinds[j]) for j, s in enumerate(AT)}
    when.update({s: (2, kinds[len(AT) + j]) for j, s in enumerate(AT_LATER)})
    units = [good] * N
    spans = [R.spans_of(good, cases[0][1])] * N
    run = Run(hip, units)
    neighbours = check_sample(run, units, spans, [(out, data)] * N, _neighbours(when))
    given = {}
    for i in range(3):
        st = run.states()
        for s, (first, what) in when.items():
            if first == i:
                assert st[s]["kind"] == capi.CODER_ENC and st[s]["flags"] == 0
                if what == "sticky":
                    st[s]["flags"] = H.RES_OVERFLOW
                else:
                    st[s] = _spoil(st[s], what, int(run.caps[s]))
                given[s] = st[s].copy()
        run.put_states(st)
        before = _snapshot(run, when)
        res = run.launch([sp[i] for sp in spans], [i == 2] * N)
        st, sets, image = run.states(), run.sets(), run.bytes()
        neighbours(i, res, N)
        for s, (first, what) in when.items():
            if i < first:                                           # still a valid one
                assert tuple(res[s]) == out[i][:2], (i, s)
                assert_open(run, st, s, out[i][0], data, (i, s))
            else:
                assert tuple(res[s]) == ((0, H.RES_OVERFLOW) if what == "sticky" else (0, capi.RES_BAD_STATE)), (i, s, what, res[s])
                _assert_nothing_written(run, s, st, sets, image, before, given[s], (i, s, what))
