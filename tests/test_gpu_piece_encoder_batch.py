"""GPU: the pieces on the lane-serial encoder at batch scale (include/cabac_hip_piece_encoder.h): cabac_hip_encode_pieces_device
under cabac_hip_piece_encoder_set(ctx, 7) in calls of 1 024 substreams and more, where launch_encode_pieces picks the geometry of
sixteen substreams per workgroup — four context waves that each export the sets of their own four rows, a chain wave with sixteen
live lanes, low and output waves with all 64 lanes live, the longest piece of sixteen substreams deciding the steps of all.

The directed substreams of tests/test_gpu_piece_encoder.py are hosted in a batch of N = 1 043 substreams (65 workgroups of
sixteen and a last one of three: unit 0 with three rows, units 1 .. 3 empty) at positions that are asserted on the CPU before
anything is launched; the rest of the batch are fillers from a pool of sixteen short record lists, so that the CPU model
(tests/pieces_model.py) runs once per pool entry and way of cutting.  Every substream of a batch gets the same number of launches:
a substream with fewer pieces is padded with empty ones (repeated cuts), so that no call falls below 1 024 substreams unless a
test says so.  Every batch is a Pair: the same launches under setting 4 on a second Run, and after every launch all slot bytes,
results, sets and all 32 bytes of every state are the same (D1); the sentinels around slots, states and sets are looked at every
time.  Everything is compared exactly.  Every test leaves setting 4."""
import collections
import functools

import numpy as np
import pytest

import ctx_sets_model as M
import emit_model as E
import helpers as H
import pieces_model as P
from entropy_coding_amd import capi
from test_gpu_piece_encoder import (ENC_REFUSED, POOL, SENT8, SENT32, Pair, Run, _spoil, burst_case, dev, emission_cases, host, one_call,
                                    short_case)

pytestmark = pytest.mark.gpu

N = 1043                                                           # 65 workgroups of sixteen and one of three
WG = 16
THRESHOLD = 1024                                                   # from here on launch_encode_pieces takes sixteen per workgroup


@pytest.fixture(scope="module")
def ctx():
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    c.set_variant(7, 1)   # the pieces calls ignore the variant: they must not follow this one
    yield c
    c.close()


@pytest.fixture
def hip(ctx):
    ctx.piece_encoder_set(7)
    yield ctx
    ctx.piece_encoder_set(4)


# ---------------------------------------------------------------------------------------------- the shared device
Case = collections.namedtuple("Case", "rec cuts qp init ctx cap", defaults=(None, None))


@functools.lru_cache(None)
def init_set(qp, init):
    return M.init_set(qp, init)


@functools.lru_cache(None)
def filler_pool():
    """Sixteen short record lists of 0 .. 40 records (one step, a step and a bin, three steps short of a bin), each with its qp
    and init_id"""
    rng = np.random.default_rng(9900)
    out = []
    for k, n in enumerate((0, 1, 2, 5, 9, 15, 16, 17, 23, 31, 32, 33, 36, 38, 39, 40)):
        rec = H.random_records(rng, n - 1, ctx_frac=0.8, ctx_pool=POOL) if n else np.zeros(0, np.uint16)
        assert len(rec) == n
        out.append((rec, 20 + k, k % 3))
    for w in range(N // WG):
        assert {filler_of(WG * w + r) for r in range(WG)} == set(range(16)), w
    return out


def filler_of(s):
    """The pool entry at position s: 5 s is a permutation modulo 16, so every full workgroup of fillers holds all sixteen entries,
    the empty one included, each time in another row"""
    return (5 * s + s // WG) % WG


def filler_cuts(n, pieces, s):
    """`pieces` pieces of a filler of n records.  Even positions: cut at the thirds, the pieces behind them empty and the last one
    only finishing; odd positions: empty pieces first — a fresh state passed through — and the thirds at the end."""
    thirds = [n // 3, 2 * n // 3][:pieces - 1]
    rest = pieces - 1 - len(thirds)
    return thirds + [n] * rest if s % 2 == 0 else [0] * rest + thirds


_models = {}


def model_of(c):
    """pieces_model.encode_pieces of one way of cutting one record list from one start set, evaluated once:
    ([n_bits behind every piece], [packed set behind every piece], the bytes of the whole)"""
    start = c.ctx if c.ctx is not None else init_set(c.qp, c.init)
    key = (c.rec.tobytes(), tuple(c.cuts), id(start))
    if key not in _models:
        out, data = P.encode_pieces(c.rec, list(c.cuts), start)
        _models[key] = ([o[0] for o in out], [M.pack(o[2]) for o in out], data, start)
    return _models[key][:3]


def place(n_cases, n=N):
    """The fixed permutation: the first sixteen cases fill workgroup 1, the next ones the last, partial workgroup, the others
    every second row of later workgroups — the even rows of workgroups 3, 6, 9, ..., the odd rows of workgroups 4, 7, 10, ...; in
    between a workgroup of fillers, so that a directed case stands between two fillers across the workgroups' borders too."""
    last = (n - 1) // WG * WG
    assert n_cases >= WG + n - last
    pos = list(range(WG, 2 * WG)) + list(range(last, n))
    k = 0
    while len(pos) < n_cases:
        w = 3 + 3 * (k // 2) + k % 2
        assert WG * (w + 2) < last
        pos += [WG * w + r for r in range(WG) if r % 2 == k % 2]
        k += 1
    return pos[:n_cases]


def assert_placement(where, n=N, every_row=False):
    """(a) a workgroup of directed cases alone, (b) directed cases in the last, partial workgroup, (c) everywhere else a directed
    case stands between two fillers of its workgroup, (d) every_row: a directed case in each of the sixteen rows"""
    at = set(where)
    last = (n - 1) // WG * WG
    assert len(at) == len(where) and all(0 <= s < n for s in where) and n - last < WG, "the last workgroup is a partial one"
    full = {w for w in range(last // WG) if all(WG * w + r in at for r in range(WG))}
    assert full, "(a)"
    assert any(s >= last for s in where), "(b)"
    for s in where:
        if s // WG not in full and s < last:
            beside = [t for t in (s - 1, s + 1) if t // WG == s // WG]
            assert beside and not any(t in at for t in beside), ("(c)", s)
    if every_row:
        assert {s % WG for s in where} == set(range(WG)), "(d)"


class Batch:
    """Directed cases at the positions `where` of a batch of n substreams, fillers everywhere else, as a Pair.  pieces: how many
    pieces a filler at position s is cut into (a number, or a function of s); a directed case brings its cuts.  launch() codes the
    next piece of the first n_sub substreams and compares every substream that is `exact` — its bytes fit its slot, and no test
    has spoiled its state — with the model: result, state, slot and set."""

    def __init__(self, hip, cases, where, n=N, pieces=2, setting=7, exact_fillers=False):
        assert len(cases) == len(where) == len(set(where)) and all(0 <= s < n for s in where)
        count = pieces if callable(pieces) else (lambda s: pieces)
        pool = filler_pool()
        at = dict(zip(where, cases))
        self.n, self.where = n, list(where)
        self.subs = []
        for s in range(n):
            if s in at:
                self.subs.append(at[s])
            else:
                rec, qp, init = pool[filler_of(s)]
                self.subs.append(Case(rec, tuple(filler_cuts(len(rec), count(s), s)), qp, init))
        self.model = [model_of(c) for c in self.subs]
        self.caps = [c.cap if c.cap is not None else len(m[2]) + (0 if exact_fillers and s not in at else 1 + 2 * (s % 2))
                     for s, (c, m) in enumerate(zip(self.subs, self.model))]
        self.exact = [len(m[2]) <= cap for m, cap in zip(self.model, self.caps)]
        self.spans = [P.pieces_of(len(c.rec), c.cuts) for c in self.subs]
        self.done = [0] * n
        self.pair = Pair(hip, [c.rec for c in self.subs], [c.qp for c in self.subs], [c.init for c in self.subs], caps=self.caps,
                         ctxs=[c.ctx if c.ctx is not None else init_set(c.qp, c.init) for c in self.subs], setting=setting)
        self.run = self.pair.a

    def launch(self, n_sub=None):
        n_sub = self.n if n_sub is None else n_sub
        assert all(self.done[s] < len(self.spans[s]) for s in range(n_sub)), "a piece for every substream of the launch"
        res = self.pair.launch([self.spans[s][self.done[s]] for s in range(n_sub)],
                               [self.done[s] == len(self.spans[s]) - 1 for s in range(n_sub)], n_sub)
        for s in range(n_sub):
            self.done[s] += 1
        self.check(res, n_sub)
        return res

    def check(self, res, n_sub):
        run = self.run
        st, image = run.states(), run.bytes()
        set_state, set_rate = host(run.d_state, np.uint32), host(run.d_rate, np.uint8)     # (Pair.launch has looked at the sentinels)
        for s in range(n_sub):
            if not self.exact[s]:
                continue
            bits, sets, data = self.model[s]
            i = self.done[s] - 1
            w, slot = st[s], run.slot(image, s)
            assert tuple(res[s]) == (bits[i], 0), (s, i, res[s])
            if i < len(bits) - 1:
                assert (w["kind"], w["flags"], w["bits"]) == (capi.CODER_ENC, 0, bits[i]), (s, i)
                nf = int(w["bytes_final"])
                assert nf % 2 == 0 and 8 * nf <= bits[i] and nf <= len(data), (s, i, nf)
            else:
                nf = len(data)
                assert (w["kind"], w["flags"], w["bits"], w["bytes_final"]) == (capi.CODER_CLOSED, 0, bits[i], nf) and not w["priv"].any(), (s, i)
            assert np.array_equal(slot[:nf], data[:nf]) and (slot[nf:] == SENT8).all(), (s, i, nf)
            a = (s + 1) * H.NUM_CTX
            assert np.array_equal(set_state[a:a + H.NUM_CTX], sets[i][0]) and np.array_equal(set_rate[a:a + H.NUM_CTX], sets[i][1]), (s, i)
        return st, image

    def put_states(self, st):
        """These states into both Runs, between the sentinel states"""
        given = np.concatenate([np.full(8, SENT32, np.uint32), np.ascontiguousarray(st).view(np.uint32), np.full(8, SENT32, np.uint32)])
        self.pair.a.d_coder, self.pair.b.d_coder = dev(given), dev(given)

    def against_one_call(self, hip):
        """Behind the last piece of every substream: results, slots and sets are those of the one-call sets form under variants 7 and 4"""
        run = self.run
        assert all(d == len(sp) for d, sp in zip(self.done, self.spans))
        for variant in (7, 4):
            ref, ref_res = one_call(hip, run, variant)
            assert np.array_equal(host(run.d_res, H.RESULT_DTYPE), ref_res), variant
            assert np.array_equal(run.bytes(), ref.bytes()), variant
            assert np.array_equal(host(run.d_state, np.uint32), host(ref.d_state, np.uint32)), variant
            assert np.array_equal(host(run.d_rate, np.uint8), host(ref.d_rate, np.uint8)), variant


# ---------------------------------------------------------------------------------------------- 1. every cut phase, every row
@functools.lru_cache(None)
def every_cut_case():
    rec, ctx, data, n_bits, left, probe = short_case()
    cases = [Case(rec, (k,), 31, 1) for k in range(71)]
    where = place(len(cases))
    assert_placement(where, every_row=True)
    return cases, where


def test_every_cut_of_a_short_substream_in_every_row(hip):
    rec, ctx, data, n_bits, left, probe = short_case()
    cases, where = every_cut_case()
    batch = Batch(hip, cases, where, pieces=2)
    run = batch.run
    res = batch.launch()                                 # (states, bytes_final, the slot up to it, the sentinels behind it, the sets:
    st = run.states()                                    #  Batch.check, for the directed cases and for every filler)
    for k, s in enumerate(where):
        assert tuple(res[s]) == (probe[k], 0) and st[s]["bits"] == probe[k], (k, s)
        assert np.array_equal(run.set_of(s)[0], M.pack(M.advance_from(rec[:k], ctx))[0]), (k, s)
    res = batch.launch()
    st, image = run.states(), run.bytes()
    for k, s in enumerate(where):
        assert tuple(res[s]) == (n_bits, 0) and st[s]["kind"] == capi.CODER_CLOSED and st[s]["bytes_final"] == len(data), (k, s)
        assert np.array_equal(run.slot(image, s, len(data)), data), (k, s)
    assert batch.pair.launches == 2


# ---------------------------------------------------------------------------------------------- 2. ragged lengths in one workgroup
RAGGED = (0, 1, 15, 16, 17, 33, 48, 65, 300, 1999, 2, 31, 32, 64, 129, 640)
RAGGED_LAUNCHES = 12


def ragged_cuts(n, r):
    """Eleven cuts: pieces of 1 (48 records and fewer), 7, 16, 17, 64 and 65 records in an order that turns with r, an empty piece
    in the middle, then the rest, then empty pieces; the twelfth piece only finishes"""
    sizes = [7, 16, 17, 64, 65]
    sizes = sizes[r % 5:] + sizes[:r % 5]
    if n <= 48:
        sizes = [1, 1] + sizes
    cuts, at = [], 0
    for k, size in enumerate(sizes):
        at = min(n, at + size)
        cuts.append(at)
        if k == 2:
            cuts.append(at)
    cuts.append(n)
    cuts += [n] * (RAGGED_LAUNCHES - 1 - len(cuts))
    assert len(cuts) == RAGGED_LAUNCHES - 1 and cuts[-1] == n
    return tuple(cuts)


@functools.lru_cache(None)
def ragged_case():
    """Workgroup 1: the sixteen lengths in the order above; workgroup 2: the same lists the other way round, 640 records in row 0
    and 1 999 in row 6; three more in the last workgroup and eight between fillers"""
    rng = np.random.default_rng(9910)
    recs = [H.random_records(rng, n - 1, ctx_frac=float(rng.choice([0.5, 0.8, 0.95])), ctx_pool=POOL) if n else np.zeros(0, np.uint16)
            for n in RAGGED]
    by_len = sorted(range(16), key=lambda k: len(recs[k]))
    order = list(range(16)) + by_len[::-1] + [8, 0, 4] + [9, 6, 1, 15, 5, 14, 3, 7]
    where = list(range(16, 32)) + list(range(32, 48)) + [1040, 1041, 1042] + list(range(65, 80, 2))
    cases = [Case(recs[k], ragged_cuts(len(recs[k]), s), int(rng.integers(0, 64)), int(rng.integers(0, 3))) for k, s in zip(order, where)]
    assert_placement(where, every_row=True)
    assert [len(c.rec) for c in cases[:16]] == list(RAGGED) and len(cases[16].rec) == 1999 and len(cases[31].rec) == 0
    sizes = {b - a for c in cases for a, b in P.pieces_of(len(c.rec), c.cuts)}
    assert {0, 1, 7, 16, 17, 64, 65} <= sizes and max(sizes) > 1000
    return cases, where


def test_ragged_lengths_inside_one_workgroup(hip):
    cases, where = ragged_case()
    batch = Batch(hip, cases, where, pieces=RAGGED_LAUNCHES)
    for i in range(RAGGED_LAUNCHES):
        batch.launch()                                   # (against the model after every launch: Batch.check)
    assert batch.pair.launches == RAGGED_LAUNCHES <= 12
    assert all(w["kind"] == capi.CODER_CLOSED for w in batch.run.states())
    batch.against_one_call(hip)


# ---------------------------------------------------------------------------------------------- 3. emission across a cut
CARRY_LATER = {"carry_run", "fin_carry_run"}


@functools.lru_cache(None)
def emission_batch_case():
    """The context-free cases of test_gpu_piece_encoder.emission_cases(), four pieces each, dealt so that every row of a workgroup
    gets a case in which a run of 0xFFFF units crosses a cut and is resolved without a carry, and one in which a carry arrives in a
    later piece than the run began in.  -> (cases as (records, cuts), positions, {row: events of its cases})"""
    cases = emission_cases()
    events = []
    for rec, cuts in cases:
        rp, _ = P.replay_pieces(rec, cuts)
        events.append({e[1] for e in rp.ev if isinstance(e, tuple)})
    carry = [k for k, ev in enumerate(events) if ev & CARRY_LATER]
    plain = [k for k, ev in enumerate(events) if ev and not ev & CARRY_LATER]
    assert len(carry) >= 19 and len(plain) >= 16
    order = carry[:19] + plain[:16]                      # workgroup 1 and the last one: carries; rows of workgroups 3 and 4: runs
    order += [k for k in range(len(cases)) if k not in set(order)][::4]     # and every fourth of the others
    where = place(len(order))
    assert_placement(where, every_row=True)
    by_row = {}
    for k, s in zip(order, where):
        by_row.setdefault(s % WG, []).append(events[k])
    return [cases[k] for k in order], where, by_row


def assert_emission_census(by_row):
    for r in range(WG):
        assert any(ev & CARRY_LATER for ev in by_row[r]), ("a carry resolved in a later piece", r)
        assert any(ev & {"ff_extend", "fin_nocarry_run"} for ev in by_row[r]), ("a run of 0xFFFF units across a cut", r)


def test_emission_across_a_cut_on_every_unit(hip):
    cases, where, by_row = emission_batch_case()
    assert_emission_census(by_row)
    cen = P.cross_census(cases)
    for ev in P.CROSS_EVENTS + ("run3",):
        assert len(cen.get(ev, ())) >= 1, ev
    want = [E.finished_bytes(E.code(rec)) for rec, _ in cases]
    directed = [Case(rec, tuple(cuts), 30, 1, cap=len(w[0]) + 1 + 2 * (k % 2)) for    # roomy, 1 or 3 bytes to spare
                k, ((rec, cuts), w) in enumerate(zip(cases, want))]
    batch = Batch(hip, directed, where, pieces=4)
    run = batch.run
    replay = [P.PieceReplay() for _ in cases]
    for i in range(4):
        res = batch.launch()
        st, image = run.states(), run.bytes()
        for k, s in enumerate(where):
            first, end = batch.spans[s][i]
            replay[k].feed(cases[k][0][first:end])
            if i < 3:
                w = replay[k].state()
                assert tuple(res[s]) == (w["bits"], 0), (k, s, i)
                assert (st[s]["kind"], st[s]["flags"], st[s]["bits"], st[s]["bytes_final"]) == (capi.CODER_ENC, 0, w["bits"], replay[k].pos), (k, s, i)
                assert tuple(int(x) for x in st[s]["priv"]) == w["priv"], (k, s, i)
                assert np.array_equal(run.slot(image, s, replay[k].pos), want[k][0][:replay[k].pos]), (k, s, i)
            else:
                assert tuple(res[s]) == (want[k][1], 0), (k, s, i)
                assert np.array_equal(run.slot(image, s, len(want[k][0])), want[k][0]), (k, s, i)


# ---------------------------------------------------------------------------------------------- 4. more than four units in a step
@functools.lru_cache(None)
def burst_batch_case():
    """burst_case()'s six substreams (it asserts grow >= 80 for each) in the rows of every unit: workgroup 1 holds the first four
    in rows 4 u .. 4 u + 3 of unit u; the other two of unit 0 stand in the last workgroup, those of units 1 .. 3 in rows 4 u and
    4 u + 2 of workgroup 3, between fillers.  -> (cases, positions, unit of every case)"""
    six = [Case(rec, (cut,), qp, init, ctx=ctx) for rec, cut, ctx, qp, init in burst_case()]
    cases, where, unit = [], [], []
    for u in range(4):
        for k in range(6):
            cases.append(six[k])
            unit.append(u)
            where.append(WG + 4 * u + k if k < 4 else (1040 + k - 4 if u == 0 else 3 * WG + 4 * u + 2 * (k - 4)))
    assert_placement(where, every_row=True)
    assert len(cases) == 24 and all(u == 0 if s >= 1040 else (s % WG) // 4 == u for s, u in zip(where, unit))
    for u in range(4):
        assert sorted(id(c) for c, v in zip(cases, unit) if v == u) == sorted(id(c) for c in six), u
    return cases, where


def test_a_step_of_more_than_four_units_on_every_unit(hip):
    cases, where = burst_batch_case()
    batch = Batch(hip, cases, where, pieces=2)
    run = batch.run
    ref = [M.encode_from(c.rec, c.ctx, 3) for c in cases]
    res = batch.launch()
    st, image = run.states(), run.bytes()
    for k, (c, s) in enumerate(zip(cases, where)):
        cut = c.cuts[0]
        want = M.encode_from(c.rec[:cut], c.ctx, 4)[2]
        assert tuple(res[s]) == (want, 0) and (st[s]["kind"], st[s]["flags"], st[s]["bits"]) == (capi.CODER_ENC, 0, want), s
        nf = int(st[s]["bytes_final"])
        assert nf % 2 == 0 and np.array_equal(run.slot(image, s, nf), ref[k][1][:nf]) and (run.slot(image, s)[nf:] == SENT8).all(), s
        assert want - 8 * nf < 16 * int(st[s]["priv"][3]) + 16, s
        got = run.set_of(s)
        assert all(np.array_equal(x, y) for x, y in zip(got, M.pack(M.advance_from(c.rec[:cut], c.ctx)))), s
    res = batch.launch()
    st, image = run.states(), run.bytes()
    for k, (c, s) in enumerate(zip(cases, where)):
        nb = len(ref[k][1])
        assert tuple(res[s]) == (ref[k][2], 0) and st[s]["kind"] == capi.CODER_CLOSED and st[s]["bytes_final"] == nb, s
        assert np.array_equal(run.slot(image, s, nb), ref[k][1]) and (run.slot(image, s)[nb:] == SENT8).all(), s
        assert all(np.array_equal(x, y) for x, y in zip(run.set_of(s), M.pack(ref[k][3]))), s


# ---------------------------------------------------------------------------------------------- 5. capacity
@functools.lru_cache(None)
def capacity_batch_case():
    """emit_model.capacity_cases() x eight capacities, three pieces, the last only finishing.  Workgroup 1: too small a slot in
    every even row, an exact one (cap == the coded bytes) in every odd row; the last workgroup: exact, too small, exact; the rest
    between fillers, whose slots are exact in this batch.  -> (cases, positions, coded bytes per case)"""
    small, fits, roomy, coded = [], [], [], {}
    for name, rec in E.capacity_cases():
        data, _ = E.roomy(rec, 30, 1)
        n = len(data)
        for cap in (0, 1, 2, n // 2, n - 2, n - 1, n, n + 2):
            c = Case(rec, (len(rec) // 2, len(rec)), 30, 1, cap=cap)
            coded[id(c)] = data
            (small if cap < n else fits if cap == n else roomy).append(c)
    assert len(fits) >= 10 and len(small) >= 9
    first = small[::8][:9]                               # (every eighth: other cases, other capacities)
    order = [x for pair in zip(first[:8], fits[:8]) for x in pair] + [fits[8], first[8], fits[9]]
    order += [c for c in small if id(c) not in {id(x) for x in first}] + fits[10:] + roomy
    where = place(len(order))
    assert_placement(where)
    return order, where, [coded[id(c)] for c in order]


def test_capacity_flags_the_same_substreams_beside_exact_slots(hip):
    cases, where, coded = capacity_batch_case()
    batch = Batch(hip, cases, where, pieces=3, exact_fillers=True)
    over = {s for s in range(N) if not batch.exact[s]}
    assert over == {s for c, s, data in zip(cases, where, coded) if c.cap < len(data)} and len(over) == 72
    for s in over:                                       # both neighbours' slots hold their bytes to the byte
        for t in (s - 1, s + 1):
            assert batch.caps[t] == len(batch.model[t][2]), (s, t)
    run = batch.run
    out = [batch.launch() for _ in range(3)]             # (no byte outside any slot, the neighbours byte-exact: after every launch;
    st = run.states()                                    #  the same substreams flagged, piece by piece, as under setting 4: the Pair)
    for s in over:
        flagged = [bool(o[s]["flags"] & H.RES_OVERFLOW) for o in out]
        assert flagged[2] and flagged == sorted(flagged), (s, flagged)       # once raised it stays
        assert all(int(o[s]["flags"]) in (0, H.RES_OVERFLOW) for o in out), s
        if flagged[1]:                                                        # raised before the last piece: it codes nothing
            assert tuple(out[2][s]) == (0, H.RES_OVERFLOW) and st[s]["flags"] == H.RES_OVERFLOW and st[s]["kind"] == capi.CODER_ENC, s
    for c, s, data in zip(cases, where, coded):
        if s not in over:
            assert out[2][s]["n_bits"] == 8 * len(data) and np.array_equal(run.slot(run.bytes(), s, len(data)), data), s


# ---------------------------------------------------------------------------------------------- 6. refused, flagged, bad set
@functools.lru_cache(None)
def refused_batch_case():
    """Workgroups 1 .. 4 and the last one hold one directed substream, 120 records cut at 50.  What the second piece of a row
    finds — -> {position: condition}:
      workgroup 1   a refused state in every odd row, eight conditions: refused and valid lanes alternate in the chain wave
      workgroup 2   the other two conditions, a state with a sticky flag and a start set out of range in rows 0, 2, 4, 6
      workgroup 3   one whole unit refused: rows 8 .. 11, the four rows of one context wave
      workgroup 4   all sixteen rows refused, flagged or without their set: the workgroup's longest piece has no record, no step runs
      the last one  a refused state between two valid ones"""
    bad = {WG + 2 * k + 1: c for k, c in enumerate(ENC_REFUSED[:8])}
    bad.update({2 * WG: ENC_REFUSED[8], 2 * WG + 2: ENC_REFUSED[9], 2 * WG + 4: "sticky", 2 * WG + 6: "bad-set"})
    bad.update({3 * WG + 8 + k: c for k, c in enumerate(("enc-bits", "kind-closed", "enc-low", "enc-capacity"))})
    kinds = ENC_REFUSED + ("sticky", "bad-set")
    bad.update({4 * WG + r: kinds[(5 * r) % len(kinds)] for r in range(WG)})
    bad[1041] = "enc-pend"
    where = list(range(WG, 5 * WG)) + [1040, 1041, 1042]
    assert_placement(where, every_row=True)
    assert set(bad.values()) == set(kinds) and set(bad) <= set(where)
    return where, bad


def test_refused_flagged_and_bad_set_pieces_beside_valid_neighbours(hip):
    """These are states the header defines; no arbitrary garbage is fed.  A refused row is given set 0 — the sentinel set in
    front of the array — as its out set: a set exported for it would land there and is seen.  (A flagged row keeps its own, in
    place: the header does not say that a piece which only copies its state leaves the out set alone.)"""
    where, bad = refused_batch_case()
    rng = np.random.default_rng(9970)
    rec = H.random_records(rng, 119, ctx_frac=0.8, ctx_pool=POOL)
    data = M.encode_from(rec, init_set(32, 0), 3)[1]
    batch = Batch(hip, [Case(rec, (50,), 32, 0, cap=len(data) + 5)] * len(where), where, pieces=2)
    run = batch.run
    batch.launch()
    st = run.states()
    assert all(st[s]["kind"] == capi.CODER_ENC and st[s]["flags"] == 0 for s in where)
    given = st.copy()
    start = np.arange(1, N + 1, dtype=np.uint32)
    out = start.copy()
    for s, what in bad.items():
        if what == "sticky":
            given[s]["flags"] = H.RES_OVERFLOW
        elif what == "bad-set":
            start[s] = N + 2                             # the first index behind the sets
        else:
            given[s] = _spoil(st[s], what, batch.caps[s])
            out[s] = 0
        batch.exact[s] = False                           # not the model's any more: looked at below
    batch.put_states(given)
    for r in (batch.pair.a, batch.pair.b):
        r.d_idx = dev(start)
    d_out = dev(out)
    bytes_before, sets_before, rates_before = host(run.d_bytes, np.uint8).copy(), host(run.d_state, np.uint32).copy(), host(run.d_rate, np.uint8).copy()

    class OutSets:
        """The ctx with the out set indices of the pieces call from an array of their own (Run passes one array for both)"""
        def __getattr__(self, name):
            return getattr(hip, name)

        def encode_pieces_device(self, *args):
            return hip.encode_pieces_device(*args[:9], d_out.data_ptr(), *args[10:])
    for r in (batch.pair.a, batch.pair.b):
        r.hip = OutSets()
    res = batch.launch()                                 # (the valid neighbours and all fillers: exact, their sets right, CLOSED)
    after, image = run.states(), run.bytes()
    for s, what in bad.items():
        want = given[s].copy()
        if what == "sticky":
            assert tuple(res[s]) == (0, H.RES_OVERFLOW), (s, what, res[s])
        elif what == "bad-set":                          # {0, CABAC_RES_BAD_SET}, the state copied with the flag
            assert tuple(res[s]) == (0, M.RES_BAD_SET), (s, what, res[s])
            want["flags"] = M.RES_BAD_SET
        else:
            assert tuple(res[s]) == (0, capi.RES_BAD_STATE), (s, what, res[s])
        assert after[s].tobytes() == want.tobytes(), (s, what)                                  # untouched / copied
        assert np.array_equal(run.slot(image, s), run.slot(bytes_before, s)), (s, what)          # no byte
        a = (s + 1) * H.NUM_CTX
        assert np.array_equal(host(run.d_state, np.uint32)[a:a + H.NUM_CTX], sets_before[a:a + H.NUM_CTX]), (s, what)   # no set
        assert np.array_equal(host(run.d_rate, np.uint8)[a:a + H.NUM_CTX], rates_before[a:a + H.NUM_CTX]), (s, what)
    run.set_of(0)                                        # the sentinel sets are what they were
    assert sum(1 for s in where if s not in bad and after[s]["kind"] == capi.CODER_CLOSED) == len(where) - len(bad)


# ---------------------------------------------------------------------------------------------- 7. no state arrays
def test_all_fresh_all_final_without_state_arrays(hip):
    cases, where = ragged_case()
    cases = [c._replace(cuts=()) for c in cases]
    batch = Batch(hip, cases, where, pieces=1)           # (its Pair is not launched: the three ways of passing states are)
    subs = batch.subs
    spans, fin = [(0, len(c.rec)) for c in subs], [True] * N
    make = lambda: Run(hip, [c.rec for c in subs], [c.qp for c in subs], [c.init for c in subs], caps=batch.caps,
                       ctxs=[init_set(c.qp, c.init) for c in subs])
    refs = [one_call(hip, make(), variant) for variant in (7, 4)]
    assert not refs[0][1]["flags"].any()
    untouched = np.full(8 * (N + 2), SENT32, np.uint32)
    for coder_in, coder_out in ((False, False), (False, True), (True, False)):
        got = []
        for setting in (4, 7):
            hip.piece_encoder_set(setting)
            run = make()
            if not coder_in:
                run.d_coder = dev(untouched)             # no state is read: sentinel states everywhere
            before = host(run.d_coder, np.uint32).copy()
            res = run.launch(False, spans, fin, coder_in=coder_in, coder_out=coder_out)
            for ref, ref_res in refs:
                assert np.array_equal(res, ref_res), (coder_in, coder_out, setting)
                assert np.array_equal(run.bytes(), ref.bytes()), (coder_in, coder_out, setting)
                assert np.array_equal(host(run.d_state, np.uint32), host(ref.d_state, np.uint32)), (coder_in, coder_out, setting)
                assert np.array_equal(host(run.d_rate, np.uint8), host(ref.d_rate, np.uint8)), (coder_in, coder_out, setting)
            if coder_out:
                st = run.states()
                for s in range(N):
                    bits, _, data = batch.model[s]
                    assert (st[s]["kind"], st[s]["flags"], st[s]["bits"], st[s]["bytes_final"]) == (capi.CODER_CLOSED, 0, bits[0], len(data)), s
                    assert tuple(res[s]) == (bits[0], 0) and not st[s]["priv"].any(), s
            else:
                assert np.array_equal(host(run.d_coder, np.uint32), before), "a state written without coder_out"
            got.append(run.everything())
        for k, (x, y) in enumerate(zip(*got)):           # D1
            assert np.array_equal(x, y), (coder_in, coder_out, k)


# ---------------------------------------------------------------------------------------------- 8. the threshold
@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_one_substream_below_at_and_above_the_threshold(hip, n):
    """1 023: four per workgroup; 1 024: sixty-four full workgroups of sixteen; 1 025: a last workgroup of one substream"""
    rec = short_case()[0]
    where = [0, 1, n - 3, n - 2, n - 1]
    cases = [Case(rec, (k,), 31, 1) for k in (0, 16, 33, 69, 70)]
    batch = Batch(hip, cases, where, n=n, pieces=2)
    assert (n >= THRESHOLD) == (n != 1023) and (n - 1) % WG == (14, 15, 0)[n - 1023]
    batch.launch()
    batch.launch()
    batch.against_one_call(hip)


CROSSING = (1040, 1023, 1024, 1000)


@functools.lru_cache(None)
def crossing_case():
    """1 040 substreams and four launches over the first 1 040, 1 023, 1 024 and 1 000 of them: substreams 0 .. 999 have four
    pieces, 1 000 .. 1 022 three, 1 024 .. 1 039 one — and substream 1 023 two, the second of which is not ready for the second
    launch and goes with the third (a prefix cannot grow otherwise).  So the states of the first 1 000 are written by sixteen
    per workgroup, continued by four per workgroup, and again.  -> (cases, positions, pieces of every position)"""
    n = CROSSING[0]
    pieces = lambda s: 4 if s < 1000 else 3 if s < 1023 else 2 if s == 1023 else 1
    done = [0] * n
    for n_sub in CROSSING:                               # every launch finds a piece for each of its substreams ...
        assert all(done[s] < pieces(s) for s in range(n_sub)), n_sub
        for s in range(n_sub):
            done[s] += 1
    assert done == [pieces(s) for s in range(n)]         # ... and the four launches are all the pieces there are
    assert [sum(1 for s in range(n) if pieces(s) > i) for i in range(4)] == [1040, 1024, 1023, 1000]
    assert [(n_sub >= THRESHOLD) for n_sub in CROSSING] == [True, False, True, False]
    rec = short_case()[0]
    where = list(range(16)) + [999, 1000, 1022, 1023, 1024, 1039]
    cuts = {4: (17, 33, 64), 3: (16, 70), 2: (35,), 1: ()}
    return [Case(rec, cuts[pieces(s)], 31, 1) for s in where], where, pieces


@pytest.mark.parametrize("setting", [7, 0])
def test_states_cross_the_threshold_and_back(hip, setting):
    cases, where, pieces = crossing_case()
    batch = Batch(hip, cases, where, n=CROSSING[0], pieces=pieces, setting=setting)
    for n_sub in CROSSING:
        batch.launch(n_sub)                              # (D1 and the model after every launch)
    assert all(w["kind"] == capi.CODER_CLOSED for w in batch.run.states())
    batch.against_one_call(hip)
