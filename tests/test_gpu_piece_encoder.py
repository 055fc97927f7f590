"""GPU: the pieces on the lane-serial encoder (include/cabac_hip_piece_encoder.h): cabac_hip_encode_pieces_device and the encode
leg of cabac_hip_plan_continue_write_device under cabac_hip_piece_encoder_set(ctx, 7) and (ctx, 0), against tests/pieces_model.py
(the oracle's record coder on prefixes, the sets between pieces, the emission replayed piece by piece), against the one-call sets
form on the device, and against the same cuts under setting 4 on a second Run: D1 says every byte, result, set and all 32 bytes of
every state are the same.  Everything is compared exactly; there are sentinels around every byte slot, around the state array and
around the sets, and they are looked at after every launch.  Setting 7 is used unless said otherwise; every test leaves setting 4.

Every test calls piece_encoder_set, so none passes without it."""
import functools

import numpy as np
import pytest
import torch

import ctx_sets_model as M
import emit_model as E
import helpers as H
import pieces_model as P
from entropy_coding_amd import capi

pytestmark = pytest.mark.gpu

FIN = H.SUB_FINISH | H.SUB_ALIGN_RBSP
SENT32, SENT8 = 0x5A5A5A5A, 0xA5
GUARD = 64
POOL = np.arange(86, 292)
ST = capi.CODER_STATE_DTYPE


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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same_ctx(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


class Run:
    """n_sub substreams coded in pieces on the device.  Byte slots of exact capacity at 16-aligned offsets with GUARD sentinel bytes
    around each; one state per substream in ONE array (in and out the same) with a sentinel state in front and behind; one set
    per substream, started from and written back in place, with a sentinel set in front and behind."""

    def __init__(self, hip, recs, qps, inits, caps=None, ctxs=None, data=None):
        self.hip, self.n = hip, len(recs)
        self.recs = [np.ascontiguousarray(r, np.uint16) for r in recs]
        self.qps, self.inits = np.asarray(qps, np.int32), np.asarray(inits, np.uint32)
        lens = np.array([len(r) for r in recs], np.int64)
        self.base = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        self.records = np.concatenate(self.recs + [np.zeros(8, np.uint16)]).astype(np.uint16)
        self.d_rec = dev(self.records)
        self.caps = np.asarray(caps if caps is not None else [len(r) + 64 for r in recs], np.int64)
        self.off = np.zeros(self.n, np.int64)
        at = GUARD
        for s in range(self.n):
            self.off[s] = at
            at = (at + int(self.caps[s]) + GUARD + 15) // 16 * 16
        self.total = at + GUARD
        image = np.full(self.total + 16, SENT8, np.uint8)
        if data is not None:                       # decode: the substreams' bytes, zeros up to the capacity
            for s in range(self.n):
                o, c = int(self.off[s]), int(self.caps[s])
                image[o:o + c] = 0
                k = min(c, len(data[s]))
                image[o:o + k] = data[s][:k]
        self.d_bytes = dev(image)
        self.outside = np.ones(self.total + 16, bool)
        for s in range(self.n):
            self.outside[int(self.off[s]):int(self.off[s]) + int(self.caps[s])] = False
        self.ctxs = ctxs if ctxs is not None else [M.init_set(int(q), int(i)) for q, i in zip(self.qps, self.inits)]
        state = np.full((self.n + 2) * H.NUM_CTX, SENT32, np.uint32)
        rate = np.full((self.n + 2) * H.NUM_CTX, SENT8, np.uint8)
        for s, c in enumerate(self.ctxs):
            a = (s + 1) * H.NUM_CTX
            state[a:a + H.NUM_CTX], rate[a:a + H.NUM_CTX] = M.pack(c)
        self.d_state, self.d_rate = dev(state), dev(rate)
        self.d_idx = dev(np.arange(1, self.n + 1, dtype=np.uint32))
        self.d_coder = dev(np.concatenate([np.full(8, SENT32, np.uint32), np.zeros(8 * self.n, np.uint32), np.full(8, SENT32, np.uint32)]))
        self.d_bins = torch.full((len(self.records) + 16,), SENT8, dtype=torch.uint8, device="cuda")
        self.d_res = dev(np.full(2 * self.n, SENT32, np.uint32))

    def launch(self, decode, spans, fin, n_sub=None, coder_in=True, coder_out=True):
        """One piece of the first n_sub substreams: spans[s] = (first, end) in the substream's records, fin[s]: the last piece."""
        n_sub = self.n if n_sub is None else n_sub
        d = np.zeros(n_sub, H.DESC_DTYPE)
        for s in range(n_sub):
            first, end = spans[s]
            d[s] = (self.base[s] + first, self.off[s], end - first, self.caps[s], self.qps[s], int(self.inits[s]) | (FIN if fin[s] else 0))
        d_desc = dev(d)
        args = (self.n + 2, self.d_state.data_ptr(), self.d_rate.data_ptr(), self.d_idx.data_ptr(), self.d_idx.data_ptr(),
                self.d_state.data_ptr(), self.d_rate.data_ptr(), self.d_coder.data_ptr() + 32 if coder_in else 0,
                self.d_coder.data_ptr() + 32 if coder_out else 0)
        if decode:
            self.hip.decode_pieces_device(n_sub, d_desc.data_ptr(), self.d_rec.data_ptr(), self.d_bytes.data_ptr(), self.d_bins.data_ptr(),
                                          self.d_res.data_ptr(), *args)
        else:
            self.hip.encode_pieces_device(n_sub, d_desc.data_ptr(), self.d_rec.data_ptr(), self.d_bytes.data_ptr(), self.d_res.data_ptr(), *args)
        self.hip.synchronize()
        return host(self.d_res, H.RESULT_DTYPE).copy()

    def states(self):
        raw = host(self.d_coder, np.uint32)
        assert (raw[:8] == SENT32).all() and (raw[-8:] == SENT32).all(), "the states around the array"
        return raw[8:-8].view(ST).copy()

    def bytes(self, encode=True):
        b = host(self.d_bytes, np.uint8)
        if encode:
            assert (b[self.outside] == SENT8).all(), "a byte outside the slots"
        return b

    def slot(self, b, s, n=None):
        o = int(self.off[s])
        return b[o:o + (int(self.caps[s]) if n is None else n)]

    def set_of(self, s):
        st, rt = host(self.d_state, np.uint32), host(self.d_rate, np.uint8)
        assert (st[:H.NUM_CTX] == SENT32).all() and (st[-H.NUM_CTX:] == SENT32).all(), "the sets around the array"
        assert (rt[:H.NUM_CTX] == SENT8).all() and (rt[-H.NUM_CTX:] == SENT8).all()
        a = (s + 1) * H.NUM_CTX
        return st[a:a + H.NUM_CTX], rt[a:a + H.NUM_CTX]

    def bins(self, s):
        b = host(self.d_bins, np.uint8)
        assert (b[len(self.records) - 8:] == SENT8).all()
        return b[int(self.base[s]):int(self.base[s]) + len(self.recs[s])]

    def everything(self, encode=True):
        """All the call writes, sentinels included and looked at: slots, results, states, sets"""
        self.states(), self.set_of(0)
        return [self.bytes(encode).copy(), host(self.d_res, np.uint32).copy(), host(self.d_coder, np.uint32).copy(),
                host(self.d_state, np.uint32).copy(), host(self.d_rate, np.uint8).copy()]


class Pair:
    """The same substreams on two Runs: `a` launched under `setting`, `b` under setting 4, and after every launch everything
    the two have written is the same (D1) — all slot bytes, results, sets and all 32 bytes of every state."""

    def __init__(self, hip, *args, setting=7, **kw):
        self.hip, self.setting = hip, setting
        self.a, self.b = Run(hip, *args, **kw), Run(hip, *args, **kw)
        self.launches = 0

    def launch(self, spans, fin, n_sub=None):
        self.hip.piece_encoder_set(4)
        self.b.launch(False, spans, fin, n_sub)
        self.hip.piece_encoder_set(self.setting)
        res = self.a.launch(False, spans, fin, n_sub)
        for k, (x, y) in enumerate(zip(self.a.everything(), self.b.everything())):
            assert np.array_equal(x, y), (self.launches, ("bytes", "results", "states", "set states", "set rates")[k],
                                          np.flatnonzero(x != y)[:8])
        self.launches += 1
        return res


def one_call(hip, run, variant=4):
    """The sets form on the device under the forced variant, on the whole substreams of `run`, from the same start contexts"""
    hip.set_variant(variant, 4 if variant == 4 else 1)
    try:
        ref = Run(hip, run.recs, run.qps, run.inits, run.caps, run.ctxs)
        d = np.zeros(ref.n, H.DESC_DTYPE)
        for s in range(ref.n):
            d[s] = (ref.base[s], ref.off[s], len(ref.recs[s]), ref.caps[s], ref.qps[s], int(ref.inits[s]) | FIN)
        d_desc = dev(d)
        hip.encode_sets_device(ref.n, d_desc.data_ptr(), ref.d_rec.data_ptr(), ref.d_bytes.data_ptr(), ref.d_res.data_ptr(), ref.n + 2,
                               ref.d_state.data_ptr(), ref.d_rate.data_ptr(), ref.d_idx.data_ptr(), ref.d_idx.data_ptr(),
                               ref.d_state.data_ptr(), ref.d_rate.data_ptr())
        hip.synchronize()
        return ref, host(ref.d_res, H.RESULT_DTYPE).copy()
    finally:
        hip.set_variant(7, 1)


def run_pieces(run, cuts, check=None):
    """All pieces of every substream, longest lists first in `run` (a Run or a Pair): launch i codes piece i of the substreams that
    have one.  -> [results after each launch].  check(i, results, n_sub) runs after launch i."""
    recs = run.a.recs if isinstance(run, Pair) else run.recs
    spans = [P.pieces_of(len(r), c) for r, c in zip(recs, cuts)]
    counts = [len(sp) for sp in spans]
    assert counts == sorted(counts, reverse=True), "substreams with more pieces come first"
    out = []
    for i in range(counts[0]):
        n_sub = sum(1 for c in counts if c > i)
        args = ([sp[i] for sp in spans[:n_sub]], [i == len(sp) - 1 for sp in spans[:n_sub]], n_sub)
        res = run.launch(*args) if isinstance(run, Pair) else run.launch(False, *args)
        if check:
            check(i, res, n_sub)
        out.append(res)
    return out


# ---------------------------------------------------------------------------------------------- 1. the setter
def test_the_setter_takes_4_7_and_0_and_the_decoder_does_not_follow_it():
    c = H.gpu_ctx()
    try:
        assert c.piece_encoder_get() == 4, "a fresh ctx"
        for v in (7, 0, 4, 7):
            c.piece_encoder_set(v)
            assert c.piece_encoder_get() == v
            for bad in (5, -1):
                with pytest.raises(capi.CabacHipError) as e:
                    c.piece_encoder_set(bad)
                assert e.value.status == -2 and c.piece_encoder_get() == v      # CABAC_HIP_ERR_INVALID, and the value stays
        c.set_variant(4, 4)
        assert c.piece_encoder_get() == 7, "cabac_hip_set_variant is another setting"
        # decode in pieces: the same under 4 and 7
        rng = np.random.default_rng(9800)
        recs = [H.random_records(rng, n - 1, ctx_frac=0.8, ctx_pool=POOL) for n in (150, 70, 33, 1, 90)]
        qps, inits = [30] * 5, [1] * 5
        ref = [M.encode_from(r, M.init_set(30, 1), 3) for r in recs]
        got = []
        for v in (4, 7):
            c.piece_encoder_set(v)
            run = Run(c, recs, qps, inits, caps=[len(x[1]) for x in ref], data=[x[1] for x in ref])
            for i, (spans, fin) in enumerate(zip(zip(*[P.pieces_of(len(r), [len(r) // 3, len(r) // 2]) for r in recs]), (False, False, True))):
                run.launch(True, list(spans), [fin] * 5)
                got.append((v, i, run.everything(encode=False) + [host(run.d_bins, np.uint8).copy()]))
            for s in range(5):
                assert np.array_equal(run.bins(s), recs[s] >> 15), (v, s)
        for (_, i, x), (_, k, y) in zip(got[:3], got[3:]):
            assert i == k and all(np.array_equal(p, q) for p, q in zip(x, y)), i
        c.piece_encoder_set(4)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------- 2. every cut of a short substream
@functools.lru_cache(None)
def short_case():
    rng = np.random.default_rng(9700)
    rec = H.random_records(rng, 69, ctx_frac=0.8, ctx_pool=POOL)     # 70 records, the last a terminate bin 1
    ctx = M.init_set(31, 1)
    rc, data, n_bits, left = M.encode_from(rec, ctx, 3)
    assert rc >= 0
    probe = [M.encode_from(rec[:k], ctx, 4)[2] for k in range(71)]
    return rec, ctx, data, n_bits, left, probe


def test_every_cut_of_a_short_substream(hip):
    rec, ctx, data, n_bits, left, probe = short_case()
    n = 71                                           # the cut at k = 0 .. 70; 71 substreams: four per workgroup, a partial last one
    run = Run(hip, [rec] * n, [31] * n, [1] * n)
    res = run.launch(False, [(0, k) for k in range(n)], [False] * n)
    st, b = run.states(), run.bytes()
    for k in range(n):
        assert tuple(res[k]) == (probe[k], 0), k
        assert st[k]["kind"] == capi.CODER_ENC and st[k]["flags"] == 0 and st[k]["bits"] == probe[k], k
        nf = int(st[k]["bytes_final"])
        assert nf % 2 == 0 and 8 * nf <= probe[k] and np.array_equal(run.slot(b, k, nf), data[:nf]), k
        assert (run.slot(b, k)[nf:] == SENT8).all(), k
        assert np.array_equal(run.set_of(k)[0], M.pack(M.advance_from(rec[:k], ctx))[0]), k
    res = run.launch(False, [(k, 70) for k in range(n)], [True] * n)
    st, b = run.states(), run.bytes()
    for k in range(n):
        assert tuple(res[k]) == (n_bits, 0), k
        assert np.array_equal(run.slot(b, k, len(data)), data) and (run.slot(b, k)[len(data):] == SENT8).all(), k
        assert st[k]["kind"] == capi.CODER_CLOSED and st[k]["bits"] == n_bits and st[k]["bytes_final"] == len(data), k
        assert same_ctx(run.set_of(k), M.pack(left)), k


# ---------------------------------------------------------------------------------------------- 3. many pieces
@functools.lru_cache(None)
def many_case():
    """(records, cuts) per substream, most pieces first.  Lengths 48, 300 and 1 999 in pieces of 1 (the 48 only), 7, 16, 17, 64 and
    65; some with empty pieces in the middle and as the last piece; the rest (0, 1, 65, 300, 48 records) fresh and final in one
    piece.  All of them in one launch while they last: the short ones run the surplus steps of the long ones between their own."""
    rng = np.random.default_rng(9710)
    mk = lambda n: H.random_records(rng, n - 1, ctx_frac=float(rng.choice([0.5, 0.8, 0.95])), ctx_pool=POOL) if n else np.zeros(0, np.uint16)
    plan = [(48, 1, ""), (300, 7, ""), (300, 7, "empty-mid"), (1999, 64, ""), (1999, 65, "empty-last"), (300, 16, ""), (300, 17, "empty-mid"),
            (48, 7, "empty-last"), (300, 64, ""), (300, 65, "empty-last"), (48, 16, "empty-mid"), (48, 17, "")]
    cases = []
    for n, size, kind in plan:
        cuts = P.equal_cuts(n, size)
        if kind == "empty-mid":
            cuts = sorted(cuts + [cuts[len(cuts) // 2]] * 2)
        if kind == "empty-last":
            cuts = cuts + [n]
        cases.append((mk(n), cuts))
    cases += [(mk(n), []) for n in (0, 1, 65, 300, 48)]
    cases.sort(key=lambda c: -len(c[1]))
    qps = [int(rng.integers(0, 64)) for _ in cases]
    inits = [int(rng.integers(0, 3)) for _ in cases]
    ctxs = [M.init_set(q, i) for q, i in zip(qps, inits)]
    ref = [M.encode_from(c[0], x, 3) for c, x in zip(cases, ctxs)]
    assert all(x[0] >= 0 for x in ref)
    spans = [P.pieces_of(len(c[0]), c[1]) for c in cases]
    probes = [[M.encode_from(c[0][:end], x, 4)[2] for _, end in sp[:-1]] for c, x, sp in zip(cases, ctxs, spans)]
    return cases, qps, inits, ref, spans, probes


def _many_pieces(hip, setting):
    cases, qps, inits, ref, spans, probes = many_case()
    recs, cuts = [c[0] for c in cases], [c[1] for c in cases]
    pair = Pair(hip, recs, qps, inits, setting=setting)
    run = pair.a

    def check(i, res, n_sub):
        st = run.states()
        for s in range(n_sub):
            if i == len(spans[s]) - 1:
                assert tuple(res[s]) == (ref[s][2], 0) and st[s]["kind"] == capi.CODER_CLOSED, (s, i)
            else:
                want = probes[s][i]
                assert tuple(res[s]) == (want, 0) and st[s]["bits"] == want and st[s]["kind"] == capi.CODER_ENC, (s, i)
    run_pieces(pair, cuts, check)
    assert pair.launches == len(spans[0]) >= 48
    b = run.bytes()
    for s in range(run.n):
        nb = len(ref[s][1])
        assert np.array_equal(run.slot(b, s, nb), ref[s][1]) and (run.slot(b, s)[nb:] == SENT8).all(), s
        assert same_ctx(run.set_of(s), M.pack(ref[s][3])), s


def test_many_pieces_of_unequal_lengths_in_one_workgroup(hip):
    _many_pieces(hip, 7)


# ---------------------------------------------------------------------------------------------- 4. emission across a cut
@functools.lru_cache(None)
def emission_cases():
    """Context-free families cut so that runs of 0xFFFF units cross the boundaries; every substream in four pieces (repeated cuts:
    empty pieces).  Directed: the cut directly in front of the finish that resolves a run, with and without a carry."""
    rng = np.random.default_rng(9720)
    fams = [(name, rec) for name, rec, n_head in E.all_families() if n_head == len(rec)]
    cases = []
    for name, rec in fams[::4]:
        cuts = sorted(int(x) for x in rng.integers(0, len(rec) + 1, size=3))
        cases.append((rec, cuts))
    for name, rec in fams:
        if name.startswith(("long-sibling/K8", "long-sibling/K40", "ends/0", "ends/3", "trm1/16/0", "trm1/64/2")):
            cases.append((rec, [len(rec) // 3, 2 * len(rec) // 3, len(rec)]))       # the last piece only finishes
            cases.append((rec, [len(rec) // 2, len(rec), len(rec)]))
    return cases


def test_emission_across_a_cut(hip):
    cases = emission_cases()
    cen = P.cross_census(cases)
    for ev in P.CROSS_EVENTS + ("run3",):
        assert len(cen.get(ev, ())) >= 1, (ev, {k: len(v) for k, v in cen.items()})
    recs, cuts = [c[0] for c in cases], [c[1] for c in cases]
    want = [E.finished_bytes(E.code(r)) for r in recs]
    caps = [len(w[0]) + 1 + 2 * (s % 2) for s, w in enumerate(want)]         # roomy odd capacities
    run = Run(hip, recs, [30] * len(recs), [1] * len(recs), caps=caps)
    replay = [P.PieceReplay() for _ in recs]
    spans = [P.pieces_of(len(r), c) for r, c in zip(recs, cuts)]

    def check(i, res, n_sub):
        st, b = run.states(), run.bytes()
        for s in range(n_sub):
            first, end = spans[s][i]
            replay[s].feed(recs[s][first:end])
            if i < 3:
                w = replay[s].state()
                assert tuple(res[s]) == (w["bits"], 0), (s, i)
                assert (st[s]["kind"], st[s]["flags"], st[s]["bits"], st[s]["bytes_final"]) == (capi.CODER_ENC, 0, w["bits"], replay[s].pos), (s, i)
                assert tuple(int(x) for x in st[s]["priv"]) == w["priv"], (s, i)
                assert np.array_equal(run.slot(b, s, replay[s].pos), want[s][0][:replay[s].pos]), (s, i)
            else:
                assert tuple(res[s]) == (want[s][1], 0), (s, i)
                assert np.array_equal(run.slot(b, s, len(want[s][0])), want[s][0]), (s, i)
    run_pieces(run, cuts, check)


# ---------------------------------------------------------------------------------------------- 5. more than four units in a step
@functools.lru_cache(None)
def burst_case():
    """Sixteen distinct contexts driven to the end of their range by 1 000 zeros each (a reachable state), then sixteen ones on
    them — sixteen LPS bins of about seven bits — as ONE step of a piece: (a) the last step before a cut, (b) the first step
    behind one.  The rest of the records stays off those contexts.  -> (records, cut, start contexts) per substream"""
    rng = np.random.default_rng(9790)
    hot, calm = POOL[:16], POOL[16:]
    out = []
    for k, (qp, init) in enumerate(((30, 1), (22, 0), (41, 2))):
        ctx = M.advance_from(np.repeat(hot, 1000).astype(np.uint16), M.init_set(qp, init))
        burst = (hot | H.REC_BIN).astype(np.uint16)
        head = H.random_records(rng, 32, ctx_frac=0.8, ctx_pool=calm, end_trm=False, trm0_frac=0.0)
        tail = H.random_records(rng, 40 + k, ctx_frac=0.8, ctx_pool=calm)
        assert len(head) == 32
        rec = np.concatenate([head, burst, tail]).astype(np.uint16)
        grow = M.encode_from(rec[:48], ctx, 4)[2] - M.encode_from(rec[:32], ctx, 4)[2]
        assert grow >= 80, grow                              # the step writes five whole units or more: past the four lanes
        out.append((rec, 48, ctx, qp, init))                 # (a): steps 0, 1, burst | cut
        out.append((rec, 32, ctx, qp, init))                 # (b): cut | burst as step 0 of the second piece
    return out


def test_a_step_of_more_than_four_units_at_a_cut(hip):
    cases = burst_case()
    recs, cut, ctxs = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    pair = Pair(hip, recs, [c[3] for c in cases], [c[4] for c in cases], ctxs=ctxs)
    run = pair.a
    ref = [M.encode_from(r, x, 3) for r, x in zip(recs, ctxs)]
    res = pair.launch([(0, k) for k in cut], [False] * run.n)
    st, b = run.states(), run.bytes()
    for s in range(run.n):
        want = M.encode_from(recs[s][:cut[s]], ctxs[s], 4)[2]
        assert tuple(res[s]) == (want, 0) and (st[s]["kind"], st[s]["flags"], st[s]["bits"]) == (capi.CODER_ENC, 0, want), s
        nf = int(st[s]["bytes_final"])
        assert nf % 2 == 0 and np.array_equal(run.slot(b, s, nf), ref[s][1][:nf]) and (run.slot(b, s)[nf:] == SENT8).all(), s
        assert want - 8 * nf < 16 * int(st[s]["priv"][3]) + 16, s
        assert same_ctx(run.set_of(s), M.pack(M.advance_from(recs[s][:cut[s]], ctxs[s]))), s
    res = pair.launch([(k, len(r)) for k, r in zip(cut, recs)], [True] * run.n)
    st, b = run.states(), run.bytes()
    for s in range(run.n):
        nb = len(ref[s][1])
        assert tuple(res[s]) == (ref[s][2], 0) and st[s]["kind"] == capi.CODER_CLOSED and st[s]["bytes_final"] == nb, s
        assert np.array_equal(run.slot(b, s, nb), ref[s][1]) and (run.slot(b, s)[nb:] == SENT8).all(), s
        assert same_ctx(run.set_of(s), M.pack(ref[s][3])), s


# ---------------------------------------------------------------------------------------------- 6. capacity
def test_capacity_flags_the_same_substreams_and_stays_inside_the_slot(hip):
    recs, caps, coded = [], [], []
    for name, rec in E.capacity_cases():
        data, _ = E.roomy(rec, 30, 1)
        n = len(data)
        for cap in (0, 1, 2, n // 2, n - 2, n - 1, n, n + 2):
            recs.append(rec)
            caps.append(cap)
            coded.append(data)
    run = Run(hip, recs, [30] * len(recs), [1] * len(recs), caps=caps)
    cuts = [[len(r) // 2, len(r)] for r in recs]            # two pieces that do not finish, then a third that only finishes
    out = run_pieces(run, cuts, lambda i, res, n_sub: run.everything())   # (nothing outside the slots, states, sets: after every launch)
    b, st = run.bytes(), run.states()
    for s in range(run.n):
        over = len(coded[s]) > caps[s]
        flagged = [bool(o[s]["flags"] & H.RES_OVERFLOW) for o in out]
        assert flagged[2] == over, (s, caps[s], flagged)
        assert flagged == sorted(flagged), (s, flagged)                    # once raised it stays
        assert int(out[2][s]["flags"]) in (0, H.RES_OVERFLOW), s
        if flagged[1]:                                                      # raised before the last piece: it codes nothing
            assert tuple(out[2][s]) == (0, H.RES_OVERFLOW) and st[s]["flags"] == H.RES_OVERFLOW and st[s]["kind"] == capi.CODER_ENC, s
        if not over:
            assert out[2][s]["n_bits"] == 8 * len(coded[s]) and np.array_equal(run.slot(b, s, len(coded[s])), coded[s]), s
    # the same substreams are flagged, piece by piece, as under setting 4 (the bytes of a flagged one are unspecified)
    hip.piece_encoder_set(4)
    run4 = Run(hip, recs, [30] * len(recs), [1] * len(recs), caps=caps)
    out4 = run_pieces(run4, cuts)
    for o, o4 in zip(out, out4):
        assert np.array_equal(o, o4)
    assert run4.states().tobytes() == st.tobytes()


# ---------------------------------------------------------------------------------------------- 7. refused and flagged states
def _spoil(st, what, cap):
    """One refused condition of cabac_hip_pieces.h on a valid encoder state behind a piece, as its eight words: kind, flags, bits,
    bytes_final, low, range | pend << 16, buffered unit, nbuf"""
    w = np.frombuffer(st.tobytes(), np.uint32).astype(np.int64)
    pend = int(w[5]) >> 16
    if what == "kind-unknown":
        w[0] = 7
    elif what == "kind-other":
        w[0] = capi.CODER_DEC
    elif what == "kind-closed":
        w[0] = capi.CODER_CLOSED
    elif what == "enc-range-low":
        w[5] = (pend << 16) | 255
    elif what == "enc-range-high":
        w[5] = (pend << 16) | 511
    elif what == "enc-pend":
        w[5] = (int(w[5]) & 0xFFFF) | (16 << 16)
        w[2] += 16 - pend
    elif what == "enc-low":
        w[4] = 1 << (10 + pend)
    elif what == "enc-bits":
        w[2] += 1
    elif what == "enc-odd":
        w[3] += 1
        w[2] += 8
    elif what == "enc-capacity":
        more = (cap - int(w[3])) // 2 + 1 - int(w[7])
        w[7] += more
        w[2] += 16 * more
    else:
        raise ValueError(what)
    return np.frombuffer(w.astype(np.uint32).tobytes(), ST)[0]


ENC_REFUSED = ("kind-unknown", "kind-other", "kind-closed", "enc-range-low", "enc-range-high", "enc-pend", "enc-low", "enc-bits", "enc-odd",
               "enc-capacity")


def test_refused_and_flagged_states_beside_valid_neighbours(hip):
    """One substream per condition the pieces header lists as refused, all in one launch, every other substream a valid neighbour:
    refused and valid substreams alternate over the lanes of the chain wave.  The last substream comes with a sticky flag.
    These are states the header defines; no arbitrary garbage is fed."""
    n = 2 * len(ENC_REFUSED) + 2
    sticky = n - 1
    rng = np.random.default_rng(9770)
    rec = H.random_records(rng, 119, ctx_frac=0.8, ctx_pool=POOL)
    ctx = M.init_set(32, 0)
    rc, data, n_bits, left = M.encode_from(rec, ctx, 3)
    run = Run(hip, [rec] * n, [32] * n, [0] * n, caps=[len(data) + 5] * n)
    run.launch(False, [(0, 50)] * n, [False] * n)
    st = run.states()
    bad = {2 * k + 1: c for k, c in enumerate(ENC_REFUSED)}
    for s, c in bad.items():
        st[s] = _spoil(st[s], c, int(run.caps[s]))
    st[sticky]["flags"] = H.RES_OVERFLOW
    given = np.concatenate([np.full(8, SENT32, np.uint32), st.view(np.uint32), np.full(8, SENT32, np.uint32)])
    run.d_coder = dev(given)
    bytes_before, sets_before = host(run.d_bytes, np.uint8).copy(), host(run.d_state, np.uint32).copy()
    res = run.launch(False, [(50, 120)] * n, [True] * n)
    after, b = run.states(), run.bytes()
    for s in range(n):
        a = (s + 1) * H.NUM_CTX
        if s in bad or s == sticky:
            assert tuple(res[s]) == ((0, capi.RES_BAD_STATE) if s in bad else (0, H.RES_OVERFLOW)), (s, bad.get(s), res[s])
            assert after[s].tobytes() == st[s].tobytes(), (s, bad.get(s))                    # not written / copied
            assert np.array_equal(run.slot(b, s), run.slot(bytes_before, s)), (s, bad.get(s))  # no byte
            assert np.array_equal(host(run.d_state, np.uint32)[a:a + H.NUM_CTX], sets_before[a:a + H.NUM_CTX]), (s, bad.get(s))
        else:
            assert tuple(res[s]) == (n_bits, 0) and np.array_equal(run.slot(b, s, len(data)), data), s
            assert after[s]["kind"] == capi.CODER_CLOSED and same_ctx(run.set_of(s), M.pack(left)), s


# ---------------------------------------------------------------------------------------------- 8. several workgroups
@pytest.mark.parametrize("n", [1030, 5], ids=["sixteen-per-workgroup", "four-per-workgroup"])
def test_a_batch_of_several_workgroups_against_the_one_call_forms(hip, n):
    """1 030 substreams: sixteen per workgroup, the last workgroup with 6; 5 substreams: four per workgroup, 4 + 1"""
    rng = np.random.default_rng(9780)
    pool = [H.random_records(rng, int(rng.integers(150, 250)), ctx_frac=0.8, ctx_pool=POOL) for _ in range(40)]
    recs = [pool[int(k)] for k in rng.integers(0, len(pool), n)]
    qps, inits = rng.integers(20, 45, n), rng.integers(0, 3, n)
    cuts = [[int(len(r) * 0.3), int(len(r) * 0.3) + 64] for r in recs]
    pair = Pair(hip, recs, qps, inits)
    run_pieces(pair, cuts)
    run = pair.a
    assert all(w["kind"] == capi.CODER_CLOSED for w in run.states())
    for variant in (7, 4):
        ref, ref_res = one_call(hip, run, variant)
        assert not ref_res["flags"].any()
        assert np.array_equal(host(run.d_res, H.RESULT_DTYPE), ref_res), variant
        assert np.array_equal(run.bytes(), ref.bytes()), variant
        assert np.array_equal(host(run.d_state, np.uint32), host(ref.d_state, np.uint32)), variant
        assert np.array_equal(host(run.d_rate, np.uint8), host(ref.d_rate, np.uint8)), variant


# ---------------------------------------------------------------------------------------------- 9. interchange
def test_a_state_continues_under_the_other_setting_and_after_a_copy_through_the_host(hip):
    rng = np.random.default_rng(9760)
    recs = [H.random_records(rng, n - 1, ctx_frac=0.8, ctx_pool=POOL) for n in (300, 129, 65, 48, 207)]
    cuts = [[len(r) // 4, len(r) // 2, 3 * len(r) // 4] for r in recs]
    qps, inits = [27, 30, 33, 36, 39], [0, 1, 2, 0, 1]
    ctxs = [M.init_set(q, i) for q, i in zip(qps, inits)]
    ref = [M.encode_from(r, c, 3) for r, c in zip(recs, ctxs)]
    run = Run(hip, recs, qps, inits)
    spans = [P.pieces_of(len(r), c) for r, c in zip(recs, cuts)]
    for i, setting in enumerate((7, 4, 7, 4)):
        hip.piece_encoder_set(setting)
        assert hip.piece_encoder_get() == setting
        res = run.launch(False, [sp[i] for sp in spans], [i == 3] * run.n)
        if i < 3:
            for s in range(run.n):
                assert tuple(res[s]) == (M.encode_from(recs[s][:spans[s][i][1]], ctxs[s], 4)[2], 0), (i, s)
        saved = host(run.d_coder, np.uint32).copy()          # to the host ...
        run.d_coder = dev(saved)                             # ... and back, into other memory
    b = run.bytes()
    for s in range(run.n):
        assert tuple(res[s]) == (ref[s][2], 0) and np.array_equal(run.slot(b, s, len(ref[s][1])), ref[s][1]), s
        assert same_ctx(run.set_of(s), M.pack(ref[s][3])), s


# ---------------------------------------------------------------------------------------------- 10. setting 0
def test_setting_0_gives_the_same(hip):
    _many_pieces(hip, 0)


# ---------------------------------------------------------------------------------------------- 11. the plan write continued
def test_the_plan_write_continued_follows_the_setting(hip):
    """The five-unit batch of tests/test_gpu_plan_continue.py (more pieces first, pieces of nothing, final and open pieces in one
    launch), built from plan_continue_model: under setting 7 and under setting 4 on the same inputs"""
    import plan_resume_model as R
    from test_gpu_plan_continue import Run as PlanRun, batch_case, check_against_model
    cases, exp = batch_case()
    units, cuts = [c[0] for c in cases], [c[1] for c in cases]
    run7, run4 = PlanRun(hip, units), PlanRun(hip, units)
    check = check_against_model(run7, units, cuts, exp)
    spans = [R.spans_of(u, c) for u, c in zip(units, cuts)]
    assert len(spans[0]) >= 3
    for i in range(len(spans[0])):
        n_sub = sum(1 for sp in spans if len(sp) > i)
        args = ([sp[i] for sp in spans[:n_sub]], [i == len(sp) - 1 for sp in spans[:n_sub]], n_sub)
        hip.piece_encoder_set(4)
        res4 = run4.launch(*args)
        hip.piece_encoder_set(7)
        res7 = run7.launch(*args)
        check(i, res7, n_sub)
        assert np.array_equal(res7, res4), i
        assert run7.states().tobytes() == run4.states().tobytes(), i
        assert np.array_equal(run7.bytes(), run4.bytes()), i
        assert np.array_equal(run7.values(), run4.values()) and np.array_equal(run7.info, run4.info), i
        assert np.array_equal(run7.last_info, run4.last_info), i
        for x, y in zip(run7.sets(), run4.sets()):
            assert np.array_equal(x, y), i
    assert all(w["kind"] == capi.CODER_CLOSED for w in run7.states())
