"""GPU: the plan parse in pieces (include/cabac_hip_plan_resume.h; the pieces instantiation of the plan walk in
csrc/cabac_residual_parse.hip) against tests/plan_resume_model.py, against the one-call cabac_hip_plan_parse_sets_device on the
device (R1, R2) and against cabac_hip_decode_pieces_device (R3).  Everything is bit-exact: == on integers.  Values, coefficients
and results sit between guard words, the states between two sentinel states, the sets between two sentinel sets; all of them are
looked at after every launch.  States and sets are in place: every launch reads and writes the same arrays.

Every test calls cabac_hip_plan_resume_parse_device, so none passes without it."""
import functools

import numpy as np
import pytest
import torch

import ctx_sets_model as CS
import helpers as H
import parse_elements_model as E
import parse_plan_model as PM
import plan_resume_model as R
from entropy_coding_amd import capi
from test_gpu_parse_elements import VAL_GUARD, WORD_GUARD_U, Out
from test_gpu_parse_plan import _flip_middle
from test_gpu_parse_unit import G, WORD_GUARD, coded, sentinel
from test_gpu_pieces import Run as BinRun
from test_parse_plan_model import TU_OUTCOMES
from test_plan_resume_model import mixed

pytestmark = pytest.mark.gpu

SENT32, SENT8 = 0x5A5A5A5A, 0xA5
ST = capi.CODER_STATE_DTYPE
STICKY = H.RES_BAD_RECORD | E.RES_BAD_VALUE | H.RES_UNDERRUN | CS.RES_BAD_SET
NCTX = H.NUM_CTX


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def opt(t):
    return t.data_ptr() if t is not None else 0


class Run:
    """The substreams of `units` parsed in pieces.  The bytes, the plan and the block descriptors of the whole units lie on the
    device once (parse_plan_model.pack); every launch gets descriptors, block lists and positions of its pieces.  One state per
    substream in ONE array (in and out the same) and one set per substream, started from and written back in place."""

    def __init__(self, hip, units, int16=False, capacities=None):
        self.hip, self.units, self.n, self.int16 = hip, units, len(units), int16
        self.P = P = PM.pack(units, capacities)
        self.out = Out(P, int16)
        self.d_bytes, self.d_plan = dev(P["bytes"]), dev(np.concatenate([P["plan"].reshape(-1), np.zeros(4, np.uint32)]))
        self.pos = [R.positions(u) for u in units]
        self.info = np.full(P["n_tu"], WORD_GUARD_U, np.uint32)
        state = np.full((self.n + 2) * NCTX, SENT32, np.uint32)
        rate = np.full((self.n + 2) * NCTX, SENT8, np.uint8)
        for s, u in enumerate(units):
            state[(s + 1) * NCTX:(s + 2) * NCTX], rate[(s + 1) * NCTX:(s + 2) * NCTX] = CS.pack(CS.init_set(u["qp"], R.INIT_ID))
        self.d_state, self.d_rate = dev(state), dev(rate)
        self.d_idx = dev(np.arange(1, self.n + 1, dtype=np.uint32))
        self.d_coder = dev(np.concatenate([np.full(8, SENT32, np.uint32), np.zeros(8 * self.n, np.uint32), np.full(8, SENT32, np.uint32)]))

    def _call(self, entry, desc, tile_first, tus, at, guard, d_info, coder=True):
        n_sub = len(desc)
        p_co, p_val, _, p_res = self.out.ptrs()
        t_desc, t_first = dev(desc), dev(np.asarray(tile_first, np.uint32))
        t_tu = dev(tus) if len(tus) else None
        t_at = dev(np.asarray(at, np.uint32)) if len(tus) else None
        t_guard = dev(np.asarray(guard, np.uint32)) if len(tus) else None
        args = (n_sub, t_desc.data_ptr(), self.d_bytes.data_ptr(), t_first.data_ptr(), opt(t_tu), opt(t_at), opt(t_guard),
                self.d_plan.data_ptr(), p_co if self.P["n_tu"] else 0, p_val, p_res)
        kw = dict(d_tu_info=d_info, int16=self.int16, n_sets=self.n + 2, d_state=self.d_state.data_ptr(), d_rate=self.d_rate.data_ptr(),
                  d_start_set=self.d_idx.data_ptr(), d_out_set=self.d_idx.data_ptr(), d_out_state=self.d_state.data_ptr(),
                  d_out_rate=self.d_rate.data_ptr())
        if entry == "sets":
            self.hip.plan_parse_sets_device(*args, **kw)
        else:
            p = self.d_coder.data_ptr() + 32 if coder else 0
            self.hip.plan_resume_parse_device(*args, **kw, d_coder_in=p, d_coder_out=p)
        self.hip.synchronize()
        return host(self.out.res, np.uint32)[G:G + 2 * n_sub].view(H.RESULT_DTYPE).copy()

    def launch(self, spans, last, n_sub=None):
        """One piece of the first n_sub substreams: spans[s] = (e0, b0, e1, b1), last[s]: the final piece -> results"""
        n_sub = self.n if n_sub is None else n_sub
        P = self.P
        desc = P["desc"][:n_sub].copy()
        tus, at, guard, first, where = [], [], [], [0], []
        for s in range(n_sub):
            e0, b0, e1, b1 = spans[s]
            t0 = int(P["tile_first"][s])
            desc["rec_offset"][s] = int(P["desc"]["rec_offset"][s]) + e0
            desc["n_records"][s] = e1 - e0
            desc["init_id"][s] = R.INIT_ID | (H.SUB_FINISH if last[s] else 0)
            tus.append(P["tus"][t0 + b0:t0 + b1])
            at += [p - e0 for p in self.pos[s][b0:b1]]
            g = self.units[s]["guards"]
            guard += [0] * (b1 - b0) if g is None else [int(x) for x in g[b0:b1]]
            where += list(range(t0 + b0, t0 + b1))
            first.append(first[-1] + b1 - b0)
        tus = np.concatenate(tus + [np.zeros(0, H.TU_DTYPE)])
        d_info = torch.full((len(tus) + 2 * G,), WORD_GUARD, dtype=torch.int32, device="cuda")
        res = self._call("resume", desc, first, tus, at, guard, d_info.data_ptr() + 4 * G)
        info = d_info.cpu().numpy().view(np.uint32)
        assert (info[:G] == WORD_GUARD_U).all() and (info[G + len(tus):] == WORD_GUARD_U).all(), "an info word outside the launch's blocks"
        self.info[np.asarray(where, np.int64)] = info[G:G + len(tus)]
        return res

    def whole(self, entry, coder=True):
        """ONE call over the whole substreams, every descriptor final: cabac_hip_plan_parse_sets_device ("sets"), or the new call
        from fresh states ("resume")"""
        P = self.P
        guard = [0] * P["n_tu"] if P["tu_guard"] is None else P["tu_guard"]
        d_info = torch.full((P["n_tu"] + 2 * G,), WORD_GUARD, dtype=torch.int32, device="cuda")
        res = self._call(entry, P["desc"], P["tile_first"], P["tus"][:P["n_tu"]], [p for ps in self.pos for p in ps], guard,
                         d_info.data_ptr() + 4 * G, coder)
        info = d_info.cpu().numpy().view(np.uint32)
        assert (info[:G] == WORD_GUARD_U).all() and (info[G + P["n_tu"]:] == WORD_GUARD_U).all()
        self.info[:] = info[G:G + P["n_tu"]]
        return res

    def pieces(self, cuts, check=None):
        """All pieces of every substream, the substreams with more pieces first: launch i parses piece i of those that have one"""
        spans = [R.spans_of(u, c) for u, c in zip(self.units, cuts)]
        counts = [len(sp) for sp in spans]
        assert counts == sorted(counts, reverse=True), "substreams with more pieces come first"
        out = []
        for i in range(counts[0]):
            n_sub = sum(1 for c in counts if c > i)
            res = self.launch([sp[i] for sp in spans[:n_sub]], [i == len(sp) - 1 for sp in spans[:n_sub]], n_sub)
            self.states(), self.sets()
            if check:
                check(i, res, n_sub)
            out.append(res)
        return out

    # ---- what lies on the device now
    def states(self):
        raw = host(self.d_coder, np.uint32)
        assert (raw[:8] == SENT32).all() and (raw[-8:] == SENT32).all(), "the states around the array"
        return raw[8:-8].view(ST).copy()

    def put_states(self, st):
        self.d_coder[32:32 + 32 * self.n] = torch.from_numpy(np.ascontiguousarray(st).view(np.uint8).reshape(-1).copy()).cuda()

    def sets(self):
        st, rt = host(self.d_state, np.uint32), host(self.d_rate, np.uint8)
        assert (st[:NCTX] == SENT32).all() and (st[-NCTX:] == SENT32).all(), "the sets around the array"
        assert (rt[:NCTX] == SENT8).all() and (rt[-NCTX:] == SENT8).all()
        return st[NCTX:-NCTX].reshape(self.n, NCTX).copy(), rt[NCTX:-NCTX].reshape(self.n, NCTX).copy()

    def read(self):
        """-> dict(co, val, info: the whole arrays; values, blocks, infos: per substream), the guards checked"""
        co, val, _, _ = self.out.read()
        P = self.P
        values, blocks, infos, t = [], [], [], 0
        for s, u in enumerate(self.units):
            r0 = int(P["desc"]["rec_offset"][s])
            values.append(val[r0:r0 + len(u["plan"])])
            bl = []
            for m in u["metas"]:
                bl.append(co[int(P["offsets"][t]):int(P["offsets"][t]) + m[0] * m[1]].reshape(m[1], m[0]))
                t += 1
            blocks.append(bl)
            infos.append(self.info[t - len(bl):t].copy())
        return dict(co=co, val=val, info=self.info.copy(), values=values, blocks=blocks, infos=infos)


def assert_set(sets, s, ctx, what=""):
    state, rate = CS.pack(ctx)
    assert np.array_equal(sets[0][s], state) and np.array_equal(sets[1][s], rate), what


def assert_unit(r, s, u, e1=None, b1=None, what=""):
    """Substream s holds the unit's values, info words and coded blocks in front of the cut (e1, b1), and nothing behind it"""
    e1 = len(u["plan"]) if e1 is None else e1
    b1 = len(u["metas"]) if b1 is None else b1
    assert r["values"][s][:e1].tolist() == [v & 0xFFFFFFFF for v in u["values"][:e1]], (what, s)
    assert (r["values"][s][e1:] == VAL_GUARD).all(), (what, s)
    assert r["infos"][s][:b1].tolist() == u["infos"][:b1] and (r["infos"][s][b1:] == WORD_GUARD_U).all(), (what, s)
    for k, on in enumerate(u["coded"]):
        if on and k < b1:
            assert np.array_equal(coded(r["blocks"][s][k]), coded(u["blocks"][k])), (what, s, k)
        else:
            assert (r["blocks"][s][k] == np.int32(np.int16(sentinel(True)) if r["int16"] else sentinel(False))).all(), (what, s, k)


def assert_open(st, s, S, what=""):
    """A decoder between two pieces with S bits shifted, flagless and inside the format"""
    w = st[s]
    assert (w["kind"], w["flags"], w["bits"], w["bytes_final"]) == (capi.CODER_DEC, 0, S, 0), (what, s)
    rng, value, mark, zero = (int(x) for x in w["priv"])
    assert 256 <= rng <= 510 and value < rng << 7 and mark == 0 and zero == 0, (what, s)


def assert_closed(st, s, flags=0, what=""):
    w = st[s]
    assert (w["kind"], w["flags"], w["bytes_final"]) == (capi.CODER_CLOSED, flags, 0) and not w["priv"].any(), (what, s)


def same_outputs(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("co", "val", "info"))


def read(run):
    return dict(run.read(), int16=run.int16)


# ---------------------------------------------------------------------------------------------- 1. every bit phase
@functools.lru_cache(maxsize=None)
def phase_case():
    """A block-free substream of single-bin and multi-bin elements, unguarded: every entry boundary is a cut.  -> (unit, cuts, S
    at every cut, what the model expects of the two pieces for every cut)"""
    rng = np.random.default_rng(0x51A0)
    u, _ = R.join(rng, [R.flat_segment(rng, 44, kinds=[E.CTX_BIN, E.CTX_BIN, E.EP_BINS, E.UNARY_MAX, E.REM_ABS, E.TRUNC_BIN, E.EXP_GOLOMB])], qp=27)
    cuts = R.entry_cuts(u)[:-1]                                     # in front of entry 0 .. in front of the terminate bin
    S = [R.shifts_at(u, e, b) for e, b in cuts]
    assert {s % 16 for s in S} == set(range(16)), "S mod 16 takes all 16 values"
    exp = [R.expect(u, [c]) for c in cuts]
    return u, cuts, S, exp


def _phase_run(hip, int16, which):
    u, cuts, S, exp = phase_case()
    run = Run(hip, [u] * len(which), int16)
    mine = [cuts[k] for k in which]

    def check(i, res, n_sub):
        st, sets, r = run.states(), run.sets(), read(run)
        for s, k in enumerate(which):
            n_bits, flags, left = exp[k][i]
            assert tuple(res[s]) == (n_bits, flags), (i, k)
            assert_set(sets, s, left, (i, k))
            if i == 0:
                assert n_bits == S[k] + 8
                assert_open(st, s, S[k], k)
                assert_unit(r, s, u, *cuts[k], what=k)
            else:
                assert_closed(st, s, what=k)
                assert_unit(r, s, u, what=k)
    run.pieces([[c] for c in mine], check)


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_a_cut_at_every_entry_boundary_takes_every_bit_phase(hip, int16):
    _phase_run(hip, int16, list(range(len(phase_case()[1]))))


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
@pytest.mark.parametrize("n_sub", [1, 5, 1027])
def test_one_wave_four_waves_and_a_partial_last_workgroup(hip, n_sub, int16):
    n = len(phase_case()[1])
    _phase_run(hip, int16, [(7 * s + 3) % n for s in range(n_sub)])


# ---------------------------------------------------------------------------------------------- 2. block edges of the input ring
EDGES = (252, 254, 256, 258, 508, 510, 512, 514)


@functools.lru_cache(maxsize=None)
def edge_case():
    """Substreams of about 600 bytes of EP_BINS 32 entries, with 32, 16, 24 and 8 bins in front, so that the byte offset of stream
    bit S + 16 takes every value; -> [(unit, cut, that byte offset)] for the EDGES and for the last unit of the slot"""
    rng = np.random.default_rng(0x51A1)
    out, slot_end = [], 0
    for lead in (32, 16, 24, 8):                                     # (the last two for the end of the slot alone: odd byte offsets)
        plan = np.zeros((150, 2), np.uint32)
        plan[:, 0] = [capi.element(E.EP_BINS, n=lead)] + [capi.element(E.EP_BINS, n=32)] * 149
        values = [int(rng.integers(0, 1 << lead))] + [int(x) for x in rng.integers(0, 1 << 32, 149)]
        u, _ = R.join(rng, [("plan", plan, values)], qp=33)
        assert 590 <= len(u["data"]) <= 620
        for e, b in R.entry_cuts(u)[1:-1]:
            S = R.shifts_at(u, e, b)
            assert S == lead + 32 * (e - 1)                         # bypass bins: one shift each
            at = (S + 16) >> 3
            if at in EDGES and lead >= 16 and lead != 24:
                out.append((u, (e, b), at))
            elif at // 2 == (len(u["data"]) - 1) // 2:              # the 16-bit unit that holds the last byte of the slot
                out.append((u, (e, b), at))
                slot_end += 1
    assert sorted(a for _, _, a in out if a in EDGES) == sorted(EDGES) and slot_end >= 1
    return out


def test_cuts_at_the_block_edges_of_the_input_ring(hip):
    cases = edge_case()
    units = [c[0] for c in cases]
    ref = Run(hip, units)
    want_res = ref.whole("sets")
    want, want_sets = read(ref), ref.sets()
    run = Run(hip, units)
    res = run.pieces([[c[1]] for c in cases])
    st, got = run.states(), read(run)
    for s, (u, (e, b), at) in enumerate(cases):
        assert tuple(res[0][s]) == (8 * at - 16 + 8, 0), at
        assert tuple(res[1][s]) == tuple(want_res[s]) == PM.want_walk(u), at
        assert_closed(st, s, what=at)
        assert_unit(got, s, u, what=at)
    assert same_outputs(got, want)                                  # R1
    assert np.array_equal(run.sets()[0], want_sets[0]) and np.array_equal(run.sets()[1], want_sets[1])


# ---------------------------------------------------------------------------------------------- 3. pieces around blocks
@functools.lru_cache(maxsize=None)
def block_cases():
    """[(unit, cuts)], more pieces first: the mixed unit of the model's test cut between all its segments (a piece of one block and
    no entry, pieces of one entry, a transform-skip and a zero-out block among them), the same with pieces of nothing, and
    transform units in a row cut between the units"""
    rng = np.random.default_rng(0x51A2)
    u, cuts = mixed()
    tu = PM.tu_unit(rng, [PM.tu_case(rng, *TU_OUTCOMES[k]) for k in (7, 40, 21)], qp=24)
    tu_cuts = [(PM.TU_LEN * k, 3 * k) for k in (1, 2, 3)]
    assert R.references_stay_inside(tu, tu_cuts)
    cases = [(u, [cuts[0], cuts[0]] + cuts[1:] + [cuts[-1]]), (u, cuts), (tu, [(0, 0)] + tu_cuts)]
    metas = [m for m in u["metas"]]
    assert any(m[3] & H.TU_TRANSFORM_SKIP for m in metas) and any(m[3] & H.TU_SBT_ZERO_OUT for m in metas)
    return cases, [R.expect(c[0], c[1]) for c in cases]


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_pieces_around_blocks_of_one_block_of_one_entry_and_of_nothing(hip, int16):
    cases, exp = block_cases()
    units = [c[0] for c in cases]
    ref = Run(hip, units, int16)
    want_res = ref.whole("sets")
    want, want_sets = read(ref), ref.sets()
    run = Run(hip, units, int16)
    spans = [R.spans_of(u, c) for u, c in cases]

    def check(i, res, n_sub):
        st, sets, r = run.states(), run.sets(), read(run)
        for s in range(n_sub):
            n_bits, flags, left = exp[s][i]
            assert tuple(res[s]) == (n_bits, flags), (i, s)
            assert_set(sets, s, left, (i, s))                       # the out set is behind the piece, always
            assert_unit(r, s, units[s], spans[s][i][2], spans[s][i][3], what=(i, s))
            if i < len(spans[s]) - 1:
                assert_open(st, s, n_bits - 8, (i, s))
            else:
                assert_closed(st, s, what=(i, s))
                assert tuple(res[s]) == tuple(want_res[s])
    run.pieces([c[1] for c in cases], check)
    got = read(run)
    assert same_outputs(got, want)
    assert np.array_equal(run.sets()[0], want_sets[0]) and np.array_equal(run.sets()[1], want_sets[1])


# ---------------------------------------------------------------------------------------------- 4. terminate
def test_a_cut_behind_the_terminate_bin_gives_a_marked_state_and_a_piece_of_nothing_finishes(hip):
    cases, _ = block_cases()
    units = [cases[1][0], cases[2][0], phase_case()[0]]
    ends = [(len(u["plan"]), len(u["metas"])) for u in units]
    assert all(int(u["plan"][-1, 0]) & 15 == E.TRM and u["values"][-1] == 1 for u in units)
    # the bin decoder's states behind the same terminate bins
    strings = [PM.expand(u["plan"], u["values"], u["metas"], u["blocks"], u["at"], u["guards"])[0] for u in units]
    bins = BinRun(hip, strings, [u["qp"] for u in units], [R.INIT_ID] * 3, data=[u["data"] for u in units], caps=[len(u["data"]) for u in units])
    bins.launch(True, [(0, len(x)) for x in strings], [False] * 3)
    theirs = bins.states()
    for feed in (False, True):
        run = Run(hip, units)
        res = run.launch([(0, 0) + e for e in ends], [False] * 3)
        st = run.states()
        for s, u in enumerate(units):
            w = st[s]
            rng, value, mark, zero = (int(x) for x in w["priv"])
            assert (w["kind"], w["flags"], w["bytes_final"], mark, zero) == (capi.CODER_DEC, 0, 0, 1, 0), s
            was = rng - 256 if rng >= 510 else rng                  # the decoder's range - 2 behind the bin: 254 / 255 travel as 510 / 511
            assert 256 <= rng <= 511 and was << 7 <= value < (rng + 2) << 7 and value < 1 << 16, s
            assert w["bits"] == theirs[s]["bits"] == res[s]["n_bits"] - 8 and res[s]["flags"] == 0, s
        if feed:                                                    # the decoder's state in place of the parser's own
            assert all(t["kind"] == capi.CODER_DEC and t["flags"] == 0 for t in theirs)
            run.put_states(theirs)
        res = run.launch([e + e for e in ends], [True] * 3)        # a final piece of nothing
        st, r = run.states(), read(run)
        for s, u in enumerate(units):
            assert tuple(res[s]) == PM.want_walk(u), (feed, s)
            assert_closed(st, s, what=(feed, s))
            assert_unit(r, s, u, what=(feed, s))


# ---------------------------------------------------------------------------------------------- 5. R3: one state format
def test_r3_the_state_is_the_bin_decoder_s_byte_for_byte_and_each_continues_the_other(hip):
    u, seg_cuts = mixed()
    tail = [c for c in R.entry_cuts(u) if c[0] > seg_cuts[-2][0]][:-1]
    cuts = (seg_cuts[:-2] + tail[::5])[:16]                         # in front of elements; none behind the terminate bin
    assert len(cuts) == 16 and all(e < len(u["plan"]) - 1 or b < len(u["metas"]) for e, b in cuts)
    n = len(cuts)
    string = PM.expand(u["plan"], u["values"], u["metas"], u["blocks"], u["at"], u["guards"])[0]
    at = [len(R.prefix_string(u, e, b)) for e, b in cuts]
    want = PM.want_walk(u)
    # piece 0 on both sides
    run = Run(hip, [u] * n)
    spans = [R.spans_of(u, [c]) for c in cuts]
    run.launch([sp[0] for sp in spans], [False] * n)
    bins = BinRun(hip, [string] * n, [u["qp"]] * n, [R.INIT_ID] * n, data=[u["data"]] * n, caps=[len(u["data"])] * n)
    bins.launch(True, [(0, k) for k in at], [False] * n)
    mine, theirs = run.states(), bins.states()
    assert mine.tobytes() == theirs.tobytes()
    assert all(w["kind"] == capi.CODER_DEC and w["priv"][2] == 0 for w in mine)
    # each continues from the other's state (swapped through the host; the contexts are each side's own)
    run.put_states(theirs)
    bins.d_coder[32:32 + 32 * n] = torch.from_numpy(mine.view(np.uint8).reshape(-1).copy()).cuda()
    res = run.launch([sp[1] for sp in spans], [True] * n)
    res_b = bins.launch(True, [(k, len(string)) for k in at], [True] * n)
    r = read(run)
    for s in range(n):
        assert tuple(res[s]) == want == tuple(res_b[s]), s
        assert_unit(r, s, u, what=s)
        assert np.array_equal(bins.bins(s), string >> 15), s
    assert all(w["kind"] == capi.CODER_CLOSED for w in run.states()) and all(w["kind"] == capi.CODER_CLOSED for w in bins.states())


# ---------------------------------------------------------------------------------------------- 6. damaged bytes
NO_ALIGN = [E.CTX_BIN, E.EP_BINS, E.REM_ABS, E.UNARY_MAX, E.UNARY_EP, E.EXP_GOLOMB, E.TRUNC_BIN]


@functools.lru_cache(maxsize=None)
def damaged_cases():
    """[(unit, cuts, capacity)]: valid units with one to three bits flipped in the middle (zero padding behind, so that the input
    cannot run out), and valid units in a slot cut short.  The runs between the blocks have no ALIGN entry: on damaged bytes the
    value may stand above range 256 behind one, a decoder state outside the state format (cabac_hip_pieces.h refuses it; the one
    call walks on in it), so R1 is not defined there."""
    rng = np.random.default_rng(0x51A6)
    cases = []
    for k in range(6):
        segs = [("tu", PM.tu_case(rng, *TU_OUTCOMES[int(rng.integers(0, len(TU_OUTCOMES)))])), R.flat_segment(rng, 9, NO_ALIGN),
                ("block",) + PM.chroma_block(rng), R.flat_segment(rng, 1, NO_ALIGN), ("tu", PM.tu_case(rng, *TU_OUTCOMES[5 + k]))]
        u, cuts = R.join(rng, segs, qp=20 + k)
        cuts = cuts[:1] + [cuts[1]] * (k % 2) + cuts[1:]            # some with a piece of nothing
        if k < 3:
            f = _flip_middle(rng, u)
            cases.append((f, cuts, len(f["data"])))
        else:
            S = [R.shifts_at(u, e, b) for e, b in cuts]
            cap = 2 + (S[1 + k % 3] >> 3) - (k - 3)                 # runs out in the piece behind that cut, or the one in front
            cases.append((u, cuts, cap))
    cases.sort(key=lambda c: -len(c[1]))
    return cases


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_damaged_bytes_and_short_slots_against_the_one_call_parse(hip, int16):
    cases = damaged_cases()
    units, caps = [c[0] for c in cases], [c[2] for c in cases]
    ref = Run(hip, units, int16, caps)
    want_res = ref.whole("sets")                                    # existing code: the reference here
    want, want_sets = read(ref), ref.sets()
    run = Run(hip, units, int16, caps)
    res = run.pieces([c[1] for c in cases])
    got, st, sets = read(run), run.states(), run.sets()
    underruns = 0
    for s, (u, cuts, cap) in enumerate(cases):
        spans = R.spans_of(u, cuts)
        flags = [int(res[i][s]["flags"]) for i in range(len(spans))]
        first = next((i for i, f in enumerate(flags) if f & STICKY), None)
        assert all(f & H.RES_BAD_STOP == 0 for f in flags[:-1]), s
        if first is None:                                           # nothing sticky: everything is the one call's
            assert tuple(res[len(spans) - 1][s]) == (int(want_res[s]["n_bits"]), int(want_res[s]["flags"]) & ~H.RES_RANGE | flags[-1] & H.RES_RANGE), s
            assert np.bitwise_or.reduce(flags) & H.RES_RANGE == int(want_res[s]["flags"]) & H.RES_RANGE, s
            e1, b1 = len(u["plan"]), len(u["metas"])
            assert np.array_equal(sets[0][s], want_sets[0][s]) and np.array_equal(sets[1][s], want_sets[1][s]), s
            assert st[s]["kind"] == capi.CODER_CLOSED, s
        else:                                                       # the piece that raised it is the last that parsed
            stuck = flags[first] & STICKY
            assert stuck == int(want_res[s]["flags"]) & STICKY, s
            for i in range(first + 1, len(spans)):
                assert tuple(res[i][s]) == (0, stuck), (s, i)
            e1, b1 = spans[first][2:]
            assert st[s]["flags"] == stuck and st[s]["kind"] == (capi.CODER_CLOSED if first == len(spans) - 1 else capi.CODER_DEC), s
        if cap < len(u["data"]):                                    # valid bytes, short slot: the model knows S behind every piece
            S = [R.shifts_at(u, sp[2], sp[3]) for sp in spans]
            over = [2 + (x >> 3) > cap for x in S]
            assert first == over.index(True) and flags[first] & ~H.RES_RANGE == H.RES_UNDERRUN, s
            assert all(f & ~H.RES_RANGE == 0 for f in flags[:first]), s
            underruns += 1
        # in front of the end of that piece the one call's outputs; behind it nothing
        r0, t0 = int(run.P["desc"]["rec_offset"][s]), int(run.P["tile_first"][s])
        assert np.array_equal(got["values"][s][:e1], want["values"][s][:e1]) and (got["values"][s][e1:] == VAL_GUARD).all(), s
        assert np.array_equal(got["infos"][s][:b1], want["infos"][s][:b1]) and (got["infos"][s][b1:] == WORD_GUARD_U).all(), s
        for k in range(len(u["metas"])):
            if k < b1:
                assert np.array_equal(got["blocks"][s][k], want["blocks"][s][k]), (s, k)
            else:
                assert (got["blocks"][s][k] == np.int32(np.int16(sentinel(True)) if int16 else sentinel(False))).all(), (s, k)
    flipped = [s for s, c in enumerate(cases) if c[2] == len(c[0]["data"])]
    assert underruns == 3 and len(flipped) == 3
    assert any(want["values"][s].tolist() != [v & 0xFFFFFFFF for v in units[s]["values"]] or int(want_res[s]["flags"]) for s in flipped), \
        "the flips change nothing"


# ---------------------------------------------------------------------------------------------- 7. refusals
def _bad_states(good, cap):
    """Every refusal of the header, made from a state the call wrote itself -> [(what, state words)]"""
    def mod(**kw):
        w = np.zeros(1, ST)
        w[0] = good
        for k, v in kw.items():
            if k[0] == "p":
                w["priv"][0, int(k[1])] = v
            else:
                w[k][0] = v
        return w[0]
    rng, value = int(good["priv"][0]), int(good["priv"][1])
    return [("unknown kind", mod(kind=7)), ("ENC", mod(kind=capi.CODER_ENC)), ("CLOSED", mod(kind=capi.CODER_CLOSED)),
            ("range 255", mod(p0=255, p1=0)), ("range 511 unmarked", mod(p0=511, p1=0)), ("range 512 marked", mod(p0=512, p1=0, p2=1)),
            ("value at range << 7", mod(p1=rng << 7)), ("marked value at (range + 2) << 7", mod(p0=300, p1=302 << 7, p2=1)),
            ("mark 2", mod(p2=2)), ("outside the slot", mod(bits=8 * (cap - 1)))]


def test_each_refusal_in_a_batch_mixed_with_fresh_resumed_and_flagged_substreams(hip):
    u, cuts, S, exp = phase_case()
    k = 17
    cut, cap = cuts[k], len(u["data"])
    n_bad = len(_bad_states(np.zeros(1, ST)[0], cap))
    n = n_bad + 4                                                   # 0: resumed, 1: fresh, 2: flagged, then the refusals, last: resumed
    run = Run(hip, [u] * n)
    sp = R.spans_of(u, [cut])
    run.launch([sp[0], (0, 0, 0, 0)] + [sp[0]] * (n - 2), [False] * n)   # (the fresh one: a piece of nothing, its contexts stay)
    st = run.states()
    for s in range(n):
        assert_open(st, s, 0 if s == 1 else S[k], s)
    bad = _bad_states(st[0], cap)
    given = st.copy()
    given[1] = np.zeros(1, ST)[0]
    given[2]["flags"] = H.RES_UNDERRUN
    for j, (_, w) in enumerate(bad):
        given[3 + j] = w
    run.put_states(given)
    sets_before = run.sets()
    whole = [(0, 0, len(u["plan"]), 0)]
    res = run.launch([sp[1], whole[0], sp[1]] + [sp[1]] * n_bad + [sp[1]], [True] * n)
    st, sets, r = run.states(), run.sets(), read(run)
    want = PM.want_walk(u)
    for s in (0, 1, n - 1):                                         # the neighbours: resumed, fresh (parsed again from the start), resumed
        assert tuple(res[s]) == want, s
        assert_closed(st, s, what=s)
        assert_unit(r, s, u, what=s)
        assert_set(sets, s, exp[k][1][2], s)
    # flags from an earlier piece: {0, flags}, the state copied, nothing parsed
    assert tuple(res[2]) == (0, H.RES_UNDERRUN) and st[2].tobytes() == given[2].tobytes()
    for s in range(2, n - 1):
        assert_unit(r, s, u, *cut, what=s)                          # what piece 0 wrote and not a word more
        assert np.array_equal(sets[0][s], sets_before[0][s]) and np.array_equal(sets[1][s], sets_before[1][s]), s
    for j, (what, w) in enumerate(bad):
        assert tuple(res[3 + j]) == (0, capi.RES_BAD_STATE), what
        assert st[3 + j].tobytes() == w.tobytes(), what             # no state written


def test_a_reference_across_a_piece_boundary_is_a_bad_record_and_the_next_piece_passes(hip):
    rng = np.random.default_rng(0x51A7)
    u = PM.tu_unit(rng, [PM.tu_case(rng, *TU_OUTCOMES[7])], qp=31)
    cuts = [(2, 0), (PM.TU_LEN, 3)]                                 # tu_cbf_cr's guard looks back at tu_cbf_cb, in front of the piece
    assert not R.references_stay_inside(u, cuts)
    run = Run(hip, [u, u])
    S = R.shifts_at(u, 2, 0)
    res = run.pieces([cuts, [cuts[1], cuts[1]]])                    # the neighbour is cut where no reference crosses
    st, r = run.states(), read(run)
    assert tuple(res[0][0]) == (S + 8, 0)
    assert tuple(res[1][0]) == (S + 8, H.RES_BAD_RECORD)            # stopped in front of the entry: nothing shifted
    assert tuple(res[2][0]) == (0, H.RES_BAD_RECORD)
    assert (st[0]["kind"], st[0]["flags"], st[0]["bits"]) == (capi.CODER_DEC, H.RES_BAD_RECORD, S)
    assert_unit(r, 0, u, 2, 0)
    assert tuple(res[2][1]) == PM.want_walk(u)
    assert_unit(r, 1, u)
    assert_closed(st, 1)


# ---------------------------------------------------------------------------------------------- 8. R2
@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_r2_all_fresh_all_final_is_the_sets_form_bit_for_bit(hip, int16):
    rng = np.random.default_rng(0x51A8)
    units = [c[0] for c in block_cases()[0]] + [c[0] for c in damaged_cases()] + [phase_case()[0]]
    for _ in range(5):
        units.append(R.join(rng, R.random_segments(rng, [int(rng.integers(1, 90))]), qp=int(rng.integers(0, 64)))[0])
    ff = dict(units[0], data=np.concatenate([[0xFF], units[0]["data"][1:]]).astype(np.uint8))   # the refused start
    units = units + [ff, dict(units[1], data=units[1]["data"][:5])]
    ref = Run(hip, units, int16)
    want_res = ref.whole("sets")
    want, want_sets = read(ref), ref.sets()
    assert int(want_res[len(units) - 2]["flags"]) == H.RES_BAD_STOP and int(want_res[len(units) - 1]["flags"]) & H.RES_UNDERRUN
    for coder in (True, False):                                     # zeroed states in place, and no state arrays at all
        run = Run(hip, units, int16)
        res = run.whole("resume", coder)
        got, sets, st = read(run), run.sets(), run.states()
        assert np.array_equal(res, want_res), coder
        assert same_outputs(got, want), coder
        assert np.array_equal(sets[0], want_sets[0]) and np.array_equal(sets[1], want_sets[1]), coder
        if coder:
            assert all(w["kind"] == capi.CODER_CLOSED and w["flags"] == int(f) & ~H.RES_RANGE for w, f in zip(st, want_res["flags"]))
        else:
            assert not st.view(np.uint32).any()


# ---------------------------------------------------------------------------------------------- 9. profile
def test_profile_reports_kind_50_once_per_piece(hip):
    u, cuts, S, exp = phase_case()
    own = capi.CabacHip(0)
    own.profile_enable(4)
    run = Run(own, [u])
    res = run.pieces([[cuts[20]]])
    assert tuple(res[1][0]) == PM.want_walk(u)
    prof = own.profile_read()
    assert [k for k, _ in prof] == [50, 50] and all(ms > 0 for _, ms in prof)
    own.close()
