"""GPU: the plan write in pieces (include/cabac_hip_plan_continue.h; the pieces instantiation of the plan walks in
csrc/cabac_plan_write.hip) against tests/plan_continue_model.py, against the one-call cabac_hip_plan_write_sets_device on the device
(C1, C3), against cabac_hip_encode_pieces_device (C2), and read back by cabac_hip_plan_resume_parse_device.  Everything is
bit-exact: == on integers.  Values, info words and results sit between guard words, every byte slot between sentinel bytes, the
states between two sentinel states, the sets between two sentinel sets; all of them are looked at after every launch.  States and
sets are in place: every launch reads and writes the same arrays.

Every test calls cabac_hip_plan_continue_write_device, so none passes without it."""
import functools

import numpy as np
import pytest
import torch

import ctx_sets_model as CS
import helpers as H
import parse_elements_model as E
import parse_plan_model as PM
import pieces_model as PC
import plan_continue_model as C
import plan_resume_model as R
import write_plan_model as W
from entropy_coding_amd import capi
from test_gpu_pieces import ENC_REFUSED, Run as BinRun, _spoil
from test_gpu_plan_resume import Run as ParseRun, assert_unit as assert_parsed, read as parse_read
from test_parse_plan_model import TU_OUTCOMES
from test_plan_resume_model import mixed

pytestmark = pytest.mark.gpu

G = 64                                                             # guard elements on either side of every output
SENT32, SENT8 = 0x5A5A5A5A, 0xA5
VAL_GUARD, WORD_GUARD = 0xEEEEEEEE, 0xEEDDCCBB
FIN = H.SUB_FINISH | H.SUB_ALIGN_RBSP
ST = capi.CODER_STATE_DTYPE
NCTX = H.NUM_CTX
STOPS = H.RES_BAD_RECORD | E.RES_BAD_VALUE
NO_CTX = [E.EP_BINS, E.UNARY_EP, E.EXP_GOLOMB, E.TRUNC_BIN, E.REM_ABS]     # elements of bypass bins alone


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


def u32(values):
    return np.array([int(v) & 0xFFFFFFFF for v in values], np.uint64).astype(np.uint32)


class Run:
    """The substreams of `units` written in pieces.  The plan, the values, the block descriptors and the coefficients of the whole
    units lie on the device once; every launch gets descriptors, block lists and positions of its pieces.  Byte slots of capacity
    caps[s] (default: exactly the bytes of the finished substream) at 16-aligned offsets with G sentinel bytes around each; one
    state per substream in ONE array (in and out the same) and one set per substream, started from and written back in place.  The
    slots of the values that the call does not read (computed entries, skipped elements of a valid unit) hold garbage."""

    def __init__(self, hip, units, int16=False, caps=None, in_place=False):
        self.hip, self.units, self.n, self.int16, self.in_place = hip, units, len(units), int16, in_place
        self.P = P = PM.pack(units)
        self.n_el = len(P["plan"])
        self.pos = [R.positions(u) for u in units]
        coeff = np.zeros(max(P["total"], 1), np.int16 if int16 else np.int32)
        t = 0
        for u in units:
            for b in u["blocks"]:
                b = np.asarray(b, np.int32)
                assert np.abs(b).max(initial=0) <= 32767
                coeff[int(P["offsets"][t]):int(P["offsets"][t]) + b.size] = b.reshape(-1)
                t += 1
        vin = []
        for u in units:
            v = u32(u["values"])
            if u.get("valid", True):
                active = PM.expand(u["plan"], u["values"], u["metas"], u["blocks"], u["at"], u["guards"])[2]
                for i, on in enumerate(active):
                    if not on:
                        v[i] = 0xDEAD0000 + (i & 0xFFFF)
            vin.append(v)
        self.vin = np.concatenate(vin + [np.zeros(0, np.uint32)]).astype(np.uint32)
        self.d_plan = dev(np.concatenate([P["plan"].reshape(-1), np.zeros(4, np.uint32)]))
        self.d_vin = dev(np.concatenate([self.vin, np.zeros(2, np.uint32)]))
        self.d_coeff = dev(coeff)
        self.d_val = torch.from_numpy(np.full(self.n_el + 2 * G, VAL_GUARD, np.uint32).view(np.int32)).cuda()
        if in_place:
            self.d_val[G:G + self.n_el] = torch.from_numpy(self.vin.view(np.int32).copy()).cuda()
        self.info = np.full(P["n_tu"], WORD_GUARD, np.uint32)
        # the slots
        self.caps = np.asarray(caps if caps is not None else [len(u["data"]) for u in units], np.int64)
        self.off = np.zeros(self.n, np.int64)
        at = G
        for s in range(self.n):
            self.off[s] = at
            at = (at + int(self.caps[s]) + G + 15) // 16 * 16
        self.total = at + G
        self.d_bytes = dev(np.full(self.total + 16, SENT8, np.uint8))
        self.outside = np.ones(self.total + 16, bool)
        for s in range(self.n):
            self.outside[int(self.off[s]):int(self.off[s]) + int(self.caps[s])] = False
        # the sets and the states
        state = np.full((self.n + 2) * NCTX, SENT32, np.uint32)
        rate = np.full((self.n + 2) * NCTX, SENT8, np.uint8)
        for s, u in enumerate(units):
            state[(s + 1) * NCTX:(s + 2) * NCTX], rate[(s + 1) * NCTX:(s + 2) * NCTX] = CS.pack(CS.init_set(u["qp"], C.INIT_ID))
        self.d_state, self.d_rate = dev(state), dev(rate)
        self.d_idx = dev(np.arange(1, self.n + 1, dtype=np.uint32))
        self.d_coder = dev(np.concatenate([np.full(8, SENT32, np.uint32), np.zeros(8 * self.n, np.uint32), np.full(8, SENT32, np.uint32)]))
        self.d_res = dev(np.full(2 * self.n + 2 * G, WORD_GUARD, np.uint32))

    # ---- the calls
    def _inputs(self, desc, tile_first, tus, at, guard):
        t_desc, t_first = dev(desc), dev(np.asarray(tile_first, np.uint32))
        t_tu = dev(tus) if len(tus) else None
        t_at = dev(np.asarray(at, np.uint32)) if len(tus) else None
        t_guard = dev(np.asarray(guard, np.uint32)) if len(tus) else None
        p_vin = self.d_val.data_ptr() + 4 * G if self.in_place else self.d_vin.data_ptr()
        keep = (t_desc, t_first, t_tu, t_at, t_guard)
        return keep, (len(desc), t_desc.data_ptr(), self.d_plan.data_ptr(), p_vin, t_first.data_ptr(), len(tus), opt(t_tu), opt(t_at),
                      opt(t_guard), self.d_coeff.data_ptr() if len(tus) else 0)

    def _sets(self):
        return dict(n_sets=self.n + 2, d_state=self.d_state.data_ptr(), d_rate=self.d_rate.data_ptr(), d_start_set=self.d_idx.data_ptr(),
                    d_out_set=self.d_idx.data_ptr(), d_out_state=self.d_state.data_ptr(), d_out_rate=self.d_rate.data_ptr())

    def _results(self, n_sub):
        raw = host(self.d_res, np.uint32)
        assert (raw[:G] == WORD_GUARD).all() and (raw[G + 2 * n_sub:] == WORD_GUARD).all(), "a result outside the launch's substreams"
        res = raw[G:G + 2 * n_sub].view(H.RESULT_DTYPE).copy()
        self.d_res[4 * G:4 * G + 8 * n_sub] = dev(np.full(2 * n_sub, WORD_GUARD, np.uint32))
        return res

    def _call(self, desc, tile_first, tus, at, guard, where, coder=True, hip=None):
        keep, args = self._inputs(desc, tile_first, tus, at, guard)
        d_info = torch.from_numpy(np.full(len(tus) + 2 * G, WORD_GUARD, np.uint32).view(np.int32)).cuda()
        p = self.d_coder.data_ptr() + 32 if coder else 0
        (hip or self.hip).plan_continue_write_device(*args, self.d_bytes.data_ptr(), self.d_res.data_ptr() + 4 * G,
                                                     d_values_out=self.d_val.data_ptr() + 4 * G, d_tu_info=d_info.data_ptr() + 4 * G,
                                                     int16=self.int16, **self._sets(), d_coder_in=p, d_coder_out=p)
        (hip or self.hip).synchronize()
        info = host(d_info, np.uint32)
        assert (info[:G] == WORD_GUARD).all() and (info[G + len(tus):] == WORD_GUARD).all(), "an info word outside the launch's blocks"
        if len(where):
            self.info[np.asarray(where, np.int64)] = info[G:G + len(tus)]
        self.last_info = info[G:G + len(tus)].copy()
        self.bytes(), self.states(), self.sets(), self.values()      # the sentinels, after every launch
        return self._results(len(desc))

    def launch(self, spans, last, n_sub=None, hip=None):
        """One piece of the first n_sub substreams: spans[s] = (e0, b0, e1, b1), last[s]: the final piece -> results"""
        n_sub = self.n if n_sub is None else n_sub
        P = self.P
        desc = np.zeros(n_sub, H.DESC_DTYPE)
        tus, at, guard, first, where = [], [], [], [0], []
        for s in range(n_sub):
            e0, b0, e1, b1 = spans[s]
            t0 = int(P["tile_first"][s])
            desc[s] = (int(P["desc"]["rec_offset"][s]) + e0, self.off[s], e1 - e0, self.caps[s], self.units[s]["qp"],
                       C.INIT_ID | (FIN if last[s] else 0))
            tus.append(P["tus"][t0 + b0:t0 + b1])
            at += [p - e0 for p in self.pos[s][b0:b1]]
            g = self.units[s]["guards"]
            guard += [0] * (b1 - b0) if g is None else [int(x) for x in g[b0:b1]]
            where += list(range(t0 + b0, t0 + b1))
            first.append(first[-1] + b1 - b0)
        tus = np.concatenate(tus + [np.zeros(0, H.TU_DTYPE)])
        return self._call(desc, first, tus, at, guard, where, hip=hip)

    def _whole_args(self):
        P = self.P
        desc = np.zeros(self.n, H.DESC_DTYPE)
        for s in range(self.n):
            desc[s] = (int(P["desc"]["rec_offset"][s]), self.off[s], len(self.units[s]["plan"]), self.caps[s], self.units[s]["qp"], C.INIT_ID | FIN)
        guard = [0] * P["n_tu"] if P["tu_guard"] is None else P["tu_guard"]
        return desc, P["tile_first"], P["tus"][:P["n_tu"]], [p for ps in self.pos for p in ps], guard

    def whole(self, coder=True):
        """ONE call of the new entry point over the whole substreams, every descriptor final, from fresh states"""
        return self._call(*self._whole_args(), list(range(self.P["n_tu"])), coder)

    def whole_sets(self):
        """ONE cabac_hip_plan_write_sets_device over the whole substreams -> (results, [payload bytes per substream]); the
        values, the info words and the sets land where the new call's land"""
        desc, first, tus, at, guard = self._whole_args()
        desc["byte_offset"], desc["byte_capacity"] = 0x7FFFFFF0, 0     # ignored by the one-call form
        keep, args = self._inputs(desc, first, tus, at, guard)
        cap = int(sum(len(u["data"]) for u in self.units)) + 64
        t_pay = torch.full((cap + 2 * G,), SENT8, dtype=torch.uint8, device="cuda")
        t_off = torch.full((self.n + 1 + 2 * G,), -7, dtype=torch.int64, device="cuda")
        d_info = torch.from_numpy(np.full(len(tus) + 2 * G, WORD_GUARD, np.uint32).view(np.int32)).cuda()
        self.hip.plan_write_sets_device(*args, t_pay.data_ptr() + G, cap, t_off.data_ptr() + 8 * G, self.d_res.data_ptr() + 4 * G,
                                        d_values_out=self.d_val.data_ptr() + 4 * G, d_tu_info=d_info.data_ptr() + 4 * G, int16=self.int16,
                                        **self._sets())
        self.hip.synchronize()
        pay, off = t_pay.cpu().numpy(), t_off.cpu().numpy()[G:G + self.n + 1]
        self.info[:] = host(d_info, np.uint32)[G:G + len(tus)]
        return self._results(self.n), [pay[G + int(off[s]):G + int(off[s + 1])].copy() for s in range(self.n)]

    def pieces(self, cuts, check=None):
        """All pieces of every substream, the substreams with more pieces first: launch i writes piece i of those that have one"""
        spans = [R.spans_of(u, c) for u, c in zip(self.units, cuts)]
        counts = [len(sp) for sp in spans]
        assert counts == sorted(counts, reverse=True), "substreams with more pieces come first"
        out = []
        for i in range(counts[0]):
            n_sub = sum(1 for c in counts if c > i)
            res = self.launch([sp[i] for sp in spans[:n_sub]], [i == len(sp) - 1 for sp in spans[:n_sub]], n_sub)
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
        self.d_coder[32:32 + 32 * self.n] = dev(np.ascontiguousarray(st).view(np.uint8))

    def sets(self):
        st, rt = host(self.d_state, np.uint32), host(self.d_rate, np.uint8)
        assert (st[:NCTX] == SENT32).all() and (st[-NCTX:] == SENT32).all(), "the sets around the array"
        assert (rt[:NCTX] == SENT8).all() and (rt[-NCTX:] == SENT8).all()
        return st[NCTX:-NCTX].reshape(self.n, NCTX).copy(), rt[NCTX:-NCTX].reshape(self.n, NCTX).copy()

    def bytes(self):
        b = host(self.d_bytes, np.uint8).copy()
        assert (b[self.outside] == SENT8).all(), "a byte outside the slots"
        return b

    def slot(self, s, n=None, image=None):
        b = self.bytes() if image is None else image
        o = int(self.off[s])
        return b[o:o + (int(self.caps[s]) if n is None else n)]

    def values(self, s=None):
        val = host(self.d_val, np.uint32)
        assert (val[:G] == VAL_GUARD).all() and (val[G + self.n_el:] == VAL_GUARD).all(), "a value outside the array"
        if s is None:
            return val[G:G + self.n_el].copy()
        r0 = int(self.P["desc"]["rec_offset"][s])
        return val[G + r0:G + r0 + len(self.units[s]["plan"])].copy()

    def untouched(self, s):
        """What the values of substream s hold where the call has not written"""
        r0 = int(self.P["desc"]["rec_offset"][s])
        n = len(self.units[s]["plan"])
        return self.vin[r0:r0 + n] if self.in_place else np.full(n, VAL_GUARD, np.uint32)

    def infos(self, s):
        return self.info[int(self.P["tile_first"][s]):int(self.P["tile_first"][s + 1])].copy()


def assert_set(sets, s, ctx, what=""):
    state, rate = CS.pack(ctx)
    assert np.array_equal(sets[0][s], state) and np.array_equal(sets[1][s], rate), what


def assert_written(run, s, u, e1=None, b1=None, what=""):
    """Substream s holds the unit's filled values and info words in front of the cut (e1, b1), and nothing behind it"""
    e1 = len(u["plan"]) if e1 is None else e1
    b1 = len(u["metas"]) if b1 is None else b1
    v = run.values(s)
    assert v[:e1].tolist() == u32(u["values"][:e1]).tolist(), (what, s)
    assert np.array_equal(v[e1:], run.untouched(s)[e1:]), (what, s)
    w = run.infos(s)
    assert w[:b1].tolist() == [int(x) for x in u["infos"][:b1]] and (w[b1:] == WORD_GUARD).all(), (what, s)


def assert_open(run, st, s, n_bits, data, what=""):
    """An encoder between two pieces, flagless and inside the format: bits is the result's n_bits, the first bytes_final bytes of
    the slot are the final bytes -> pend"""
    w = st[s]
    assert (w["kind"], w["flags"], w["bits"]) == (capi.CODER_ENC, 0, n_bits), (what, s)
    low, rp, buf, nbuf = (int(x) for x in w["priv"])
    rng, pend, pos = rp & 0xFFFF, rp >> 16, int(w["bytes_final"])
    assert 256 <= rng <= 510 and pend < 16 and low < 1 << (10 + pend) and pos % 2 == 0, (what, s)
    assert n_bits == 8 * pos + 16 * nbuf + pend and pos + 2 * nbuf <= run.caps[s], (what, s)
    assert np.array_equal(run.slot(s, pos), data[:pos]), (what, s)
    return pend


def assert_closed(run, st, s, n_bits, data, flags=0, what=""):
    w = st[s]
    assert (w["kind"], w["flags"], w["bits"], w["bytes_final"]) == (capi.CODER_CLOSED, flags, n_bits, len(data)) and not w["priv"].any(), (what, s)
    assert (n_bits + 7) // 8 == len(data) and np.array_equal(run.slot(s, len(data)), data), (what, s)


def check_against_model(run, units, cuts, exp):
    """-> check(i, res, n_sub) for Run.pieces: results, states, sets, bytes, values and info words behind every piece are the
    model's; the pend of every open state is noted in check.pend"""
    spans = [R.spans_of(u, c) for u, c in zip(units, cuts)]

    def check(i, res, n_sub):
        st, sets = run.states(), run.sets()
        for s in range(n_sub):
            out, data = exp[s]
            n_bits, flags, left = out[i]
            assert tuple(res[s]) == (n_bits, flags), (i, s)
            assert_set(sets, s, left, (i, s))
            assert_written(run, s, units[s], spans[s][i][2], spans[s][i][3], what=(i, s))
            if i < len(spans[s]) - 1:
                check.pend.add(assert_open(run, st, s, n_bits, data, (i, s)))
            else:
                assert_closed(run, st, s, n_bits, data, what=(i, s))
    check.pend = set()
    return check


def assert_c1(run, ref_run, units, exp):
    """The slots, the last results, the out sets, the values and the info words are the one call's"""
    want_res, payload = ref_run.whole_sets()
    st = run.states()
    for s, u in enumerate(units):
        out, data = exp[s]
        assert tuple(want_res[s]) == out[-1][:2], s
        assert np.array_equal(payload[s], data) and np.array_equal(run.slot(s, len(data)), payload[s]), s
        assert st[s]["kind"] == capi.CODER_CLOSED and st[s]["bits"] == want_res[s]["n_bits"], s
    assert np.array_equal(run.values(), ref_run.values()) and np.array_equal(run.info, ref_run.info)
    assert np.array_equal(run.sets()[0], ref_run.sets()[0]) and np.array_equal(run.sets()[1], ref_run.sets()[1])


# ---------------------------------------------------------------------------------------------- 1. every entry boundary
@functools.lru_cache(maxsize=None)
def boundary_case():
    """One joined unit — flat runs, a transform unit with three blocks, the terminate bin in a piece of its own — and every entry
    boundary of it that is a cut no reference crosses.  -> (unit, [cuts per substream], [model per substream]): substream 0 is
    cut at ALL of them, substream 1 + k at the k-th alone."""
    rng = np.random.default_rng(0xC0BF)
    kinds = [E.CTX_BIN, E.CTX_BIN, E.EP_BINS, E.UNARY_MAX, E.REM_ABS, E.TRUNC_BIN, E.EXP_GOLOMB]
    u, _ = R.join(rng, [R.flat_segment(rng, 20, kinds), ("tu", PM.tu_case(rng, *TU_OUTCOMES[7])), R.flat_segment(rng, 16, kinds)], qp=27)
    every = [c for c in R.entry_cuts(u)[1:-1] if R.references_stay_inside(u, [c])]
    chain = [c for k, c in enumerate(every) if R.references_stay_inside(u, every[:k + 1])]
    assert len(chain) >= 36 and (len(u["plan"]) - 1, 3) in chain and (20, 0) in chain and (44, 3) in chain
    cuts = [chain] + [[c] for c in every]
    exp = [C.expect(u, c) for c in cuts]
    # bits = 8 bytes_final + 16 nbuf + pend with an even bytes_final: the model knows pend behind every piece
    assert {out[0] % 16 for e in exp for out in e[0][:-1]} == set(range(16)), "the shifts not yet a whole unit take all 16 values"
    return u, cuts, exp


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_a_cut_at_every_entry_boundary_takes_every_pend_phase(hip, int16):
    u, cuts, exp = boundary_case()
    units = [u] * len(cuts)
    run = Run(hip, units, int16)
    check = check_against_model(run, units, cuts, exp)
    run.pieces(cuts, check)
    assert check.pend == set(range(16)), "the shifts not yet a whole unit take all 16 values"
    assert_c1(run, Run(hip, units, int16), units, exp)


# ---------------------------------------------------------------------------------------------- 2. batch sizes
@functools.lru_cache(maxsize=None)
def batch_case():
    """Five different units, more pieces first, some with pieces of nothing: one launch mixes final, non-final and empty pieces"""
    rng = np.random.default_rng(0xC0B1)
    cases = []
    for k, n_seg in enumerate((5, 4, 3, 2, 1)):
        segs = []
        for j in range(n_seg):
            segs.append([("tu", PM.tu_case(rng, *TU_OUTCOMES[(11 * k + 5 * j) % len(TU_OUTCOMES)])), R.flat_segment(rng, 3 + 2 * k),
                         ("block",) + PM.chroma_block(rng)][(k + j) % 3])
        u, cuts = R.join(rng, segs, qp=22 + 4 * k)
        if k % 2:
            cuts = cuts[:1] * 2 + cuts[1:]                          # a piece of nothing behind the first
        cases.append((u, cuts))
    cases.sort(key=lambda c: -len(c[1]))
    return cases, [C.expect(u, c) for u, c in cases]


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
@pytest.mark.parametrize("n_sub", [1, 4, 5])
def test_one_wave_a_full_workgroup_and_a_partial_last_one(hip, n_sub, int16):
    cases, exp = batch_case()
    cases, exp = cases[-n_sub:] if n_sub < 4 else cases[:n_sub], exp[-n_sub:] if n_sub < 4 else exp[:n_sub]
    units, cuts = [c[0] for c in cases], [c[1] for c in cases]
    run = Run(hip, units, int16, in_place=n_sub == 4)
    mixed_launch = []

    def check(i, res, n_sub_now, inner=check_against_model(run, units, cuts, exp)):
        inner(i, res, n_sub_now)
        kinds = {"final" if i == len(c) else "empty" if i and c[i - 1] == (c[i] if i < len(c) else None) else "open" for c in cuts[:n_sub_now]}
        mixed_launch.append(kinds)
    run.pieces(cuts, check)
    if n_sub == 5:
        assert any({"final", "open"} <= k for k in mixed_launch) and any("empty" in k for k in mixed_launch)
    assert_c1(run, Run(hip, units, int16), units, exp)


# ---------------------------------------------------------------------------------------------- 3. piece shapes
@functools.lru_cache(maxsize=None)
def shape_case():
    """The mixed unit of the model's test cut between all its segments (a piece of one block and no entry, pieces of one entry),
    the same with pieces of nothing and an empty final piece on a resumed state, and a substream that is nothing but "end the
    slice here" on a fresh state"""
    u, cuts = mixed()
    end = (len(u["plan"]), len(u["metas"]))
    nothing = PM.build(np.random.default_rng(1), np.zeros((0, 2), np.uint32), [], qp=30)
    cases = [(u, [cuts[0], cuts[0]] + cuts[1:] + [end, end]), (u, cuts), (nothing, [])]
    spans = R.spans_of(u, cuts)
    assert any(sp[0] == sp[2] and sp[3] == sp[1] + 1 for sp in spans) and any(sp[2] == sp[0] + 1 and sp[1] == sp[3] for sp in spans)
    return cases, [C.expect(c[0], c[1]) for c in cases]


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_pieces_of_one_block_of_one_entry_of_nothing_and_end_the_slice_here(hip, int16):
    cases, exp = shape_case()
    units, cuts = [c[0] for c in cases], [c[1] for c in cases]
    run = Run(hip, units, int16)
    res = run.pieces(cuts, check_against_model(run, units, cuts, exp))
    # the empty final piece on the resumed state finished the substream; the one in front of it passed the state through
    assert tuple(res[-1][0]) == exp[0][0][-1][:2] and tuple(res[-3][0]) == tuple(res[-2][0])
    # the fresh one: finish() alone
    assert tuple(res[0][2]) == exp[2][0][0][:2] and len(exp[2][1]) <= 2
    assert_c1(run, Run(hip, units, int16), units, exp)


# ---------------------------------------------------------------------------------------------- 4. C2: one state format
def test_c2_the_state_is_the_bin_encoder_s_byte_for_byte_and_each_continues_the_other(hip):
    cases, exp = batch_case()
    units, cuts = [c[0] for c in cases], [c[1] for c in cases]
    n = len(units)
    strings = [C.whole_string(u) for u in units]
    rcuts = [C.record_cuts(u, c) for u, c in zip(units, cuts)]
    caps = [len(u["data"]) for u in units]
    run = Run(hip, units)
    bins = BinRun(hip, strings, [u["qp"] for u in units], [C.INIT_ID] * n, caps=caps)
    spans = [R.spans_of(u, c) for u, c in zip(units, cuts)]
    rspans = [PC.pieces_of(len(x), c) for x, c in zip(strings, rcuts)]
    open_states = 0
    for i in range(len(spans[0])):
        n_sub = sum(1 for sp in spans if len(sp) > i)
        last = [i == len(sp) - 1 for sp in spans[:n_sub]]
        res = run.launch([sp[i] for sp in spans[:n_sub]], last, n_sub)
        res_b = bins.launch(False, [sp[i] for sp in rspans[:n_sub]], last, n_sub)
        mine, theirs = run.states(), bins.states()
        assert mine.tobytes() == theirs.tobytes(), i
        assert np.array_equal(res, res_b[:n_sub]), i
        open_states += sum(1 for w in mine[:n_sub] if w["kind"] == capi.CODER_ENC)
        # each continues from the other's state (swapped through the host; the slots and the contexts are each side's own)
        run.put_states(theirs)
        bins.d_coder[32:32 + 32 * n] = dev(mine.view(np.uint8))
    assert open_states >= 10
    b = bins.bytes()
    for s, u in enumerate(units):
        data = exp[s][1]
        assert np.array_equal(run.slot(s, len(data)), data) and np.array_equal(bins.slot(b, s, len(data)), data), s
        assert_written(run, s, u, what=s)
    assert all(w["kind"] == capi.CODER_CLOSED for w in run.states()) and all(w["kind"] == capi.CODER_CLOSED for w in bins.states())


# ---------------------------------------------------------------------------------------------- 5. C3
def _stopped_units():
    """(unit, flag): a valid unit with a value outside its element's code, and one with a bad entry"""
    u, _ = mixed()
    i = next(k for k in range(len(u["plan"]) - 1, 0, -1) if W.domain_top(int(u["plan"][k, 0])) not in (None, 0xFFFFFFFF) and
             int(u["plan"][k, 1]) == 0 and not PM.is_computed(int(u["plan"][k, 0])))
    outside = next(v for v, ok in W.edge_values(int(u["plan"][i, 0])) if not ok)
    bad_value = dict(u, values=u["values"][:i] + [outside] + u["values"][i + 1:], valid=False)
    plan = u["plan"].copy()
    plan[3, 0] = 15                                                 # no such kind
    bad_entry = dict(u, plan=plan, valid=False)
    for x, flag in ((bad_value, W.BAD_VALUE), (bad_entry, W.BAD_RECORD)):
        assert W.stop_of(x["plan"], x["values"], x["metas"], x["blocks"], x["at"], x["guards"]) == flag
    return [(bad_value, W.BAD_VALUE), (bad_entry, W.BAD_RECORD)]


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_c3_all_fresh_all_final_is_the_sets_form(hip, int16):
    rng = np.random.default_rng(0xC0B5)
    units = [c[0] for c in shape_case()[0]] + [c[0] for c in batch_case()[0]] + [boundary_case()[0]]
    for _ in range(4):
        units.append(R.join(rng, R.random_segments(rng, [int(rng.integers(1, 90))]), qp=int(rng.integers(0, 64)))[0])
    stopped = _stopped_units()
    units += [x for x, _ in stopped]
    ref = Run(hip, units, int16)
    want_res, payload = ref.whole_sets()
    for k, (_, flag) in enumerate(stopped):
        assert tuple(want_res[len(units) - 2 + k]) == (0, flag)
    assert not want_res["flags"][:-2].any()
    for coder in (True, False):                                     # zeroed states in place, and no state arrays at all
        run = Run(hip, units, int16)
        res = run.whole(coder)
        assert np.array_equal(res, want_res), coder
        for s in range(len(units)):
            assert np.array_equal(run.slot(s, len(payload[s])), payload[s]), (coder, s)
            if s >= len(units) - 2:
                assert (run.slot(s) == SENT8).all(), "a stopped substream writes no byte"
        assert np.array_equal(run.values(), ref.values()) and np.array_equal(run.info, ref.info), coder
        assert np.array_equal(run.sets()[0], ref.sets()[0]) and np.array_equal(run.sets()[1], ref.sets()[1]), coder
        st = run.states()
        if coder:
            for s, w in enumerate(st[:-2]):
                assert (w["kind"], w["flags"], w["bits"], w["bytes_final"]) == (capi.CODER_CLOSED, 0, want_res[s]["n_bits"], len(payload[s])), s
            for w, (_, flag) in zip(st[-2:], stopped):              # a fresh in state comes out as the state of start(), flagged
                assert (w["kind"], w["flags"], w["bits"], w["bytes_final"]) == (capi.CODER_ENC, flag, 0, 0) and w["priv"].tolist() == [0, 510, 0, 0]
        else:
            assert not st.view(np.uint32).any()


# ---------------------------------------------------------------------------------------------- 6. round trip
def test_the_slots_are_parsed_back_in_pieces_under_the_same_cuts(hip):
    cases, exp = batch_case()
    units, cuts = [c[0] for c in cases], [c[1] for c in cases]
    run = Run(hip, units)
    run.pieces(cuts)
    written = [dict(u, data=run.slot(s, len(exp[s][1])).copy()) for s, u in enumerate(units)]
    back = ParseRun(hip, written)
    res = back.pieces(cuts)
    r = parse_read(back)
    for s, u in enumerate(units):
        assert tuple(res[len(cuts[s])][s]) == PM.want_walk(u), s
        assert_parsed(r, s, u, what=s)                               # the values and the coefficients come back


# ---------------------------------------------------------------------------------------------- 7. stops
@functools.lru_cache(maxsize=None)
def stop_case():
    """Substreams of three pieces — a flat run, a transform unit, a flat run with the terminate bin — in which piece 1 stops, or
    piece 0 does, between neighbours that are coded.  -> [(unit, cuts, stopped piece or None, flag)], the good unit, its model"""
    rng = np.random.default_rng(0xC0B7)
    good, cuts = R.join(rng, [R.flat_segment(rng, 6), ("tu", PM.tu_case(rng, 1, 1, 1, 0, 0, 0)), R.flat_segment(rng, 8)], qp=29)
    cuts = cuts[:2]
    tu0 = 6
    assert cuts == [(tu0, 0), (tu0 + PM.TU_LEN, 3)] and all(good["coded"])

    def changed(**kw):
        return dict(good, valid=False, **kw)

    def with_value(i, v):
        return changed(values=good["values"][:i] + [v] + good["values"][i + 1:])
    cases = [(good, cuts, None, 0)]
    # a value outside its element's code: tu_cbf_cb, and an element of the first run
    w0 = int(good["plan"][tu0, 0])
    assert w0 & 15 == E.CTX_BIN and int(good["plan"][tu0, 1]) == 0
    cases.append((with_value(tu0, next(v for v, ok in W.edge_values(w0) if not ok)), cuts, 1, W.BAD_VALUE))
    i = next(k for k in range(tu0) if W.domain_top(int(good["plan"][k, 0])) not in (None, 0xFFFFFFFF))
    cases.append((with_value(i, next(v for v, ok in W.edge_values(int(good["plan"][i, 0])) if not ok)), cuts, 0, W.BAD_VALUE))
    # a bad entry
    plan = good["plan"].copy()
    plan[tu0 + 5, 0] = 15
    cases.append((changed(plan=plan), cuts, 1, W.BAD_RECORD))
    # a coded block without a coefficient
    cases.append((changed(blocks=[good["blocks"][0], np.zeros_like(good["blocks"][1]), good["blocks"][2]]), cuts, 1, W.BAD_VALUE))
    # a reference across a piece boundary: tu_cbf_cr's guard looks back at tu_cbf_cb, in front of the piece
    across = [(tu0 + 2, 0), cuts[1]]
    assert not R.references_stay_inside(good, across)
    cases.append((good, across, 1, W.BAD_RECORD))
    cases.append((good, cuts, None, 0))
    for u, c, k, flag in cases:
        stops = [C.piece_stop(u, sp) for sp in R.spans_of(good, c)]
        assert stops == [flag if j == k else 0 for j in range(3)], (stops, k, flag)
    return cases, good, C.expect(good, cuts)


def test_each_stop_raises_its_flag_in_its_own_piece_and_the_next_piece_passes(hip):
    cases, good, (out, data) = stop_case()
    units, cuts = [c[0] for c in cases], [c[1] for c in cases]
    n = len(cases)
    run = Run(hip, units)
    spans = [R.spans_of(good, c) for c in cuts]
    before = (run.states(), run.sets(), run.bytes(), [run.values(s) for s in range(n)], [run.infos(s) for s in range(n)])
    for i in range(3):
        res = run.launch([sp[i] for sp in spans], [i == 2] * n)
        st, sets, image = run.states(), run.sets(), run.bytes()
        for s, (u, c, k, flag) in enumerate(cases):
            e1, b1 = spans[s][i][2:]
            if k is None:                                           # the neighbours are unaffected
                assert tuple(res[s]) == out[i][:2], (i, s)
                assert_set(sets, s, out[i][2], (i, s))
                assert_written(run, s, good, e1, b1, what=(i, s))
                (assert_open if i < 2 else assert_closed)(run, st, s, out[i][0], data, what=(i, s))
            elif i < k:                                             # in front of the stop: the prefix of the good unit
                n_bits = H.load_oracle().encode_records(R.prefix_string(good, e1, b1), good["qp"], C.INIT_ID, 4)[1]   # the probe
                assert tuple(res[s]) == (n_bits, 0), (i, s)
                assert_open(run, st, s, n_bits, data, (i, s))
            else:
                was_st, was_sets, was_image, was_val, was_info = before
                assert tuple(res[s]) == (0, flag), (i, s)
                want = was_st[s].copy()
                if i == k and want["kind"] == capi.CODER_FRESH:     # a fresh in state comes out as the state of start()
                    want["kind"], want["priv"] = capi.CODER_ENC, [0, 510, 0, 0]
                want["flags"] |= flag
                assert st[s].tobytes() == want.tobytes(), (i, s)
                assert st[s]["kind"] == capi.CODER_ENC and st[s]["flags"] == flag, (i, s)
                assert np.array_equal(run.slot(s, image=image), run.slot(s, image=was_image)), "a byte of a stopped piece"
                assert np.array_equal(sets[0][s], was_sets[0][s]) and np.array_equal(sets[1][s], was_sets[1][s]), "a set of a stopped piece"
                assert np.array_equal(run.values(s), was_val[s]) and np.array_equal(run.infos(s), was_info[s]), "a value or an info word"
                bf = int(st[s]["bytes_final"])
                assert np.array_equal(run.slot(s, bf, image), data[:bf])
        before = (st, sets, image, [run.values(s) for s in range(n)], [run.infos(s) for s in range(n)])
    assert sum(1 for c in cases if c[2] is not None) == 5


# ---------------------------------------------------------------------------------------------- 8. small slots
@functools.lru_cache(maxsize=None)
def small_slot_case():
    """A unit of bypass elements and the terminate bin (pieces_model.overflows_at replays context-free strings) cut into five
    pieces, in slots of several capacities below the need -> (unit, cuts, record cuts, [(capacity, first piece that overflows)])"""
    rng = np.random.default_rng(0xC0B8)
    u, cuts = R.join(rng, [R.flat_segment(rng, 14, NO_CTX, small=False) for _ in range(4)], qp=31)
    string, rcuts = C.whole_string(u), C.record_cuts(u, cuts)
    need = len(u["data"])
    caps = [(cap, PC.overflows_at(string, rcuts, cap)) for cap in (need, need - 1, need - 2, need // 2 + 1, need // 2, need // 4, 3, 0)]
    assert caps[0][1] is None and all(k is not None for _, k in caps[1:]) and len({k for _, k in caps}) >= 4
    return u, cuts, rcuts, caps


def test_small_slots_overflow_at_the_piece_the_encoder_in_pieces_reports(hip):
    u, cuts, rcuts, caps = small_slot_case()
    n = len(caps)
    string = C.whole_string(u)
    run = Run(hip, [u] * n, caps=[c for c, _ in caps])
    bins = BinRun(hip, [string] * n, [u["qp"]] * n, [C.INIT_ID] * n, caps=[c for c, _ in caps])
    spans, rspans = R.spans_of(u, cuts), PC.pieces_of(len(string), rcuts)
    for i in range(len(spans)):
        last = [i == len(spans) - 1] * n
        res = run.launch([spans[i]] * n, last)                      # (every launch checks that nothing lies outside the slots)
        res_b = bins.launch(False, [rspans[i]] * n, last)
        bins.bytes()
        assert np.array_equal(res, res_b), i
        st = run.states()
        assert st.tobytes() == bins.states().tobytes(), i
        for s, (cap, first) in enumerate(caps):
            if first is not None and i >= first:
                assert tuple(res[s]) == ((res[s]["n_bits"], H.RES_OVERFLOW) if i == first else (0, H.RES_OVERFLOW)), (i, s)
                assert st[s]["flags"] == H.RES_OVERFLOW, (i, s)
            else:
                assert res[s]["flags"] == 0, (i, s)
    assert np.array_equal(run.slot(0), u["data"])


# ---------------------------------------------------------------------------------------------- 9. refusals
def test_each_refused_state_in_a_batch_mixed_with_fresh_resumed_and_flagged_substreams(hip):
    cases, good, (out, data) = stop_case()
    cuts = cases[0][1]
    n = len(ENC_REFUSED) + 4                                        # 0: resumed, 1: fresh, 2: flagged, then the refusals, last: resumed
    run = Run(hip, [good] * n)
    sp = R.spans_of(good, cuts)
    run.launch([sp[0], (0, 0, 0, 0)] + [sp[0]] * (n - 2), [False] * n)   # (the fresh one: a piece of nothing)
    st = run.states()
    for s in range(n):
        assert_open(run, st, s, 0 if s == 1 else out[0][0], data, s)
    given = st.copy()
    given[1] = np.zeros(1, ST)[0]
    given[2]["flags"] = H.RES_OVERFLOW
    for j, what in enumerate(ENC_REFUSED):
        given[3 + j] = _spoil(st[3 + j], what, int(run.caps[3 + j]))
    run.put_states(given)
    sets_before, image_before = run.sets(), run.bytes()
    val_before, info_before = [run.values(s) for s in range(n)], [run.infos(s) for s in range(n)]
    rest = (sp[1][0], sp[1][1], sp[2][2], sp[2][3])                 # pieces 1 and 2 in one
    whole = (0, 0, sp[2][2], sp[2][3])
    res = run.launch([rest, whole] + [rest] * (n - 2), [True] * n)
    st, sets, image = run.states(), run.sets(), run.bytes()
    for s in (0, 1, n - 1):                                         # the neighbours: resumed, fresh (written from the start), resumed
        assert tuple(res[s]) == out[-1][:2], s
        assert_closed(run, st, s, out[-1][0], data, what=s)
        assert_written(run, s, good, what=s)
        assert_set(sets, s, out[-1][2], s)
    # flags from an earlier piece: {0, flags}, the state copied, nothing written
    assert tuple(res[2]) == (0, H.RES_OVERFLOW) and st[2].tobytes() == given[2].tobytes()
    for s in range(2, n - 1):
        assert np.array_equal(run.values(s), val_before[s]) and np.array_equal(run.infos(s), info_before[s]), s
        assert np.array_equal(sets[0][s], sets_before[0][s]) and np.array_equal(sets[1][s], sets_before[1][s]), s
        assert np.array_equal(run.slot(s, image=image), run.slot(s, image=image_before)), s
    assert (run.last_info[3 * 2:3 * (n - 1)] == WORD_GUARD).all()
    for j, what in enumerate(ENC_REFUSED):
        assert tuple(res[3 + j]) == (0, capi.RES_BAD_STATE), what
        assert st[3 + j].tobytes() == given[3 + j].tobytes(), what  # no state written


# ---------------------------------------------------------------------------------------------- 10. profile, workspace
def test_profile_reports_kind_51_once_per_piece(hip):
    cases, good, (out, data) = stop_case()
    own = capi.CabacHip(0)
    own.profile_enable(32)
    run = Run(own, [good])
    res = run.pieces([cases[0][1]])
    assert tuple(res[2][0]) == out[-1][:2]
    prof = own.profile_read()
    assert [k for k, _ in prof].count(51) == 3 and all(ms > 0 for k, ms in prof if k == 51)
    own.close()


def test_while_the_workspace_is_fixed_the_call_is_refused_with_nothing_queued(hip):
    cases, good, (out, data) = stop_case()
    own = capi.CabacHip(0)
    run = Run(own, [good])
    sp = R.spans_of(good, cases[0][1])
    own.workspace_fix(1, 3, 4096, 4096)
    w0 = own.workspace_waits()
    with pytest.raises(capi.CabacHipError) as e:
        run.launch([sp[0]], [False])
    assert e.value.status == -2 and "workspace is fixed" in str(e.value)
    assert own.workspace_waits() == w0
    own.synchronize()
    assert (run.slot(0) == SENT8).all() and not run.states().view(np.uint32).any() and (run.values() == VAL_GUARD).all()
    own.workspace_release()
    res = run.pieces([cases[0][1]])                                 # a good run right after
    assert tuple(res[2][0]) == out[-1][:2] and np.array_equal(run.slot(0), data)
    own.close()
