"""GPU: the fixed workspace (include/cabac_hip_workspace.h; csrc/cabac_workspace.hip and the gated kernels of cabac_splice.hip,
cabac_search_emit.hip) — the nine calls that code a slice to bytes queue their work and return; what the host used to decide after
its wait is decided on the device and reported in the status.

Expected values come from the oracle through the models under tests/ (splice_rows_model, plan_rows_model / write_plan_model,
search_emit_model), exactly as in the existing GPU tests of these calls, whose plumbing is imported.  Everything is bit-exact.  The
"no wait" is read from cabac_hip_workspace_waits between the call and the first synchronise of the test.

Shapes: five substreams, one without a block and one without a host record; blocks 4 x 4, 8 x 8, 16 x 4, 2 x 8 and one 32 x 32,
regular and transform-skip; rows: three levels of two substreams; log: three chains."""
import functools

import numpy as np
import pytest

import ctx_sets_model as CS
import helpers as H
import nal_model as NAL
import plan_rows_model as R
import search_emit_model as E
import search_unit_model as U
import splice_rows_model as M
from entropy_coding_amd import capi
from test_gpu_plan_rows import N_SETS, _write_desc, assert_row, assert_set, assert_set_guard, assert_written, parse, unit_of, write
from test_gpu_residual_estimate import dev, make_sets
from test_gpu_search import t_u32
from test_gpu_search_emit import Cands, Round, Tail, assert_log_equals, start_sets
from test_gpu_search_unit import SH, TS, Case, _block
from test_gpu_splice_rows import Form, Out, assert_coded

pytestmark = pytest.mark.gpu

NO_SET = M.NO_SET
RBSP = H.SUB_FINISH | H.SUB_ALIGN_RBSP
OVERFLOW = 1                                                        # CABAC_RES_OVERFLOW
W = capi.BIN_COUNT_WORDS


def slot_bytes(n):
    """the byte slot of a substream of n records (cabac_splice.hip: 7 bits per record, 8 bytes, rounded up to 16)"""
    return ((7 * n + 7) // 8 + 8 + 15) // 16 * 16


def needs(strings):
    """(expanded records, slot bytes) of a call, as the status reports them"""
    return sum(len(s) for s in strings), sum(slot_bytes(len(s)) for s in strings)


@pytest.fixture()
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(None)
def splice_case(rows=False):
    """rows False: five substreams; True: six in three levels of two.  -> dict(case, subs, qp, init, form)"""
    rng = np.random.default_rng(0x3A5E + int(rows))
    reg = lambda w, h, ch, fl, at: (_block(rng, w, h), ch, fl, at)
    ts = lambda w, h, ch, at: (_block(rng, w, h, "ts"), ch, TS, at)
    run = lambda n: U.side_run(rng, n)
    end = lambda r: np.concatenate([np.asarray(r, np.uint16), np.array([U.REC_TRM | 0x8000], np.uint16)])
    case = Case()
    case.add(end(run(20)), [reg(4, 4, 0, 0, 3), reg(8, 8, 1, SH, 3), ts(4, 4, 0, 9)])       # two blocks at one position
    case.add(end(run(15)), [])                                                              # no block
    case.add([], [reg(16, 4, 0, 1, 0)])                                                     # no host record
    case.add(end(run(30)), [reg(2, 8, 1, 2, 0), reg(32, 32, 0, 3, 17), ts(8, 8, 1, 30)])
    case.add(run(10), [reg(8, 8, 0, 0, 10)])                                                # a block behind the last record
    if rows:
        case.add(end(run(25)), [reg(4, 4, 1, 0, 5), reg(16, 4, 0, SH, 20)])
    case.finish()
    subs = M.subs_of(case)
    n = len(subs)
    qp, init = rng.integers(20, 45, n), rng.integers(0, 3, n)
    return dict(case=case, subs=subs, qp=qp, init=init, form=M.device_form(case, subs, qp, init), n=n,
                strings=[s.string for s in subs], info=M.tu_info(subs))


LEVELS = np.array([0, 2, 4, 6], np.uint32)
SYNC_FROM = np.array([NO_SET, NO_SET, 0, 1, 2, NO_SET], np.uint32)
SYNC_AT = np.array([4, 10 ** 6, 0, 17, 3, 0], np.uint32)


def fix_bound(hip, C, rows=False, log_records=0, n_tu=None):
    """a workspace from cabac_hip_workspace_bound for the case"""
    desc, records, first, splices, tus, coeff = C["form"]
    rec, slots = capi.workspace_bound(len(desc), len(records), len(tus), len(coeff))
    hip.workspace_fix(len(desc), len(tus) if n_tu is None else n_tu, rec, slots, rows=rows, log_records=log_records)
    return rec, slots


def queue_splice(hip, F, out, mode, kw):
    if mode == "plain":
        hip.encode_residual_device(*F.head(), *out.args(), out.t_info.data_ptr(), out.t_cnt.data_ptr(), int16=F.int16)
    elif mode == "sets":
        hip.encode_residual_sets_device(*F.head(), *out.args(), int16=F.int16, **out.tail(), **kw)
    else:
        hip.encode_residual_rows_device(*F.head(), *out.args(), LEVELS, kw["d_sync_from"], kw["d_sync_at"], 0, int16=F.int16, **out.tail())


class SpliceCall:
    """One of the four splice calls on its case: the tensors, the model's outputs, and the call queued without a synchronise."""

    def __init__(self, mode, int16=False):
        self.mode, self.C = mode, splice_case(mode == "rows")
        C = self.C
        self.F = Form(C["form"], int16)
        self.kw, self.sets = {}, None
        if mode == "plain":
            chunks, bits = M.encode_plain(C["subs"], C["qp"], C["init"])
            res = np.zeros(C["n"], H.RESULT_DTYPE)
            res["n_bits"] = bits
        elif mode == "sets":
            self.sets = make_sets(np.random.default_rng(0x5E7), 8)
            self.start, self.out_set = np.array([NO_SET, 3, 5, 5, 2], np.uint32), np.array([NO_SET, 3, 7, NO_SET, 6], np.uint32)
            chunks, res, self.written = M.encode_sets(C["subs"], C["qp"], C["init"], self.sets, self.start, self.out_set)
            assert sorted(self.written) == [3, 6, 7] and not res["flags"].any()
            self.state = np.concatenate([CS.pack(s)[0] for s in self.sets]).astype(np.uint32)
            self.rate = np.concatenate([CS.pack(s)[1] for s in self.sets]).astype(np.uint8)
            self.t_state, self.t_rate = dev(self.state, np.int32), dev(self.rate)
            self.keep = (t_u32(self.start), t_u32(self.out_set))
            self.kw = dict(n_sets=8, d_state=self.t_state.data_ptr(), d_rate=self.t_rate.data_ptr(), d_start_set=self.keep[0].data_ptr(),
                           d_out_set=self.keep[1].data_ptr(), d_out_state=self.t_state.data_ptr(), d_out_rate=self.t_rate.data_ptr())
        else:
            chunks, res, _, _ = M.encode_rows(C["subs"], C["qp"], C["init"], LEVELS, SYNC_FROM, SYNC_AT, None)
            assert not res["flags"].any()
            self.keep = (t_u32(SYNC_FROM), t_u32(SYNC_AT))
            self.kw = dict(d_sync_from=self.keep[0].data_ptr(), d_sync_at=self.keep[1].data_ptr())
        self.chunks, self.res = chunks, res
        self.total = sum(len(c) for c in chunks)
        self.needs = needs(C["strings"])

    def new_out(self):
        return Out(self.C["n"], self.F.n_tu, self.total)

    def queue(self, hip, out):
        queue_splice(hip, self.F, out, self.mode, self.kw)

    def assert_good(self, out, what):
        assert_coded(out.read(), self.chunks, self.res, self.C["info"], self.C["strings"], what)
        if self.mode == "sets":
            st, rt = self.t_state.cpu().numpy().view(np.uint32).reshape(8, -1), self.t_rate.cpu().numpy().reshape(8, -1)
            for k in range(8):
                ws, wr = CS.pack(self.written.get(k, self.sets[k]))
                assert np.array_equal(st[k], ws) and np.array_equal(rt[k], wr), (what, k)

    def assert_voided(self, out, what):
        """results all {0, OVERFLOW}, offsets all 0, no payload byte (Out.read checks the canaries and the guard words), no out set"""
        pay, off, res, info, cnt = out.read()
        assert len(pay) == 0 and not off.any(), what
        assert (res["n_bits"] == 0).all() and (res["flags"] == OVERFLOW).all(), what
        if self.mode == "sets":
            assert np.array_equal(self.t_state.cpu().numpy().view(np.uint32), self.state), what
            assert np.array_equal(self.t_rate.cpu().numpy(), self.rate), what


def status_is(hip, flags, n_calls, n_voided, first=capi.WS_NONE_VOIDED, need=None):
    st = hip.workspace_status()
    assert (int(st["flags"]), int(st["n_calls"]), int(st["n_voided"]), int(st["first_voided"])) == (flags, n_calls, n_voided, first), st
    if need is not None:
        assert (int(st["records_needed"]), int(st["slot_bytes_needed"])) == need, (st, need)
    return st


# ---------------------------------------------------------------------------------------------- 1. the nine calls, no wait
@pytest.mark.parametrize("mode,int16", [("plain", False), ("plain", True), ("sets", False), ("rows", False)])
def test_splice_calls_queue_without_a_wait_and_equal_the_model(hip, mode, int16):
    call = SpliceCall(mode, int16)
    rec, slots = fix_bound(hip, call.C, rows=mode == "rows")
    assert rec >= call.needs[0] and slots >= call.needs[1]
    out = call.new_out()
    w0 = hip.workspace_waits()
    call.queue(hip, out)
    assert hip.workspace_waits() == w0, "a fixed-mode call waited, allocated or freed"
    hip.synchronize()
    call.assert_good(out, mode)
    status_is(hip, 0, 1, 0, need=call.needs)
    # the same call on a fresh ctx without a workspace: it waits (the counter counts) and gives the same
    other = H.gpu_ctx()
    call2 = SpliceCall(mode, int16)
    out2 = call2.new_out()
    w0 = other.workspace_waits()
    call2.queue(other, out2)
    assert other.workspace_waits() >= w0 + 1
    other.synchronize()
    call2.assert_good(out2, mode + ", on demand")
    for a, b in zip(out.read(), out2.read()):
        assert np.array_equal(a, b)
    other.close()


@functools.lru_cache(None)
def plan_batch():
    """two pictures of three rows in level order, every row written from its link"""
    rows, level_first, sync_from, sync_at = R.batch(0x9B07, n_pic=2, n_row=3)
    written, ok = R.rows(rows, level_first, sync_from, sync_at)
    assert all(ok) and len(rows) == 6
    alone, _ = R.rows(rows, [0, len(rows)], [NO_SET] * len(rows), [0] * len(rows))
    return rows, (level_first, sync_from, sync_at), written, alone


def plan_needs(written):
    return needs([w["string"] for w in written])


def fix_plan(hip, rows, rows_flag=False, rec=None, slots=None):
    P = R.pack(rows)
    n_bins = 320 * len(P["plan"])                                   # no element gives more than 255 context bins and a 64-bin code word
    b_rec, b_slots = capi.workspace_bound(len(rows), n_bins, P["n_tu"], len(P["coeff"]))
    hip.workspace_fix(len(rows), P["n_tu"], b_rec if rec is None else rec, b_slots if slots is None else slots, n_entries=len(P["plan"]),
                      rows=rows_flag)
    return b_rec, b_slots


@pytest.mark.parametrize("entry", ["plain", "sets", "rows"])
def test_plan_write_calls_queue_without_a_wait_and_equal_the_model(hip, entry):
    """test_gpu_plan_rows.write queues the call and synchronises ONCE itself: that one wait is all the counter may show."""
    rows, links, linked, alone = plan_batch()
    n = len(rows)
    b_rec, b_slots = fix_plan(hip, rows, rows_flag=entry == "rows")
    kw = dict(links=links) if entry == "rows" else dict(start=[NO_SET] * n, out_set=list(range(n))) if entry == "sets" else {}
    want = linked if entry == "rows" else alone
    assert b_rec >= plan_needs(want)[0] and b_slots >= plan_needs(want)[1]
    w0 = hip.workspace_waits()
    r = write(hip, rows, entry=entry, **kw)
    assert hip.workspace_waits() == w0 + 1, "more than the helper's own synchronise"
    for s, w in enumerate(want):
        assert_written(r, s, w, entry)
        if entry == "sets":
            assert_set(r["sets"], s, w["left"], s)
    status_is(hip, 0, 1, 0, need=plan_needs(want))
    other = H.gpu_ctx()
    w0 = other.workspace_waits()
    r2 = write(other, rows, entry=entry, **kw)
    assert other.workspace_waits() >= w0 + 2
    for key in ("raw", "offsets", "res", "all_values", "info"):
        assert np.array_equal(r[key], r2[key]), key
    other.close()


class LogCase:
    """A log of three chains on `hip` and its model: `n_round` positions appended (the first alternative of every group wins), then
    the terminate record of every chain."""

    K = 3

    def __init__(self, hip, n_round=2, tu_capacity=None, record_capacity=4096, seed=0x10C7):
        rng = np.random.default_rng(seed)
        K = self.K
        self.qp, self.init = rng.integers(20, 45, K), rng.integers(0, 3, K)
        self.model = M.MarkedLog(K)
        rounds = [E.search_round(rng, K, 3) for _ in range(n_round)]
        n_tu = sum(int(c.cand_first[int(g) + 1] - c.cand_first[int(g)]) for c, gf, _ in rounds for g in gf[:-1])
        self.tu_cap = n_tu if tu_capacity is None else tu_capacity
        self.rec_cap = record_capacity
        self.log = hip.search_log(K, (n_round + 1) * K + 1, record_capacity, self.tu_cap, max(self.tu_cap, 1) * 1024)
        self.t_chain = t_u32(np.arange(K, dtype=np.uint32))
        self.keep = []
        chain = np.arange(K, dtype=np.uint32)
        for r, (case, gf, _) in enumerate(rounds):
            cands, pick = Cands.of(case), gf[:-1].copy()
            t_pick = t_u32(pick)
            self.keep += [cands, t_pick]
            cands.append(self.log, t_pick, self.t_chain, K)
            assert cands.model_append(self.model, pick, chain)
            if r == 0:
                self.log.search_log_mark_device(K, self.t_chain.data_ptr())
                self.model.mark(chain)
        tail = Tail(K)
        self.keep.append(tail)
        tail.cands.append(self.log, tail.t_pick, self.t_chain, K)
        assert tail.cands.model_append(self.model, tail.pick, chain)
        self.n_tu = len(self.model.log.tu)
        assert self.n_tu == n_tu and self.n_tu <= self.tu_cap
        self.subs = self.model.subs()
        self.strings, self.info = [s.string for s in self.subs], self.model.info()
        desc = np.zeros(K, H.DESC_DTYPE)
        desc["qp"], desc["init_id"] = self.qp, np.asarray(self.init, np.uint32) | RBSP
        self.t_desc = dev(desc, np.uint8)
        self.level_first, self.sync_from = np.array([0, 1, 2, 3], np.uint32), np.array([NO_SET, 0, 1], np.uint32)
        self.t_from = t_u32(self.sync_from)

    def want(self, mode):
        if mode == "rows":
            chunks, res, _, _ = self.model.encode_rows(self.qp, self.init, self.level_first, self.sync_from)
        else:
            chunks, bits = M.encode_plain(self.subs, self.qp, self.init)
            res = np.zeros(self.K, H.RESULT_DTYPE)
            res["n_bits"] = bits
        assert not res["flags"].any()
        return chunks, res

    def fix(self, hip, rows=False, rec=None, slots=None):
        n_rec = sum(len(s.side) for s in self.subs)
        n_coeff = sum(E.block_size(d) for d in self.model.log.tu)
        b_rec, b_slots = capi.workspace_bound(self.K, n_rec, self.n_tu, n_coeff)
        hip.workspace_fix(self.K, self.tu_cap, b_rec if rec is None else rec, b_slots if slots is None else slots,
                          log_records=self.rec_cap, rows=rows)
        return b_rec, b_slots

    def new_out(self, total):
        return Out(self.K, self.n_tu, total)

    def queue(self, mode, out):
        if mode == "plain":
            self.log.encode_device(self.t_desc.data_ptr(), *out.args(), **out.tail())
        elif mode == "sets":
            self.log.search_log_encode_sets_device(self.t_desc.data_ptr(), *out.args(), **out.tail())
        else:
            self.log.search_log_encode_rows_device(self.t_desc.data_ptr(), *out.args(), self.level_first, self.t_from.data_ptr(), **out.tail())


@pytest.mark.parametrize("mode", ["plain", "sets", "rows"])
def test_log_emit_calls_queue_without_a_wait_and_equal_the_model(hip, mode):
    L = LogCase(hip)
    chunks, res = L.want(mode)
    b_rec, b_slots = L.fix(hip, rows=mode == "rows")
    assert b_rec >= needs(L.strings)[0] and b_slots >= needs(L.strings)[1]
    out = L.new_out(sum(len(c) for c in chunks))
    w0 = hip.workspace_waits()
    L.queue(mode, out)
    assert hip.workspace_waits() == w0, "a fixed-mode emit waited, allocated or freed"
    hip.synchronize()
    assert_coded(out.read(), chunks, res, L.info, L.strings, "log " + mode)
    status_is(hip, 0, 1, 0, need=needs(L.strings))
    hip.workspace_release()
    out2 = L.new_out(sum(len(c) for c in chunks))
    w0 = hip.workspace_waits()
    L.queue(mode, out2)                                             # on demand again: the emit waits for the counters and in the middle
    assert hip.workspace_waits() >= w0 + 2
    hip.synchronize()
    for a, b in zip(out.read(), out2.read()):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- 2. exact fit, one less, repeat
def test_splice_exact_fit_one_record_or_one_byte_less_voids_and_the_repeat_is_good(hip):
    call = SpliceCall("sets")
    C, (rec, slots) = call.C, call.needs
    n, n_tu = C["n"], call.F.n_tu
    out = call.new_out()                                            # the SAME arrays in every call below
    hip.workspace_fix(n, n_tu, rec, slots)
    call.queue(hip, out)
    hip.synchronize()
    call.assert_good(out, "exact fit")
    status_is(hip, 0, 1, 0, need=call.needs)
    call = SpliceCall("sets")                                       # the sets again as they were (the good call wrote out sets)
    for k, (r, s, flag) in enumerate([(rec - 1, slots, capi.WS_OVER_RECORDS), (rec, slots - 1, capi.WS_OVER_SLOTS)]):
        out = call.new_out()
        hip.workspace_fix(n, n_tu, r, s)
        w0 = hip.workspace_waits()
        call.queue(hip, out)
        assert hip.workspace_waits() == w0
        hip.synchronize()
        call.assert_voided(out, "one less (%d)" % k)
        status_is(hip, flag, 1, 1, first=0, need=call.needs)
    st = hip.workspace_status()
    hip.workspace_fix(n, n_tu, int(st["records_needed"]), int(st["slot_bytes_needed"]))
    call.queue(hip, out)                                            # the arrays of the voided call
    hip.synchronize()
    call.assert_good(out, "repeated")
    status_is(hip, 0, 1, 0, need=call.needs)


def test_plan_write_exact_fit_one_less_voids_also_with_values_in_place_and_the_repeat_is_good(hip):
    rows, links, linked, alone = plan_batch()
    n = len(rows)
    rec, slots = plan_needs(alone)
    kw = dict(entry="sets", start=[NO_SET] * n, out_set=list(range(n)))
    fix_plan(hip, rows, rec=rec, slots=slots)
    r = write(hip, rows, **kw)
    for s, w in enumerate(alone):
        assert_written(r, s, w, "exact fit")
    status_is(hip, 0, 1, 0, need=(rec, slots))
    for k, (a, b, flag) in enumerate([(rec - 1, slots, capi.WS_OVER_RECORDS), (rec, slots - 1, capi.WS_OVER_SLOTS)]):
        fix_plan(hip, rows, rec=a, slots=b)
        r = write(hip, rows, **kw)                                  # its guards: nothing outside any array, no byte behind offsets[n] = 0
        assert not r["offsets"].any() and len(r["raw"]) == 0
        assert (r["res"]["n_bits"] == 0).all() and (r["res"]["flags"] == OVERFLOW).all()
        assert (r["all_values"] == r["all_values"][0]).all() and int(r["all_values"][0]) not in (0, 1), "a values_out word was written"
        for s in range(N_SETS):
            assert_set_guard(r["sets"], s, "voided")
        status_is(hip, flag, 1, 1, first=0, need=(rec, slots))
    # d_values_out == d_values_in: a voided call leaves the values as the caller gave them, so that the call can be repeated
    import torch
    P = R.pack(rows)
    t_desc, t_first = dev(_write_desc(P), np.uint8), dev(P["tile_first"].view(np.int32))
    t_plan, t_val = dev(P["plan"].reshape(-1).view(np.int32)), dev(P["values_in"].view(np.int32))
    t_co, t_tu = dev(P["coeff"]), dev(P["tus"], np.uint8)
    t_at, t_gd = dev(P["tu_at"].view(np.int32)), dev(P["tu_guard"].view(np.int32))
    t_pay = torch.full((1 << 14,), 0xA5, dtype=torch.uint8, device="cuda")
    t_off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    t_res = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")

    def call():
        hip.write_plan_device(n, t_desc.data_ptr(), t_plan.data_ptr(), t_val.data_ptr(), t_first.data_ptr(), P["n_tu"], t_tu.data_ptr(),
                              t_at.data_ptr(), t_gd.data_ptr(), t_co.data_ptr(), t_pay.data_ptr(), 1 << 14, t_off.data_ptr(), t_res.data_ptr(),
                              d_values_out=t_val.data_ptr())
        hip.synchronize()
        return t_off.cpu().numpy(), t_res.cpu().numpy().view(H.RESULT_DTYPE), t_pay.cpu().numpy(), t_val.cpu().numpy().view(np.uint32)

    off, res, pay, val = call()                                     # the workspace of the last voided call: one slot byte short
    assert not off.any() and (res["flags"] == OVERFLOW).all() and (pay == 0xA5).all()
    assert np.array_equal(val, P["values_in"].view(np.uint32))
    st = status_is(hip, capi.WS_OVER_SLOTS, 2, 2, first=0, need=(rec, slots))
    fix_plan(hip, rows, rec=int(st["records_needed"]), slots=int(st["slot_bytes_needed"]))
    off, res, pay, val = call()                                     # the same arrays
    for s, w in enumerate(alone):
        assert (int(res["n_bits"][s]), int(res["flags"][s])) == (w["n_bits"], 0), s
        assert np.array_equal(pay[int(off[s]):int(off[s + 1])], w["data"]), s
        r0 = int(P["desc"]["rec_offset"][s])
        assert val[r0:r0 + len(w["values"])].tolist() == w["values"], s
    status_is(hip, 0, 1, 0, need=(rec, slots))


def test_log_emit_exact_fit_one_less_voids_and_the_repeat_is_good(hip):
    L = LogCase(hip)
    chunks, res = L.want("rows")
    rec, slots = needs(L.strings)
    out = L.new_out(sum(len(c) for c in chunks))
    for k, (a, b, flag) in enumerate([(rec - 1, slots, capi.WS_OVER_RECORDS), (rec, slots - 1, capi.WS_OVER_SLOTS)]):
        L.fix(hip, rows=True, rec=a, slots=b)
        L.queue("rows", out)
        hip.synchronize()
        pay, off, gres, info, cnt = out.read()
        assert len(pay) == 0 and not off.any() and (gres["n_bits"] == 0).all() and (gres["flags"] == OVERFLOW).all(), k
        status_is(hip, flag, 1, 1, first=0, need=(rec, slots))
    assert_log_equals(L.log, L.model.log, "a voided emit writes nothing to the log")
    L.fix(hip, rows=True, rec=rec, slots=slots)
    L.queue("rows", out)                                            # the same arrays
    hip.synchronize()
    assert_coded(out.read(), chunks, res, L.info, L.strings, "exact fit after two voided calls")
    status_is(hip, 0, 1, 0, need=(rec, slots))


# ---------------------------------------------------------------------------------------------- 3. conditions found on the device
def test_bad_splice_lists_and_an_overflowed_log_void_the_call_without_a_host_error(hip):
    call = SpliceCall("plain")
    C = call.C
    desc, records, first, splices, tus, coeff = C["form"]
    fix_bound(hip, C)
    unsorted = splices.copy()
    j = int(first[3])
    assert unsorted["at"][j] != unsorted["at"][j + 1]
    unsorted["at"][j], unsorted["at"][j + 1] = unsorted["at"][j + 1], unsorted["at"][j]
    twice = splices.copy()
    twice["tu"][1] = twice["tu"][0]
    for k, bad in enumerate((unsorted, twice)):
        F = Form((desc, records, first, bad, tus, coeff))
        out = call.new_out()
        w0 = hip.workspace_waits()
        queue_splice(hip, F, out, "plain", {})                      # returns CABAC_HIP_OK: it cannot know
        assert hip.workspace_waits() == w0
        hip.synchronize()
        call.assert_voided(out, "bad list %d" % k)
        status_is(hip, capi.WS_BAD_SPLICES, k + 1, k + 1, first=0, need=(0, 0))
    out = call.new_out()
    call.queue(hip, out)                                            # and a good call right behind them
    hip.synchronize()
    call.assert_good(out, "after the bad lists")
    status_is(hip, capi.WS_BAD_SPLICES, 3, 2, first=0, need=call.needs)
    # a log whose append was dropped for capacity
    L = LogCase(hip, record_capacity=400)
    big = Case()
    big.add(U.side_run(np.random.default_rng(5), 600), [])
    big.finish()
    cb = Cands.of(big)
    t_pick, t_chain = t_u32([0]), t_u32([1])
    cb.append(L.log, t_pick, t_chain, 1)
    L.fix(hip)
    out = L.new_out(4096)
    L.queue("plain", out)
    hip.synchronize()
    pay, off, gres, info, cnt = out.read()
    assert len(pay) == 0 and not off.any() and (gres["flags"] == OVERFLOW).all() and (gres["n_bits"] == 0).all()
    status_is(hip, capi.WS_LOG_OVERFLOW, 1, 1, first=0, need=(0, 0))


# ---------------------------------------------------------------------------------------------- 4. capacity far above content
def test_log_with_far_more_capacity_than_content(hip):
    """tu_capacity 64: with the blocks of one position logged, then (after a reset) with none — every chain codes its bare end"""
    L = LogCase(hip, n_round=1, tu_capacity=64)
    assert 0 < L.n_tu <= 6
    for mode in ("plain", "rows"):
        chunks, res = L.want(mode)
        L.fix(hip, rows=mode == "rows")
        out = L.new_out(sum(len(c) for c in chunks))
        w0 = hip.workspace_waits()
        L.queue(mode, out)
        assert hip.workspace_waits() == w0
        hip.synchronize()
        assert_coded(out.read(), chunks, res, L.info, L.strings, "capacity 64, " + mode)
        status_is(hip, 0, 1, 0, need=needs(L.strings))
    L.log.reset()
    L.model.reset()
    tail = Tail(L.K)
    tail.cands.append(L.log, tail.t_pick, L.t_chain, L.K)
    assert tail.cands.model_append(L.model, tail.pick, np.arange(L.K, dtype=np.uint32))
    subs = L.model.subs()
    strings = [s.string for s in subs]
    assert [len(s) for s in strings] == [1, 1, 1]
    chunks, bits = M.encode_plain(subs, L.qp, L.init)
    res = np.zeros(L.K, H.RESULT_DTYPE)
    res["n_bits"] = bits
    out = Out(L.K, 0, sum(len(c) for c in chunks))
    L.queue("rows", out)                                            # unmarked after the reset, linked: the starts are inits advanced by nothing
    hip.synchronize()
    chunks_r, res_r, _, _ = L.model.encode_rows(L.qp, L.init, L.level_first, L.sync_from)
    assert_coded(out.read(), chunks_r, res_r, np.zeros(0, np.uint32), strings, "no block logged")
    status_is(hip, 0, 2, 0, need=needs(L.strings))


# ---------------------------------------------------------------------------------------------- 5. host-known overruns
def test_host_known_overruns_are_refused_with_nothing_queued(hip):
    call = SpliceCall("rows")
    C = call.C
    desc, records, first, splices, tus, coeff = C["form"]
    rec, slots = capi.workspace_bound(len(desc), len(records), len(tus), len(coeff))
    out = call.new_out()

    def refused(word):
        w0 = hip.workspace_waits()
        with pytest.raises(capi.CabacHipError) as e:
            call.queue(hip, out)
        assert e.value.status == -2 and word in str(e.value), str(e.value)
        assert hip.workspace_waits() == w0
        hip.synchronize()
        assert (out.t_pay.cpu().numpy() == 0xEE).all() and (out.t_off.cpu().numpy() == -1).all() and (out.t_res.cpu().numpy() == -1).all()
        assert (out.t_info.cpu().numpy() == -1).all() and (out.t_cnt.cpu().numpy() == -1).all()

    hip.workspace_fix(len(desc) - 1, len(tus), rec, slots, rows=True)
    refused("n_sub")
    hip.workspace_fix(len(desc), len(tus) - 1, rec, slots, rows=True)
    refused("n_tu")
    hip.workspace_fix(len(desc), len(tus), rec, slots)
    refused("CABAC_WS_ROWS")
    status_is(hip, 0, 0, 0, need=(0, 0))
    hip.workspace_fix(len(desc), len(tus), rec, slots, rows=True)
    call.queue(hip, out)                                            # a good call right after
    hip.synchronize()
    call.assert_good(out, "after the refusals")
    # the log's capacities are host-known too
    L = LogCase(hip)
    hip.workspace_fix(L.K, L.tu_cap, rec, slots, log_records=L.rec_cap - 1)
    lo = L.new_out(64)
    with pytest.raises(capi.CabacHipError) as e:
        L.queue("plain", lo)
    assert e.value.status == -2 and "record_capacity" in str(e.value)
    hip.workspace_fix(L.K, L.tu_cap - 1, rec, slots, log_records=L.rec_cap)
    with pytest.raises(capi.CabacHipError) as e:
        L.queue("plain", lo)
    assert e.value.status == -2 and "n_tu" in str(e.value)
    hip.synchronize()
    assert (lo.t_pay.cpu().numpy() == 0xEE).all() and (lo.t_off.cpu().numpy() == -1).all()


# ---------------------------------------------------------------------------------------------- 6. back to back; a whole chain
def test_two_different_calls_back_to_back_then_one_synchronise(hip):
    a, b = SpliceCall("rows"), SpliceCall("plain")
    rows, links, linked, alone = plan_batch()
    desc, records, first, splices, tus, coeff = a.C["form"]
    P = R.pack(rows)
    rec_a, slots_a = capi.workspace_bound(len(desc), len(records), len(tus), len(coeff))
    rec_p, slots_p = capi.workspace_bound(len(rows), 320 * len(P["plan"]), P["n_tu"], len(P["coeff"]))
    hip.workspace_fix(max(len(desc), len(rows)), max(len(tus), P["n_tu"]), max(rec_a, rec_p), max(slots_a, slots_p), rows=True)
    oa, ob = a.new_out(), b.new_out()
    w0 = hip.workspace_waits()
    a.queue(hip, oa)
    b.queue(hip, ob)                                                # the second call's kernels reuse the buffers behind the first's
    assert hip.workspace_waits() == w0
    r = write(hip, rows, entry="rows", links=links)                 # a plan write behind both; its helper synchronises
    assert hip.workspace_waits() == w0 + 1
    a.assert_good(oa, "first of three")
    b.assert_good(ob, "second of three")
    for s, w in enumerate(linked):
        assert_written(r, s, w, "third of three")
    status_is(hip, 0, 3, 0)


def test_a_whole_chain_with_one_synchronise_at_its_end(hip):
    """Search unit rounds, the log's appends and a mark, the emit in rows, the escape of the payload: queued twice over.  The first
    pass lets the scratch of the rounds, the append and the escape — which is not part of the fixed workspace — grow; across the
    second pass, from its first search round to the escaped NAL payload, the counter does not move."""
    import torch
    rng = np.random.default_rng(0xC4A1)
    K, lam = 2, int(1.3 * (1 << 16))
    qp, init = rng.integers(22, 40, K), rng.integers(0, 3, K)
    protos = []
    for t in range(3):
        case, gf, which = E.search_round(rng, K, 4)
        protos.append((case, gf, which, rng.integers(0, 3000, case.n_cand).astype(np.uint64)))
    t_chain, t_mark, t_from = t_u32(np.arange(K, dtype=np.uint32)), t_u32([0]), t_u32([NO_SET, 0])
    desc = np.zeros(K, H.DESC_DTYPE)
    desc["qp"], desc["init_id"] = qp, np.asarray(init, np.uint32) | RBSP
    t_desc = dev(desc, np.uint8)
    log = hip.search_log(K, 16, 4096, 32, 32 * 256)
    rec, slots = capi.workspace_bound(K, 4096, 32, 32 * 256)
    hip.workspace_fix(K, 32, rec, slots, log_records=4096, rows=True)
    cap = 1 << 14
    ncap = NAL.escape_bound(cap)
    n = H.NUM_CTX
    passes = []
    for p in range(2):
        steps = [Round(*pr, K) for pr in protos]                    # torch allocates here, before the pass is queued
        tail = Tail(K)
        out = Out(K, 32, cap - 64)
        t_nal = torch.full((ncap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        t_noff = torch.full((K + 1,), -1, dtype=torch.int64, device="cuda")
        t_st = torch.zeros(16, dtype=torch.uint8, device="cuda")
        t_ws = torch.zeros(32, dtype=torch.uint8, device="cuda")
        t_state, t_rate, sets, keep = start_sets(hip, qp, init)
        log.reset()
        w0 = hip.workspace_waits()
        for t, rd in enumerate(steps):
            rd.enqueue(hip, log, t_state, t_rate, t_chain, lam)
            if t == 0:
                log.search_log_mark_device(1, t_mark.data_ptr())
                t_state[n:2 * n] = t_state[:n]
                t_rate[n:2 * n] = t_rate[:n]
        tail.cands.append(log, tail.t_pick, t_chain, K)
        log.search_log_encode_rows_device(t_desc.data_ptr(), *out.args(), [0, 1, 2], t_from.data_ptr(), **out.tail())
        hip.nal_escape_device(K, out.t_off.data_ptr(), out.t_pay.data_ptr(), cap, t_nal.data_ptr(), ncap, t_noff.data_ptr(), t_st.data_ptr())
        hip.workspace_status_device(t_ws.data_ptr())
        waits = hip.workspace_waits() - w0
        hip.synchronize()                                           # the one synchronisation, at the end
        passes.append((steps, tail, out, t_nal, t_noff, t_st, t_ws, sets, waits, keep))
    assert passes[1][8] == 0, "the second pass waited, allocated or freed %d times" % passes[1][8]
    for p, (steps, tail, out, t_nal, t_noff, t_st, t_ws, sets, waits, keep) in enumerate(passes):
        model = M.MarkedLog(K)
        for t, rd in enumerate(steps):
            sets = rd.model(model, sets, lam)
            if t == 0:
                model.mark([0])
                sets[1] = sets[0]
        assert tail.cands.model_append(model, tail.pick, np.arange(K, dtype=np.uint32))
        subs = model.subs()
        chunks, res, idx, _ = model.encode_rows(qp, init, [0, 1, 2], [NO_SET, 0])
        assert not res["flags"].any()
        out.n_tu = len(model.log.tu)
        got = out.read()
        assert_coded(got, chunks, res, model.info(), [s.string for s in subs], "chain, pass %d" % p)
        w_nal, w_off, w_st = NAL.escape(got[1], got[0], capacity=ncap, bytes_max=cap)
        nal = t_nal.cpu().numpy()
        assert np.array_equal(nal[:len(w_nal)], w_nal) and (nal[len(w_nal):] == 0xEE).all()
        assert np.array_equal(t_noff.cpu().numpy().view(np.uint64), w_off)
        st = t_ws.cpu().numpy().view(capi.WORKSPACE_STATUS_DTYPE)[0]  # stream-ordered: it reflects the emit queued in front of it
        assert (int(st["n_calls"]), int(st["n_voided"]), int(st["flags"]), int(st["first_voided"])) == (p + 1, 0, 0, capi.WS_NONE_VOIDED)
        assert (int(st["records_needed"]), int(st["slot_bytes_needed"])) == needs([s.string for s in subs])
    status_is(hip, 0, 2, 0)
    log.close()


# ---------------------------------------------------------------------------------------------- 7. release; the other entry points
def test_release_puts_the_ctx_back_on_the_on_demand_path_and_batch_forms_are_refused_while_fixed(hip):
    call = SpliceCall("plain")
    C = call.C
    desc, records, first, splices, tus, coeff = C["form"]
    rows, links, linked, alone = plan_batch()
    P = R.pack(rows)
    fix_bound(hip, C, rows=True)
    out = call.new_out()
    call.queue(hip, out)
    hip.synchronize()
    call.assert_good(out, "fixed")
    payload = np.full(1 << 16, 0xEE, np.uint8)
    lv, sf, sa = [0, C["n"]], np.full(C["n"], NO_SET, np.uint32), np.zeros(C["n"], np.uint32)
    batches = [lambda: hip.encode_batch_residual(desc, records, first, splices, tus, coeff, payload),
               lambda: hip.encode_batch_residual(desc, records, first, splices, tus, coeff.astype(np.int16), payload),
               lambda: hip.encode_residual_rows_batch(desc, records, first, splices, tus, coeff, payload, lv, sf, sa, None),
               lambda: hip.write_plan_batch(_write_desc(P), P["plan"], P["values_in"], P["tile_first"], P["tus"][:P["n_tu"]], P["tu_at"],
                                            P["tu_guard"], P["coeff"], payload),
               lambda: hip.plan_write_rows_batch(_write_desc(P), P["plan"], P["values_in"], P["tile_first"], P["tus"][:P["n_tu"]],
                                                 P["tu_at"], P["tu_guard"], P["coeff"], payload, *links)]
    for k, f in enumerate(batches):
        with pytest.raises(capi.CabacHipError) as e:
            f()
        assert e.value.status == -2 and "cabac_hip_workspace_release" in str(e.value), (k, str(e.value))
        assert (payload == 0xEE).all()
    # the entry points outside the nine run unchanged on a fixed ctx: the bin codec, the plan parse, an estimate
    sub = C["subs"][0]
    d1, total1 = H.make_desc([len(sub.string)], [int(C["qp"][0])], [int(C["init"][0])], RBSP)
    got, res1 = hip.encode_batch(d1, sub.string, total1)
    chunks, bits = M.encode_plain(C["subs"][:1], C["qp"], C["init"])
    assert int(res1["n_bits"][0]) == int(bits[0]) and np.array_equal(got[:len(chunks[0])], chunks[0])
    t_d1, t_r1 = dev(d1, np.uint8), dev(sub.string.astype(np.uint16), np.int16)
    import torch
    t_b1 = torch.zeros(total1 + 16, dtype=torch.uint8, device="cuda")
    t_res1 = torch.zeros(2, dtype=torch.int32, device="cuda")
    hip.encode_device(1, t_d1.data_ptr(), t_r1.data_ptr(), t_b1.data_ptr(), t_res1.data_ptr())
    hip.synchronize()
    assert np.array_equal(t_b1.cpu().numpy()[:len(chunks[0])], chunks[0])
    bits_est, _ = hip.estimate_batch(d1, sub.string)
    assert int(bits_est[0]) == H.load_oracle().estimate_records(sub.string, int(C["qp"][0]), int(C["init"][0]))[1]
    units = [unit_of(r, w) for r, w in zip(rows, alone)]
    pr = parse(hip, units, entry="sets")
    for s, (row, w) in enumerate(zip(rows, alone)):
        assert_row(pr, s, row, w, "plan parse on a fixed ctx")
    st = status_is(hip, 0, 1, 0, need=call.needs)
    # release: the same call waits again, with the same result; the batch forms work; the status is what the release found
    hip.workspace_release()
    out2 = call.new_out()
    w0 = hip.workspace_waits()
    call.queue(hip, out2)
    assert hip.workspace_waits() >= w0 + 1
    hip.synchronize()
    for a, b in zip(out.read(), out2.read()):
        assert np.array_equal(a, b)
    offs, hres = hip.encode_batch_residual(desc, records, first, splices, tus, coeff, payload)
    assert np.array_equal(hres, call.res)
    for s in range(C["n"]):
        assert np.array_equal(payload[int(offs[s]):int(offs[s + 1])], call.chunks[s]), s
    assert hip.workspace_status() == st
    with pytest.raises(capi.CabacHipError):
        hip.workspace_status_device(out.t_off.data_ptr())           # not fixed
