"""GPU: the splice pipeline and the winner log's emit from and into context sets and in WPP rows
(include/cabac_hip_splice_rows.h; csrc/cabac_splice.hip, csrc/cabac_search_emit.hip) against tests/splice_rows_model.py, which
tests/test_splice_rows_model.py pins to the parts it is composed of.  Everything is bit-exact: == on integers, no tolerance.  Every
output sits between guard words that are checked; every test has its own bounded input."""
import functools

import numpy as np
import pytest

import ctx_sets_model as CS
import helpers as H
import search_emit_model as E
import search_unit_model as U
import splice_rows_model as M
from entropy_coding_amd import capi
from test_gpu_residual_estimate import dev, make_sets
from test_gpu_search import t_u32
from test_gpu_search_emit import Cands, Round, Tail, append_both, assert_emitted, assert_log_equals, encode_log, start_sets
from test_gpu_search_unit import Case, t_rec

pytestmark = pytest.mark.gpu

NO_SET = M.NO_SET
RBSP = H.SUB_FINISH | H.SUB_ALIGN_RBSP
SEED = 0x5B11CE
W = capi.BIN_COUNT_WORDS


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------- plumbing
class Form:
    """The arguments of the spliced calls on the device."""

    def __init__(self, form, int16=False):
        import torch
        self.desc, self.records, self.first, self.splices, self.tus, self.coeff = form
        self.n_sub, self.n_tu, self.int16 = len(self.desc), len(self.tus), int16
        if int16:
            assert np.abs(self.coeff).max() <= 32767
        self.t_desc, self.t_rec, self.t_first = dev(self.desc, np.uint8), t_rec(self.records), t_u32(self.first)
        self.t_sp = dev(self.splices, np.uint8) if self.n_tu else None
        self.t_tu = dev(self.tus, np.uint8) if self.n_tu else None
        self.t_co = dev(np.asarray(self.coeff).astype(np.int16 if int16 else np.int32)) if self.n_tu else torch.zeros(8, dtype=torch.int32, device="cuda")

    def head(self):
        p = lambda t: t.data_ptr() if t is not None else 0
        return (self.n_sub, p(self.t_desc), p(self.t_rec), p(self.t_first), p(self.t_sp), self.n_tu, self.n_tu, p(self.t_tu),
                p(self.t_co) if self.n_tu else 0)


class Out:
    """payload, offsets, results, tu_info and bin counts between guard words"""

    def __init__(self, n_sub, n_tu, total):
        import torch
        self.n_sub, self.n_tu, self.total = n_sub, n_tu, total
        self.t_pay = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        self.t_off = torch.full((n_sub + 2,), -1, dtype=torch.int64, device="cuda")
        self.t_res = torch.full((2 * n_sub + 2,), -1, dtype=torch.int32, device="cuda")
        self.t_info = torch.full((n_tu + 2,), -1, dtype=torch.int32, device="cuda")
        self.t_cnt = torch.full((n_sub * W + 1,), -1, dtype=torch.int32, device="cuda")

    def args(self):
        return (self.t_pay.data_ptr(), self.total + 64, self.t_off.data_ptr(), self.t_res.data_ptr())

    def tail(self):
        return dict(d_tu_info=self.t_info.data_ptr(), d_bin_counts=self.t_cnt.data_ptr())

    def read(self):
        K, n_tu = self.n_sub, self.n_tu
        off, res, info, cnt = self.t_off.cpu().numpy(), self.t_res.cpu().numpy(), self.t_info.cpu().numpy(), self.t_cnt.cpu().numpy()
        assert off[-1] == -1 and (res[-2:] == -1).all() and (info[n_tu:] == -1).all() and cnt[-1] == -1   # nothing behind the outputs
        pay = self.t_pay.cpu().numpy()
        n = int(off[K])
        assert n <= self.total and (pay[n:] == 0xEE).all()
        return (pay[:n], off[:K + 1].view(np.uint64), res[:2 * K].view(H.RESULT_DTYPE), info[:n_tu].view(np.uint32),
                cnt[:-1].view(np.uint32).reshape(K, W))


def run(hip, F, total, mode="plain", **kw):
    """One device call -> (payload, offsets, results, tu_info, counts).  mode plain / sets / rows."""
    out = Out(F.n_sub, F.n_tu, total)
    if mode == "plain":
        hip.encode_residual_device(*F.head(), *out.args(), out.t_info.data_ptr(), out.t_cnt.data_ptr(), int16=F.int16)
    elif mode == "sets":
        hip.encode_residual_sets_device(*F.head(), *out.args(), int16=F.int16, **out.tail(), **kw)
    else:
        hip.encode_residual_rows_device(*F.head(), *out.args(), kw["level_first"], kw["d_sync_from"], kw["d_sync_at"],
                                        kw.get("d_sync_splice", 0), int16=F.int16, **out.tail())
    hip.synchronize()
    return out.read()


def assert_coded(got, chunks, res, info, strings, what="", skip=()):
    """the device's outputs against the model's chunks (one per substream), results, info words and — but for the substreams in
    `skip`, which code nothing — the bin counts of the expanded strings"""
    pay, off, gres, ginfo, cnt = got
    w_pay, w_off = M.payload_of(chunks)
    assert np.array_equal(gres, res), (what, gres, res)
    assert np.array_equal(off, w_off), (what, off, w_off)
    assert np.array_equal(pay, w_pay), (what, np.nonzero(pay != w_pay)[0][:8])
    assert np.array_equal(ginfo, info), what
    for s, string in enumerate(strings):
        if s not in skip:
            assert np.array_equal(cnt[s], E.counts_of(string)), (what, s)


@functools.lru_cache(None)
def rows_case():
    B = M.rows_batch(SEED)
    n = len(B["subs"])
    rng = np.random.default_rng(77)
    qp, init = rng.integers(20, 45, n), rng.integers(0, 3, n)
    return B, qp, init, M.device_form(B["case"], B["subs"], qp, init)


# ---------------------------------------------------------------------------------------------- (a) identity
@pytest.mark.parametrize("int16", [False, True])
def test_no_sets_and_one_level_are_the_plain_call(hip, int16):
    B, qp, init, form = rows_case()
    subs, n = B["subs"], len(B["subs"])
    F = Form(form, int16)
    want, want_bits = M.encode_plain(subs, qp, init)
    total = sum(len(w) for w in want)
    plain = run(hip, F, total)
    res = np.zeros(n, H.RESULT_DTYPE)
    res["n_bits"] = want_bits
    assert_coded(plain, want, res, M.tu_info(subs), [s.string for s in subs], "plain")
    sets = run(hip, F, total, "sets")                                                       # no sets at all
    t_none = t_u32(np.full(n, NO_SET, np.uint32))
    sets2 = run(hip, F, total, "sets", n_sets=0, d_start_set=t_none.data_ptr())             # every start "no set"
    t_at, t_sp = t_u32(B["sync_at"]), t_u32(B["splice"]["lower"])
    rows = run(hip, F, total, "rows", level_first=[0, n], d_sync_from=t_none.data_ptr(), d_sync_at=t_at.data_ptr(),
               d_sync_splice=t_sp.data_ptr())
    rows2 = run(hip, F, total, "rows", level_first=[0, n], d_sync_from=t_none.data_ptr(), d_sync_at=t_at.data_ptr())
    for other in (sets, sets2, rows, rows2):
        for a, b in zip(plain, other):
            assert a.dtype == b.dtype and np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- (b) sets
def test_sets_mixed_starts_in_place_bad_indices_and_an_empty_substream(hip):
    import torch
    rng = np.random.default_rng(0x5E75)
    N_SETS = 16
    sets = make_sets(rng, N_SETS)
    case = Case()
    n = 10
    for s in range(n):
        if s in (6, 8):
            case.add([], [])                                                                # no records and no splices
        else:
            case.add(*M.row([M.ctu(rng) for _ in range(int(rng.integers(1, 3)))])[:2])
    case.finish()
    subs = M.subs_of(case)
    qp, init = rng.integers(20, 45, n), rng.integers(0, 3, n)
    start = np.array([NO_SET, 3, 5, 5, 16, 2, 9, NO_SET, NO_SET, 0xFFFFFFFE], np.uint32)
    out = np.array([NO_SET, 3, 7, NO_SET, 8, 1000, 10, 11, 12, NO_SET], np.uint32)
    assert len(subs[6].string) == 0 and len(subs[4].string) > 0 and len(subs[5].string) > 0
    chunks, res, written = M.encode_sets(subs, qp, init, sets, start, out)
    assert sorted(written) == [3, 7, 10, 11, 12] and [int(f) for f in res["flags"]] == [0, 0, 0, 0, 0x40, 0x40, 0, 0, 0, 0x40]
    assert np.array_equal(written[10][0], sets[9][0]) and np.array_equal(written[10][1], sets[9][1])   # a copy of the start set
    assert np.array_equal(written[12][0], CS.init_set(int(qp[8]), int(init[8]))[0])
    assert not np.array_equal(written[3][0], sets[3][0])
    F = Form(M.device_form(case, subs, qp, init))
    state = np.concatenate([CS.pack(s)[0] for s in sets]).astype(np.uint32)
    rate = np.concatenate([CS.pack(s)[1] for s in sets]).astype(np.uint8)
    guard = np.full(H.NUM_CTX, 0x5A5A5A5A, np.uint32)
    t_state = dev(np.concatenate([guard, state, guard]), np.int32)                          # in place: the out arrays are the start arrays
    t_rate = dev(np.concatenate([guard.view(np.uint8)[:H.NUM_CTX], rate, guard.view(np.uint8)[:H.NUM_CTX]]))
    t_start, t_out = t_u32(start), t_u32(out)
    ps, pr = t_state.data_ptr() + 4 * H.NUM_CTX, t_rate.data_ptr() + H.NUM_CTX
    total = sum(len(c) for c in chunks)
    got = run(hip, F, total, "sets", n_sets=N_SETS, d_state=ps, d_rate=pr, d_start_set=t_start.data_ptr(), d_out_set=t_out.data_ptr(),
              d_out_state=ps, d_out_rate=pr)
    assert_coded(got, chunks, res, M.tu_info(subs), [s.string for s in subs], "sets", skip=(4, 5, 9))
    assert all(got[1][s] == got[1][s + 1] for s in (4, 5, 9))                               # no payload byte for a bad index
    st, rt = t_state.cpu().numpy().view(np.uint32).reshape(N_SETS + 2, -1), t_rate.cpu().numpy().reshape(N_SETS + 2, -1)
    assert (st[0] == 0x5A5A5A5A).all() and (st[-1] == 0x5A5A5A5A).all() and (rt[0] == 0x5A).all() and (rt[-1] == 0x5A).all()
    for k in range(N_SETS):
        ws, wr = CS.pack(written.get(k, sets[k]))
        assert np.array_equal(st[k + 1], ws) and np.array_equal(rt[k + 1], wr), k
    # the same starts with no out set: the same bytes but for the substream refused for its out index, and no set written
    t_state2, t_rate2 = dev(state, np.int32), dev(rate)
    got2 = run(hip, F, total + 4096, "sets", n_sets=N_SETS, d_state=t_state2.data_ptr(), d_rate=t_rate2.data_ptr(),
               d_start_set=t_start.data_ptr())
    chunks2, res2, written2 = M.encode_sets(subs, qp, init, sets, start, None)
    assert not written2 and len(chunks2[5]) > 0
    assert_coded(got2, chunks2, res2, M.tu_info(subs), [s.string for s in subs], "sets, no out", skip=(4, 9))
    assert torch.equal(t_state2, dev(state, np.int32)) and torch.equal(t_rate2, dev(rate))


# ---------------------------------------------------------------------------------------------- (c) rows
def test_rows_against_the_model(hip):
    B, qp, init, form = rows_case()
    subs, n, n_pic = B["subs"], len(B["subs"]), int(B["level_first"][1])
    F = Form(form)
    strings, info = [s.string for s in subs], M.tu_info(subs)
    t_from, t_at = t_u32(B["sync_from"]), t_u32(B["sync_at"])
    coded = {}
    for name in ("lower", "middle", "upper", None):
        sp = None if name is None else B["splice"][name]
        chunks, res, idx, _ = M.encode_rows(subs, qp, init, B["level_first"], B["sync_from"], B["sync_at"], sp)
        t_sp = None if sp is None else t_u32(sp)
        got = run(hip, F, sum(len(c) for c in chunks), "rows", level_first=B["level_first"], d_sync_from=t_from.data_ptr(),
                  d_sync_at=t_at.data_ptr(), d_sync_splice=0 if sp is None else t_sp.data_ptr())
        assert not res["flags"].any()
        assert_coded(got, chunks, res, info, strings, "rows %s" % name)
        c = B["child"]
        coded[name] = got[0][int(got[1][c]):int(got[1][c + 1])].tobytes()
    assert len({coded["lower"], coded["middle"], coded["upper"]}) == 3 and coded[None] == coded["upper"]
    # a link into the same level: BAD_SET for that row alone (it is in the last level: nobody starts from it)
    sf = B["sync_from"].copy()
    bad = 3 * n_pic + 1
    sf[bad] = bad - 1
    chunks, res, _, _ = M.encode_rows(subs, qp, init, B["level_first"], sf, B["sync_at"], None)
    assert tuple(res[bad]) == (0, M.RES_BAD_SET) and len(chunks[bad]) == 0 and int((res["flags"] != 0).sum()) == 1
    t_sf = t_u32(sf)
    got = run(hip, F, sum(len(c) for c in chunks), "rows", level_first=B["level_first"], d_sync_from=t_sf.data_ptr(),
              d_sync_at=t_at.data_ptr())
    assert_coded(got, chunks, res, info, strings, "same-level link", skip=(bad,))
    # the host-pointer form: the device form's outputs (the rejected and the empty block make it CABAC_HIP_ERR_SUBSTREAM)
    chunks, res, _, _ = M.encode_rows(subs, qp, init, B["level_first"], B["sync_from"], B["sync_at"], B["splice"]["lower"])
    payload = np.full(sum(len(c) for c in chunks) + 64, 0xEE, np.uint8)
    desc, records, first, splices, tus, coeff = form
    with pytest.raises(capi.CabacHipError) as e:
        hip.encode_residual_rows_batch(desc, records, first, splices, tus, coeff, payload, B["level_first"], B["sync_from"], B["sync_at"],
                                       B["splice"]["lower"])
    assert e.value.status == -5
    off, hres, hinfo, hcnt = hip.encode_residual_rows_batch(desc, records, first, splices, tus, coeff, payload, B["level_first"],
                                                            B["sync_from"], B["sync_at"], B["splice"]["lower"], check=False)
    assert (payload[int(off[n]):] == 0xEE).all()
    assert_coded((payload[:int(off[n])], off, hres, hinfo, hcnt), chunks, res, info, strings, "batch form")
    for narrow in (True,):                                                  # ... and on int16 coefficients, with no sync_splice
        chunks, res, _, _ = M.encode_rows(subs, qp, init, B["level_first"], B["sync_from"], B["sync_at"], None)
        off, hres, hinfo, hcnt = hip.encode_residual_rows_batch(desc, records, first, splices, tus, coeff.astype(np.int16), payload,
                                                                B["level_first"], B["sync_from"], B["sync_at"], None, check=False)
        assert_coded((payload[:int(off[n])], off, hres, hinfo, hcnt), chunks, res, info, strings, "batch form, int16")


# ---------------------------------------------------------------------------------------------- (d) scale
def test_eleven_hundred_short_rows_in_two_levels(hip):
    """1 100 substreams of two records, every fifth with a 4 x 4 block between them: more than the 1 024 substreams one tile of the
    scan covers, and more than four workgroups of the index kernel; level 1 starts from level 0 after 0, 1 or 2 records."""
    from test_gpu_search_unit import _block
    rng = np.random.default_rng(0x1100)
    n, half = 1100, 550
    case = Case()
    for s in range(n):
        run_ = U.side_run(rng, 2)
        case.add(run_, [(_block(rng, 4, 4), 0, 0, 1)] if s % 5 == 0 else [])
    case.finish()
    subs = M.subs_of(case)
    qp, init = rng.integers(20, 45, n), rng.integers(0, 3, n)
    sync_from = np.concatenate([np.full(half, NO_SET, np.uint32), np.arange(half, dtype=np.uint32)])
    sync_at = (np.arange(n) % 3).astype(np.uint32)
    sync_sp = np.where(np.arange(n) % 2 == 0, 0, M.END).astype(np.uint32)
    chunks, res, idx, _ = M.encode_rows(subs, qp, init, [0, half, n], sync_from, sync_at, sync_sp)
    assert len(set(idx.tolist())) > 3 and not res["flags"].any()
    alone, _ = M.encode_plain(subs, qp, init)
    assert sum(not np.array_equal(a, b) for a, b in zip(alone[half:], chunks[half:])) > 300       # the links matter
    F = Form(M.device_form(case, subs, qp, init))
    t_from, t_at, t_sp = t_u32(sync_from), t_u32(sync_at), t_u32(sync_sp)
    got = run(hip, F, sum(len(c) for c in chunks), "rows", level_first=[0, half, n], d_sync_from=t_from.data_ptr(),
              d_sync_at=t_at.data_ptr(), d_sync_splice=t_sp.data_ptr())
    assert_coded(got, chunks, res, M.tu_info(subs), [s.string for s in subs], "1100 rows")


# ---------------------------------------------------------------------------------------------- (e) round trip
def test_rows_payload_splits_and_decodes_back_into_the_bins(hip):
    import torch
    B, qp, init, form = rows_case()
    subs, n = B["subs"], len(B["subs"])
    F = Form(form)
    sp = B["splice"]["lower"]
    chunks, res, idx, _ = M.encode_rows(subs, qp, init, B["level_first"], B["sync_from"], B["sync_at"], sp)
    total = sum(len(c) for c in chunks)
    out = Out(n, F.n_tu, total)
    t_from, t_at, t_sp = t_u32(B["sync_from"]), t_u32(B["sync_at"]), t_u32(sp)
    hip.encode_residual_rows_device(*F.head(), *out.args(), B["level_first"], t_from.data_ptr(), t_at.data_ptr(), t_sp.data_ptr(),
                                    **out.tail())
    # the reader's side, from the model: the expanded records, their descriptors, the expanded hand-over indices
    desc2, slots = H.make_desc([len(s.string) for s in subs], qp, init, H.SUB_FINISH, capacities=[len(c) + 16 for c in chunks])
    records = np.concatenate([s.string for s in subs]).astype(np.uint16)
    t_desc2, t_rec2, t_idx = dev(desc2, np.uint8), t_rec(np.concatenate([records, np.zeros(8, np.uint16)])), t_u32(idx)
    t_bytes = torch.zeros(slots + 16, dtype=torch.uint8, device="cuda")
    t_bins = torch.full((len(records) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    t_res = torch.full((2 * n + 2,), -1, dtype=torch.int32, device="cuda")
    hip.split_device(n, t_desc2.data_ptr(), out.t_off.data_ptr(), out.t_pay.data_ptr(), t_bytes.data_ptr())
    hip.decode_wpp_device(n, t_desc2.data_ptr(), t_rec2.data_ptr(), t_bytes.data_ptr(), t_bins.data_ptr(), t_res.data_ptr(), B["level_first"],
                          t_from.data_ptr(), t_idx.data_ptr())
    hip.synchronize()
    got = out.read()
    assert_coded(got, chunks, res, M.tu_info(subs), [s.string for s in subs], "rows")
    bins, dres = t_bins.cpu().numpy(), t_res.cpu().numpy()
    assert (dres[-2:] == -1).all() and not dres[:2 * n].view(H.RESULT_DTYPE)["flags"].any()
    assert np.array_equal(bins[:len(records)], records >> 15) and (bins[len(records):] == 0xA5).all()


# ---------------------------------------------------------------------------------------------- (f) the log
def _log_rounds(rng, K, n):
    """n positions of K chains: the first alternative of every group wins -> [(Cands, pick)]"""
    out = []
    for _ in range(n):
        case, gf, _ = E.search_round(rng, K, 3)
        out.append((Cands.of(case), gf[:-1].copy()))
    return out


def _encode_log(hip, log, K, n_tu, total, qp, init, mode, **kw):
    import torch
    desc = np.zeros(K, H.DESC_DTYPE)
    desc["qp"], desc["init_id"] = qp, np.asarray(init, np.uint32) | RBSP
    desc["rec_offset"], desc["n_records"], desc["byte_offset"], desc["byte_capacity"] = 0xDEAD, 0xBEEF, 0xF00D, 0xFACE   # not read
    t_desc = dev(desc, np.uint8)
    out = Out(K, n_tu, total)
    if mode == "rows":
        log.search_log_encode_rows_device(t_desc.data_ptr(), *out.args(), kw["level_first"], kw["d_sync_from"], **out.tail())
    else:
        log.search_log_encode_sets_device(t_desc.data_ptr(), *out.args(), **out.tail(), **kw)
    hip.synchronize()
    del torch
    return out.read()


def test_log_marks_and_the_emit_in_rows_and_from_sets(hip):
    rng = np.random.default_rng(0x10C5)
    K = 6                                                                    # 3 pictures x 2 rows, in level order
    level_first = np.array([0, 3, 6], np.uint32)
    sync_from = np.array([NO_SET, NO_SET, NO_SET, 0, 1, 2], np.uint32)
    qp, init = rng.integers(20, 45, K), rng.integers(0, 3, K)
    rounds = _log_rounds(rng, K, 3)
    chain = np.arange(K, dtype=np.uint32)
    t_chain, t_from = t_u32(chain), t_u32(sync_from)
    model = M.MarkedLog(K)
    log = hip.search_log(K, 3 * K, 4096, 3 * K * 2, 3 * K * 2 * 256)
    model.log.caps = (3 * K, 4096, 3 * K * 2, 3 * K * 2 * 256)
    marks1, marks2 = np.array([0, 2, 0xFFFFFFFF, K + 5, 4], np.uint32), np.array([2], np.uint32)
    t_m1, t_m2 = t_u32(marks1), t_u32(marks2)
    keep = []
    # append, mark, append, re-mark, append: nothing synchronises in between
    for r, (cands, pick) in enumerate(rounds):
        t_pick = t_u32(pick)
        keep.append(t_pick)
        cands.append(log, t_pick, t_chain, K)
        assert cands.model_append(model, pick, chain)
        if r == 0:
            log.search_log_mark_device(len(marks1), t_m1.data_ptr())
            model.mark(marks1)
        if r == 1:
            log.search_log_mark_device(1, t_m2.data_ptr())                 # replaces the mark of chain 2
            model.mark(marks2)
    at, sp = model.pairs()
    assert at[1] == M.END and at[0] < at[2] < model.log.chain_rec[2] and at[4] != M.END and at[5] == M.END
    subs = model.subs()
    info, strings = model.info(), [s.string for s in subs]
    chunks, res, idx, _ = model.encode_rows(qp, init, level_first, sync_from)
    assert 0 < idx[0] < len(strings[0]) and idx[1] == len(strings[1]) and not res["flags"].any()       # chain 1: unmarked, its end
    at1, sp1 = _first(model, rounds, marks1).pairs()
    assert subs[2].index(at1[2], sp1[2]) < idx[2]                            # the re-mark moved the point of chain 2
    total = sum(len(c) for c in chunks)
    got = _encode_log(hip, log, K, len(model.log.tu), total, qp, init, "rows", level_first=level_first, d_sync_from=t_from.data_ptr())
    assert_coded(got, chunks, res, info, strings, "log rows")
    assert_log_equals(log, model.log, "not consumed")
    # one level, no link; and no sets: both are the plain emit
    plain, want = encode_log(hip, log, model.log, qp, init, RBSP)
    assert_emitted(plain, want, "plain emit")
    assert sum(chunks[k].tobytes() != want[0][int(want[1][k]):int(want[1][k + 1])].tobytes() for k in (3, 4, 5)) >= 2   # the links matter
    t_none = t_u32(np.full(K, NO_SET, np.uint32))
    for other in (_encode_log(hip, log, K, len(model.log.tu), len(want[0]), qp, init, "rows", level_first=[0, K], d_sync_from=t_none.data_ptr()),
                  _encode_log(hip, log, K, len(model.log.tu), len(want[0]), qp, init, "sets")):
        for a, b in zip(plain, other):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    # from sets: chain k from set k + 1, its final contexts into set k + 8; one bad index
    sets = make_sets(rng, 16)
    start, out = (chain + 1).astype(np.uint32), (chain + 8).astype(np.uint32)
    start[3], out[5] = NO_SET, 99
    chunks, res, written = model.encode_sets(qp, init, sets, start, out)
    assert tuple(res[5]) == (0, M.RES_BAD_SET) and sorted(written) == [8, 9, 10, 11, 12]
    state = np.concatenate([CS.pack(s)[0] for s in sets]).astype(np.uint32)
    rate = np.concatenate([CS.pack(s)[1] for s in sets]).astype(np.uint8)
    t_state, t_rate, t_start, t_out = dev(state, np.int32), dev(rate), t_u32(start), t_u32(out)
    got = _encode_log(hip, log, K, len(model.log.tu), sum(len(c) for c in chunks), qp, init, "sets", n_sets=16, d_state=t_state.data_ptr(),
                      d_rate=t_rate.data_ptr(), d_start_set=t_start.data_ptr(), d_out_set=t_out.data_ptr(), d_out_state=t_state.data_ptr(),
                      d_out_rate=t_rate.data_ptr())
    assert_coded(got, chunks, res, info, strings, "log sets", skip=(5,))
    st, rt = t_state.cpu().numpy().view(np.uint32).reshape(16, -1), t_rate.cpu().numpy().reshape(16, -1)
    for k in range(16):
        ws, wr = CS.pack(written.get(k, sets[k]))
        assert np.array_equal(st[k], ws) and np.array_equal(rt[k], wr), k
    # a call that does not fit is dropped; the mark behind it marks the unchanged cursors and nothing else changes; the
    # overflowed log is refused as the plain emit refuses it
    big = Case()
    big.add(U.side_run(rng, 5000), [])
    big.finish()
    cb = Cands.of(big)
    ok, k1 = append_both(log, model.log, cb, [0], [1])
    assert not ok
    t_m3 = t_u32([1])
    log.search_log_mark_device(1, t_m3.data_ptr())
    model.mark([1])
    assert model.pairs()[0][1] == model.log.chain_rec[1]
    assert_log_equals(log, model.log, "dropped")
    with pytest.raises(capi.CabacHipError) as e:
        _encode_log(hip, log, K, len(model.log.tu), total, qp, init, "rows", level_first=level_first, d_sync_from=t_from.data_ptr())
    assert e.value.status == -2 and "record_capacity" in str(e.value)
    # reset clears every mark: the first round again, unmarked — every chain hands over its final contexts
    log.reset()
    model.reset()
    cands, pick = rounds[0]
    cands.append(log, keep[0], t_chain, K)
    assert cands.model_append(model, pick, chain)
    subs = model.subs()
    chunks, res, idx, _ = model.encode_rows(qp, init, level_first, sync_from)
    assert idx.tolist() == [len(s.string) for s in subs]
    got = _encode_log(hip, log, K, len(model.log.tu), sum(len(c) for c in chunks), qp, init, "rows", level_first=level_first,
                      d_sync_from=t_from.data_ptr())
    assert_coded(got, chunks, res, model.info(), [s.string for s in subs], "after reset")
    marked = M.MarkedLog(K)
    assert cands.model_append(marked, pick, chain)
    marked.marks[:3] = [(0, 0)] * 3
    left_over = marked.encode_rows(qp, init, level_first, sync_from)[0]
    assert any(left_over[k].tobytes() != chunks[k].tobytes() for k in (3, 4, 5))                        # a mark left over would show
    # a same-level link and a bad level_first
    sf = sync_from.copy()
    sf[4] = 5
    t_sf = t_u32(sf)
    chunks, res, _, _ = model.encode_rows(qp, init, level_first, sf)
    got = _encode_log(hip, log, K, len(model.log.tu), sum(len(c) for c in chunks), qp, init, "rows", level_first=level_first,
                      d_sync_from=t_sf.data_ptr())
    assert tuple(res[4]) == (0, M.RES_BAD_SET)
    assert_coded(got, chunks, res, model.info(), [s.string for s in subs], "log, same-level link", skip=(4,))
    with pytest.raises(capi.CabacHipError) as e:
        _encode_log(hip, log, K, len(model.log.tu), 64, qp, init, "rows", level_first=[0, 4, 3, K], d_sync_from=t_from.data_ptr())
    assert e.value.status == -2 and "level_first" in str(e.value)
    log.close()
    del keep, k1


def _first(model, rounds, marks1):
    """the model of the first round and its marks alone"""
    m = M.MarkedLog(model.n_chain)
    cands, pick = rounds[0]
    assert cands.model_append(m, pick, np.arange(model.n_chain, dtype=np.uint32))
    m.mark(marks1)
    return m


# ---------------------------------------------------------------------------------------------- (g) end to end
def test_two_rows_searched_in_wavefront_order_logged_marked_and_emitted(hip):
    """2 rows x 3 CTUs.  Step t searches CTU t of row 0 and CTU t - 1 of row 1 (a row that has nothing to search has no finite
    cost: it picks nothing).  After step 0 row 0 is marked and its set is copied over row 1's on the device.  Then one terminate
    record per row, and the emit in rows.  Nothing synchronises before the emit."""
    rng = np.random.default_rng(0xE2E5)
    K, lam = 2, int(1.3 * (1 << 16))
    qp, init = rng.integers(22, 40, K), rng.integers(0, 3, K)
    steps = []
    for t in range(4):
        case, gf, which = E.search_round(rng, K, 4)
        dist = rng.integers(0, 3000, case.n_cand).astype(np.uint64)
        idle = 1 if t == 0 else 0 if t == 3 else None
        if idle is not None:
            dist[int(gf[idle]):int(gf[idle + 1])] = (1 << 64) - 1
        steps.append(Round(case, gf, which, dist, K))
    tail = Tail(K)
    t_state, t_rate, sets, keep = start_sets(hip, qp, init)
    t_chain, t_mark = t_u32(np.arange(K, dtype=np.uint32)), t_u32([0])
    t_from = t_u32([NO_SET, 0])
    log = hip.search_log(K, 16, 4096, 32, 32 * 256)
    n = H.NUM_CTX
    for t, rd in enumerate(steps):
        rd.enqueue(hip, log, t_state, t_rate, t_chain, lam)
        if t == 0:
            log.search_log_mark_device(1, t_mark.data_ptr())
            t_state[n:2 * n] = t_state[:n]                                   # row 1 starts where row 0 stands after its first CTU
            t_rate[n:2 * n] = t_rate[:n]
    tail.cands.append(log, tail.t_pick, t_chain, K)
    desc = np.zeros(K, H.DESC_DTYPE)
    desc["qp"], desc["init_id"] = qp, np.asarray(init, np.uint32) | RBSP
    t_desc = dev(desc, np.uint8)
    out = Out(K, 32, 1 << 16)
    log.search_log_encode_rows_device(t_desc.data_ptr(), *out.args(), [0, 1, 2], t_from.data_ptr(), **out.tail())
    hip.synchronize()
    # the model of the same
    model = M.MarkedLog(K)
    for t, rd in enumerate(steps):
        sets = rd.model(model, sets, lam)
        if t == 0:
            model.mark([0])
            sets[1] = sets[0]
    assert tail.cands.model_append(model, tail.pick, np.arange(K, dtype=np.uint32))
    for t, rd in enumerate(steps):
        assert np.array_equal(rd.t_pick.cpu().numpy().view(np.uint32), rd.want_pick), t
    assert int(steps[0].want_pick[1]) == U.NONE and int(steps[3].want_pick[0]) == U.NONE and len(model.log.entries) == 8
    assert_log_equals(log, model.log, "after the steps")
    subs = model.subs()
    chunks, res, idx, start = model.encode_rows(qp, init, [0, 1, 2], [NO_SET, 0])
    assert 0 < idx[0] < len(subs[0].string) and not res["flags"].any()
    # row 1 is coded from the very contexts its search ran on
    assert np.array_equal(start[1][0], CS.advance_from(subs[0].string[:idx[0]], CS.init_set(int(qp[0]), int(init[0])))[0])
    out.n_tu = len(model.log.tu)
    got = out.read()
    assert_coded(got, chunks, res, model.info(), [s.string for s in subs], "end to end")
    alone = M.encode_plain(subs, qp, init)[0]
    assert not np.array_equal(alone[1], chunks[1]) and np.array_equal(alone[0], chunks[0])
    log.close()
    del keep


# ---------------------------------------------------------------------------------------------- (h) refusals of the batch form
def test_batch_form_refusals_leave_the_outputs_untouched(hip):
    B, qp, init, form = rows_case()
    desc, records, first, splices, tus, coeff = form
    n, n_pic = len(desc), int(B["level_first"][1])
    payload = np.full(1 << 16, 0xEE, np.uint8)
    offsets, results = np.full(n + 1, 0x1111111111111111, np.uint64), np.full(n, 0x22222222, np.uint32).repeat(2).view(H.RESULT_DTYPE)
    info, counts = np.full(len(tus), 0x33333333, np.uint32), np.full((n, W), 0x44444444, np.uint32)

    def refused(names, lf=B["level_first"], sf=B["sync_from"], sa=B["sync_at"], ss=B["splice"]["lower"], d=desc, fi=first):
        with pytest.raises(capi.CabacHipError) as e:
            hip.encode_residual_rows_batch(d, records, fi, splices, tus, coeff, payload, lf, sf, sa, ss, offsets=offsets, results=results,
                                           info=info, counts=counts)
        assert e.value.status == -2 and names in str(e.value), str(e.value)
        assert (payload == 0xEE).all() and (offsets == 0x1111111111111111).all() and (results.view(np.uint32) == 0x22222222).all()
        assert (info == 0x33333333).all() and (counts == 0x44444444).all()

    bad = B["level_first"].copy()
    bad[2] = bad[1] - 1
    refused("level_first", lf=bad)                                           # not non-decreasing
    bad = B["level_first"].copy()
    bad[-1] -= 1
    refused("level_first", lf=bad)                                           # does not end at n_sub
    sf = B["sync_from"].copy()
    sf[n_pic + 1] = n_pic + 2
    refused("substream %d " % (n_pic + 1), sf=sf)                            # into the same level
    sf = B["sync_from"].copy()
    sf[n_pic + 1] = 3 * n_pic
    refused("substream %d " % (n_pic + 1), sf=sf)                            # into a later level
    sf = B["sync_from"].copy()
    sf[2 * n_pic] = n
    refused("substream %d " % (2 * n_pic), sf=sf)                            # beyond the batch
    refused("substream %d " % (n - 1), ss=B["splice"]["lower"][:n - 1])      # a sync_splice shorter than n_sub
    refused("substream %d " % (n - 2), sa=B["sync_at"][:n - 2])
    d = desc.copy()
    d["n_records"][4] = len(records) + 1
    refused("substream 4", d=d)                                              # what the plain host-pointer form refuses
    d = desc.copy()
    d["init_id"][7] |= 3
    refused("substream 7", d=d)
    fi = first.copy()
    fi[3] = fi[4] + 1
    refused("splice_first", fi=fi)
    fi = first.copy()
    fi[-1] -= 1
    refused("spliced exactly once", fi=fi)
    # and the ctx still works
    subs = B["subs"]
    chunks, res, _, _ = M.encode_rows(subs, qp, init, B["level_first"], B["sync_from"], B["sync_at"], B["splice"]["lower"])
    off, hres, hinfo, hcnt = hip.encode_residual_rows_batch(desc, records, first, splices, tus, coeff, payload, B["level_first"],
                                                            B["sync_from"], B["sync_at"], B["splice"]["lower"], check=False)
    assert_coded((payload[:int(off[n])], off, hres, hinfo, hcnt), chunks, res, M.tu_info(subs), [s.string for s in subs], "after refusals")
