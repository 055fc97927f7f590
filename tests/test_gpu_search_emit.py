"""GPU: the winner log (include/cabac_hip_search_emit.h; csrc/cabac_search_emit.hip) against tests/search_emit_model.py, which
tests/test_search_emit_model.py pins to the compiled reference, and against cabac_hip_encode_residual_device on the same strings
built on the host.  Everything is bit-exact: == on integers, no tolerance, no case left out of a comparison.  Every test has its
own bounded input, and nothing is run again after a failure."""
import numpy as np
import pytest

import helpers as H
import search_emit_model as E
import search_unit_model as U
from entropy_coding_amd import capi
from test_gpu_residual_estimate import dev
from test_gpu_search import t_u32, t_u64
from test_gpu_search_unit import t_rec

pytestmark = pytest.mark.gpu

NONE = NO_CHAIN = 0xFFFFFFFF
FIN, RBSP = H.SUB_FINISH, H.SUB_FINISH | H.SUB_ALIGN_RBSP


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


class Cands:
    """The candidate arrays of one append on the device (coefficients int32 or int16)."""

    def __init__(self, cand_first, tus, coeff, rec_first, records, tu_at, int16=False):
        import torch
        self.n_cand, self.int16 = len(cand_first) - 1, int16
        self.host = (np.asarray(cand_first, np.uint32), np.asarray(tus, H.TU_DTYPE), np.asarray(coeff), np.asarray(rec_first, np.uint64),
                     np.asarray(records, np.uint16), None if tu_at is None else np.asarray(tu_at, np.uint32))
        self.t_cf, self.t_rf = t_u32(cand_first), t_u64(rec_first)
        self.t_tu = dev(tus, np.uint8) if len(tus) else torch.zeros(16, dtype=torch.uint8, device="cuda")
        self.t_co = dev(np.asarray(coeff).astype(np.int16 if int16 else np.int32)) if len(coeff) else torch.zeros(8, dtype=torch.int32, device="cuda")
        self.t_rec = t_rec(records)
        self.t_at = t_u32(tu_at) if tu_at is not None and len(tu_at) else None
        self.null_records = len(records) == 0

    @classmethod
    def of(cls, case, int16=False, null_at=False):
        return cls(case.cand_first, case.tus, case.coeff, case.rec_first, case.records, None if null_at else case.tu_at, int16)

    def append(self, log, t_pick, t_chain, n_group, pick=None, chain=None):
        log.append_device(n_group, t_pick.data_ptr(), t_chain.data_ptr(), self.n_cand, self.t_cf.data_ptr(), self.t_tu.data_ptr(),
                          self.t_co.data_ptr(), self.t_rf.data_ptr(), 0 if self.null_records else self.t_rec.data_ptr(),
                          self.t_at.data_ptr() if self.t_at is not None else 0, int16=self.int16, pick=pick, group_chain=chain)

    def model_append(self, model, pick, chain):
        cf, tus, coeff, rf, rec, at = self.host
        return model.append(pick, chain, cf, tus, coeff, rf, rec, at)

    def overwrite(self):
        """the next position's data lands in the candidate arrays, in stream order"""
        for t in (self.t_cf, self.t_rf, self.t_tu, self.t_co, self.t_rec, self.t_at):
            if t is not None:
                t.fill_(0x55)


def append_both(log, model, cands, pick, chain):
    pick, chain = np.asarray(pick, np.uint32), np.asarray(chain, np.uint32)
    t_pick, t_chain = t_u32(pick), t_u32(chain)
    cands.append(log, t_pick, t_chain, len(pick), pick, chain)
    return cands.model_append(model, pick, chain), (t_pick, t_chain)


def assert_log_equals(log, model, what=""):
    got, want = log.read(), model.arrays()
    for k in ("n_entry", "n_record", "n_tu", "n_coeff", "flags"):
        assert int(got["counters"][k]) == int(want["counters"][k]), (what, k, got["counters"], want["counters"])
    for k in ("entries", "records", "tu", "tu_at", "coeff"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


def encode_log(hip, log, model, qp, init, flags, n_tu=None):
    """log.encode_device into guarded tensors -> (payload, offsets, results, tu_info, counts); the payload buffer is what the model
    needs plus 64 bytes that must stay as they were"""
    import torch
    K = model.n_chain
    want = model.emit(qp, init, flags >> 8)
    total, n_tu = len(want[0]), len(model.tu)
    desc = np.zeros(K, H.DESC_DTYPE)
    desc["qp"], desc["init_id"] = qp, np.asarray(init, np.uint32) | flags
    desc["rec_offset"], desc["n_records"], desc["byte_offset"], desc["byte_capacity"] = 0xDEAD, 0xBEEF, 0xF00D, 0xFACE   # not read
    t_desc = dev(desc, np.uint8)
    t_pay = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    t_off = torch.full((K + 2,), -1, dtype=torch.int64, device="cuda")
    t_res = torch.full((2 * K + 2,), -1, dtype=torch.int32, device="cuda")
    t_info = torch.full((n_tu + 2,), -1, dtype=torch.int32, device="cuda")
    t_cnt = torch.full((K * capi.BIN_COUNT_WORDS + 1,), -1, dtype=torch.int32, device="cuda")
    log.encode_device(t_desc.data_ptr(), t_pay.data_ptr(), total + 64, t_off.data_ptr(), t_res.data_ptr(), t_info.data_ptr(), t_cnt.data_ptr())
    hip.synchronize()
    off, res, info, cnt = t_off.cpu().numpy(), t_res.cpu().numpy(), t_info.cpu().numpy(), t_cnt.cpu().numpy()
    assert off[-1] == -1 and (res[-2:] == -1).all() and (info[-2:] == -1).all() and cnt[-1] == -1      # nothing behind the outputs
    pay = t_pay.cpu().numpy()
    assert (pay[total:] == 0xEE).all()
    got = (pay[:total], off[:K + 1].view(np.uint64), res[:2 * K].view(H.RESULT_DTYPE), info[:n_tu].view(np.uint32),
           cnt[:-1].view(np.uint32).reshape(K, -1))
    return got, want


def assert_emitted(got, want, what=""):
    pay, off, res, info, cnt = got
    w_pay, w_off, w_bits, w_info, w_cnt, _ = want
    assert np.array_equal(off, w_off), (what, off, w_off)
    assert np.array_equal(res["n_bits"], w_bits) and not res["flags"].any(), what
    assert np.array_equal(pay, w_pay), (what, np.nonzero(pay != w_pay)[0][:8])
    assert np.array_equal(info, w_info), what
    assert np.array_equal(cnt, w_cnt), what


def encode_host_form(hip, model, qp, init, flags):
    """cabac_hip_encode_residual_device on the strings and splices the host builds from the model's log -> as encode_log"""
    import torch
    K, a = model.n_chain, model.arrays()
    lens, records, first, splices = model.host_form()
    desc = np.zeros(K, H.DESC_DTYPE)
    desc["qp"], desc["init_id"], desc["n_records"] = qp, np.asarray(init, np.uint32) | flags, lens
    desc["rec_offset"] = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.uint64))])
    total = len(model.emit(qp, init, flags >> 8)[0])
    n_tu = len(a["tu"])
    t_desc, t_rec_, t_first = dev(desc, np.uint8), t_rec(records), t_u32(first)
    t_sp = dev(splices, np.uint8) if n_tu else None
    t_tu = dev(a["tu"], np.uint8) if n_tu else None
    t_co = dev(a["coeff"]) if len(a["coeff"]) else torch.zeros(8, dtype=torch.int32, device="cuda")
    t_pay = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    t_off = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
    t_res = torch.zeros(2 * K, dtype=torch.int32, device="cuda")
    t_info = torch.zeros(max(n_tu, 1), dtype=torch.int32, device="cuda")
    t_cnt = torch.zeros(K * capi.BIN_COUNT_WORDS, dtype=torch.int32, device="cuda")
    hip.encode_residual_device(K, t_desc.data_ptr(), t_rec_.data_ptr(), t_first.data_ptr(), t_sp.data_ptr() if n_tu else 0, n_tu, n_tu,
                               t_tu.data_ptr() if n_tu else 0, t_co.data_ptr() if n_tu else 0, t_pay.data_ptr(), total + 64, t_off.data_ptr(),
                               t_res.data_ptr(), t_info.data_ptr(), t_cnt.data_ptr(), int16=a["coeff"].dtype == np.int16)
    hip.synchronize()
    return (t_pay.cpu().numpy()[:total], t_off.cpu().numpy().view(np.uint64), t_res.cpu().numpy().view(H.RESULT_DTYPE),
            t_info.cpu().numpy()[:n_tu].view(np.uint32), t_cnt.cpu().numpy().view(np.uint32).reshape(K, -1))


# ---------------------------------------------------------------------------------------------- log content
def _content_case(rng):
    """Candidates written by hand — (side records, [(log2 w, log2 h, raw position, channel)]) — laid out with GAPS between the
    blocks' coefficients, so that sources start at odd offsets, and runs of odd and even lengths behind one another; 17 of them
    win, one per chain."""
    spec = [
        (9, []),                                                            # 0: zero blocks
        (0, [(2, 2, 0, 0), (3, 3, 5, 1)]),                                  # 1: zero records (positions clip to 0)
        (0, []),                                                            # 2: neither blocks nor records
        (12, [(2, 2, 5, 0), (3, 2, 5, 1), (2, 3, 5, 0)]),                   # 3: three blocks at one position
        (11, [(2, 2, 9, 0), (2, 2, 2, 1), (3, 3, 0xFFFFFFFF, 0)]),          # 4: a position going backwards, one past the run
        (5, [(2, 2, 0x80000000, 0), (2, 2, 0, 0)]),                         # 5: clipped to the end, then held there
        (7, [(2, 2, 1, 0), (6, 6, 3, 0), (2, 2, 6, 1)]),                    # 6: a 64 x 64 block next to 4 x 4 ones
        (6, [(2, 2, 1, 0), (7, 2, 2, 0), (3, 3, 4, 0)]),                    # 7: a log2 size above 6: nothing of it is copied
        (6, [(3, 3, 2, 2), (2, 2, 3, 0)]),                                  # 8: channel 2: copied, refused by the binariser later
        (1, [(0, 0, 0, 0), (2, 2, 1, 0), (0, 1, 1, 1)]),                    # 9: 1 x 1 and 1 x 2 blocks: odd sizes, odd offsets behind
        (40, [(2, 2, k, k & 1) for k in range(0, 38, 2)]),                  # 10: 19 blocks: more than one tile of a row
        (100, [(5, 5, 50, 0)]),                                             # 11: a long run, a 32 x 32 block
        (3, [(6, 6, 0, 1), (6, 6, 3, 0)]),                                  # 12: two 64 x 64 blocks
        (17, [(4, 4, 16, 0)]),
        (16, [(3, 4, 0, 1)]),
        (2, [(2, 6, 1, 0)]),
        (33, [(6, 2, 33, 1), (1, 1, 33, 0)]),
    ]
    loser = (4, [(3, 3, 1, 0)])
    order = []                                                              # winners between losers, in a shuffled order
    for k in rng.permutation(len(spec)):
        order += [("w", int(k)), ("l", -1)] if rng.random() < 0.6 else [("w", int(k))]
    cand_first, rec_first, tus, at, runs, where = [0], [], [], [], [], {}
    n_coeff = n_rec = 0
    for c, (kind, k) in enumerate(order):
        n, blocks = spec[k] if kind == "w" else loser
        if kind == "w":
            where[k] = c
        rec_first.append(n_rec)
        runs.append((n_rec, U.side_run(rng, n)))
        n_rec += n
        for lw, lh, a, ch in blocks:
            n_coeff += int(rng.integers(0, 4))                              # a gap in front of the block
            d = np.zeros(1, H.TU_DTYPE)
            d["coeff_offset"], d["log2_width"], d["log2_height"], d["channel"], d["flags"] = n_coeff, lw, lh, ch, int(rng.integers(0, 4))
            tus.append(d)
            at.append(a)
            n_coeff += (1 << (lw + lh)) if max(lw, lh) <= 6 else 5
        cand_first.append(len(tus))
    rec_first.append(n_rec)
    rec_first = np.asarray(rec_first, np.uint64)
    records = np.zeros(n_rec, np.uint16)
    for r0, run in runs:
        records[r0:r0 + len(run)] = run
    coeff = rng.integers(-32768, 32768, n_coeff + 8).astype(np.int32)
    tus = np.concatenate(tus)
    # groups: the 17 winners on a permutation of the 17 chains, among 23 groups that append nothing
    n_cand, n_chain = len(order), len(spec)
    chains = rng.permutation(n_chain)
    groups = [(where[k], int(chains[k])) for k in range(len(spec))]
    nothing = [(NONE, 3), (n_cand, 4), (n_cand + 7, NO_CHAIN), (where[6], NO_CHAIN), (where[3], n_chain), (where[0], n_chain + 100), (NONE, NO_CHAIN)]
    for j in range(23):
        groups.insert(int(rng.integers(0, len(groups) + 1)), nothing[j % len(nothing)])
    pick, chain = np.array([g[0] for g in groups], np.uint32), np.array([g[1] for g in groups], np.uint32)
    return spec, where, np.asarray(cand_first, np.uint32), tus, coeff, rec_first, records, np.asarray(at, np.uint64).astype(np.uint32), pick, chain


def coded_region_only(tus, coeff):
    """`coeff` with zeros outside the top-left 32 x 32 of every 64-wide / tall block, as the codec leaves such a block
    (cabac_hip.h: only that region is coded).  The reference's templates still read the neighbours at x, y = 32, 33, so what it
    codes for a block that holds anything there is not what the binariser codes, which never looks: such a block can be LOGGED — the
    log copies all w x h — but has no defined CODED form, and only its log content is compared."""
    coeff = np.array(coeff)
    for d in tus:
        lw, lh = int(d["log2_width"]), int(d["log2_height"])
        if max(lw, lh) == 6:
            off = int(d["coeff_offset"])
            b = coeff[off:off + (1 << (lw + lh))].reshape(1 << lh, 1 << lw)     # a view: written through
            b[:, 32:] = 0
            b[32:, :] = 0
    return coeff


@pytest.mark.parametrize("int16,null_at", [(False, False), (True, False), (False, True), (True, True)])
def test_log_content_is_the_model_s(hip, int16, null_at):
    """One append of 40 groups over 17 chains into a log whose four capacities fit EXACTLY: every counter, every entry, every logged
    record, descriptor, position and coefficient equals the model's; a second append then fits none of the capacities and leaves
    everything as it was but the flags; into a log with room it lands behind a coefficient cursor that is odd by then.  Up to there
    every coefficient of every block is random, the 64 x 64 ones beyond their coded 32 x 32 too: the copy is checked on all of
    them.  What is CODED at the end are the same winners with those blocks zero outside the coded region (coded_region_only)."""
    rng = np.random.default_rng(0x106C0 + int16)
    spec, where, cand_first, tus, coeff, rec_first, records, tu_at, pick, chain = _content_case(rng)
    n_cand, n_chain = len(cand_first) - 1, 17
    # ---- the input really holds what this test is about ----
    app = (pick < n_cand) & (chain < n_chain)
    assert len(pick) == 40 and app.sum() == 17 and sorted(chain[app].tolist()) == list(range(17))
    assert (pick == NONE).any() and ((pick >= n_cand) & (pick != NONE)).any() and (chain == NO_CHAIN).any() and ((chain >= n_chain) & (chain != NO_CHAIN)).any()
    n_blk = np.diff(cand_first.astype(np.int64))[pick[app]]
    n_rec = np.diff(rec_first.astype(np.int64))[pick[app]]
    assert ((n_blk == 0) & (n_rec > 0)).any() and ((n_blk > 0) & (n_rec == 0)).any() and ((n_blk == 0) & (n_rec == 0)).any() and (n_blk > 16).any()
    t3 = int(cand_first[where[3]])
    assert tu_at[t3] == tu_at[t3 + 1] == tu_at[t3 + 2]                         # three blocks at one position
    t4 = int(cand_first[where[4]])
    assert tu_at[t4 + 1] < tu_at[t4] and tu_at[t4 + 2] > n_rec.max()           # positions to clip
    t6 = tus[int(cand_first[where[6]]):int(cand_first[where[6] + 1])]
    assert t6["log2_width"].tolist() == [2, 6, 2] and t6["log2_height"].tolist() == [2, 6, 2]
    assert (tus["log2_width"] == 7).sum() == 1 and (tus["channel"] == 2).sum() == 1
    picked_tus = np.concatenate([tus[int(cand_first[c]):int(cand_first[c + 1])] for c in pick[app]])
    assert (picked_tus["coeff_offset"] % 2 == 1).sum() >= 5 and (picked_tus["coeff_offset"] % 8 != 0).sum() >= 10
    assert (rec_first[pick[app]] % 2 == 1).sum() >= 3 and (rec_first[pick[app]] % 2 == 0).sum() >= 3
    assert np.abs(coeff).max() <= 32768
    # ---- the model, then a log that fits it exactly ----
    at = None if null_at else tu_at
    model = E.LogModel(n_chain, int16=int16)
    assert model.append(pick, chain, cand_first, tus, coeff, rec_first, records, at)
    a = model.arrays()
    if not null_at:
        e4 = [e for e in a["entries"] if e["n_rec"] == 11 and e["n_tu"] == 3][0]
        assert a["tu_at"][int(e4["tu_first"]):int(e4["tu_first"]) + 3].tolist() == [9, 9, 11]
    else:
        assert all((a["tu_at"][int(e["tu_first"]):int(e["tu_first"] + e["n_tu"])] == e["n_rec"]).all() for e in a["entries"])
    assert len(a["coeff"]) % 2 == 1 and len(a["coeff"]) > 3 * 4096                # 1 x 1 blocks: the cursor ends up odd
    caps = (len(a["entries"]), len(a["records"]), len(a["tu"]), len(a["coeff"]))
    model.caps = caps
    log = hip.search_log(n_chain, *caps, int16=int16)
    cands = Cands(cand_first, tus, coeff, rec_first, records, at, int16)
    keep = append_both(log, E.LogModel(n_chain), cands, pick, chain)[1]
    assert_log_equals(log, model, "exact fit")
    one = append_both(log, E.LogModel(n_chain), cands, [where[9]], [0])        # one entry, one record, three blocks, 19 coefficients more
    assert not model.append([where[9]], [0], cand_first, tus, coeff, rec_first, records, at)
    assert_log_equals(log, model, "one too many")
    log.close()
    # ---- the same two appends into a log with room: the second lands behind an odd coefficient cursor ----
    model = E.LogModel(n_chain, int16=int16)
    log = hip.search_log(n_chain, caps[0] + 1, caps[1] + 1, caps[2] + 3, caps[3] + 19, int16=int16)
    coded = coded_region_only(tus, coeff)
    assert (coded != coeff).sum() > 3 * 3000 and np.array_equal(coded != 0, (coeff != 0) & (coded == coeff))
    cands = Cands(cand_first, tus, coded, rec_first, records, at, int16)
    for p, c in ((pick, chain), ([where[9]], [0])):
        ok, k = append_both(log, model, cands, p, c)
        assert ok
    assert_log_equals(log, model, "two calls")
    assert int(model.arrays()["tu"]["coeff_offset"][-3]) == caps[3]
    # ... and is coded: the two bad descriptors are reported and add nothing, the 64 x 64 blocks and the 1 x 1 ones are there
    got, want = encode_log(hip, log, model, np.arange(20, 37), np.arange(17) % 3, RBSP)
    assert_emitted(got, want, "hand-written winners")
    assert (want[3] == H.TU_INFO_BAD_DESC).sum() == 2 and not (want[3] & H.TU_INFO_EMPTY).any()
    log.close()
    del keep, one, k


def test_more_groups_than_one_pass_of_any_kernel(hip):
    """40 000 groups on 40 000 chains, each the winner of an 8 x 8 int32 block and one record: more than the 1024 groups of a scan
    tile, more than the 32 768 rows and the 2048 chunks of 4 KiB (10 MB of coefficients) one pass of the copy's grid covers."""
    rng = np.random.default_rng(0xB16)
    n = 40000
    pick = rng.permutation(n).astype(np.uint32)
    chain = rng.permutation(n).astype(np.uint32)
    tus = np.zeros(n, H.TU_DTYPE)
    tus["coeff_offset"], tus["log2_width"], tus["log2_height"] = np.arange(n, dtype=np.uint64) * 64, 3, 3
    coeff = rng.integers(-1 << 20, 1 << 20, n * 64).astype(np.int32)
    records = rng.integers(0, 379, n).astype(np.uint16)
    tu_at = rng.integers(0, 3, n).astype(np.uint32)
    first = np.arange(n + 1)
    log = hip.search_log(n, n, n, n, n * 64)
    cands = Cands(first, tus, coeff, first, records, tu_at)
    t_pick, t_chain = t_u32(pick), t_u32(chain)
    cands.append(log, t_pick, t_chain, n, pick, chain)
    got = log.read()
    assert [int(got["counters"][k]) for k in ("n_entry", "n_record", "n_tu", "n_coeff", "flags")] == [n, n, n, n * 64, 0]
    e = got["entries"]
    idx = np.arange(n)
    assert np.array_equal(e["chain"], chain) and np.array_equal(e["rec_first"], idx) and np.array_equal(e["tu_first"], idx)
    assert (e["n_rec"] == 1).all() and (e["n_tu"] == 1).all() and not e["chain_rec_first"].any() and not e["chain_tu_first"].any()
    assert np.array_equal(got["records"], records[pick]) and np.array_equal(got["tu_at"], np.minimum(tu_at[pick], 1))
    assert np.array_equal(got["tu"]["coeff_offset"], idx.astype(np.uint64) * 64) and (got["tu"]["log2_width"] == 3).all()
    assert np.array_equal(got["coeff"].reshape(n, 64), coeff.reshape(n, 64)[pick])
    log.close()
    del t_pick, t_chain


# ---------------------------------------------------------------------------------------------- end to end
class Round:
    """One position on the device: the buffers of cabac_hip_search_unit_round_device and the append behind it."""

    def __init__(self, case, gf, which, dist, K):
        import torch
        self.case, self.gf, self.which, self.dist, self.K = case, gf, which, dist, K
        self.cands = Cands.of(case)
        self.t_gf, self.t_set, self.t_dist = t_u32(gf), t_u32(which), t_u64(dist)
        self.t_out = t_u32(np.arange(K, dtype=np.uint32))
        self.t_bits = torch.zeros(case.n_cand, dtype=torch.int64, device="cuda")
        self.t_pick = torch.full((K,), -2, dtype=torch.int32, device="cuda")
        self.t_cost = torch.zeros(K, dtype=torch.int64, device="cuda")

    def enqueue(self, hip, log, t_state, t_rate, t_chain, lam):
        c = self.cands
        hip.search_unit_round_device(self.K, self.t_gf.data_ptr(), c.n_cand, c.t_cf.data_ptr(), c.t_tu.data_ptr(), c.t_co.data_ptr(),
                                     t_state.data_ptr(), t_rate.data_ptr(), self.t_set.data_ptr(), c.t_rf.data_ptr(), c.t_rec.data_ptr(),
                                     c.t_at.data_ptr() if c.t_at is not None else 0, self.t_out.data_ptr(), self.t_dist.data_ptr(), lam,
                                     self.t_bits.data_ptr(), self.t_pick.data_ptr(), self.t_cost.data_ptr())
        c.append(log, self.t_pick, t_chain, self.K)
        c.overwrite()                                                         # a log that kept pointers reads 0x55 from here on

    def model(self, log_model, sets, lam):
        c = self.case
        _, pick, _, sets, _, _, _, fl = U.round_model(self.gf, c.cand_first, c.blocks, c.tus, sets, self.which, c.rec_first, c.records,
                                                      c.tu_at, np.arange(self.K, dtype=np.uint32), self.dist, lam)
        assert not fl.any()
        assert self.cands.model_append(log_model, pick, np.arange(self.K, dtype=np.uint32))
        self.want_pick = pick
        return sets


def make_rounds(rng, K, n_round, exclude=None):
    rounds = []
    for r in range(n_round):
        case, gf, which = E.search_round(rng, K, 5)
        dist = rng.integers(0, 3000, case.n_cand).astype(np.uint64)
        if exclude == r:                                                      # chain 1 has nothing to pick in this round
            dist[int(gf[1]):int(gf[2])] = (1 << 64) - 1
        rounds.append(Round(case, gf, which, dist, K))
    return rounds


class Tail:
    def __init__(self, K):
        self.pick, cf, rf, rec = E.tail_round(K)
        self.cands = Cands(cf, np.zeros(0, H.TU_DTYPE), np.zeros(0, np.int32), rf, rec, None)
        self.t_pick = t_u32(self.pick)


def start_sets(hip, qp, init):
    """cabac_hip_ctx_init_device for every chain -> (state, rate tensors, the same sets from the oracle)"""
    import torch
    K, orc = len(qp), H.load_oracle()
    t_state = torch.zeros(K * 379, dtype=torch.int32, device="cuda")
    t_rate = torch.zeros(K * 379, dtype=torch.uint8, device="cuda")
    t_qp, t_init = dev(np.asarray(qp, np.int32)), t_u32(init)
    hip.ctx_init_device(K, t_qp.data_ptr(), t_init.data_ptr(), t_state.data_ptr(), t_rate.data_ptr())
    return t_state, t_rate, [orc.ctx_init(int(q), int(i)) for q, i in zip(qp, init)], (t_qp, t_init)


@pytest.mark.parametrize("K", [3, 17])
def test_search_to_bytes_on_one_stream(hip, K):
    """Five rounds from cabac_hip_ctx_init_device, each followed by its append and by the candidate arrays being overwritten, then a
    tail append of one terminate record per chain — all enqueued before the first synchronise — and encode_device with FINISH |
    ALIGN_RBSP: payload, offsets, results, tu_info and bin counts equal the model's (the oracle's bytes of the concatenated
    winners' strings) and what cabac_hip_encode_residual_device gives for the same strings and splices built on the host."""
    rng = np.random.default_rng(0xE2E + K)
    qp, init = rng.integers(18, 42, K), rng.integers(0, 3, K)
    lam = int(1.7 * (1 << 16))
    rounds, tail = make_rounds(rng, K, 5, exclude=2), Tail(K)
    model = E.LogModel(K)
    t_state, t_rate, sets, keep = start_sets(hip, qp, init)
    t_chain = t_u32(np.arange(K, dtype=np.uint32))
    log = hip.search_log(K, 6 * K, 6 * K * 30, 6 * K * 2, 6 * K * 2 * 256)
    for rd in rounds:
        rd.enqueue(hip, log, t_state, t_rate, t_chain, lam)
    tail.cands.append(log, tail.t_pick, t_chain, K)
    for rd in rounds:                                                         # the model of the same: picks, sets, log
        sets = rd.model(model, sets, lam)
    assert tail.cands.model_append(model, tail.pick, np.arange(K, dtype=np.uint32))
    got, want = encode_log(hip, log, model, qp, init, RBSP)
    for r, rd in enumerate(rounds):
        assert np.array_equal(rd.t_pick.cpu().numpy().view(np.uint32), rd.want_pick), r
    assert int(rounds[2].want_pick[1]) == NONE and len(model.entries) == 6 * K - 1
    assert_log_equals(log, model, "after the rounds")
    assert_emitted(got, want, "log")
    host = encode_host_form(hip, model, qp, init, RBSP)
    for a, b in zip(got, host):
        assert np.array_equal(a, b)
    assert len({len(s) for s in want[5]}) > 1 and (want[4][:, 380] == 1).all()   # every chain ends in its terminate bin
    log.close()
    del keep


# ---------------------------------------------------------------------------------------------- overflow
def _two_calls(rng, K):
    a, gf_a, _ = E.search_round(rng, K, 2)
    b, gf_b, _ = E.search_round(rng, K, 2)
    return (a, gf_a[:-1].copy()), (b, gf_b[1:] - 1)                            # the first / the last alternative of every group wins


@pytest.mark.parametrize("short", [0, 1, 2, 3])
def test_a_call_that_does_not_fit_is_dropped_whole(hip, short):
    """Capacity `short` (entries, records, blocks, coefficients) is one too small for the second of two calls: counters and arrays
    stay what the first call left, only the flag is set, encode_device refuses; after reset() the log takes the first call again
    and codes it, and a log with room takes both and codes them."""
    rng = np.random.default_rng(0x0F10)
    K = 4
    (a, pick_a), (b, pick_b) = _two_calls(rng, K)
    chain = np.arange(K, dtype=np.uint32)
    qp, init = [30, 31, 32, 33], [0, 1, 2, 0]
    both = E.LogModel(K)
    ca, cb = Cands.of(a), Cands.of(b)
    assert ca.model_append(both, pick_a, chain) and cb.model_append(both, pick_b, chain)
    arr, only_a = both.arrays(), E.LogModel(K)
    assert ca.model_append(only_a, pick_a, chain)
    assert all(len(arr[k]) > len(only_a.arrays()[k]) > 0 for k in ("entries", "records", "tu", "coeff"))   # both calls add to all four
    caps = [len(arr["entries"]), len(arr["records"]), len(arr["tu"]), len(arr["coeff"])]
    caps[short] -= 1
    model = E.LogModel(K, *caps)
    log = hip.search_log(K, *caps)
    keep = [append_both(log, model, ca, pick_a, chain)]
    assert keep[0][0]
    assert_log_equals(log, model, "first call")
    keep.append(append_both(log, model, cb, pick_b, chain))
    assert not keep[1][0] and model.flags == E.OVERFLOW | (0x10 << short)
    assert_log_equals(log, model, "second call dropped")
    with pytest.raises(capi.CabacHipError) as e:
        encode_log(hip, log, model, qp, init, RBSP)
    assert e.value.status == -2 and ["entry_capacity", "record_capacity", "tu_capacity", "coeff_capacity"][short] in str(e.value)
    log.reset()
    model.reset()
    keep.append(append_both(log, model, ca, pick_a, chain))
    assert keep[2][0]
    assert_log_equals(log, model, "after reset")
    assert_emitted(*encode_log(hip, log, model, qp, init, RBSP), what="after reset")
    log.close()
    caps[short] += 1
    log = hip.search_log(K, *caps)
    model = E.LogModel(K, *caps)
    keep.append(append_both(log, model, ca, pick_a, chain))
    keep.append(append_both(log, model, cb, pick_b, chain))
    assert keep[3][0] and keep[4][0]
    assert_log_equals(log, model, "room for both")
    assert_emitted(*encode_log(hip, log, model, qp, init, RBSP), what="room for both")
    log.close()


# ---------------------------------------------------------------------------------------------- re-encode and continue
def test_encode_append_encode_again_with_another_qp(hip):
    rng = np.random.default_rng(0x2E2E)
    K = 5
    qp, init = rng.integers(20, 40, K), rng.integers(0, 3, K)
    lam = 3 << 15
    rounds = make_rounds(rng, K, 3)
    model = E.LogModel(K)
    t_state, t_rate, sets, keep = start_sets(hip, qp, init)
    t_chain = t_u32(np.arange(K, dtype=np.uint32))
    log = hip.search_log(K, 64, 4096, 64, 1 << 16)
    for rd in rounds[:2]:
        rd.enqueue(hip, log, t_state, t_rate, t_chain, lam)
        sets = rd.model(model, sets, lam)
    got, want = encode_log(hip, log, model, qp, init, RBSP)
    assert_emitted(got, want, "first")
    first_payload = got[0].copy()
    rounds[2].enqueue(hip, log, t_state, t_rate, t_chain, lam)                 # the log was not consumed: it goes on
    sets = rounds[2].model(model, sets, lam)
    qp2 = (qp + 7) % 52
    got, want = encode_log(hip, log, model, qp2, init, FIN)
    assert_emitted(got, want, "second")
    assert len(got[0]) > len(first_payload) and not np.array_equal(got[0][:len(first_payload)], first_payload)
    got, want = encode_log(hip, log, model, qp, init, RBSP)                    # and once more as at first: the longer strings
    assert_emitted(got, want, "third")
    assert_log_equals(log, model, "after three encodes")
    log.close()
    del keep


# ---------------------------------------------------------------------------------------------- empty edges
def test_empty_edges(hip):
    """A log that was never appended to codes empty substreams (FINISH only: the oracle's bytes of an empty string); n_group = 0
    changes nothing; one chain with one entry of one 4 x 4 block; a coeff_bytes that is not the log's is refused."""
    from test_gpu_search_unit import Case
    rng = np.random.default_rng(0xED6E)
    model, log = E.LogModel(3), hip.search_log(3, 0, 0, 0, 0)
    got, want = encode_log(hip, log, model, [22, 30, 37], [0, 1, 2], FIN)
    assert_emitted(got, want, "never appended")
    assert len(want[0]) > 0 and all(len(s) == 0 for s in want[5])
    c = Case()
    c.add([], [(H.random_block(rng, 4, 4, density=0.8), 0, 0, 0)])
    c.finish()
    assert np.abs(c.coeff).max() <= 32767
    cands = Cands.of(c)
    t_none = t_u32([0])
    cands.append(log, t_none, t_none, 0)                                      # n_group = 0
    assert_log_equals(log, model, "n_group 0")
    log.close()
    for int16 in (False, True):
        model, log = E.LogModel(1, 1, 0, 1, 16, int16=int16), hip.search_log(1, 1, 0, 1, 16, int16=int16)
        cands = Cands.of(c, int16)
        keep = append_both(log, model, cands, [0], [0])
        assert keep[0]
        assert_log_equals(log, model, "one block")
        got, want = encode_log(hip, log, model, [27], [1], RBSP)
        assert_emitted(got, want, "one block")
        assert len(want[5][0]) > 0 and int(want[3][0]) & 0xFFFF == int(got[3][0]) & 0xFFFF
        with pytest.raises(capi.CabacHipError) as e:
            cands.int16 = not int16
            cands.append(log, t_none, t_none, 1)
        assert e.value.status == -2 and "coeff_bytes" in str(e.value)
        assert_log_equals(log, model, "refused call")
        log.close()
