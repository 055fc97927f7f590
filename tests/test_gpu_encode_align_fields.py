"""align() in the lane-serial encoder (encode_kernel_v7).  The chain wave has no case for an align record: the context waves
give it the fields of an LPS of width 256 (k = 0, c2 = 512, lpsm = ~0; lp9 = 0 and ep = 0 for the low wave), and the ordinary
step then leaves range = 256 and adds nothing to the code value.

Every GPU case is coded by the device and by the oracle and compared exactly: the coded bytes up to ceil(n_bits / 8), n_bits
and flags.  The cases run under encode variant 7 with a handful of substreams (encode_kernel_v7<1>) and padded to 1 025
substreams (encode_kernel_v7<4>, whose last workgroup then has ONE live substream: the chain and the low wave's lanes past it
mirror it), and under variants 6 and 4, which share the context waves' helpers, as controls.  The arithmetic itself is
checked for every range on the CPU."""
import functools

import numpy as np
import pytest

import helpers as H

FIN = H.SUB_FINISH | H.SUB_ALIGN_RBSP
ALIGN = np.uint16(H.REC_ALIGN)
TRM1 = np.uint16(H.REC_TRM | H.REC_BIN)
TRM0 = np.uint16(H.REC_TRM)
EP0, EP1 = np.uint16(H.REC_EP), np.uint16(H.REC_EP | H.REC_BIN)
QUIET = 200                        # a context the random records never use: its two bins in front of an align are one on the
CTX0, CTX1 = np.uint16(QUIET), np.uint16(QUIET | H.REC_BIN)   # MPS and one on the LPS path of its initial state
POOL = np.array([c for c in range(H.NUM_CTX) if c != QUIET])
BIG = 1025                         # 64 full workgroups of sixteen and one with a single live substream


# ------------------------------------------------------------------ the arithmetic, every range (CPU)
def _chain_step(k, c2, lpsm, rng):
    """lane_rng_step: -> (posted word, range)."""
    t = (((rng >> 5) & 15) * k + c2) >> 1
    rm = rng - t
    x = np.where(lpsm != 0, t, rm)
    nb = (31 - np.floor(np.log2(x)).astype(np.int64)) - 23      # clz(x) - 23, x in 1 .. 511
    return (nb << 9) + rm, x << nb, nb


def _low_step(w, lp9, ep, low, pend):
    nb = w >> 9
    term = (w & lp9) << nb
    sh = nb + ep
    return (low << sh) + term, pend + sh


def test_align_fields_arithmetic():
    """(k, c2, lpsm) = (0, 512, ~0) for every range 256 .. 511: range 256, no shift, the posted word is range - 256 (below 512:
    the shift field and it do not overlap, so the sum is the OR); the low step with lp9 = ep = 0 leaves low and pend alone."""
    rng = np.arange(256, 512, dtype=np.int64)
    w, new_range, nb = _chain_step(np.int64(0), np.int64(512), np.int64(-1), rng)
    assert (new_range == 256).all() and (nb == 0).all()
    assert np.array_equal(w, rng - 256) and (w < 512).all() and np.array_equal(w, (rng - 256) | (nb << 9))
    for low0, pend0 in ((0, 0), (0x1234567, 9), ((1 << 40) - 1, 15)):
        low, pend = _low_step(w, np.int64(0), np.int64(0), np.full_like(w, low0), np.full_like(w, pend0))
        assert (low == low0).all() and (pend == pend0).all()
    # the same restated step is the ordinary one elsewhere: a terminate bin (k = 0, c2 = 4) has LPS width 2
    w, new_range, nb = _chain_step(np.int64(0), np.int64(4), np.int64(0), rng)
    assert np.array_equal(w & 511, rng - 2) and ((new_range >= 256) & (new_range < 512)).all()


# ------------------------------------------------------------------ GPU plumbing
@pytest.fixture(scope="module", params=[(7, False), (7, True), (6, False), (4, False)], ids=["v7x1", "v7x4", "v6", "v4"])
def enc(request):
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    c.set_variant(request.param[0], 0)
    yield c, request.param[1]
    c.close()


def _plain(rng, n):
    return H.random_records(rng, n, ctx_pool=POOL, end_trm=False, trm0_frac=0.0)


@functools.lru_cache(None)
def _filler():
    """What pads a batch to BIG substreams: random ones of 1 .. 40 records, some with an align."""
    rng = np.random.default_rng(4100)
    recs = []
    for s in range(BIG):
        r = np.concatenate([_plain(rng, int(rng.integers(0, 40))), [TRM1]]).astype(np.uint16)
        if s % 5 == 0 and len(r) > 1:
            r[int(rng.integers(0, len(r) - 1))] = ALIGN
        recs.append(r)
    return recs


def _batch(recs, big):
    """(desc, records, total, oracle bytes, oracle results); big: the cases first, filler up to BIG - 1, and the first case once
    more as substream BIG - 1, alone in the last workgroup."""
    recs = list(recs)
    if big:
        assert len(recs) < BIG
        recs = recs + _filler()[len(recs):BIG - 1] + [recs[0]]
        assert len(recs) == BIG
    lens = [len(r) for r in recs]
    assert max(lens) <= 49
    records = np.concatenate(recs).astype(np.uint16)
    rng = np.random.default_rng(len(recs))
    desc, total = H.make_desc(lens, rng.integers(20, 45, len(recs)), rng.integers(0, 3, len(recs)), FIN, capacities=[n + 64 for n in lens])
    want_b, want_r = H.load_oracle().encode_batch(desc, records, total)
    assert not want_r["flags"].any()
    return desc, records, total, want_b, want_r


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _compare(desc, got_b, got_r, want_b, want_r):
    assert np.array_equal(got_r["flags"], want_r["flags"]), np.flatnonzero(got_r["flags"] != want_r["flags"])
    assert np.array_equal(got_r["n_bits"], want_r["n_bits"]), np.flatnonzero(got_r["n_bits"] != want_r["n_bits"])
    for s in range(len(desc)):
        o, n = int(desc[s]["byte_offset"]), (int(want_r[s]["n_bits"]) + 7) // 8
        assert np.array_equal(got_b[o:o + n], want_b[o:o + n]), s


def _check(hip, case):
    import torch
    desc, records, total, want_b, want_r = case
    d_desc, d_rec = _dev(desc), _dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    d_bytes = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    d_res = _dev(np.full(2 * len(desc), 0x5A5A5A5A, np.uint32))
    hip.encode_device(len(desc), d_desc.data_ptr(), d_rec.data_ptr(), d_bytes.data_ptr(), d_res.data_ptr())
    hip.synchronize()
    _compare(desc, d_bytes.cpu().numpy(), d_res.cpu().numpy().view(H.RESULT_DTYPE), want_b, want_r)


# ------------------------------------------------------------------ every position
def _with_align(rng, at, before, n):
    """n records, an align at `at`, `before` (a record or None) in front of it."""
    r = _plain(rng, n)
    r[at] = ALIGN
    if before is not None and at > 0:
        r[at - 1] = before
    return r


def _position_recs():
    rng = np.random.default_rng(4101)
    recs = []
    for lane in range(16):
        for before in (CTX0, CTX1, EP0, EP1, TRM0, ALIGN):          # ALIGN in front: the range in front of the align is 256
            recs.append(np.concatenate([_with_align(rng, lane, before, 33 + lane), [TRM1]]))            # the first step (lane 0: range 510)
            recs.append(np.concatenate([_with_align(rng, 16 + lane, before, 48), [TRM1]]))              # a middle step
            recs.append(_with_align(rng, 32 + lane, before, 33 + lane))                                 # the last step, its last record
    return recs


@functools.lru_cache(None)
def _position_case(big):
    recs = _position_recs()
    assert all(17 <= len(r) <= 49 for r in recs)
    return _batch(recs, big)


@pytest.mark.gpu
def test_every_position(enc):
    """One align at each of the sixteen lanes of the first, of a middle and of the last step, behind a context bin 0 and a context
    bin 1 of an untouched context (one is its MPS, the other its LPS path), a bypass 0, a bypass 1, a terminate 0 and another
    align (range 256); at lane 0 of the first step it is the very first record (range 510)."""
    hip, big = enc
    _check(hip, _position_case(big))


# ------------------------------------------------------------------ neighbours and ends
@functools.lru_cache(None)
def _neighbour_case(big):
    rng = np.random.default_rng(4102)
    recs = []
    for at in (0, 5, 14, 15, 16, 30):
        for run in (2, 3):                                             # two and three in a row (also across a step boundary)
            r = _plain(rng, 40)
            r[at:at + run] = ALIGN
            recs.append(np.concatenate([r, [TRM1]]))
    for n in (1, 15, 16, 17, 31, 32, 33, 40):                          # the last record before the terminating bin
        recs.append(np.concatenate([_plain(rng, n - 1), [ALIGN, TRM1]]).astype(np.uint16))
    for step in (0, 1):                                                # lane 15, then a context bin at lane 0 of the next step
        for nxt in (CTX0, CTX1):
            r = _plain(rng, 40)
            r[16 * step + 15] = ALIGN
            r[16 * step + 16] = nxt
            recs.append(np.concatenate([r, [TRM1]]))
    recs.append(np.array([ALIGN], np.uint16))                          # nothing but an align
    recs.append(np.full(35, ALIGN, np.uint16))
    return _batch(recs, big)


@pytest.mark.gpu
def test_neighbours_and_ends(enc):
    hip, big = enc
    _check(hip, _neighbour_case(big))


# ------------------------------------------------------------------ rows of a unit
@functools.lru_cache(None)
def _rows_case(big):
    rng = np.random.default_rng(4103)
    recs = []
    for at in (3, 15, 16, 37):
        for rows in ((0, 1, 2, 3), (0,), (1,), (2,), (3,)):            # all four rows of a unit in the same step, or exactly one
            for row in range(4):
                r = _plain(rng, 39)
                if row in rows:
                    r[at] = ALIGN
                recs.append(np.concatenate([r, [TRM1]]))
    return _batch(recs, big)


@pytest.mark.gpu
def test_rows(enc):
    hip, big = enc
    _check(hip, _rows_case(big))


# ------------------------------------------------------------------ from context sets
@pytest.mark.gpu
def test_from_context_sets(enc):
    """The position cases through cabac_hip_encode_sets_device (encode_kernel_v7<., CtxSets>), started from given sets, against
    the oracle's record coder started from the same contexts."""
    import torch
    import ctx_sets_model as M
    from test_gpu_residual_estimate import make_sets
    hip, big = enc
    desc, records, total, _, _ = _position_case(big)
    sets = make_sets(np.random.default_rng(4104), 3)
    state = np.concatenate([M.pack(s)[0] for s in sets]).astype(np.uint32)
    rate = np.concatenate([M.pack(s)[1] for s in sets]).astype(np.uint8)
    start = np.array([M.NO_SET if s % 4 == 0 else s % 3 for s in range(len(desc))], np.uint32)
    want_b, want_r, _ = M.encode_sets(desc, records, total, sets, start)
    assert not want_r["flags"].any()
    d_desc, d_rec = _dev(desc), _dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    d_bytes = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    d_res = _dev(np.full(2 * len(desc), 0x5A5A5A5A, np.uint32))
    d_state, d_rate, d_start = _dev(state), _dev(rate), _dev(start)
    hip.encode_sets_device(len(desc), d_desc.data_ptr(), d_rec.data_ptr(), d_bytes.data_ptr(), d_res.data_ptr(), 3,
                           d_state.data_ptr(), d_rate.data_ptr(), d_start.data_ptr())
    hip.synchronize()
    _compare(desc, d_bytes.cpu().numpy(), d_res.cpu().numpy().view(H.RESULT_DTYPE), want_b, want_r)
