"""GPU: the bin codec from and into context sets (include/cabac_hip_ctx_sets.h, part 1): cabac_hip_encode_sets_device,
cabac_hip_decode_sets_device and cabac_hip_ctx_advance_device against tests/ctx_sets_model.py (the oracle's record coder started
from given contexts; tests/test_ctx_sets_model.py pins it).  Everything is compared exactly — bytes, n_bits, flags, bins and all
379 states and rates of every set.  Every case runs under the forced geometries encode 4 / 6 / 7 and decode 4 / 8 / 1 and under
the dispatch.  Batches: 1, 5 and 17 substreams (a partial quad wave, one row into a second wave, a partial sixteen-per-wave
group) of lengths around the step and trip boundaries; one more batch is large enough for the geometries of big batches."""
import functools

import numpy as np
import pytest
import torch

import ctx_sets_model as M
import helpers as H
from test_gpu_residual_estimate import make_sets

pytestmark = pytest.mark.gpu

FIN = H.SUB_FINISH | H.SUB_ALIGN_RBSP
LENGTHS = [0, 1, 15, 16, 17, 33, 63, 64, 65, 300, 48, 2, 129, 31, 1999, 32, 207]     # 17 of them
SENT32, SENT8 = 0x5A5A5A5A, 0xA5
N_SETS = 3


@pytest.fixture(scope="module", params=[(0, 0), (4, 4), (6, 8), (7, 1)], ids=["dispatch", "enc4-dec4", "enc6-dec8", "enc7-dec1"])
def hip(request):
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    c.set_variant(*request.param)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------- plumbing
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def ptr(t):
    return t.data_ptr() if t is not None else 0


@functools.lru_cache(None)
def start_sets():
    sets = make_sets(np.random.default_rng(9100), N_SETS)
    state = np.concatenate([M.pack(s)[0] for s in sets]).astype(np.uint32)
    rate = np.concatenate([M.pack(s)[1] for s in sets]).astype(np.uint8)
    return sets, state, rate


@functools.lru_cache(None)
def batch(n_sub, seed=0, lengths=None, flags=FIN):
    rng = np.random.default_rng(9200 + 31 * n_sub + seed)
    lens = list(lengths) if lengths is not None else {1: [65], 5: [65, 0, 300, 16, 33]}.get(n_sub, LENGTHS)[:n_sub]
    recs = [H.random_records(rng, n - 1, ctx_frac=float(rng.choice([0.5, 0.8, 0.95])),
                             ctx_pool=np.arange(86, 292)) if n else np.zeros(0, np.uint16) for n in lens]
    desc, total = H.make_desc([len(r) for r in recs], [int(rng.integers(0, 64)) for _ in recs], [int(rng.integers(0, 3)) for _ in recs],
                              flags)
    return desc, np.concatenate(recs + [np.zeros(0, np.uint16)]).astype(np.uint16), total


def padded(n):
    """The start arrays as n sets (one n_sets bounds the start and the out arrays): the real ones, then copies of set 0."""
    _, state, rate = start_sets()
    k = max(n - N_SETS, 0)
    return (np.concatenate([state, np.tile(state[:H.NUM_CTX], k)]).astype(np.uint32),
            np.concatenate([rate, np.tile(rate[:H.NUM_CTX], k)]).astype(np.uint8))


def mixed_starts(n_sub):
    """NO_SET and set starts in rows of the same wave; set 1 is shared by several substreams."""
    return np.array([M.NO_SET if s % 3 == 0 else (1 if s % 3 == 1 else (s % N_SETS)) for s in range(n_sub)], np.uint32)


def run_encode(hip, desc, records, total, state=None, rate=None, start=None, out_set=None, out_state=None, out_rate=None, plain=False,
               n_sets=None):
    """One device call on fresh buffers: (bytes, results).  out_state / out_rate are device tensors of the caller."""
    d_desc, d_rec = dev(desc), dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    d_bytes = torch.full((total + 16,), SENT8, dtype=torch.uint8, device="cuda")
    d_res = dev(np.full(2 * len(desc), SENT32, np.uint32))
    if plain:
        hip.encode_device(len(desc), ptr(d_desc), ptr(d_rec), ptr(d_bytes), ptr(d_res))
    else:
        t = [dev(a) if a is not None else None for a in (state, rate, start, out_set)]
        ns = n_sets if n_sets is not None else (len(state) // H.NUM_CTX if state is not None else 0)
        hip.encode_sets_device(len(desc), ptr(d_desc), ptr(d_rec), ptr(d_bytes), ptr(d_res), ns, ptr(t[0]), ptr(t[1]), ptr(t[2]),
                               ptr(t[3]), ptr(out_state), ptr(out_rate))
    hip.synchronize()
    return host(d_bytes, np.uint8), host(d_res, H.RESULT_DTYPE)


def run_decode(hip, desc, records, data, state=None, rate=None, start=None, out_set=None, out_state=None, out_rate=None, plain=False,
               n_sets=None):
    d_desc, d_rec = dev(desc), dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    d_bytes = dev(np.concatenate([data, np.zeros(16, np.uint8)]))
    d_bins = torch.full((len(records) + 16,), SENT8, dtype=torch.uint8, device="cuda")
    d_res = dev(np.full(2 * len(desc), SENT32, np.uint32))
    if plain:
        hip.decode_device(len(desc), ptr(d_desc), ptr(d_rec), ptr(d_bytes), ptr(d_bins), ptr(d_res))
    else:
        t = [dev(a) if a is not None else None for a in (state, rate, start, out_set)]
        ns = n_sets if n_sets is not None else (len(state) // H.NUM_CTX if state is not None else 0)
        hip.decode_sets_device(len(desc), ptr(d_desc), ptr(d_rec), ptr(d_bytes), ptr(d_bins), ptr(d_res), ns, ptr(t[0]), ptr(t[1]),
                               ptr(t[2]), ptr(t[3]), ptr(out_state), ptr(out_rate))
    hip.synchronize()
    return host(d_bins, np.uint8), host(d_res, H.RESULT_DTYPE)


def same_coded_bytes(desc, got, want, res, subs=None):
    for s in (range(len(desc)) if subs is None else subs):
        o, n = int(desc[s]["byte_offset"]), (int(res[s]["n_bits"]) + 7) // 8
        assert np.array_equal(got[o:o + n], want[o:o + n]), s


def sentinel_sets(n):
    return (torch.full((n * H.NUM_CTX,), SENT32, dtype=torch.int32, device="cuda"),
            torch.full((n * H.NUM_CTX,), SENT8, dtype=torch.uint8, device="cuda"))


def check_out_sets(out_state, out_rate, n_out, expect):
    """expect: {set index: contexts}; every other set still holds the sentinel."""
    st, rt = host(out_state, np.uint32).reshape(n_out, H.NUM_CTX), host(out_rate, np.uint8).reshape(n_out, H.NUM_CTX)
    for k in range(n_out):
        if k in expect:
            ws, wr = M.pack(expect[k])
            assert np.array_equal(st[k], ws) and np.array_equal(rt[k], wr), k
        else:
            assert (st[k] == SENT32).all() and (rt[k] == SENT8).all(), k


# ---------------------------------------------------------------------------------------------- 1. nothing changes without sets
@pytest.mark.parametrize("n_sub", [1, 5, 17])
def test_all_no_set_is_the_plain_call(hip, n_sub):
    desc, records, total = batch(n_sub)
    want_b, want_r = run_encode(hip, desc, records, total, plain=True)
    for start in (None, np.full(n_sub, M.NO_SET, np.uint32)):
        got_b, got_r = run_encode(hip, desc, records, total, start=start)
        assert np.array_equal(got_b, want_b) and np.array_equal(got_r, want_r)
    ref_b, ref_r, _ = M.encode_sets(desc, records, total, [], None)
    assert np.array_equal(want_r, ref_r)
    same_coded_bytes(desc, want_b, ref_b, ref_r)
    bins_p, res_p = run_decode(hip, desc, records, ref_b, plain=True)
    for start in (None, np.full(n_sub, M.NO_SET, np.uint32)):
        bins_s, res_s = run_decode(hip, desc, records, ref_b, start=start)
        assert np.array_equal(bins_s, bins_p) and np.array_equal(res_s, res_p)
    # (the decoder's finish() finds no stop bit where nothing was read: an empty substream has CABAC_RES_BAD_STOP, as in the reference)
    res_w = M.decode_sets(desc, records, ref_b, [], None)[1]
    assert np.array_equal(bins_p[:len(records)], records >> 15) and np.array_equal(res_p, res_w)
    assert not res_p["flags"][desc["n_records"] > 0].any()


# ---------------------------------------------------------------------------------------------- 2 / 3. sets in, sets out
@pytest.mark.parametrize("n_sub", [1, 5, 17])
def test_start_sets_and_out_sets_against_the_reference(hip, n_sub):
    sets, state, rate = start_sets()
    desc, records, total = batch(n_sub)
    start = mixed_starts(n_sub) if n_sub > 1 else np.array([2], np.uint32)
    ref_b, ref_r, left = M.encode_sets(desc, records, total, sets, start)
    assert not ref_r["flags"].any()
    # out sets in arrays of their own: set s + 1 for substream s, none for every fourth; sets 0 and n_sub + 1 nobody names
    n_out = n_sub + 2
    state, rate = padded(n_out)
    out_set = np.array([M.NO_SET if s % 4 == 3 else s + 1 for s in range(n_sub)], np.uint32)
    expect = {s + 1: left[s] for s in range(n_sub) if s % 4 != 3}
    os_, or_ = sentinel_sets(n_out)
    got_b, got_r = run_encode(hip, desc, records, total, state, rate, start, out_set, os_, or_)
    assert np.array_equal(got_r, ref_r), (got_r, ref_r)
    same_coded_bytes(desc, got_b, ref_b, ref_r)
    check_out_sets(os_, or_, n_out, expect)
    # the decoder, from the same sets, on the reference's bytes
    bins_w, dres_w, dleft = M.decode_sets(desc, records, ref_b, sets, start)
    os_, or_ = sentinel_sets(n_out)
    bins, dres = run_decode(hip, desc, records, ref_b, state, rate, start, out_set, os_, or_)
    assert np.array_equal(dres, dres_w) and not dres["flags"][desc["n_records"] > 0].any()
    assert np.array_equal(bins[:len(records)], bins_w) and np.array_equal(bins_w, records >> 15)
    check_out_sets(os_, or_, n_out, {s + 1: dleft[s] for s in range(n_sub) if s % 4 != 3})
    # an empty substream hands on a copy of where it started (batch(5) and batch(17) have one; its start is set 1 / NO_SET)
    for s in np.flatnonzero(desc["n_records"] == 0):
        if s % 4 != 3:
            want = M.init_set(desc[s]["qp"], desc[s]["init_id"]) if start[s] == M.NO_SET else sets[int(start[s])]
            assert all(np.array_equal(a, b) for a, b in zip(expect[s + 1], want))


def test_every_length_alone_in_its_wave(hip):
    """n_sub = 1 for each of the boundary lengths: the surplus no-op steps of the last trip must not disturb the export."""
    sets, state, rate = start_sets()
    for n in (0, 1, 15, 16, 17, 33, 63, 64, 65, 300):
        desc, records, total = batch(1, seed=n, lengths=(n,))
        start = np.array([n % N_SETS], np.uint32)
        ref_b, ref_r, left = M.encode_sets(desc, records, total, sets, start)
        os_, or_ = sentinel_sets(N_SETS)
        got_b, got_r = run_encode(hip, desc, records, total, state, rate, start, np.array([1], np.uint32), os_, or_)
        assert np.array_equal(got_r, ref_r), n
        same_coded_bytes(desc, got_b, ref_b, ref_r)
        check_out_sets(os_, or_, N_SETS, {1: left[0]})
        os_, or_ = sentinel_sets(N_SETS)
        bins, dres = run_decode(hip, desc, records, ref_b, state, rate, start, np.array([1], np.uint32), os_, or_)
        assert np.array_equal(bins[:n], records >> 15) and np.array_equal(dres, M.decode_sets(desc, records, ref_b, sets, start)[1]), n
        assert n == 0 or not dres["flags"].any(), n
        check_out_sets(os_, or_, N_SETS, {1: left[0]})


def test_in_place_out_set_is_the_own_start_set(hip):
    sets, _, _ = start_sets()
    n_sub = 5
    desc, records, total = batch(n_sub)
    own = [sets[s % N_SETS] for s in range(n_sub)]          # every substream a set of its own, started from and written back
    state = np.concatenate([M.pack(c)[0] for c in own]).astype(np.uint32)
    rate = np.concatenate([M.pack(c)[1] for c in own]).astype(np.uint8)
    idx = np.arange(n_sub, dtype=np.uint32)
    ref_b, ref_r, left = M.encode_sets(desc, records, total, own, idx)
    for coder in ("encode", "decode"):
        d_state, d_rate = dev(state), dev(rate)
        d = [dev(a) for a in (desc, np.concatenate([records, np.zeros(8, np.uint16)]), idx)]
        d_res = dev(np.zeros(2 * n_sub, np.uint32))
        if coder == "encode":
            d_bytes = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
            hip.encode_sets_device(n_sub, ptr(d[0]), ptr(d[1]), ptr(d_bytes), ptr(d_res), n_sub, ptr(d_state), ptr(d_rate), ptr(d[2]),
                                   ptr(d[2]), ptr(d_state), ptr(d_rate))
        else:
            d_bytes = dev(np.concatenate([ref_b, np.zeros(16, np.uint8)]))
            d_bins = torch.zeros(len(records) + 16, dtype=torch.uint8, device="cuda")
            hip.decode_sets_device(n_sub, ptr(d[0]), ptr(d[1]), ptr(d_bytes), ptr(d_bins), ptr(d_res), n_sub, ptr(d_state),
                                   ptr(d_rate), ptr(d[2]), ptr(d[2]), ptr(d_state), ptr(d_rate))
        hip.synchronize()
        want_r = ref_r if coder == "encode" else M.decode_sets(desc, records, ref_b, own, idx)[1]
        assert np.array_equal(host(d_res, H.RESULT_DTYPE), want_r), coder
        check_out_sets(d_state, d_rate, n_sub, {s: left[s] for s in range(n_sub)})


def _last_step(rng, kind, avoid):
    """Sixteen records without a terminate or align record.  pairs: every context once but one twice, its occurrences in
    different aligned fours (the decoder's pairs variant takes the step); generic: one context three times."""
    pool = np.setdiff1d(np.arange(86, 292), avoid)
    ids = rng.choice(pool, size=16, replace=False).astype(np.uint32)
    if kind == "pairs":
        ids[9] = ids[1]
    else:
        ids[5] = ids[6] = ids[1]
    return (ids | (rng.integers(0, 2, size=16).astype(np.uint32) << 15)).astype(np.uint16)


@pytest.mark.parametrize("kind", ["pairs", "generic"])
def test_decode_out_sets_after_a_last_step_of_each_variant(hip, kind):
    """Five substreams of three steps whose last step, in every row of the wave, qualifies for the pairs variant (or in no row
    does): the states the pairs variant brings up to date behind its chain must be the ones exported.  The bytes are those of
    the three steps and a terminate bin (what makes finish() decodable); the decoder is given the three steps only, so that its
    last step is the one under test."""
    sets, _, _ = start_sets()
    rng = np.random.default_rng(9300 + (kind == "pairs"))
    n_sub = 5
    state, rate = padded(n_sub)
    recs = []
    for s in range(n_sub):
        body = H.random_records(rng, 32, ctx_frac=0.9, ctx_pool=np.arange(86, 292), end_trm=False, trm0_frac=0.0)
        recs.append(np.concatenate([body, _last_step(rng, kind, []), [H.REC_TRM | H.REC_BIN]]).astype(np.uint16))
    for r in recs:                                   # the last step is what it is meant to be
        ids = (r[32:48] & 0x1FF).astype(int)
        cnt = np.bincount(ids, minlength=512)
        assert cnt.max() == (2 if kind == "pairs" else 3) and not (ids >= H.NUM_CTX).any()
    enc_desc, total = H.make_desc([49] * n_sub, [30] * n_sub, [1] * n_sub, flags=H.SUB_FINISH, capacities=[128] * n_sub)
    desc = enc_desc.copy()
    desc["n_records"] = 48
    desc["init_id"] &= 3
    records = np.concatenate(recs).astype(np.uint16)
    start = mixed_starts(n_sub)
    ref_b, ref_r, left = M.encode_sets(enc_desc, records, total, sets, start)
    out_set = np.arange(n_sub, dtype=np.uint32)
    os_, or_ = sentinel_sets(n_sub)
    bins, dres = run_decode(hip, desc, records, ref_b, state, rate, start, out_set, os_, or_)
    bins_w, dres_w, dleft = M.decode_sets(desc, records, ref_b, sets, start)
    for s in range(n_sub):
        a = int(desc[s]["rec_offset"])
        assert np.array_equal(bins[a:a + 48], records[a:a + 48] >> 15) and np.array_equal(bins_w[a:a + 48], bins[a:a + 48]), s
        assert bins[a + 48] == SENT8                 # the record behind the substream's end has no bin
    assert np.array_equal(dres, dres_w) and not dres["flags"].any()
    check_out_sets(os_, or_, n_sub, {s: left[s] for s in range(n_sub)})
    os_, or_ = sentinel_sets(n_sub)
    got_b, got_r = run_encode(hip, enc_desc, records, total, state, rate, start, out_set, os_, or_)
    assert np.array_equal(got_r, ref_r)
    same_coded_bytes(desc, got_b, ref_b, ref_r)
    check_out_sets(os_, or_, n_sub, {s: left[s] for s in range(n_sub)})


# ---------------------------------------------------------------------------------------------- 4. a bad set index
def test_bad_set_index_codes_nothing_and_leaves_the_neighbours_alone(hip):
    sets, state, rate = start_sets()
    n_sub = 5
    desc, records, total = batch(n_sub)
    desc = desc.copy()
    desc["n_records"][1] = desc["n_records"][4]     # (the empty substream of the batch gets records: a bad set must stop them)
    desc["rec_offset"][1] = desc["rec_offset"][4]
    start = np.array([1, N_SETS, M.NO_SET, 2, 0], np.uint32)             # substream 1: a start index >= n_sets
    out_set = np.array([0, 1, N_SETS, M.NO_SET, 2], np.uint32)           # substream 2: an out index >= n_sets
    good = np.array([0, 3, 4])
    ref_b, ref_r, left = M.encode_sets(desc, records, total, sets, np.where(start >= N_SETS, M.NO_SET, start))
    os_, or_ = sentinel_sets(N_SETS + 1)          # one set more than the call is told of: it must stay untouched
    got_b, got_r = run_encode(hip, desc, records, total, state, rate, start, out_set, os_, or_, n_sets=N_SETS)
    for s in (1, 2):
        assert tuple(got_r[s]) == (0, M.RES_BAD_SET)
        o, c = int(desc[s]["byte_offset"]), int(desc[s]["byte_capacity"])
        assert (got_b[o:o + c] == SENT8).all()
    assert np.array_equal(got_r[good], ref_r[good])
    same_coded_bytes(desc, got_b, ref_b, ref_r, good)
    check_out_sets(os_, or_, N_SETS + 1, {0: left[0], 2: left[4]})
    os_, or_ = sentinel_sets(N_SETS + 1)
    bins, dres = run_decode(hip, desc, records, ref_b, state, rate, start, out_set, os_, or_, n_sets=N_SETS)
    for s in (1, 2):
        assert tuple(dres[s]) == (0, M.RES_BAD_SET)
    a, n = int(desc[2]["rec_offset"]), int(desc[2]["n_records"])
    assert (bins[a:a + n] == SENT8).all()
    for s in good:
        a, n = int(desc[s]["rec_offset"]), int(desc[s]["n_records"])
        assert np.array_equal(bins[a:a + n], records[a:a + n] >> 15) and dres[s]["flags"] == 0
    check_out_sets(os_, or_, N_SETS + 1, {0: left[0], 2: left[4]})


# ---------------------------------------------------------------------------------------------- 5. the context advance
def run_advance(hip, desc, records, n_sets, d_state, d_rate, start, out_set, d_out_state, d_out_rate):
    d = [dev(a) for a in (desc, np.concatenate([records, np.zeros(8, np.uint16)]), start, out_set)]
    d_flags = dev(np.full(len(desc), SENT32, np.uint32))
    hip.ctx_advance_device(len(desc), ptr(d[0]), ptr(d[1]), n_sets, ptr(d_state), ptr(d_rate), ptr(d[2]), ptr(d[3]), ptr(d_out_state),
                           ptr(d_out_rate), ptr(d_flags))
    hip.synchronize()
    return host(d_flags, np.uint32)


@pytest.mark.parametrize("n_sub", [1, 5, 17])
def test_advance_is_update_for_every_context_record(hip, n_sub):
    sets, _, _ = start_sets()
    state, rate = padded(n_sub + 2)
    desc, records, total = batch(n_sub)
    start = mixed_starts(n_sub) if n_sub > 1 else np.array([0], np.uint32)
    records = records.copy()
    bad = None
    if n_sub == 17:                                  # a pseudo-record of the estimator is no record of a coded substream
        bad = 9
        records[int(desc[bad]["rec_offset"]) + 40] = 0x1FC
    want = {}
    for s in range(n_sub):
        a, n = int(desc[s]["rec_offset"]), int(desc[s]["n_records"])
        ctx = M.init_set(desc[s]["qp"], desc[s]["init_id"]) if start[s] == M.NO_SET else sets[int(start[s])]
        if s != bad:
            want[s + 1] = M.advance_from(records[a:a + n], ctx)
    os_, or_ = sentinel_sets(n_sub + 2)
    flags = run_advance(hip, desc, records, n_sub + 2, dev(state), dev(rate), start, np.arange(1, n_sub + 1, dtype=np.uint32), os_, or_)
    assert [int(f) for f in flags] == [H.RES_BAD_RECORD if s == bad else 0 for s in range(n_sub)]
    st, rt = host(os_, np.uint32).reshape(-1, H.NUM_CTX), host(or_, np.uint8).reshape(-1, H.NUM_CTX)
    for k in range(n_sub + 2):
        if k in want:
            assert np.array_equal(st[k], M.pack(want[k])[0]) and np.array_equal(rt[k], M.pack(want[k])[1]), k
        elif bad is None or k != bad + 1:            # (the out set of a substream with a bad record is unspecified)
            assert (st[k] == SENT32).all() and (rt[k] == SENT8).all(), k


def test_advance_in_place_and_a_bad_set(hip):
    sets, _, _ = start_sets()
    n_sub = 5
    desc, records, total = batch(n_sub)
    own = [sets[s % N_SETS] for s in range(n_sub)]
    d_state = dev(np.concatenate([M.pack(c)[0] for c in own]).astype(np.uint32))
    d_rate = dev(np.concatenate([M.pack(c)[1] for c in own]).astype(np.uint8))
    idx = np.arange(n_sub, dtype=np.uint32)
    start = idx.copy()
    start[3] = n_sub                                 # refused: its set stays as it was
    flags = run_advance(hip, desc, records, n_sub, d_state, d_rate, start, idx, d_state, d_rate)
    assert [int(f) for f in flags] == [0, 0, 0, M.RES_BAD_SET, 0]
    want = {}
    for s in range(n_sub):
        a, n = int(desc[s]["rec_offset"]), int(desc[s]["n_records"])
        want[s] = own[s] if s == 3 else M.advance_from(records[a:a + n], own[s])
    check_out_sets(d_state, d_rate, n_sub, want)


# ---------------------------------------------------------------------------------------------- 6. rounds back to back
def test_two_rounds_without_a_host_wait_between(hip):
    """advance in place, then encode from the advanced sets, on one stream with nothing between the two calls — against the
    same with a synchronise in between and against the reference."""
    sets, _, _ = start_sets()
    n_sub = 17
    desc, records, total = batch(n_sub)
    hist_desc, hist, _ = batch(n_sub, seed=5)
    own = [sets[s % N_SETS] for s in range(n_sub)]
    idx = np.arange(n_sub, dtype=np.uint32)
    outs = []
    for wait in (False, True):
        d_state = dev(np.concatenate([M.pack(c)[0] for c in own]).astype(np.uint32))
        d_rate = dev(np.concatenate([M.pack(c)[1] for c in own]).astype(np.uint8))
        d = [dev(a) for a in (hist_desc, np.concatenate([hist, np.zeros(8, np.uint16)]), idx, desc,
                              np.concatenate([records, np.zeros(8, np.uint16)]))]
        d_bytes = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        d_res = dev(np.zeros(2 * n_sub, np.uint32))
        torch.cuda.synchronize()
        hip.ctx_advance_device(n_sub, ptr(d[0]), ptr(d[1]), n_sub, ptr(d_state), ptr(d_rate), ptr(d[2]), ptr(d[2]), ptr(d_state),
                               ptr(d_rate))
        if wait:
            hip.synchronize()
        hip.encode_sets_device(n_sub, ptr(d[3]), ptr(d[4]), ptr(d_bytes), ptr(d_res), n_sub, ptr(d_state), ptr(d_rate), ptr(d[2]))
        hip.synchronize()
        outs.append((host(d_bytes, np.uint8), host(d_res, H.RESULT_DTYPE)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    advanced = []
    for s in range(n_sub):
        a, n = int(hist_desc[s]["rec_offset"]), int(hist_desc[s]["n_records"])
        advanced.append(M.advance_from(hist[a:a + n], own[s]))
    ref_b, ref_r, _ = M.encode_sets(desc, records, total, advanced, idx)
    assert np.array_equal(outs[0][1], ref_r)
    same_coded_bytes(desc, outs[0][0], ref_b, ref_r)


# ---------------------------------------------------------------------------------------------- the geometries of big batches
def test_a_batch_large_enough_for_the_big_geometries(hip):
    """1 040 short substreams: the encoders' sixteen-per-workgroup / four-unit workgroups, the decoder's four-wave workgroups and
    the device-side choice of the dispatch run their sets instantiations (a 64-substream batch never reaches them)."""
    sets, _, _ = start_sets()
    n_sub = 1040
    state, rate = padded(n_sub)
    rng = np.random.default_rng(9400)
    lens = rng.integers(0, 70, size=n_sub)
    recs = [H.random_records(rng, int(n), ctx_frac=0.85, ctx_pool=np.arange(86, 292)) for n in lens]
    desc, total = H.make_desc([len(r) for r in recs], rng.integers(0, 64, size=n_sub), rng.integers(0, 3, size=n_sub), FIN)
    records = np.concatenate(recs).astype(np.uint16)
    start = np.where(rng.random(n_sub) < 0.3, M.NO_SET, rng.integers(0, N_SETS, size=n_sub)).astype(np.uint32)
    out_set = np.arange(n_sub, dtype=np.uint32)
    ref_b, ref_r, left = M.encode_sets(desc, records, total, sets, start)
    os_, or_ = sentinel_sets(n_sub)
    got_b, got_r = run_encode(hip, desc, records, total, state, rate, start, out_set, os_, or_)
    assert np.array_equal(got_r, ref_r)
    same_coded_bytes(desc, got_b, ref_b, ref_r)
    want_state = np.concatenate([M.pack(c)[0] for c in left]).astype(np.uint32)
    assert np.array_equal(host(os_, np.uint32), want_state)
    os_, or_ = sentinel_sets(n_sub)
    bins, dres = run_decode(hip, desc, records, ref_b, state, rate, start, out_set, os_, or_)
    assert np.array_equal(bins[:len(records)], records >> 15) and np.array_equal(dres["n_bits"], M.decode_sets(desc, records, ref_b, sets, start)[1]["n_bits"])
    assert not dres["flags"].any() and np.array_equal(host(os_, np.uint32), want_state)
    assert np.array_equal(host(or_, np.uint8), np.concatenate([M.pack(c)[1] for c in left]))


@functools.lru_cache(None)
def short_batch(n_sub, seed, lo, hi, first=None):
    """n_sub substreams of lo .. hi - 1 records, the closing terminate bin counted (first: substream 0's number instead), start
    sets mixed with NO_SET -> (desc, records, total, start, and the model's bytes, results and contexts left)"""
    sets, _, _ = start_sets()
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi, size=n_sub)
    if first is not None:
        lens[0] = first
    recs = [H.random_records(rng, int(n) - 1, ctx_frac=0.85, ctx_pool=np.arange(86, 292)) if n else np.zeros(0, np.uint16) for n in lens]
    desc, total = H.make_desc([len(r) for r in recs], rng.integers(0, 64, size=n_sub), rng.integers(0, 3, size=n_sub), FIN)
    assert desc["n_records"].tolist() == lens.tolist()
    records = np.concatenate(recs).astype(np.uint16)
    start = np.where(rng.random(n_sub) < 0.3, M.NO_SET, rng.integers(0, N_SETS, size=n_sub)).astype(np.uint32)
    return (desc, records, total, start) + M.encode_sets(desc, records, total, sets, start)


def check_decode_from_sets(c, desc, records, start, ref_b, left):
    """Decode from sets, every substream into its own out set, against the model: bins, results, out sets"""
    sets, _, _ = start_sets()
    n_sub = len(desc)
    state, rate = padded(n_sub)
    os_, or_ = sentinel_sets(n_sub)
    bins, dres = run_decode(c, desc, records, ref_b, state, rate, start, np.arange(n_sub, dtype=np.uint32), os_, or_)
    want_bins, want_res, want_left = M.decode_sets(desc, records, ref_b, sets, start)
    assert np.array_equal(bins[:len(records)], want_bins) and np.array_equal(want_bins, records >> 15)
    assert np.array_equal(dres, want_res) and not dres["flags"][desc["n_records"] != 0].any()   # (an empty one has no stop bit)
    assert np.array_equal(host(os_, np.uint32), np.concatenate([M.pack(x)[0] for x in want_left]).astype(np.uint32))
    assert np.array_equal(host(or_, np.uint8), np.concatenate([M.pack(x)[1] for x in want_left]))
    assert np.array_equal(host(os_, np.uint32), np.concatenate([M.pack(x)[0] for x in left]).astype(np.uint32))


def test_sets_in_four_wave_workgroups_of_the_forced_variants():
    """4 100 substreams of 0 .. 20 records under the forced variants (6, 4): 1 025 units, so encode_kernel_v6 and the quad decoder
    run their sets instantiations in four-unit / four-wave workgroups, the last of which holds one live unit."""
    c = H.gpu_ctx()
    try:
        c.set_variant(6, 4)
        n_sub = 4100
        desc, records, total, start, ref_b, ref_r, left = short_batch(n_sub, 9500, 0, 21)
        state, rate = padded(n_sub)
        os_, or_ = sentinel_sets(n_sub)
        got_b, got_r = run_encode(c, desc, records, total, state, rate, start, np.arange(n_sub, dtype=np.uint32), os_, or_)
        assert np.array_equal(got_r, ref_r)
        same_coded_bytes(desc, got_b, ref_b, ref_r)
        assert np.array_equal(host(os_, np.uint32), np.concatenate([M.pack(x)[0] for x in left]).astype(np.uint32))
        assert np.array_equal(host(or_, np.uint8), np.concatenate([M.pack(x)[1] for x in left]))
        check_decode_from_sets(c, desc, records, start, ref_b, left)
    finally:
        c.close()


@pytest.mark.parametrize("longest", [8, 2000], ids=["equal-sixteen-per-wave", "one-long-quad"])
def test_sets_under_the_device_side_choice_of_the_dispatch(longest):
    """9 300 substreams (from 9 216 the dispatch asks on the device) of 8 records each: the batch is worth 9 300 of its longest, so
    the device takes sixteen per wave; with substream 0 at 2 000 records it is worth 38 of them and the quad decoder runs.  Both
    geometries are launched with sets either way; the one not chosen must write nothing."""
    c = H.gpu_ctx()
    try:
        n_sub = 9300
        desc, records, total, start, ref_b, ref_r, left = short_batch(n_sub, 9600, 8, 9, first=longest)
        worth = int(desc["n_records"].sum()) // int(desc["n_records"].max())   # substreams of the longest one's length
        assert (worth >= 9216) == (longest == 8)
        check_decode_from_sets(c, desc, records, start, ref_b, left)
    finally:
        c.close()
