"""GPU: the estimator family at the switch between its two launch forms (csrc/cabac_kernels_v4.hip: launch_estimate and
launch_ctx_advance take the one-wave workgroup below 1 024 waves of four substreams and the four-wave workgroup from there on).
Batches of 4 092 substreams (the last one-wave launch), 4 093 (the first four-wave launch: its last wave has one live row) and
4 097 (257 workgroups: the last one has one live wave with one live row and three waves with nothing to do) through
  - the plain estimate with align / resetBits / restart pseudo-records — the ordered path — in some rows of a wave and not in
    others, against orc.estimate_batch;
  - the estimate from given contexts against orc.estimate_records_from;
  - cabac_hip_ctx_advance_device against tests/ctx_sets_model.py (the oracle's update()), into sets of its own and in place.
Everything is compared exactly, and the entries behind n_sub of every output array keep their sentinel."""
import functools

import numpy as np
import pytest
import torch

import ctx_sets_model as M
import helpers as H
from test_gpu_residual_estimate import make_sets

pytestmark = pytest.mark.gpu

SIZES = [4092, 4093, 4097]
EDGE_LENGTHS = [0, 1, 15, 16, 17, 33]            # around the sixteen-record step
SENT64, SENT32, SENT8 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0xA5
TAIL = 8                                         # entries behind n_sub that no launch may write
N_SETS = 5
SPECIALS = np.array([0x1FD, 0x1FC, 0x1FB], np.uint16)      # align(), resetBits(), restart()
BAD_ID = 0x1F0                                   # neither a context nor a bypass / terminate / pseudo record


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


# ---------------------------------------------------------------------------------------------- the shared batch
@functools.lru_cache(None)
def batch(n_sub, ctx_pool=False):
    """(desc, records): ragged lengths 0..70, the step-boundary lengths on the first six and on the last six substreams (so
    that the last, partly filled wave and workgroup get them), random qp and init_id; no pseudo-records yet.  ctx_pool: context
    ids 86..291 only, as the sets tests draw them."""
    rng = np.random.default_rng(0x6E0 + n_sub + (7 if ctx_pool else 0))
    lens = rng.integers(0, 71, size=n_sub)
    lens[:6] = EDGE_LENGTHS
    lens[-6:] = EDGE_LENGTHS
    records = H.random_records(rng, int(lens.sum()), ctx_frac=0.8, end_trm=False,
                               ctx_pool=np.arange(86, 292) if ctx_pool else None)
    desc, _ = H.make_desc(lens, rng.integers(0, 64, size=n_sub), rng.integers(0, 3, size=n_sub), H.SUB_FINISH)
    records.setflags(write=False)
    desc.setflags(write=False)
    return desc, records


@functools.lru_cache(None)
def start_sets():
    sets = make_sets(np.random.default_rng(0x6E5), N_SETS)
    state = np.concatenate([M.pack(s)[0] for s in sets]).astype(np.uint32)
    rate = np.concatenate([M.pack(s)[1] for s in sets]).astype(np.uint8)
    return sets, state, rate


def with_specials(n_sub):
    """The batch with pseudo-records at about one record in twenty.  Per wave of four substreams: every eighth wave has none
    at all, every eighth has them in all four rows, the others in two of their four rows only (one in ten there) — so that
    single steps have rows that need the running total in order beside rows that do not."""
    desc, records = batch(n_sub)
    rng = np.random.default_rng(0x6E1 + n_sub)
    records = records.copy()
    sub_of = np.repeat(np.arange(n_sub), desc["n_records"])
    wave, row = sub_of // 4, sub_of % 4
    rate = np.where(wave % 8 == 3, 0.0, np.where(wave % 8 == 5, 0.05, np.where((row + wave) % 2 == 0, 0.1, 0.0)))
    put = rng.random(len(records)) < rate
    records[put] = rng.choice(SPECIALS, size=int(put.sum()))
    # what the case is about, checked on the batch itself
    step = (np.arange(len(records)) - np.repeat(desc["rec_offset"], desc["n_records"]).astype(np.int64)) // 16
    special = np.isin(records & 0x1FF, SPECIALS)
    rows_with = {}
    for w, s, r in zip(wave[special], step[special], row[special]):
        rows_with.setdefault((int(w), int(s)), set()).add(int(r))
    n_rows = lambda w, s: int(np.count_nonzero(desc["n_records"][4 * w: 4 * w + 4] > 16 * s))
    assert any(len(r) < n_rows(w, s) for (w, s), r in rows_with.items())        # a step ordered for some of its rows only
    assert any(len(r) == 4 for r in rows_with.values())
    clean = np.setdiff1d(np.arange((n_sub + 3) // 4), wave[special])
    assert any(desc["n_records"][4 * w: 4 * w + 4].sum() > 64 for w in clean)   # a whole wave with records and no special
    assert 0.03 < special.mean() < 0.07
    return desc, records


def estimate_on_device(hip, desc, records, sets=None, which=None):
    """The device call on sentinel-filled outputs of n_sub + TAIL entries: (frac_bits, flags), both with their tails."""
    n_sub = len(desc)
    d_desc, d_rec = dev(desc), dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    d_bits = dev(np.full(n_sub + TAIL, SENT64, np.uint64))
    d_flags = dev(np.full(n_sub + TAIL, SENT32, np.uint32))
    if sets is None:
        hip.estimate_device(n_sub, d_desc.data_ptr(), d_rec.data_ptr(), d_bits.data_ptr(), d_flags.data_ptr())
    else:
        d_state, d_rate, d_which = dev(sets[0]), dev(sets[1]), dev(which)
        hip.estimate_from_device(n_sub, d_desc.data_ptr(), d_rec.data_ptr(), d_state.data_ptr(), d_rate.data_ptr(),
                                 d_which.data_ptr(), d_bits.data_ptr(), d_flags.data_ptr())
    hip.synchronize()
    return host(d_bits, np.uint64), host(d_flags, np.uint32)


def first_difference(got, want):
    d = np.flatnonzero(got != want)
    return "none" if not len(d) else "substream %d (wave %d, workgroup of four waves %d): got %d, want %d, %d differ" % (
        d[0], d[0] // 4, d[0] // 16, got[d[0]], want[d[0]], len(d))


# ---------------------------------------------------------------------------------------------- a. the plain estimate
@pytest.mark.parametrize("n_sub", SIZES)
def test_estimate_with_pseudo_records_at_the_switch(hip, n_sub):
    orc = H.load_oracle()
    desc, clean = with_specials(n_sub)
    # a bad record in the first workgroup of either form (substream 3: 16 records) and in the last live substream (33 records)
    records = clean.copy()
    bad_subs = [3, n_sub - 1]
    records[int(desc["rec_offset"][3]) + 7] = BAD_ID
    records[int(desc["rec_offset"][n_sub - 1]) + 20] = BAD_ID | H.REC_BIN
    want, wflags = orc.estimate_batch(desc, records)
    assert np.flatnonzero(wflags).tolist() == bad_subs and (wflags[bad_subs] == H.RES_BAD_RECORD).all()
    got, gflags = hip.estimate_batch(desc, records)
    assert np.array_equal(gflags, wflags), first_difference(gflags, wflags)
    ok = wflags == 0
    assert np.array_equal(got[ok], want[ok]), first_difference(np.where(ok, got, 0), np.where(ok, want, 0))
    # the same strings without the two bad records through the device call: every total, the last live row's included, and
    # nothing written behind n_sub
    want, wflags = orc.estimate_batch(desc, clean)
    assert not wflags.any()
    bits, flags = estimate_on_device(hip, desc, clean)
    assert (bits[n_sub:] == SENT64).all() and (flags[n_sub:] == SENT32).all()
    assert not flags[:n_sub].any(), first_difference(flags[:n_sub], wflags)
    assert np.array_equal(bits[:n_sub], want), first_difference(bits[:n_sub], want)


# ---------------------------------------------------------------------------------------------- b. from given contexts
@pytest.mark.parametrize("n_sub", SIZES)
def test_estimate_from_given_contexts_at_the_switch(hip, n_sub):
    orc = H.load_oracle()
    sets, state, rate = start_sets()
    desc, records = batch(n_sub)
    which = np.random.default_rng(0x6E2 + n_sub).integers(0, N_SETS, size=n_sub).astype(np.uint32)
    bits, flags = estimate_on_device(hip, desc, records, (state, rate), which)
    assert (bits[n_sub:] == SENT64).all() and (flags[n_sub:] == SENT32).all()
    assert not flags[:n_sub].any()
    want = np.zeros(n_sub, np.uint64)
    for s in range(n_sub):
        a, n = int(desc["rec_offset"][s]), int(desc["n_records"][s])
        rc, want[s] = orc.estimate_records_from(records[a:a + n], *sets[int(which[s])])
        assert rc == 0
    assert np.array_equal(bits[:n_sub], want), first_difference(bits[:n_sub], want)


# ---------------------------------------------------------------------------------------------- c / d. the context advance
def advance_records(n_sub):
    """Context records of ids 86..291, bypass and terminate records (random_records) and align records, which touch no context."""
    desc, records = batch(n_sub, ctx_pool=True)
    records = records.copy()
    rng = np.random.default_rng(0x6E3 + n_sub)
    records[rng.random(len(records)) < 0.02] = H.REC_ALIGN
    ids = records & 0x1FF
    assert (ids == H.REC_EP).any() and (ids == H.REC_TRM).any() and (ids == H.REC_ALIGN).any()
    assert np.isin(ids[ids < H.NUM_CTX], np.arange(86, 292)).all()
    return desc, records


def run_advance(hip, desc, records, n_sets, d_state, d_rate, start, out_set, d_out_state, d_out_rate):
    n_sub = len(desc)
    d = [dev(a) for a in (desc, np.concatenate([records, np.zeros(8, np.uint16)]), start, out_set)]
    d_flags = dev(np.full(n_sub + TAIL, SENT32, np.uint32))
    hip.ctx_advance_device(n_sub, d[0].data_ptr(), d[1].data_ptr(), n_sets, d_state.data_ptr(), d_rate.data_ptr(), d[2].data_ptr(),
                           d[3].data_ptr(), d_out_state.data_ptr(), d_out_rate.data_ptr(), d_flags.data_ptr())
    hip.synchronize()
    flags = host(d_flags, np.uint32)
    assert (flags[n_sub:] == SENT32).all()
    return flags[:n_sub]


def advanced(desc, records, s, ctx):
    a, n = int(desc["rec_offset"][s]), int(desc["n_records"][s])
    return M.pack(M.advance_from(records[a:a + n], ctx))


def first_set_difference(got, want, skip=()):
    rows = [k for k in np.flatnonzero((got != want).any(axis=1)) if k not in skip]
    return "none" if not rows else "set %d (%d sets differ): %d words, first at context %d" % (
        rows[0], len(rows), int((got[rows[0]] != want[rows[0]]).sum()), int(np.flatnonzero(got[rows[0]] != want[rows[0]])[0]))


@pytest.mark.parametrize("n_sub", SIZES)
def test_advance_into_own_sets_at_the_switch(hip, n_sub):
    sets, state5, rate5 = start_sets()
    desc, records = advance_records(n_sub)
    n_sets = n_sub + 2              # one n_sets bounds the start and the out arrays: the five real sets, then copies of set 0
    state = np.concatenate([state5, np.tile(state5[:H.NUM_CTX], n_sets - N_SETS)])
    rate = np.concatenate([rate5, np.tile(rate5[:H.NUM_CTX], n_sets - N_SETS)])
    rng = np.random.default_rng(0x6E4 + n_sub)
    start = np.where(rng.random(n_sub) < 0.3, M.NO_SET, rng.integers(0, N_SETS, size=n_sub)).astype(np.uint32)
    # a start index >= n_sets in the last workgroup (of 4 097 substreams the last workgroup has one live substream: that one)
    bad_set = n_sub - 1 if n_sub == 4097 else n_sub - 2
    start[bad_set] = n_sets
    # a pseudo-record of the estimator is no record of a coded substream
    bad_rec = 2049 + int(np.flatnonzero(desc["n_records"][2049:] > 20)[0])
    records[int(desc["rec_offset"][bad_rec]) + 10] = 0x1FC
    out_set = np.arange(1, n_sub + 1, dtype=np.uint32)
    want_state = np.full((n_sets, H.NUM_CTX), SENT32, np.uint32)
    want_rate = np.full((n_sets, H.NUM_CTX), SENT8, np.uint8)
    for s in range(n_sub):
        if s in (bad_set, bad_rec):
            continue                # the out set of a bad set keeps the sentinel; that of a bad record is unspecified
        ctx = M.init_set(desc["qp"][s], desc["init_id"][s]) if start[s] == M.NO_SET else sets[int(start[s])]
        want_state[s + 1], want_rate[s + 1] = advanced(desc, records, s, ctx)
    d_os = torch.full((n_sets * H.NUM_CTX,), SENT32, dtype=torch.int32, device="cuda")
    d_or = torch.full((n_sets * H.NUM_CTX,), SENT8, dtype=torch.uint8, device="cuda")
    flags = run_advance(hip, desc, records, n_sets, dev(state), dev(rate), start, out_set, d_os, d_or)
    want_flags = np.zeros(n_sub, np.uint32)
    want_flags[bad_set], want_flags[bad_rec] = M.RES_BAD_SET, H.RES_BAD_RECORD
    assert np.array_equal(flags, want_flags), first_difference(flags, want_flags)
    got_state, got_rate = host(d_os, np.uint32).reshape(n_sets, -1), host(d_or, np.uint8).reshape(n_sets, -1)
    for k in (0, n_sub + 1, bad_set + 1):          # the two sets nobody names and the refused substream's
        assert (got_state[k] == SENT32).all() and (got_rate[k] == SENT8).all(), k
    keep = np.arange(n_sets) != bad_rec + 1
    assert np.array_equal(got_state[keep], want_state[keep]), first_set_difference(got_state, want_state, (bad_rec + 1,))
    assert np.array_equal(got_rate[keep], want_rate[keep]), first_set_difference(got_rate, want_rate, (bad_rec + 1,))


def test_advance_in_place_in_four_wave_workgroups(hip):
    """4 097 substreams, every one a set of its own that it starts from and writes back; one start index is refused and its set
    stays as it was."""
    sets, _, _ = start_sets()
    n_sub = 4097
    desc, records = advance_records(n_sub)
    own = [sets[s % N_SETS] for s in range(n_sub)]
    packed = [M.pack(c) for c in sets]
    state = np.stack([packed[s % N_SETS][0] for s in range(n_sub)]).astype(np.uint32)
    rate = np.stack([packed[s % N_SETS][1] for s in range(n_sub)]).astype(np.uint8)
    idx = np.arange(n_sub, dtype=np.uint32)
    start = idx.copy()
    refused = 4090                                   # in the last full workgroup
    start[refused] = n_sub
    d_state, d_rate = dev(state), dev(rate)
    flags = run_advance(hip, desc, records, n_sub, d_state, d_rate, start, idx, d_state, d_rate)
    want_flags = np.zeros(n_sub, np.uint32)
    want_flags[refused] = M.RES_BAD_SET
    assert np.array_equal(flags, want_flags), first_difference(flags, want_flags)
    want_state, want_rate = state.copy(), rate.copy()
    for s in range(n_sub):
        if s != refused:
            want_state[s], want_rate[s] = advanced(desc, records, s, own[s])
    got_state, got_rate = host(d_state, np.uint32).reshape(n_sub, -1), host(d_rate, np.uint8).reshape(n_sub, -1)
    assert np.array_equal(got_state, want_state), first_set_difference(got_state, want_state)
    assert np.array_equal(got_rate, want_rate), first_set_difference(got_rate, want_rate)
