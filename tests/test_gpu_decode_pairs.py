"""The quad decoder's choice between its step variants (decode_kernel_v4, L = 16): a 16-bin step in which no row of the
wave has a context more than twice, and no two occurrences inside an aligned group of bins, is decoded without a context
update on the chain — a second occurrence picks one of two prepared states — and any other step by the generic variant.

Every case is encoded by the oracle, decoded by the device and by the oracle, and bins, n_bits and flags are compared
exactly.  All of it runs under the three decode geometries (4 = quad, 8 = hex, 1 = solo), which have to agree with the
oracle and so with each other.  Nothing here looks at which variant ran: the cases are built so that a wrong choice, a
wrong pick or rows that see each other decode other bins."""
import functools
import itertools

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

FIN = H.SUB_FINISH | H.SUB_ALIGN_RBSP
QP, INIT = 32, 2
TRM1 = np.uint16(H.REC_TRM | H.REC_BIN)
TRM0 = np.uint16(H.REC_TRM)
PAIRS = list(itertools.combinations(range(16), 2))      # the 120 pairs of positions (i, j), i < j, of a step


@pytest.fixture(scope="module", params=[4, 8, 1], ids=["quad", "hex", "solo"])
def dec(request):
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    c.set_variant(0, request.param)
    yield c
    c.close()


# ------------------------------------------------------------------ what the chain reads of a state
def _derived(q8):
    """(MPS, k) of an 8-bit state: getLPS multiplies by k (contexts.cpp:945-950)."""
    q8 = int(q8)
    return q8 >> 7, ((q8 ^ (0xFF if q8 & 0x80 else 0)) >> 2) & 31


@functools.lru_cache(None)
def _split_contexts():
    """Contexts whose state after ONE bin from initialisation differs in k or in MPS with the value of that bin — from the
    oracle's context model.  A second occurrence that picks the wrong one of its two candidates codes with another LPS width
    or another MPS."""
    orc = H.load_oracle()
    good = []
    for c in range(H.NUM_CTX):
        after = [orc.ctx_trace(QP, INIT, c, np.array([b, 0], np.uint8), 510)[0][1] for b in (0, 1)]
        if _derived(after[0]) != _derived(after[1]):
            good.append(c)
    assert len(good) >= 64, len(good)
    return good


def _fillers(rng, n, avoid):
    """n different contexts, none of them in `avoid` or among the contexts the cases place (which so stay fresh until they
    are placed), each with a random bin."""
    pool = np.setdiff1d(np.arange(H.NUM_CTX), np.asarray(sorted(set(avoid) | set(_split_contexts()[:64]))))
    ids = rng.choice(pool, size=n, replace=False).astype(np.uint32)
    return (ids | (rng.integers(0, 2, size=n).astype(np.uint32) << 15)).astype(np.uint16)


def _step(rng, ctx, places, first_bin=None):
    """One 16-bin step: context `ctx` at `places` (its first bin `first_bin` if given), sixteen different others around."""
    r = _fillers(rng, 16, {ctx})
    for n, p in enumerate(places):
        b = int(rng.integers(0, 2)) if (n or first_bin is None) else first_bin
        r[p] = ctx | (b << 15)
    return r


# ------------------------------------------------------------------ the rule of the choice, on the CPU
def _qualifies(rows, pick):
    """rows: the (up to four) 16-record steps that the rows of a wave decode together.  The pairs variant is taken iff no
    record is a terminate or an align record, no row has a context more than twice, and no row has one twice inside an
    aligned group of `pick` bins."""
    for r in rows:
        ids = np.asarray(r).astype(np.uint32) & 0x1FF
        if np.isin(ids, (H.REC_TRM, H.REC_ALIGN)).any():
            return False
        for c in np.unique(ids[ids < H.NUM_CTX]):
            at = np.flatnonzero(ids == c)
            if len(at) > 2 or (len(at) == 2 and at[0] // pick == at[1] // pick):
                return False
    return True


def _share(recs, pick):
    """Share of the wave steps of a batch (four substreams per wave, in order) that qualify."""
    got = []
    for w in range(0, len(recs), 4):
        rows = recs[w:w + 4]
        for s in range(0, max(len(r) for r in rows), 16):
            got.append(_qualifies([r[s:s + 16] for r in rows if len(r) > s], pick))
    return float(np.mean(got))


# ------------------------------------------------------------------ oracle side
def _case(recs, flags=FIN):
    """Encoded by the oracle and decoded by it from exactly the coded bytes of every substream (without the RBSP stop bit:
    plus four zero bytes for the decoder's read-ahead); an empty substream gets no bytes at all."""
    lens = [len(r) for r in recs]
    assert len(recs) <= 64 and max(lens) <= 512
    records = np.concatenate(list(recs) + [np.zeros(0, np.uint16)]).astype(np.uint16)
    desc, total = H.make_desc(lens, [QP] * len(recs), [INIT] * len(recs), flags, capacities=[n + 64 for n in lens])
    out, res = H.load_oracle().encode_batch(desc, records, total)
    assert not res["flags"].any()
    sizes = (res["n_bits"].astype(np.int64) + 7) // 8 + (0 if flags & H.SUB_ALIGN_RBSP else 4)
    dd = desc.copy()
    dd["byte_capacity"] = np.where(np.array(lens) == 0, 0, sizes)
    bins_o, ro = H.load_oracle().decode_batch(dd, records, out)
    return dd, records, out, bins_o, ro


def _check(hip, case, clean=True):
    dd, records, data, bins_o, ro = case
    bins_g, rg = hip.decode_batch(dd, records, data, check=False)
    assert np.array_equal(rg["flags"], ro["flags"]), (rg["flags"], ro["flags"])
    ran = (ro["flags"] & H.RES_UNDERRUN) == 0        # the oracle stops where the reference throws: no bit count, no bins
    assert np.array_equal(rg["n_bits"][ran], ro["n_bits"][ran]), (rg["n_bits"], ro["n_bits"])
    if clean:
        assert not ro["flags"].any(), ro["flags"]
    for s in np.flatnonzero(ran):
        o, n = int(dd["rec_offset"][s]), int(dd["n_records"][s])
        keep = (records[o:o + n] & 0x1FF) != H.REC_ALIGN   # an align record has no bin
        assert np.array_equal(bins_g[o:o + n][keep], bins_o[o:o + n][keep]), s


# ------------------------------------------------------------------ every pair of positions
def _pair_substreams(seed, order, flip):
    """Eight substreams of thirty steps: step s of every one of them has context good[s] twice — a fresh context, so that
    its two candidates are those of _split_contexts — and between them the 240 steps are every pair of positions with both
    values of the first bin, in the order `order`."""
    rng = np.random.default_rng(seed)
    good = _split_contexts()
    todo = [(PAIRS[k], b ^ flip) for k in order for b in (0, 1)]
    recs = []
    for sub in range(8):
        steps = [_step(rng, good[s], todo[30 * sub + s][0], todo[30 * sub + s][1]) for s in range(30)]
        recs.append(np.concatenate(steps + [np.array([TRM1])]))
    return recs


@functools.lru_cache(None)
def _all_pairs_case():
    recs = _pair_substreams(3101, range(120), 0)
    seen = set()
    for r in recs:                   # the input is what the docstring says
        for s in range(30):
            ids = r[16 * s:16 * s + 16] & 0x1FF
            at = np.flatnonzero(ids == _split_contexts()[s])
            assert len(at) == 2 and len(np.unique(ids)) == 15
            seen.add((at[0], at[1], int(r[16 * s + at[0]]) >> 15))
            assert _qualifies([r[16 * s:16 * s + 16]], 1)
    assert len(seen) == 240
    return _case(recs)


def test_every_pair_of_positions(dec):
    """A context twice at every (i, j) of a step with both values of the first bin, in steps at every place of a trip; all
    rows of a wave hold the SAME context in the same step, at other positions."""
    _check(dec, _all_pairs_case())


@functools.lru_cache(None)
def _two_rows_case():
    a = _pair_substreams(3101, range(120), 0)
    b = _pair_substreams(3102, [(7 * k + 3) % 120 for k in range(120)], 1)
    recs = [x for ab in zip(a, b) for x in ab]           # rows 0 / 1 and 2 / 3 of a wave: the same id, other pairs
    for r0, r1 in zip(recs[0::2], recs[1::2]):
        differ = 0
        for s in range(30):
            i0, i1 = (r[16 * s:16 * s + 16] & 0x1FF for r in (r0, r1))
            c = _split_contexts()[s]
            assert (i0 == c).sum() == 2 and (i1 == c).sum() == 2
            differ += not np.array_equal(i0 == c, i1 == c)
        assert differ >= 25
    return _case(recs)


def test_same_id_in_two_rows(dec):
    """The same pairs in neighbouring rows of one wave under the same context id, at other positions and with the other
    first bin: rows are substreams of their own and must not see each other."""
    _check(dec, _two_rows_case())


# ------------------------------------------------------------------ across steps: write-back and reload
@functools.lru_cache(None)
def _handover_case():
    rng = np.random.default_rng(3103)
    good = _split_contexts()
    recs = []
    for first in range(5):           # the step whose last bin has the context: places 0..3 of the first trip, 0 of the second
        steps = [_step(rng, good[40], ()) for _ in range(first)]
        steps += [_step(rng, good[first], (15,)), _step(rng, good[first], (0,)), _step(rng, good[first], (3, 12))]
        steps += [_step(rng, good[41], ()) for _ in range(2)]
        recs.append(np.concatenate(steps + [np.array([TRM1])]))
    return _case(recs)


def test_last_bin_then_first_bin(dec):
    """A context in the last bin of a step and in the first of the next (no pair: the state goes through the store), then
    twice in the step after that, at every place of a trip and across two trips."""
    _check(dec, _handover_case())


# ------------------------------------------------------------------ more than twice
@functools.lru_cache(None)
def _many_case():
    rng = np.random.default_rng(3104)
    good = _split_contexts()
    shapes = [(0, 1, 2), (0, 7, 15), (3, 4, 12), (5, 9, 13), (0, 1, 2, 3), (0, 5, 10, 15), (2, 6, 7, 14), (12, 13, 14, 15)]
    recs = []
    for rot in range(4):             # the row with the repetitions: each of the four, the other three hold pairs
        for row in range(4):
            steps = []
            for s, places in enumerate(shapes):
                if row == rot:
                    steps.append(_step(rng, good[s], places))
                    assert not _qualifies([steps[-1]], 1)
                else:
                    steps.append(_step(rng, good[s], PAIRS[(17 * s + 5 * row) % 120]))
            recs.append(np.concatenate(steps + [np.array([TRM1])]))
    return _case(recs)


def test_three_and_four_times(dec):
    """A context three and four times in a step of one row while the other three rows of the wave have pairs."""
    _check(dec, _many_case())


# ------------------------------------------------------------------ special records beside pairs
@functools.lru_cache(None)
def _special_case():
    rng = np.random.default_rng(3105)
    good = _split_contexts()
    recs = []
    for kind in (TRM0, np.uint16(H.REC_ALIGN)):
        for pair, at in (((0, 9), 4), ((2, 15), 0), ((0, 14), 15), ((5, 6), 11)):
            steps = []
            for s in range(6):
                st = _step(rng, good[s], pair, first_bin=s & 1)
                if s in (1, 4):
                    st[at] = kind
                steps.append(st)
            recs.append(np.concatenate(steps + [np.array([TRM1])]))
    return _case(recs)


def test_terminate_and_align_beside_pairs(dec):
    """A terminate bin 0 and an align record in steps that have a pair: in front of it, between its two bins and behind."""
    _check(dec, _special_case())


# ------------------------------------------------------------------ ragged rows
@functools.lru_cache(None)
def _ragged_case():
    rng = np.random.default_rng(3106)
    good = _split_contexts()

    def row(n):
        steps = [_step(rng, good[s], PAIRS[(11 * s + n) % 120], first_bin=(s + n) & 1) for s in range((n + 15) // 16)]
        return np.concatenate(steps + [np.zeros(0, np.uint16)])[:max(n - 1, 0)].tolist() + ([TRM1] if n else [])

    recs = []
    for short in (0, 1, 15, 17, 63):
        for rot in range(2):
            rows = [row(short), row(20 * 16 + 1), row(20 * 16 + 1), row(9 * 16 + 1)]
            recs += [np.array(r, np.uint16) for r in rows[rot * 2:] + rows[:rot * 2]]
    return _case(recs)


def test_ragged_rows(dec):
    """Rows of 0, 1, 15, 17 and 63 records beside long rows with pairs: the lanes past a row's end hold no context and match
    nothing (the empty row has read two bytes it does not have: underrun, as the reference throws in start())."""
    case = _ragged_case()
    assert np.array_equal(case[4]["flags"] != 0, case[0]["n_records"] == 0)
    _check(dec, case, clean=False)


# ------------------------------------------------------------------ all, none, every other step
def _batch(seed, kinds):
    """Eight substreams without any special record; step s of all of them qualifies (kinds[s]) or has, in one of the four
    rows of each wave, a context three times."""
    rng = np.random.default_rng(seed)
    good = _split_contexts()
    far = [p for p in PAIRS if p[0] // 4 != p[1] // 4]   # pairs that qualify at every cadence of the pick
    recs = []
    for sub in range(8):
        steps = []
        for s, ok in enumerate(kinds):
            if ok or sub % 4 != s % 4:
                steps.append(_step(rng, good[s % 64], far[(13 * s + sub) % len(far)]))
            else:
                steps.append(_step(rng, good[s % 64], (s % 5, 6 + s % 4, 11 + s % 5)))
        recs.append(np.concatenate(steps))
    return recs


@pytest.mark.parametrize("kinds, share", [((True,) * 32, 1.0), ((False,) * 32, 0.0), ((True, False) * 16, 0.5)],
                         ids=["all", "none", "alternating"])
def test_share_of_qualifying_steps(dec, kinds, share):
    """Batches of which every step, no step and every other step qualify — by the rule of the choice, computed here for
    this input at each cadence of the pick the kernel may be built with."""
    recs = _batch(3107, kinds)
    for pick in (1, 2, 4):
        assert _share(recs, pick) == share, (pick, _share(recs, pick))
    _check(dec, _share_case(kinds))


@functools.lru_cache(None)
def _share_case(kinds):
    return _case(_batch(3107, kinds), flags=0)
