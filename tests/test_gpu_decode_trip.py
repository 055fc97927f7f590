"""The decoder's step loop (decode_kernel_v4: a trip of four steps of L bins, record registers per step position, static
staging phases, the bits used since the last top-up instead of a look-ahead count) against the oracle, under the three
decode geometries: 4 = four substreams per wave (L = 16), 8 = sixteen per wave (L = 4), 1 = one per wave (L = 64, whose
loop stays rolled).

Every case encodes with the oracle, decodes with the device and with the oracle, and compares bins, n_bits and flags
exactly.  The cases are built around L, so the oracle's side of a case is computed once per L."""
import functools

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

FIN = H.SUB_FINISH | H.SUB_ALIGN_RBSP
TRM1 = np.array([H.REC_TRM | H.REC_BIN], np.uint16)
TRM0 = np.uint16(H.REC_TRM)
LANES = {4: 16, 8: 4, 1: 64}      # decode variant -> L, the bins of a step


@pytest.fixture(scope="module", params=[4, 8, 1], ids=["quad", "hex", "solo"])
def dec(request):
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    c.set_variant(0, request.param)
    yield c, LANES[request.param]
    c.close()


# ------------------------------------------------------------------ building blocks
def _ep(bits):
    return (H.REC_EP | (np.asarray(bits, np.uint16) << 15)).astype(np.uint16)


def _records(rng, n, ctx_frac=0.7, trm0_frac=0.002):
    """n records that end with a terminate bin 1 (none for n = 0)."""
    if n == 0:
        return np.zeros(0, np.uint16)
    return np.concatenate([H.random_records(rng, n - 1, ctx_frac=ctx_frac, end_trm=False, trm0_frac=trm0_frac), TRM1])


def _encode(recs, flags=FIN):
    lens = [len(r) for r in recs]
    records = np.concatenate(recs + [np.zeros(0, np.uint16)]).astype(np.uint16)
    desc, total = H.make_desc(lens, [32] * len(recs), [2] * len(recs), flags, capacities=[n + 64 for n in lens])
    out, res = H.load_oracle().encode_batch(desc, records, total)
    assert not res["flags"].any()
    return desc, records, out, (res["n_bits"].astype(np.int64) + 7) // 8


def _case(recs, flags=FIN, spare=0, cut=0):
    """Encoded by the oracle and decoded by it from exactly the coded bytes of every substream, plus `spare` (zero) bytes,
    minus `cut`; an empty substream gets no bytes at all."""
    desc, records, out, sizes = _encode(recs, flags)
    dd = desc.copy()
    lens = np.array([len(r) for r in recs])
    dd["byte_capacity"] = np.where(lens == 0, 0, np.maximum(sizes + spare - cut, 0))
    bins_o, ro = H.load_oracle().decode_batch(dd, records, out)
    return dd, records, out, bins_o, ro


def _check(hip, case, clean=True, only=None):
    dd, records, data, bins_o, ro = case
    if only is not None:    # one substream alone in the launch: its length is the wave's
        dd, ro = dd[only:only + 1], ro[only:only + 1]
    assert len(dd) <= 64
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


# ------------------------------------------------------------------ trip boundaries
def _boundary_lengths(L):
    if L == 64:
        return [63, 64, 65, 255, 256, 257]
    return [0, 1, L - 1, L, L + 1, 3 * L, 4 * L - 1, 4 * L, 4 * L + 1, 5 * L, 8 * L - 1, 8 * L, 8 * L + 1]


@functools.lru_cache(None)
def _boundary_case(L):
    rng = np.random.default_rng(2601)
    return _case([_records(rng, n) for n in _boundary_lengths(L)])


def test_trip_boundaries(dec):
    """Every length next to the end of a step and of a trip.  Each substream alone in a launch, so that its own length is
    the loop bound (among them 4L and 8L: the bound an exact multiple of the trip), then all of them sharing waves."""
    hip, L = dec
    case = _boundary_case(L)
    for s, n in enumerate(_boundary_lengths(L)):
        _check(hip, case, clean=n != 0, only=s)
    _check(hip, case, clean=0 not in _boundary_lengths(L))


# ------------------------------------------------------------------ ragged rows
@functools.lru_cache(None)
def _ragged_case(L, first):
    rng = np.random.default_rng(2602)
    lens = (first, 4 * L, 4 * L + 1, 13 * L + 5)
    recs = []
    for rot in range(4):          # with four substreams per wave every rotation is a wave of its own
        recs += [_records(rng, n) for n in lens[rot:] + lens[:rot]]
    return _case(recs)


@pytest.mark.parametrize("first", [1, 0])
def test_ragged_rows(dec, first):
    """Rows that end in different trips share a wave, in every rotation: the short ones run surplus no-op steps while the
    longest goes on.  first = 0: an empty substream without a byte in each row position (it has read two bytes it does not
    have: underrun, as the reference throws in start())."""
    hip, L = dec
    _check(hip, _ragged_case(L, first), clean=first != 0)


# ------------------------------------------------------------------ special steps
@functools.lru_cache(None)
def _special_case(L):
    rng = np.random.default_rng(2603)
    n = 10 * L + 3
    off = 5 % L                   # where in its step the special record sits
    recs = []
    _plain = functools.partial(_records, trm0_frac=0.0)   # no special records but the ones placed here
    spots = [(trip * 4 + p) * L + off for trip in (0, 1) for p in (0, 1, 2, 3)]
    for at in spots:              # align(), more bins behind it
        r = _plain(rng, n)
        r[at] = H.REC_ALIGN
        recs.append(r)
    for at in spots:              # a terminate bin 0 there
        r = _plain(rng, n)
        r[at] = TRM0
        recs.append(r)
    for at in spots:              # the terminate bin 1 that ends the substream there
        recs.append(_plain(rng, at + 1))
    for a, b in ((0, 2), (1, 3), (0, 3), (0, 1)):   # two special steps in one trip (the second trip)
        r = _plain(rng, n)
        r[(4 + a) * L + off] = H.REC_ALIGN
        r[(4 + b) * L + (off + 1) % L] = TRM0 if a else H.REC_ALIGN
        recs.append(r)
    return _case(recs)


def test_special_steps(dec):
    """align() and terminate records in step 0, 1, 2 and 3 of the first and of the second trip, and two of them in one
    trip.  All in one launch, and each alone (so that no other row makes its neighbouring steps special as well)."""
    hip, L = dec
    case = _special_case(L)
    _check(hip, case)
    for s in range(len(case[0])):
        _check(hip, case, only=s)


# ------------------------------------------------------------------ input staging across trips
@functools.lru_cache(None)
def _staging_case():
    rng = np.random.default_rng(2604)
    ep_bits = rng.integers(0, 2, size=4200)
    recs = [np.concatenate([_ep(ep_bits[:n]), TRM1]) for n in (2100, 4200)]   # 1 bit a bin: the fastest steady consumption
    pool = np.array([3, 50, 200, 300])
    p_one = np.full(H.NUM_CTX, 0.008)
    recs.append(np.concatenate([H.random_records(rng, 4200, ctx_frac=1.0, p_one=p_one, ctx_pool=pool, end_trm=False, trm0_frac=0.0),
                                TRM1]))
    case = _case(recs)
    sizes = case[0]["byte_capacity"].astype(np.int64)
    assert sizes[0] > 256 and sizes[1] > 512       # the ring wraps, once and twice
    assert 8.0 * sizes[2] / 4200 < 0.2, sizes      # about 0.1 bit a bin: many trips without a staging request
    return case


def test_staging_across_trips(dec):
    hip, _ = dec
    _check(hip, _staging_case())


# ------------------------------------------------------------------ final accounting
def _accounting_lengths(L):
    return [4 * L * k + r for k in (1, 2) for r in range(0, 3 * L + 1, L // 2)]


@functools.lru_cache(None)
def _accounting_case(L, flags, cut):
    rng = np.random.default_rng(2605)
    recs = [_records(rng, n) for n in _accounting_lengths(L)]
    # without the RBSP stop bit and its alignment the decoder's read-ahead wants two (zero) bytes behind the coded ones
    # (arith_codec.cpp:60-66; without them: the underrun flag)
    return _case(recs, flags=flags, spare=0 if flags & H.SUB_ALIGN_RBSP else 2, cut=cut)


@pytest.mark.parametrize("flags", [FIN, H.SUB_FINISH], ids=["finish_rbsp", "finish"])
def test_final_accounting(dec, flags):
    """n_bits after 0 .. 3 steps of the last trip and after half steps: the bits used since the last top-up are the
    residual of the last, incomplete group.  (Coded without the RBSP stop bit a substream fails finish()'s check of it:
    BAD_STOP, in the oracle as on the device.)"""
    hip, L = dec
    case = _accounting_case(L, flags, 0)
    assert not (case[4]["flags"] & H.RES_UNDERRUN).any()
    _check(hip, case, clean=bool(flags & H.SUB_ALIGN_RBSP))


@pytest.mark.parametrize("cut", [1, 3])
@pytest.mark.parametrize("flags", [FIN, H.SUB_FINISH], ids=["finish_rbsp", "finish"])
def test_final_accounting_cut_short(dec, flags, cut):
    """The same lengths with the last byte missing (cut = 3: the last coded byte also where two spare bytes follow it):
    BAD_STOP and UNDERRUN as the oracle sets them."""
    hip, L = dec
    case = _accounting_case(L, flags, cut)
    assert case[4]["flags"].all()
    _check(hip, case, clean=False)
