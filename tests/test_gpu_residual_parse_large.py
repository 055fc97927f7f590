"""GPU: the residual parser (csrc/cabac_residual_parse.hip) where tests/test_gpu_residual_parse.py does not go — batches on
both sides of the switch from one wave per workgroup to four (n_sub >= 1024), ragged and with empty substreams; errors
inside a four-wave workgroup; every element of the coefficient buffer, not only the coded regions; blocks made of escape
codes for max_log2_tr_range 15..20; and damaged streams.  The expectation is the oracle's parser (tests/parse_corpus.py::
expectation; pinned to the reference's reader on well-formed streams by tests/test_residual_oracle.py, run under the host
sanitizers on the damaged ones by tests/test_sanitizers.py) and, where no sign hiding is used, the blocks that were coded.
Every comparison is == on integers and covers every substream of its batch."""
import time

import numpy as np
import pytest

import helpers as H
import parse_corpus as PC
import test_gpu_residual_parse as P

pytestmark = pytest.mark.gpu

hip = P.hip   # both stores: int32 (cabac_hip_residual_parse_device) and int16 (cabac_hip_residual_parse16_device)

_cache = {}


def cached(maker, *args):
    """A corpus and the oracle's parse of it: built once, used by the int32 and the int16 run."""
    key = (maker.__name__,) + args
    if key not in _cache:
        t0 = time.time()
        c = maker(*args)
        _cache[key] = (c, PC.expectation(c))
        print("%s%r: %d substreams, %d blocks, built and parsed by the oracle in %.1f s"
              % (maker.__name__, args, len(c["subs"]), sum(len(x[0]) for x in c["subs"]), time.time() - t0))
    return _cache[key]


def coded(m):
    """(columns, rows) of a block that are coded, i.e. written: the top-left 32 x 32 of a 64-wide / tall block."""
    return min(m[0], 32), min(m[1], 32)


def expected_buffer(corpus, exp, offsets, total, fill, narrow):
    """What the coefficient buffer must hold after the parse -> (values, care): `fill` wherever the parser must not write
    (outside the coded region of every block, between, in front of and behind the blocks, blocks behind the one at which a
    substream stops), the oracle's levels (through int16 for the int16 store) in the coded regions of the blocks the oracle
    parsed to their end; care is False over the coded regions of the blocks from an underrun on, which the device parses
    from zeros while the oracle stops.  Also -> per substream whether a level the oracle gives lies outside int16."""
    want = np.full(total, fill, np.int64)
    care = np.ones(total, bool)
    outside = np.zeros(len(exp), bool)
    t = 0
    for s, (metas, _, _) in enumerate(corpus["subs"]):
        rc, blocks, _, _, n_whole = exp[s]
        for k, m in enumerate(metas):
            w, h = m[0], m[1]
            we, he = coded(m)
            if k < n_whole or rc == -4:
                at = (int(offsets[t]) + np.arange(he)[:, None] * w + np.arange(we)[None, :]).ravel()
                if k < n_whole:
                    v = blocks[k][:he, :we].ravel().astype(np.int64)
                    outside[s] |= bool(((v < -32768) | (v > 32767)).any())
                    want[at] = v.astype(np.int16) if narrow else v
                else:
                    care[at] = False
            t += 1
    return want, care, outside


def check(hip, corpus, exp, layout_seed=None, coded_blocks=True):
    """Parse the corpus on the device and compare with the oracle, substream by substream: flags, n_bits, tu_info, and the
    WHOLE coefficient buffer (see expected_buffer).  layout_seed: the blocks scattered over the buffer (P.scattered_layout)
    instead of back to back.  -> (results, rc per substream)."""
    subs = corpus["subs"]
    narrow = hip.parse_int16
    metas = [m for x in subs for m in x[0]]
    layout = P.packed_layout(metas) if layout_seed is None else P.scattered_layout(np.random.default_rng(layout_seed), metas)
    got, res, co = P.parse(hip, subs, corpus["qps"], capacities=corpus["caps"], finish=corpus["finish"], layout=layout, raw=True)
    info = P.parse.last_info
    want, care, outside = expected_buffer(corpus, exp, layout[0], layout[1], P.sentinel(narrow), narrow)
    rcs = np.array([e[0] for e in exp])
    # flags.  After an underrun the device goes on parsing zeros, so whether a level of the int16 store went out of range
    # there is not defined: the RANGE bit is required where the blocks before the underrun hold such a level, else ignored.
    want_flags = np.array([PC.RC_FLAGS[rc] for rc in rcs], np.uint32) | np.where(narrow & outside, H.RES_RANGE, 0).astype(np.uint32)
    ignore = np.where((rcs == -4) & ~outside, H.RES_RANGE, 0).astype(np.uint32)
    bad = np.flatnonzero((res["flags"] & ~ignore) != want_flags)
    assert not len(bad), ("flags", bad[:10], res["flags"][bad[:10]], want_flags[bad[:10]], rcs[bad[:10]])
    want_bits = np.array([e[2] for e in exp], np.uint32)
    bad = np.flatnonzero((res["n_bits"] != want_bits) & (rcs != -4))
    assert not len(bad), ("n_bits", bad[:10], res["n_bits"][bad[:10]], want_bits[bad[:10]], rcs[bad[:10]])
    t = 0
    for s, (m_s, blocks, _) in enumerate(subs):
        rc, w_blocks, _, w_info, n_whole = exp[s]
        for k in range(n_whole):
            assert int(info[t + k]) == int(w_info[k]), ("tu_info", s, k, m_s[k], hex(int(info[t + k])), hex(int(w_info[k])))
            we, he = coded(m_s[k])
            if not np.array_equal(got[s][k][:he, :we], (w_blocks[k][:he, :we].astype(np.int16) if narrow else w_blocks[k][:he, :we])):
                raise AssertionError(("coefficients", s, k, m_s[k], rc))
            if coded_blocks and rc == 0 and blocks is not None and not (m_s[k][3] & H.TU_SIGN_HIDING):   # decode(encode(block)) == block
                assert np.array_equal(w_blocks[k][:he, :we], blocks[k][:he, :we]), ("oracle vs coded block", s, k, m_s[k])
        if rc != -4:    # a refused block, the blocks behind it, all blocks of a refused start: tu_info as parse() filled it
            assert (info[t + n_whole: t + len(m_s)] == 0xFFFFFFFF).all(), ("tu_info written", s, rc, n_whole)
        t += len(m_s)
    bad = np.flatnonzero(care & (co != want))
    assert not len(bad), ("coefficient buffer: %d elements differ" % len(bad), bad[:10], co[bad[:10]], want[bad[:10]])
    return res, rcs


# ---- 2. both geometries, ragged -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sub", [1023, 1024, 1025, 4100])
def test_ragged_batches_around_the_four_wave_switch(hip, n_sub):
    """1 023: the last batch of one-wave workgroups; 1 024: the first of four-wave ones; 1 025: a last workgroup of one live
    wave and three dead ones; 4 100: well above.  Regular, TS_FLAG, transform-skip, BDPCM, dependent-quantisation and SBT
    zero-out blocks of every shape, a third of the substreams with sign hiding; substreams of 1 and of >= 30 blocks side by
    side; five substreams without blocks (byte_capacity 0 and 2, the last substream among them); CABAC_SUB_FINISH set and
    clear.  An empty substream is what the oracle makes of it: with its two bytes flags 0 and the bits of the terminate
    bin, with byte_capacity 0 CABAC_RES_UNDERRUN."""
    corpus, exp = cached(PC.ragged, 0x2A66ED + n_sub, n_sub)
    subs = corpus["subs"]
    n_blocks = np.array([len(x[0]) for x in subs])
    # the conditions on the input
    empty = np.flatnonzero(n_blocks == 0)
    assert len(empty) >= 3 and empty[-1] == n_sub - 1 and {0, 2} <= set(int(corpus["caps"][s]) for s in empty)
    assert any(n_blocks[s] == 1 and n_blocks[s + 1] >= 30 and s // 4 == (s + 1) // 4 for s in range(n_sub - 1))
    assert 0.5 < corpus["finish"].mean() < 0.8
    seen = set((m[3] & ~H.TU_DEP_QUANT) for x in subs for m in x[0])
    assert {0, H.TU_SIGN_HIDING, H.TU_TS_FLAG, H.TU_TS_FLAG | H.TU_TRANSFORM_SKIP, H.TU_TRANSFORM_SKIP, H.TU_TRANSFORM_SKIP | H.TU_BDPCM,
            H.TU_SBT_ZERO_OUT} <= seen and any(m[3] & H.TU_DEP_QUANT for x in subs for m in x[0])
    assert set(P.SHAPES) <= set((m[0], m[1]) for x in subs for m in x[0])
    res, rcs = check(hip, corpus, exp)
    # nothing but the empty substreams without bytes may report anything
    want_rc = np.where((n_blocks == 0) & (corpus["caps"] == 0), -4, 0)
    assert np.array_equal(rcs, want_rc), np.flatnonzero(rcs != want_rc)[:10]


# ---- 3. errors inside a four-wave workgroup -------------------------------------------------------------------------------
def test_errors_beside_intact_substreams_in_four_wave_workgroups(hip):
    """1 100 substreams, every ninth damaged (truncated; stop byte destroyed; a 64-wide transform-skip block, one whose coded
    transform_skip_flag says so, log2_width 7, channel 2): the damaged ones report exactly the oracle's flags, the blocks
    before a refused block come back and those behind it keep the sentinel (check() compares the whole buffer), and the
    three neighbours on either side — the other waves of the workgroup among them — come back exact with flags 0."""
    n_sub = 1100
    corpus, exp = cached(PC.with_errors, 0xE44, n_sub)
    damage = corpus["damage"]
    res, rcs = check(hip, corpus, exp, layout_seed=0xE45)
    kinds = set()
    for s in range(n_sub):
        d = damage[s]
        if d is None:
            assert rcs[s] == 0 and int(res["flags"][s]) == 0, s
            continue
        assert all(damage[n] is None for n in range(max(0, s - 3), min(n_sub, s + 4)) if n != s)
        if d == "truncated":
            assert int(res["flags"][s]) & ~H.RES_RANGE == H.RES_UNDERRUN and rcs[s] == -4, s
        elif d == "stop":
            assert int(res["flags"][s]) == H.RES_BAD_STOP and rcs[s] == -5, s
        else:
            assert int(res["flags"][s]) == H.RES_BAD_RECORD and rcs[s] == -2 and exp[s][4] == d[1] >= 1, (s, d)
            assert d[1] < len(corpus["subs"][s][0]) - 1      # there are blocks behind the refused one
        kinds.add(d if isinstance(d, str) else d[0])
    assert kinds == {"truncated", "stop"} | set(PC.REFUSED)
    assert set(s % 4 for s in range(n_sub) if damage[s] is not None) == {0, 1, 2, 3}     # in every wave of a workgroup


def test_underrun_comes_before_a_refused_block(hip):
    """Where an underrun and a refused block meet in one substream the underrun is reported, alone, whichever comes first in
    the block list (include/cabac_hip_parse.h): the reference's readByte throws before the block behind it is looked at, and
    when the coded transform_skip_flag of a 64-wide block is itself read past the end, before the flag can refuse the block.
    max_log2_tr_range outside 15..20 is a refused descriptor for kernel and oracle alike."""
    corpus, exp = cached(PC.underrun_meets_refusal, 0x0C0)
    assert [e[0] for e in exp] == [-4, -4, -4, -2, -2, 0]
    assert exp[0][4] < 6 and exp[1][4] < 6 and exp[2][4] == 0 and exp[3][4] == 1 and exp[4][4] == 1    # blocks parsed whole
    res, _ = check(hip, corpus, exp, layout_seed=0x0C1, coded_blocks=False)
    assert [int(f) & ~H.RES_RANGE for f in res["flags"]] == [H.RES_UNDERRUN] * 3 + [H.RES_BAD_RECORD] * 2 + [0]


# ---- 4. where the parser writes -------------------------------------------------------------------------------------------
def where_corpus(n_sub):
    return PC.with_errors(0x3E4E + n_sub, n_sub)


@pytest.mark.parametrize("n_sub", [300, 1100])
def test_device_forms_write_the_coded_regions_and_nothing_else(hip, n_sub):
    """The blocks scattered over the buffer in random order, 0..7 elements apart (odd coeff_offsets for the int16 store too)
    and with padding in front and behind: after the parse every element outside the coded min(w, 32) x min(h, 32) of a block
    — the rest of 64-wide / tall blocks, the gaps, the padding, whole blocks behind a refused one — still holds the
    sentinel, and inside the oracle's values hold, zeros included."""
    corpus, exp = cached(where_corpus, n_sub)
    metas = [m for x in corpus["subs"] for m in x[0]]
    offsets = P.scattered_layout(np.random.default_rng(0x10C + n_sub), metas)[0]
    assert (offsets & 1).sum() > len(metas) // 4 and (np.diff(offsets) < 0).sum() > len(metas) // 4    # odd, and not ascending
    assert sum(1 for m in metas if max(m[0], m[1]) == 64) > 20
    check(hip, corpus, exp, layout_seed=0x10C + n_sub)


@pytest.mark.parametrize("n_sub", [300, 1100])
def test_host_forms_keep_or_zero_what_the_parser_does_not_write(hip, n_sub):
    """cabac_hip_residual_parse_batch keeps the caller's values wherever the parser does not write;
    cabac_hip_residual_parse_batch16 returns zeros there (include/cabac_hip.h, include/cabac_hip_parse.h) — same layouts as for the device forms."""
    corpus, exp = cached(where_corpus, n_sub)
    narrow = hip.parse_int16
    metas = [m for x in corpus["subs"] for m in x[0]]
    layout = P.scattered_layout(np.random.default_rng(0x10C + n_sub), metas)
    desc, buf, first, tus, offsets, total = P.pack(corpus["subs"], corpus["qps"], corpus["caps"], corpus["finish"], layout)
    mine = np.full(total, P.sentinel(narrow), np.int16 if narrow else np.int32)     # the caller's values
    co, res, info = hip.residual_parse_batch(desc, buf, first, tus, total, check=False, with_info=True, int16=narrow, coeff=mine)
    want, care, outside = expected_buffer(corpus, exp, offsets, total, 0 if narrow else P.sentinel(narrow), narrow)
    bad = np.flatnonzero(care & (co.astype(np.int64) != want))
    assert not len(bad), ("coefficient buffer: %d elements differ" % len(bad), bad[:10], co[bad[:10]], want[bad[:10]])
    rcs = np.array([e[0] for e in exp])
    want_flags = np.array([PC.RC_FLAGS[rc] for rc in rcs], np.uint32) | np.where(narrow & outside, H.RES_RANGE, 0).astype(np.uint32)
    ignore = np.where((rcs == -4) & ~outside, H.RES_RANGE, 0).astype(np.uint32)
    assert np.array_equal(res["flags"] & ~ignore, want_flags)


# ---- 5. escapes and extended range ----------------------------------------------------------------------------------------
def test_escape_coded_blocks_of_every_dynamic_range(hip):
    """Blocks in which most levels are escape codes — Rice prefixes up to 32 - max_log2 ones, suffixes up to max_log2 bits,
    decoded 15 bypass bins at a time by a float quotient — for max_log2_tr_range 15..20 and regular, transform-skip and BDPCM
    blocks, with ordinary context-coded blocks in between so that the range register takes many values in front of the
    bypass runs.  n_bits and every level exact; in the int16 store CABAC_RES_RANGE on exactly the substreams that hold a
    level outside int16 (check() requires the bit where the oracle's levels do, and its absence elsewhere)."""
    corpus, exp = cached(PC.escapes, 0xE5C)
    n_big, limits, kinds = 0, set(), set()
    for metas, blocks, _ in corpus["subs"]:
        for m, c in zip(metas, blocks):
            n_big += int((np.abs(c) >= 1000).sum())
            kinds.add((m[4], m[3] & (H.TU_TRANSFORM_SKIP | H.TU_BDPCM)))
            limits |= {(m[4], v) for v in (-(1 << m[4]), (1 << m[4]) - 1) if (c == v).any()}
    assert n_big >= 100000, n_big
    assert limits == {(r, v) for r in range(15, 21) for v in (-(1 << r), (1 << r) - 1)}
    assert kinds >= {(r, k) for r in range(15, 21) for k in (0, H.TU_TRANSFORM_SKIP, H.TU_TRANSFORM_SKIP | H.TU_BDPCM)}
    res, rcs = check(hip, corpus, exp)
    assert not rcs.any()
    if hip.parse_int16:
        outside = np.array([any((np.abs(c.astype(np.int64) + 0.5) > 32768).any() for c in x[1]) for x in corpus["subs"]])
        assert 20 < outside.sum() < len(outside) - 20
        assert np.array_equal(res["flags"], np.where(outside, H.RES_RANGE, 0))
    else:
        assert not res["flags"].any()


# ---- 6. damaged streams (keep this the last test of the file) -------------------------------------------------------------
def test_damaged_streams_parse_as_the_oracle_parses_them(hip):
    """600 substreams each of: (a) one flipped bit, (b) one flipped bit per 16 bytes, (c) a wrong qp, (d) random bytes,
    (e) the block list reversed, (f) truncation to 3/4 — fixed seed, parsed kind by kind (600 substreams: one-wave workgroups)
    and all together (3 600: four-wave workgroups).  That the walk is bounded on arbitrary bytes is argued loop by loop in
    DESIGN.md (section 3, residual parser, "Bounds"); the oracle runs this corpus under AddressSanitizer / UBSan in
    tests/test_sanitizers.py.
    Flags are compared for every substream (parse_corpus.RC_FLAGS: 0 -> 0, -4 -> UNDERRUN and that alone, instead of any stop
    check, -5 -> BAD_STOP, -2 -> BAD_RECORD; | RANGE in the int16 store where a level the oracle gives lies outside int16).
    n_bits, tu_info and every coefficient are compared wherever the oracle does not end in an underrun; after an underrun the
    oracle stops at the block while the device parses zeros to the end, so there only the blocks before it are compared."""
    corpus, exp = cached(PC.damaged, 0xDA, 600)
    rcs = np.array([e[0] for e in exp])
    for kind in "abcde":
        assert (rcs[corpus["kind"] == kind] != -4).mean() >= 0.75, kind
    assert (rcs[corpus["kind"] == "f"] == -4).all()
    big = [s for s, e in enumerate(exp) if e[0] != -4 and any((np.abs(b[:32, :32].astype(np.int64) + 0.5) > 32768).any() for b in e[1][:e[4]])]
    assert len(big) >= 1
    assert (rcs == -5).sum() >= 50 and (rcs == 0).sum() >= 50
    # ... and substreams that begin with 0xFF, which kernel and oracle refuse as a whole (include/cabac_hip_parse.h)
    refused = [s for s, x in enumerate(corpus["subs"]) if corpus["caps"][s] >= 2 and x[2][0] == 0xFF]
    assert len(refused) >= 3 and all(exp[s][0] == -5 and exp[s][2] == 8 and exp[s][4] == 0 for s in refused)
    for kind in PC.DAMAGE_KINDS:
        pick = np.flatnonzero(corpus["kind"] == kind)
        assert len(pick) == 600
        check(hip, PC.take(corpus, pick), [exp[s] for s in pick], coded_blocks=False)
    res, _ = check(hip, corpus, exp, coded_blocks=False)
    if hip.parse_int16:
        assert all(int(res["flags"][s]) & H.RES_RANGE for s in big)
