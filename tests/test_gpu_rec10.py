"""GPU: the packed bin records (include/cabac_hip_rec10.h).  R2: cabac_hip_rec10_unpack_device against the model on arbitrary bytes
and ranges, nothing outside the range written.  R3: cabac_hip_rec10_pack_device against cabac_hip_rec10_pack_host byte for byte,
the status word, a capacity that is short.  R4: the three host-pointer forms against their 16-bit forms on the same ctx and
against the oracle — every chunk count, pinned and pageable, chunk boundaries inside a block, unordered descriptors, a bad record,
a batch larger than the bounce ring, the refusals, a payload that is too small, and the profile ring.
Device tensors are sized exactly; canaries stand only behind (and, for a records pointer that is not 16-byte aligned, in front of)
outputs."""
import functools
import os

import numpy as np
import pytest

import helpers as H
import rec10_model as M
from entropy_coding_amd import capi

pytestmark = pytest.mark.gpu

TOTALS = [1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 100003]
FILL = 0xA5A5
GUARD = 64           # canary bytes behind an output


@pytest.fixture(scope="module")
def hip():
    h = H.gpu_ctx()
    yield h
    h.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _filled(n_bytes, byte):
    import torch
    return torch.full((n_bytes,), byte, dtype=torch.uint8, device="cuda")


def _status(t):
    return t.cpu().numpy()[:16].view(capi.REC10_STATUS_DTYPE)[0]


def _torch_done():
    """torch's fills of the tensors above are finished: for a ctx that runs on a stream of its own"""
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ R2: unpack on the device
@pytest.mark.parametrize("front", [0, 3])        # 3: the records pointer is not 16-byte aligned (every group stores one by one)
@pytest.mark.parametrize("total", TOTALS)
def test_r2_unpack_device_is_unpack_host_on_arbitrary_bytes_and_ranges(hip, total, front):
    rng = np.random.default_rng(2000 + total)
    raw = rng.integers(0, 256, size=M.nbytes(total), dtype=np.uint8)       # every pattern is a valid block
    want_all = M.unpack(raw, total)
    assert capi.rec10_unpack_host(raw, 0, total).tolist() == want_all.tolist()
    t_packed = _dev(raw)
    for first in (0, 1, 63, 65, total // 2 + 3):
        for stop_short in (0, 1):
            n = total - first - stop_short
            if n < 0:
                continue
            t_rec = _filled(2 * (front + total) + GUARD, 0xA5)
            hip.rec10_unpack_device(t_packed.data_ptr(), first, n, t_rec.data_ptr() + 2 * front)
            hip.synchronize()
            got = t_rec.cpu().numpy()
            assert (got[2 * (front + total):] == 0xA5).all() and (got[: 2 * front] == 0xA5).all()
            rec = got[2 * front: 2 * (front + total)].view(np.uint16)
            want = np.full(total, FILL, np.uint16)
            want[first: first + n] = want_all[first: first + n]
            assert np.array_equal(rec, want), (first, n, np.nonzero(rec != want)[0][:8])


def test_unpack_of_no_records_writes_nothing(hip):
    t_packed, t_rec = _dev(np.zeros(160, np.uint8)), _filled(256, 0xA5)
    for first in (0, 5, 64):
        hip.rec10_unpack_device(t_packed.data_ptr(), first, 0, t_rec.data_ptr())
    hip.rec10_unpack_device(0, 0, 0, 0)
    hip.synchronize()
    assert (t_rec.cpu().numpy() == 0xA5).all()


# ------------------------------------------------------------------------------------------------ R3: pack on the device
def _pack_device(hip, rec, capacity=None, front=0):
    """pack_device on `rec` (a tensor of exactly its size, `front` elements into it); returns (packed bytes with the canary, status)"""
    need = M.nbytes(len(rec))
    t_rec = _dev(np.concatenate([np.zeros(front, np.uint16), rec]))
    t_out, t_st = _filled(need + GUARD, 0xC3), _filled(16, 0x77)
    hip.rec10_pack_device(t_rec.data_ptr() + 2 * front, len(rec), t_out.data_ptr(), need if capacity is None else capacity, t_st.data_ptr())
    hip.synchronize()
    assert np.array_equal(t_rec.cpu().numpy()[2 * front:].view(np.uint16), rec)   # the input is input
    return t_out.cpu().numpy(), _status(t_st)


@pytest.mark.parametrize("front", [0, 1])
@pytest.mark.parametrize("total", TOTALS)
def test_r3_pack_device_is_pack_host_byte_for_byte(hip, total, front):
    rng = np.random.default_rng(3000 + total)
    rec = M.random_valid(rng, total)
    want = capi.rec10_pack_host(rec)
    assert want.tolist() == M.pack(rec).tolist()
    got, st = _pack_device(hip, rec, front=front)
    assert np.array_equal(got[: len(want)], want), np.nonzero(got[: len(want)] != want)[0][:8]
    assert (got[len(want):] == 0xC3).all()
    assert int(st["flags"]) == 0 and int(st["first_bad"]) == capi.REC10_NO_BAD and int(st["reserved"]) == 0


@pytest.mark.parametrize("total", [65, 513, 100003])
def test_r3_bad_records_raise_the_flag_and_the_smallest_index(hip, total):
    rng = np.random.default_rng(3500 + total)
    rec = M.random_valid(rng, total)
    clean = capi.rec10_pack_host(rec)
    spots = [0, 63, 64, total - 1]
    cases = [(a,) for a in spots] + [(a, b) for a in spots for b in spots if a < b]
    for k, case in enumerate(cases):
        bad = rec.copy()
        for i, at in enumerate(case):
            bad[at] |= 1 << (9 + (k + 5 * i) % 6)
        with pytest.raises(capi.CabacHipError) as e:
            capi.rec10_pack_host(bad)
        assert e.value.first_bad == case[0]
        got, st = _pack_device(hip, bad)
        assert int(st["flags"]) == capi.REC10_BAD_BITS and int(st["first_bad"]) == case[0], (case, st)
        assert np.array_equal(got[: len(clean)], clean) and (got[len(clean):] == 0xC3).all()      # the bits are dropped


@pytest.mark.parametrize("total", [1, 64, 65, 4097])
def test_r3_short_capacity_raises_overflow_and_writes_nothing(hip, total):
    rec = M.random_valid(np.random.default_rng(total), total)
    rec[0] |= 0x0200                                                 # a bad record too: only the overflow is reported
    for cap in (M.nbytes(total) - 1, M.nbytes(total) - 80, 0):
        got, st = _pack_device(hip, rec, capacity=cap)
        assert int(st["flags"]) == capi.REC10_OVERFLOW and int(st["first_bad"]) == capi.REC10_NO_BAD
        assert (got == 0xC3).all()


def test_device_round_trip_without_a_host_wait(hip):
    total = 100003
    rec = M.random_valid(np.random.default_rng(77), total)
    t_rec, t_packed, t_st = _dev(rec), _filled(M.nbytes(total) + GUARD, 0xC3), _filled(16, 0x77)
    t_back = _filled(2 * total + GUARD, 0xA5)
    hip.rec10_pack_device(t_rec.data_ptr(), total, t_packed.data_ptr(), M.nbytes(total), t_st.data_ptr())
    hip.rec10_unpack_device(t_packed.data_ptr(), 0, total, t_back.data_ptr())          # stream order is the ordering
    hip.synchronize()
    back = t_back.cpu().numpy()
    assert np.array_equal(back[: 2 * total].view(np.uint16), rec) and (back[2 * total:] == 0xA5).all()
    assert int(_status(t_st)["flags"]) == 0 and (t_packed.cpu().numpy()[M.nbytes(total):] == 0xC3).all()


# ------------------------------------------------------------------------------------------------ R4: the host-pointer forms
def _ragged_batch(rng, n_sub, max_len):
    lens = [0, 1, 2, 17][: min(4, n_sub)] + [int(x) for x in rng.integers(0, max_len, size=max(n_sub - 4, 0))]
    recs = [H.random_records(rng, max(n - 1, 0), end_trm=(n > 0)) for n in lens]
    lens = [len(r) for r in recs]
    records = np.concatenate(recs)
    desc, total = H.make_desc(lens, rng.integers(0, 64, size=n_sub), rng.integers(0, 3, size=n_sub), H.SUB_FINISH | H.SUB_ALIGN_RBSP)
    return desc, records, total


def _first_chunk_substreams(desc, chunks):
    """How many substreams the first of `chunks` chunks holds: a batch is cut at substream boundaries into runs of about equal
    record counts, the first one ending with the substream at which the records so far reach total / chunks"""
    done = np.cumsum(desc["n_records"].astype(np.int64))
    return len(desc) if chunks == 1 else int(np.searchsorted(done, int(done[-1]) // chunks, side="left")) + 1


RAGGED_SEED = 4100


@functools.lru_cache(maxsize=None)
def _ragged_case():
    """The ragged batch of the R4 tests and what the oracle makes of it: computed once, shared, never written to."""
    rng = np.random.default_rng(RAGGED_SEED)
    desc, records, total = _ragged_batch(rng, 600, 400)
    orc = H.load_oracle()
    out_o, res_o = orc.encode_batch(desc, records, total)
    nbytes = np.minimum((res_o["n_bits"].astype(np.int64) + 7) // 8, desc["byte_capacity"].astype(np.int64))
    dd = desc.copy()
    dd["byte_capacity"] = (res_o["n_bits"] + 7) // 8
    bins_o, rd_o = orc.decode_batch(dd, records, out_o)
    case = dict(desc=desc, records=records, total=total, out_o=out_o, res_o=res_o, nbytes=nbytes, dd=dd, bins_o=bins_o, rd_o=rd_o,
                packed=capi.rec10_pack_host(records))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _host(a, pinned, keep):
    """a copy of `a` in pinned or in pageable memory"""
    if pinned:
        keep.append(capi.PinnedArray(a.shape, a.dtype))
        b = keep[-1].array
        b[...] = a
    else:
        b = a.copy()
    assert capi.host_is_pinned(b) == pinned
    return b


def _same_result(a, b):
    return np.array_equal(a["n_bits"], b["n_bits"]) and np.array_equal(a["flags"], b["flags"])


def _check_r4(hip, desc, records, total, pinned, out_o=None, res_o=None, dd=None, bins_o=None, rd_o=None, packed=None, nbytes=None):
    """Every rec10 form against its 16-bit form on the same ctx: everything that comes back, bit for bit (R4); and against the oracle
    where its outputs are given."""
    keep = []
    try:
        n = len(records)
        packed = capi.rec10_pack_host(records) if packed is None else packed
        assert len(packed) == M.nbytes(n)
        h_rec, h_packed = _host(records, pinned, keep), _host(packed, pinned, keep)
        out_u, res_u = hip.encode_batch(desc, h_rec, total, check=False, out=_host(np.zeros(max(total, 1), np.uint8), pinned, keep))
        out_r, res_r = hip.rec10_encode_batch(desc, h_packed, n, total, check=False, out=_host(np.zeros(max(total, 1), np.uint8), pinned, keep))
        assert _same_result(res_r, res_u) and np.array_equal(out_r, out_u)
        if res_o is not None:
            assert _same_result(res_r, res_o)
            for s in range(len(desc)):
                o, nb = int(desc["byte_offset"][s]), (int(res_o["n_bits"][s]) + 7) // 8
                assert np.array_equal(out_r[o:o + nb], out_o[o:o + nb]), s
        # the payload form, with its offsets
        if nbytes is None:
            nbytes = np.minimum((res_u["n_bits"].astype(np.int64) + 7) // 8, desc["byte_capacity"].astype(np.int64))
        need = int(nbytes.sum())
        pay_u, pay_r = (_host(np.full(need + GUARD, 0xD7, np.uint8), pinned, keep) for _ in range(2))
        off_u, pres_u = hip.encode_batch_payload(desc, h_rec, pay_u[:need], check=False)
        off_r, pres_r = hip.rec10_encode_batch_payload(desc, h_packed, n, pay_r[:need], check=False)
        assert np.array_equal(off_r, off_u) and _same_result(pres_r, pres_u) and np.array_equal(pay_r, pay_u)
        assert np.array_equal(off_r, np.concatenate([[0], np.cumsum(nbytes)]).astype(np.uint64)) and (pay_r[need:] == 0xD7).all()
        if out_o is not None:
            for s in range(len(desc)):
                o = int(desc["byte_offset"][s])
                assert np.array_equal(pay_r[int(off_r[s]): int(off_r[s + 1])], out_o[o:o + int(nbytes[s])]), s
        # decode: one bin per byte, and eight
        if dd is None:
            dd = desc.copy()
            dd["byte_capacity"] = np.minimum((res_u["n_bits"] + 7) // 8, desc["byte_capacity"])
        h_data = _host(out_u, pinned, keep)
        bins_u, rd_u = hip.decode_batch(dd, h_rec, h_data, check=False, bins=_host(np.zeros(n + 1, np.uint8), pinned, keep))
        bins_r, rd_r = hip.rec10_decode_batch(dd, h_packed, n, h_data, check=False, bins=_host(np.zeros(n + 1, np.uint8), pinned, keep))
        inside = np.zeros(n, bool)                                   # (records between substreams, if any, are nobody's)
        for s in range(len(dd)):
            inside[int(dd["rec_offset"][s]): int(dd["rec_offset"][s]) + int(dd["n_records"][s])] = True
        assert _same_result(rd_r, rd_u) and np.array_equal(bins_r[inside], bins_u[inside])
        pk_u, rp_u = hip.decode_batch_packed(dd, h_rec, h_data, check=False, packed=_host(np.zeros((n + 7) // 8 + 1, np.uint8), pinned, keep))
        pk_r, rp_r = hip.rec10_decode_batch(dd, h_packed, n, h_data, bins_packed=True, check=False,
                                            bins=_host(np.zeros((n + 7) // 8 + 1, np.uint8), pinned, keep))
        assert _same_result(rp_r, rp_u) and len(pk_r) == len(pk_u) == (n + 7) // 8
        un_r, un_u = (np.unpackbits(p, bitorder="little")[:n] for p in (pk_r, pk_u))
        assert np.array_equal(un_r[inside], un_u[inside]) and np.array_equal(un_r[inside], bins_r[inside])
        if bins_o is not None:
            assert _same_result(rd_r, rd_o) and np.array_equal(bins_r[inside], bins_o[inside])
        # the bin plane of the input is ignored by the decode
        no_bins = packed.copy().reshape(-1, 80)
        no_bins[:, 72:] = 0x5A
        bins_z, rd_z = hip.rec10_decode_batch(dd, _host(no_bins.reshape(-1), pinned, keep), n, h_data, check=False)
        assert _same_result(rd_z, rd_r) and np.array_equal(bins_z[inside], bins_r[inside])
    finally:
        for k in keep:
            k.close()


def test_the_ragged_batch_cuts_chunks_inside_a_block():
    """(no GPU work) with 2 and with 3 chunks the first chunk ends at a record index that is no multiple of 64, so that two chunks
    share a block; the seed was picked on the CPU so that this holds"""
    c = _ragged_case()
    done = np.cumsum(c["desc"]["n_records"].astype(np.int64))
    assert len(c["desc"]) == 600 and int(c["desc"]["n_records"].max()) <= 400 and (c["desc"]["n_records"] == 0).any()
    for chunks in (2, 3):
        cut = int(done[_first_chunk_substreams(c["desc"], chunks) - 1])
        assert 0 < cut < int(done[-1]) and cut % 64 != 0, (chunks, cut)


@pytest.mark.parametrize("chunks", [1, 2, 3])
@pytest.mark.parametrize("pinned", [False, True])
def test_r4_host_forms_match_the_u16_forms_and_the_oracle(chunks, pinned):
    os.environ["CABAC_HIP_CHUNKS"] = str(chunks)   # read when the ctx sets up its streams
    try:
        own = capi.CabacHip(0)
        c = _ragged_case()
        if chunks > 1:
            done = np.cumsum(c["desc"]["n_records"].astype(np.int64))
            assert int(done[_first_chunk_substreams(c["desc"], chunks) - 1]) % 64 != 0
        _check_r4(own, c["desc"], c["records"], c["total"], pinned, out_o=c["out_o"], res_o=c["res_o"], dd=c["dd"], bins_o=c["bins_o"],
                  rd_o=c["rd_o"], packed=c["packed"], nbytes=c["nbytes"])
        own.close()
    finally:
        del os.environ["CABAC_HIP_CHUNKS"]


def test_r4_unordered_descriptors_fall_back_to_one_chunk():
    os.environ["CABAC_HIP_CHUNKS"] = "4"
    try:
        own = capi.CabacHip(0)
        c = _ragged_case()
        perm = np.random.default_rng(8).permutation(len(c["desc"]))
        _check_r4(own, c["desc"][perm].copy(), c["records"], c["total"], False, out_o=c["out_o"], res_o=c["res_o"][perm],
                  dd=c["dd"][perm].copy(), bins_o=c["bins_o"], rd_o=c["rd_o"][perm], packed=c["packed"], nbytes=c["nbytes"][perm])
        own.close()
    finally:
        del os.environ["CABAC_HIP_CHUNKS"]


def test_r4_a_bad_record_flags_its_substream_alone():
    own = capi.CabacHip(0)
    rng = np.random.default_rng(31)
    desc, records, total = _ragged_batch(rng, 40, 300)
    s = 17
    assert int(desc["n_records"][s]) > 10
    at = int(desc["rec_offset"][s]) + 5
    records[at] = 400 | (records[at] & 0x8000)                       # a 9-bit id that is no context and no special id: it packs
    packed = capi.rec10_pack_host(records)
    assert int(M.unpack(packed, len(records))[at]) & 0x1FF == 400
    n = len(records)
    out_u, res_u = own.encode_batch(desc, records, total, check=False)
    out_r, res_r = own.rec10_encode_batch(desc, packed, n, total, check=False)
    want = np.zeros(len(desc), np.uint32)
    want[s] = H.RES_BAD_RECORD
    assert np.array_equal(res_r["flags"], want) and _same_result(res_r, res_u)
    good = [q for q in range(len(desc)) if q != s]
    for q in good:                                                   # (what a flagged substream leaves in its slot is unspecified)
        o, cap = int(desc["byte_offset"][q]), int(desc["byte_capacity"][q])
        assert np.array_equal(out_r[o:o + cap], out_u[o:o + cap]), q
    with pytest.raises(capi.CabacHipError) as e:
        own.rec10_encode_batch(desc, packed, n, total)
    assert e.value.status == -5
    pay_u, pay_r = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
    off_u, pres_u = own.encode_batch_payload(desc, records, pay_u, check=False)
    off_r, pres_r = own.rec10_encode_batch_payload(desc, packed, n, pay_r, check=False)
    assert _same_result(pres_r, pres_u) and _same_result(pres_r, res_r) and np.array_equal(off_r, off_u)
    for q in good:
        assert np.array_equal(pay_r[int(off_r[q]): int(off_r[q + 1])], pay_u[int(off_u[q]): int(off_u[q + 1])]), q
    dd = desc.copy()
    dd["byte_capacity"] = np.minimum((res_u["n_bits"] + 7) // 8, desc["byte_capacity"])
    bins_u, rd_u = own.decode_batch(dd, records, out_u, check=False)
    bins_r, rd_r = own.rec10_decode_batch(dd, packed, n, out_u, check=False)
    assert _same_result(rd_r, rd_u)
    for q in [q for q in good if not rd_u["flags"][q]]:              # (an empty substream underruns its one byte on both)
        lo, hi = int(dd["rec_offset"][q]), int(dd["rec_offset"][q]) + int(dd["n_records"][q])
        assert np.array_equal(bins_r[lo:hi], bins_u[lo:hi]) and np.array_equal(bins_r[lo:hi], (records[lo:hi] >> 15).astype(np.uint8)), q
    own.close()


def test_r4_large_pageable_batch_uses_the_whole_ring():
    """More than ring depth x block size of packed records (25.6 MB) from pageable memory."""
    own = capi.CabacHip(0)
    rng = np.random.default_rng(5)
    n_sub = 4096
    recs = H.random_records(rng, 4999)
    records = np.tile(recs, n_sub)
    packed = capi.rec10_pack_host(records)
    assert len(packed) == 25_600_000 and not capi.host_is_pinned(packed)
    desc, total = H.make_desc([len(recs)] * n_sub, [30] * n_sub, [2] * n_sub, H.SUB_FINISH | H.SUB_ALIGN_RBSP)
    out, res = own.rec10_encode_batch(desc, packed, len(records), total)
    one, nbits = H.load_oracle().encode_records(recs, 30, 2, 3)
    assert (res["n_bits"] == nbits).all() and not res["flags"].any()
    for s in range(0, n_sub, 113):
        o = int(desc["byte_offset"][s])
        assert np.array_equal(out[o:o + len(one)], one)
    dd = desc.copy()
    dd["byte_capacity"] = (res["n_bits"] + 7) // 8
    bins, rd = own.rec10_decode_batch(dd, packed, len(records), out)
    assert not rd["flags"].any() and np.array_equal(bins, (records >> 15).astype(np.uint8))
    own.close()


def test_refusals_queue_nothing_and_the_next_call_is_correct():
    own = capi.CabacHip(0)
    c = _ragged_case()
    desc, records, total, packed = c["desc"], c["records"], c["total"], c["packed"]
    n = len(records)
    waits = own.workspace_waits()
    refusals = [
        lambda: own.rec10_encode_batch(desc, None, n, total, packed_bytes=len(packed)),
        lambda: own.rec10_decode_batch(c["dd"], None, n, c["out_o"], packed_bytes=len(packed)),
        lambda: own.rec10_encode_batch_payload(desc, None, n, np.zeros(16, np.uint8), packed_bytes=len(packed)),
        lambda: own.rec10_encode_batch_payload(desc, packed, n, None, payload_capacity=16),
        lambda: own.rec10_encode_batch(desc, packed, n, total, packed_bytes=len(packed) - 1),
        lambda: own.rec10_encode_batch_payload(desc, packed, n, np.zeros(16, np.uint8), packed_bytes=len(packed) - 1),
        lambda: own.rec10_decode_batch(c["dd"], packed, n, c["out_o"], packed_bytes=len(packed) - 1),
        lambda: own.rec10_decode_batch(c["dd"], packed, n, c["out_o"], bins_packed=True, packed_bytes=len(packed) - 80),
    ]
    for k, call in enumerate(refusals):
        with pytest.raises(capi.CabacHipError) as e:
            call()
        assert e.value.status == -2, k
        assert ("null" in str(e.value)) == (k < 4) and ("packed_bytes" in str(e.value)) == (k >= 4), (k, str(e.value))
    assert own.workspace_waits() == waits                            # nothing was queued, nothing was waited for
    # device forms: a null pointer, and a packed pointer that is not 16-byte aligned (refused from its value alone)
    t_packed, t_rec, t_st = _dev(packed[:160]), _filled(256 + GUARD, 0xA5), _filled(16, 0x77)
    _torch_done()
    for off in (1, 2, 4, 8):
        with pytest.raises(capi.CabacHipError) as e:
            own.rec10_unpack_device(t_packed.data_ptr() + off, 0, 64, t_rec.data_ptr())
        assert e.value.status == -2 and "16-byte aligned" in str(e.value)
        with pytest.raises(capi.CabacHipError) as e:
            own.rec10_pack_device(t_rec.data_ptr(), 64, t_packed.data_ptr() + off, 80, t_st.data_ptr())
        assert e.value.status == -2 and "16-byte aligned" in str(e.value)
    for call in (lambda: own.rec10_unpack_device(0, 0, 64, t_rec.data_ptr()), lambda: own.rec10_unpack_device(t_packed.data_ptr(), 0, 64, 0),
                 lambda: own.rec10_pack_device(0, 64, t_packed.data_ptr(), 80, t_st.data_ptr()),
                 lambda: own.rec10_pack_device(t_rec.data_ptr(), 64, 0, 80, t_st.data_ptr()),
                 lambda: own.rec10_pack_device(t_rec.data_ptr(), 64, t_packed.data_ptr(), 80, 0)):
        with pytest.raises(capi.CabacHipError) as e:
            call()
        assert e.value.status == -2 and "null" in str(e.value)
    own.synchronize()
    assert (t_rec.cpu().numpy() == 0xA5).all() and (t_st.cpu().numpy() == 0x77).all()
    assert np.array_equal(t_packed.cpu().numpy(), packed[:160])
    _check_r4(own, desc, records, total, False, out_o=c["out_o"], res_o=c["res_o"], dd=c["dd"], bins_o=c["bins_o"], rd_o=c["rd_o"],
              packed=packed, nbytes=c["nbytes"])
    own.close()


@pytest.mark.parametrize("pinned", [False, True])
def test_a_payload_that_holds_the_first_chunk_only_is_refused_and_left_alone(pinned):
    os.environ["CABAC_HIP_CHUNKS"] = "2"
    keep = []
    try:
        own = capi.CabacHip(0)
        c = _ragged_case()
        desc, packed, n = c["desc"], c["packed"], len(c["records"])
        want_off = np.concatenate([[0], np.cumsum(c["nbytes"])]).astype(np.uint64)
        need = int(want_off[-1])
        first = int(want_off[_first_chunk_substreams(desc, 2)])
        assert 1 < first < need
        mine = _host(np.full(first + GUARD, 0xD7, np.uint8), pinned, keep)       # the payload is its first `first` bytes
        with pytest.raises(capi.CabacHipError) as e:
            own.rec10_encode_batch_payload(desc, packed, n, mine[:first], check=False)
        assert e.value.status == -2 and "payload_capacity too small" in str(e.value)
        snapshot = mine.copy()
        assert (mine[first:] == 0xD7).all()                          # behind what could be delivered: untouched
        payload = _host(np.full(need + GUARD, 0xD7, np.uint8), pinned, keep)
        offs, res = own.rec10_encode_batch_payload(desc, packed, n, payload[:need], check=False)
        assert _same_result(res, c["res_o"]) and np.array_equal(offs, want_off) and (payload[need:] == 0xD7).all()
        for s in range(len(desc)):
            o = int(desc["byte_offset"][s])
            assert np.array_equal(payload[int(offs[s]): int(offs[s + 1])], c["out_o"][o:o + int(c["nbytes"][s])]), s
        assert np.array_equal(mine, snapshot)                        # not written to once its call had returned
        own.close()
    finally:
        del os.environ["CABAC_HIP_CHUNKS"]
        for k in keep:
            k.close()


@pytest.mark.parametrize("chunks", [1, 2])
def test_profile_ring_reports_the_unpack_in_front_of_the_encode(chunks):
    os.environ["CABAC_HIP_CHUNKS"] = str(chunks)
    try:
        own = capi.CabacHip(0)
        c = _ragged_case()
        own.profile_enable(16)
        own.rec10_encode_batch(c["desc"], c["packed"], len(c["records"]), c["total"], check=False)
        prof = own.profile_read()
        assert [k for k, _ in prof] == [43, 0] * chunks and all(ms >= 0 for _, ms in prof), prof
        own.rec10_decode_batch(c["dd"], c["packed"], len(c["records"]), c["out_o"], check=False)
        assert [k for k, _ in own.profile_read()] == [43, 1] * chunks
        t_packed, t_rec, t_st = _dev(c["packed"][:160]), _filled(256, 0xA5), _filled(16, 0x77)
        _torch_done()
        own.rec10_unpack_device(t_packed.data_ptr(), 0, 128, t_rec.data_ptr())
        own.rec10_pack_device(t_rec.data_ptr(), 128, t_packed.data_ptr(), 160, t_st.data_ptr())
        own.synchronize()
        assert [k for k, _ in own.profile_read()] == [43, 44]
        own.encode_batch(c["desc"], c["records"], c["total"], check=False)     # the 16-bit form: as before, no unpack
        assert [k for k, _ in own.profile_read()] == [0] * chunks
        own.close()
    finally:
        del os.environ["CABAC_HIP_CHUNKS"]
