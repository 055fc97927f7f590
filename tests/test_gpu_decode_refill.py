"""The decoder's input side (decode_kernel_v4: the bit cursor, the top-up every fourth bin, the LDS ring and its staging)
against the oracle, under the three decode geometries: 4 = four substreams per wave, 8 = sixteen per wave, 1 = one per wave.

Every case encodes with the oracle, decodes with the device and with the oracle, and compares bins, n_bits and flags.
The oracle's side of a case is computed once and shared by the three geometries.  Bit-exact everywhere."""
import functools

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

FIN = H.SUB_FINISH | H.SUB_ALIGN_RBSP
PROBE = 0x400          # CABAC_SUB_PROBE: n_bits = the bits written so far, nothing flushed
RING = 256             # bytes of the decoder's input ring (quad_dec_stage_store)
TRM1 = np.array([H.REC_TRM | H.REC_BIN], np.uint16)


@pytest.fixture(scope="module", params=[4, 8, 1], ids=["quad", "hex", "solo"])
def hip(request):
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    c.set_variant(0, request.param)
    yield c
    c.close()


# ------------------------------------------------------------------ building blocks
def _ep(bits):
    return (H.REC_EP | (np.asarray(bits, np.uint16) << 15)).astype(np.uint16)


def _ctx(ctx_id, bits):
    return (np.uint16(ctx_id) | (np.asarray(bits, np.uint16) << 15)).astype(np.uint16)


def _encode(recs, qp=32, init_id=2, flags=FIN):
    """[records] -> (desc, records, bytes, coded sizes in bytes); roomy slots (6 bits a bin is the most a bin can cost)."""
    lens = [len(r) for r in recs]
    records = np.concatenate(recs + [np.zeros(0, np.uint16)]).astype(np.uint16)
    desc, total = H.make_desc(lens, [qp] * len(recs), [init_id] * len(recs), flags, capacities=[n + 64 for n in lens])
    out, res = H.load_oracle().encode_batch(desc, records, total)
    assert not res["flags"].any()
    return desc, records, out, (res["n_bits"].astype(np.int64) + 7) // 8


def _coded_bytes(rec):
    return int(_encode([rec])[3][0])


def _grow_to(make, n0, target):
    """The records make(n) whose coded size is `target` bytes, n searched upwards from n0 (coded sizes grow with n)."""
    for n in range(n0, n0 + 400):
        rec = make(n)
        if _coded_bytes(rec) == target:
            return rec
    raise AssertionError("no length codes to %d bytes" % target)


def _exact(desc, sizes):
    dd = desc.copy()
    dd["byte_capacity"] = sizes
    return dd


def _with_oracle(dd, records, data):
    bins_o, ro = H.load_oracle().decode_batch(dd, records, data)
    return dd, records, data, bins_o, ro


def _check(hip, case, clean=True):
    dd, records, data, bins_o, ro = case
    assert len(dd) <= 64
    bins_g, rg = hip.decode_batch(dd, records, data, check=False)
    assert np.array_equal(rg["flags"], ro["flags"]), (rg["flags"], ro["flags"])
    assert np.array_equal(rg["n_bits"], ro["n_bits"]), (rg["n_bits"], ro["n_bits"])
    if clean:
        assert not ro["flags"].any()
    for s in range(len(dd)):
        if not ro["flags"][s] & H.RES_UNDERRUN:     # the oracle stops where the reference throws
            o, n = int(dd["rec_offset"][s]), int(dd["n_records"][s])
            assert np.array_equal(bins_g[o:o + n], bins_o[o:o + n]), s


# ------------------------------------------------------------------ ring wrap
@functools.lru_cache(None)
def _ring_wrap_case():
    rng = np.random.default_rng(2501)
    ep_bits = rng.integers(0, 2, size=5000)
    recs = []
    for n in (2100, 4200):      # bypass only: 1 bit a bin, the fastest steady consumption (about 263 and 525 bytes)
        recs.append(np.concatenate([_ep(ep_bits[:n]), TRM1]))
    for n in (2100, 4200):
        recs.append(H.random_records(rng, n, ctx_frac=0.75))
    # the last block ends exactly on a ring boundary, and one byte either side of it; after one and after two rounds
    for target in (RING - 1, RING, RING + 1, 2 * RING - 1, 2 * RING, 2 * RING + 1):
        recs.append(_grow_to(lambda n: np.concatenate([_ep(ep_bits[:n]), TRM1]), 8 * target - 48, target))
    desc, records, out, sizes = _encode(recs)
    assert sizes[0] > RING and sizes[1] > 2 * RING
    assert list(sizes[4:]) == [RING - 1, RING, RING + 1, 2 * RING - 1, 2 * RING, 2 * RING + 1]
    return _with_oracle(_exact(desc, sizes), records, out)


def test_ring_wraps(hip):
    _check(hip, _ring_wrap_case())


# ------------------------------------------------------------------ fastest consumption
def _groups(ctx_id, lead, n_groups):
    """`lead` zeros, then n_groups times (48 zeros, 4 ones), all bins of one context."""
    bits = np.concatenate([np.zeros(lead, np.uint16)] + [np.concatenate([np.zeros(48, np.uint16), np.ones(4, np.uint16)])] * n_groups)
    return _ctx(ctx_id, bits)


def _group_costs(recs, lead, n_groups, qp, init_id):
    """Bits the coder writes for each group of ones of each record string, [string][group]: the difference of the coded
    sizes of the prefixes that end after and before the group (CABAC_SUB_PROBE: the written bits, nothing flushed)."""
    pre = []
    for r in recs:
        for g in range(1, n_groups + 1):
            pre += [r[:lead + 52 * g - 4], r[:lead + 52 * g]]
    lens = [len(r) for r in pre]
    desc, total = H.make_desc(lens, [qp] * len(pre), [init_id] * len(pre), PROBE, capacities=[n + 64 for n in lens])
    _, res = H.load_oracle().encode_batch(desc, np.concatenate(pre), total)
    assert not res["flags"].any()
    nb = res["n_bits"].astype(np.int64).reshape(len(recs), n_groups, 2)
    return nb[:, :, 1] - nb[:, :, 0]


@functools.lru_cache(None)
def _fast_case():
    n_groups = 6
    # the initial state whose four ones after 48 zeros cost most: searched over contexts, slice types and a few QPs
    best = (0, 0, 0, 0)
    for qp in (32, 51, 63):
        for init_id in (0, 1, 2):
            costs = _group_costs([_groups(c, 0, n_groups) for c in range(H.NUM_CTX)], 0, n_groups, qp, init_id).max(axis=1)
            c = int(np.argmax(costs))
            best = max(best, (int(costs[c]), -qp, -init_id, -c))
    qp, init_id, ctx_id = -best[1], -best[2], -best[3]
    recs, worst = [], []
    for lead in (0, 1, 2, 3):     # the group at each of the four positions relative to a top-up
        r = _groups(ctx_id, lead, n_groups)
        worst.append(int(_group_costs([r], lead, n_groups, qp, init_id).max()))
        recs.append(np.concatenate([r, TRM1]))
    desc, records, out, sizes = _encode(recs, qp=qp, init_id=init_id)
    return worst, _with_oracle(_exact(desc, sizes), records, out)


def test_fastest_consumption(hip):
    """Four bins between two top-ups may consume up to 24 bits: the case keeps a group of four consecutive bins of 20 bits
    or more at every position relative to the top-up (asserted, so that it cannot silently stop testing the bound)."""
    worst, case = _fast_case()
    print("bits of the dearest group of four ones, lead 0..3:", worst)
    assert min(worst) >= 20, worst
    _check(hip, case)


# ------------------------------------------------------------------ arbitrary input
@functools.lru_cache(None)
def _arbitrary_case():
    rng = np.random.default_rng(2502)
    n_sub, n = 64, 2000
    pool = np.array([0, 7, 100, 250, 378])
    recs = [H.random_records(rng, n, ctx_frac=1.0, ctx_pool=pool, end_trm=False, trm0_frac=0.0) for _ in range(n_sub)]
    records = np.concatenate(recs)
    desc, total = H.make_desc([n] * n_sub, rng.integers(0, 64, size=n_sub), rng.integers(0, 3, size=n_sub), FIN,
                              capacities=[2048] * n_sub)     # 2000 bins read 1500 bytes at the most: no underrun
    data = rng.integers(0, 256, size=total).astype(np.uint8)
    # (a first byte of 0xFF is no stream of the arithmetic coder: its value would start at or above the range,
    # include/cabac_hip_parse.h)
    first = desc["byte_offset"].astype(np.int64)
    data[first] = rng.integers(0, 255, size=n_sub)
    return _with_oracle(desc, records, data)


def test_random_bytes(hip):
    case = _arbitrary_case()
    assert not (case[4]["flags"] & H.RES_UNDERRUN).any()
    _check(hip, case, clean=False)


# ------------------------------------------------------------------ ragged wave
@functools.lru_cache(None)
def _ragged_case(lens):
    rng = np.random.default_rng(2503)
    recs = [H.random_records(rng, n - 1, ctx_frac=0.7) if n else np.zeros(0, np.uint16) for n in lens]
    desc, records, out, sizes = _encode(recs)
    sizes = np.where(np.array(lens) == 0, 0, sizes)      # zero capacity for the empty ones
    return _with_oracle(_exact(desc, sizes), records, out)


@pytest.mark.parametrize("lens", [(1, 17, 4096, 300), (0, 5, 0, 1000)])
def test_ragged_wave(hip, lens):
    """Rows of a wave that end in different steps: the finished ones are fed zeros while the others still top up.  (An empty
    substream of zero capacity has read two bytes it does not have: underrun, as the reference throws in start().)"""
    _check(hip, _ragged_case(lens), clean=0 not in lens)


# ------------------------------------------------------------------ capacity edges
@functools.lru_cache(None)
def _edge_case(rot):
    rng = np.random.default_rng(2504)
    base = H.random_records(rng, 700, ctx_frac=0.3, end_trm=False)
    recs, n0 = [], 300
    for residue in (0, 1, 2, 3):
        for n in range(n0, 700):
            r = np.concatenate([base[:n], TRM1])
            if _coded_bytes(r) % 4 == residue:
                recs.append(r)
                n0 = n + 1
                break
    assert len(recs) == 4
    recs = recs[rot:] + recs[:rot]
    desc, records, out, sizes = _encode(recs)
    assert sorted(int(x) % 4 for x in sizes) == [0, 1, 2, 3]
    # back to back at the next multiple of 16 (cabac_hip.h), the bytes in between filled with ones so that a decoder reading
    # past its capacity is found out; the buffer ends with the last substream, padded only to the multiple of 4 that
    # cabac_hip.h promises
    dd = _exact(desc, sizes)
    slots = (sizes + 15) // 16 * 16
    dd["byte_offset"] = np.concatenate([[0], np.cumsum(slots)[:-1]])
    data = np.full(int(dd["byte_offset"][3]) + (int(sizes[3]) + 3) // 4 * 4, 0xFF, np.uint8)
    for s in range(4):
        o, p = int(desc["byte_offset"][s]), int(dd["byte_offset"][s])
        data[p:p + int(sizes[s])] = out[o:o + int(sizes[s])]
    return _with_oracle(dd, records, data)


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_capacity_edges(hip, rot):
    _check(hip, _edge_case(rot))


# ------------------------------------------------------------------ truncated streams
@functools.lru_cache(None)
def _truncated_case():
    rng = np.random.default_rng(2505)
    rec = H.random_records(rng, 3000, ctx_frac=0.7)
    desc, records, out, sizes = _encode([rec] * 7, flags=FIN)
    # (6 bits a bin at the most: the slot holds whatever a decoder fed zeros can ask for)
    dd, total = H.make_desc([len(rec)] * 7, [32] * 7, [2] * 7, FIN, capacities=[2400] * 7)
    data = np.zeros(total, np.uint8)
    size = int(sizes[0])
    caps = [1, 2, 3, 8, 9, size // 2, size]
    for s, cap in enumerate(caps):
        o, p = int(desc["byte_offset"][s]), int(dd["byte_offset"][s])
        data[p:p + size] = out[o:o + size]
    roomy = dd.copy()
    dd["byte_capacity"] = caps
    # what the decoder is fed past the capacity: the rest of the dword that holds the last byte as it is in the buffer
    # (input is read as whole aligned dwords, cabac_hip.h), then zeros — the same bytes cut there, with room to read them
    zext = data.copy()
    for s, cap in enumerate(caps):
        p = int(dd["byte_offset"][s])
        zext[p + (cap + 3) // 4 * 4:p + 2400] = 0
    bins_z, rz = H.load_oracle().decode_batch(roomy, records, zext)
    assert not (rz["flags"] & H.RES_UNDERRUN).any()
    return _with_oracle(dd, records, data), (bins_z, rz)


def test_truncated_streams(hip):
    """Flags are the oracle's.  n_bits: the oracle returns from the read that underruns, as the reference throws there, and
    reports no bit count for that substream, so there is nothing of the oracle's own to compare with; what the device reports
    is held to the oracle's count on the same bytes zero-extended to a capacity that does not underrun (the decoder is fed
    zeros past the dword that holds the last byte).  include/cabac_hip.h leaves n_bits after an underrun unspecified: this
    test pins what the decoder does there today, more than the header promises, so that a change of the input code that
    alters it is seen.  Bins are compared only for the substream the oracle does not flag."""
    case, (bins_z, rz) = _truncated_case()
    dd, records, data, bins_o, ro = case
    bins_g, rg = hip.decode_batch(dd, records, data, check=False)
    assert np.array_equal(rg["flags"], ro["flags"]), (rg["flags"], ro["flags"])
    assert list(ro["flags"][:6]) == [H.RES_UNDERRUN] * 6 and ro["flags"][6] == 0
    ran = ro["flags"] == 0
    assert np.array_equal(rg["n_bits"][ran], ro["n_bits"][ran])
    assert np.array_equal(rg["n_bits"], rz["n_bits"]), (rg["n_bits"], rz["n_bits"])
    o, n = int(dd["rec_offset"][6]), int(dd["n_records"][6])
    assert np.array_equal(bins_g[o:o + n], bins_o[o:o + n])


# ------------------------------------------------------------------ write bounds
@functools.lru_cache(None)
def _bounds_case():
    rng = np.random.default_rng(2506)
    lens = [1, 17, 300, 1000, 5, 63, 64, 65, 0, 2049]
    recs = [H.random_records(rng, n - 1, ctx_frac=0.7) if n else np.zeros(0, np.uint16) for n in lens]
    desc, records, out, sizes = _encode(recs)
    gap = 16
    dd = _exact(desc, np.where(np.array(lens) == 0, 0, sizes))
    dd["rec_offset"] = gap + np.concatenate([[0], np.cumsum(np.array(lens) + gap)[:-1]])
    spaced = np.zeros(int(dd["rec_offset"][-1]) + lens[-1] + gap, np.uint16)
    for s in range(len(lens)):
        o, p = int(desc["rec_offset"][s]), int(dd["rec_offset"][s])
        spaced[p:p + lens[s]] = records[o:o + lens[s]]
    return _with_oracle(dd, spaced, out)


def test_write_bounds(hip):
    """The bins buffer carries a canary before and after every substream's slot; none is touched."""
    import torch
    dd, records, data, bins_o, ro = _bounds_case()
    n_sub = len(dd)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()
    t_desc, t_rec = dev(dd, np.uint8), dev(records, np.int16)
    t_bytes = dev(np.concatenate([data, np.zeros(4, np.uint8)]), np.uint8)
    t_bins = torch.full((len(records),), 0xAB, dtype=torch.uint8, device="cuda")
    t_res = torch.zeros(2 * n_sub, dtype=torch.int32, device="cuda")
    hip.decode_device(n_sub, t_desc.data_ptr(), t_rec.data_ptr(), t_bytes.data_ptr(), t_bins.data_ptr(), t_res.data_ptr())
    hip.synchronize()
    rg = t_res.cpu().numpy().view(H.RESULT_DTYPE)
    got = t_bins.cpu().numpy()
    assert np.array_equal(rg["flags"], ro["flags"]) and np.array_equal(rg["n_bits"], ro["n_bits"])
    slot = np.zeros(len(records), bool)
    for s in range(n_sub):
        o, n = int(dd["rec_offset"][s]), int(dd["n_records"][s])
        slot[o:o + n] = True
        assert np.array_equal(got[o:o + n], bins_o[o:o + n]), s
    assert (got[~slot] == 0xAB).all(), np.flatnonzero(got[~slot] != 0xAB)[:8]
