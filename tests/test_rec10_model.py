"""CPU: the packed bin records (include/cabac_hip_rec10.h).  The numpy model (tests/rec10_model.py) against blocks written out by
hand, byte by byte; then cabac_hip_rec10_pack_host / _unpack_host against the model: identity R1 at the block edges, the
short-capacity refusal (a canary behind the capacity stays), and the refusal of records with reserved bits."""
import numpy as np
import pytest

import rec10_model as M
from entropy_coding_amd import capi

SIZES = [0, 1, 63, 64, 65, 127, 128, 4097]
LANES = {0: 0, 1: 0x1FE, 7: 255, 8: 256, 31: 378, 32: 0x1FD, 63: 0x1FF}      # lane -> id of the hand-written block
BINS_A = {0: 1, 1: 0, 7: 0, 8: 1, 31: 0, 32: 1, 63: 1}


def _hand_block(flip):
    """(records, the 80 bytes) of the block above with BINS_A, or with every bin of its seven records flipped."""
    rec = np.zeros(64, np.uint16)
    for lane, ident in LANES.items():
        rec[lane] = ident | (BINS_A[lane] ^ flip) << 15
    blk = np.zeros(80, np.uint8)
    blk[1], blk[7], blk[31], blk[32], blk[63] = 0xFE, 0xFF, 0x7A, 0xFD, 0xFF          # bits 7..0 of 0x1FE, 255, 378, 0x1FD, 0x1FF
    blk[64], blk[65], blk[67], blk[68], blk[71] = 0x02, 0x01, 0x80, 0x01, 0x80        # bit 8: lanes 1, 8, 31, 32, 63
    if not flip:
        blk[72], blk[73], blk[76], blk[79] = 0x01, 0x01, 0x01, 0x80                   # bins: lanes 0, 8, 32, 63
    else:
        blk[72], blk[75] = 0x82, 0x80                                                 # bins: lanes 1, 7, 31
    return rec, blk


@pytest.mark.parametrize("flip", [0, 1])
def test_model_against_a_block_written_out_by_hand(flip):
    rec, blk = _hand_block(flip)
    assert M.nbytes(64) == 80 and M.nbytes(0) == 0 and M.nbytes(1) == 80 and M.nbytes(65) == 160
    assert M.pack(rec).tolist() == blk.tolist()
    assert M.unpack(blk, 64).tolist() == rec.tolist()
    assert M.pack(rec[:33]).tolist()[:33] == blk.tolist()[:33] and M.pack(rec[:33])[33:64].tolist() == [0] * 31
    assert capi.rec10_pack_host(rec).tolist() == blk.tolist()
    assert capi.rec10_unpack_host(blk, 0, 64).tolist() == rec.tolist()
    built = np.zeros(80, np.uint8)
    for lane in sorted(LANES, reverse=True):
        M.put(built, lane, int(rec[lane]))
    assert built.tolist() == blk.tolist()
    assert [M.get(blk, r) for r in range(64)] == rec.tolist()


def test_every_pattern_is_a_block_and_put_overwrites():
    rng = np.random.default_rng(10)
    raw = rng.integers(0, 256, size=3 * 80, dtype=np.uint8)
    rec = M.unpack(raw, 192)
    assert not (rec & M.RESERVED_BITS).any() and M.pack(rec).tolist() == raw.tolist()
    assert capi.rec10_unpack_host(raw, 0, 192).tolist() == rec.tolist()
    new = M.random_valid(rng, 192)
    for r in rng.permutation(192):                                   # read-modify-write: neighbours keep their bits
        M.put(raw, int(r), int(new[r]))
    assert raw.tolist() == M.pack(new).tolist()


@pytest.mark.parametrize("n", SIZES)
def test_r1_host_round_trip(n):
    rng = np.random.default_rng(100 + n)
    rec = M.random_valid(rng, n)
    assert capi.rec10_bytes(n) == M.nbytes(n)
    buf = np.full(M.nbytes(n) + 32, 0xC3, np.uint8)
    packed = capi.rec10_pack_host(rec, packed=buf, packed_capacity=M.nbytes(n))
    assert packed.tolist() == M.pack(rec).tolist() and (buf[M.nbytes(n):] == 0xC3).all()      # zero tail written, nothing behind it
    back = capi.rec10_unpack_host(packed, 0, n)
    assert back.tolist() == rec.tolist() and M.unpack(packed, n).tolist() == rec.tolist()
    assert [M.get(packed, r) for r in range(0, n, 7)] == rec[::7].tolist()
    for first, cnt in ((1, n - 1), (63, n - 64), (65, n - 66), (n // 2, n - n // 2 - 1)):   # a range: nothing outside it is written
        if cnt < 0 or first + cnt > n:
            continue
        dst = np.full(n + 3, 0xA5A5, np.uint16)
        capi.rec10_unpack_host(packed, first, cnt, records=dst)
        assert dst[first: first + cnt].tolist() == rec[first: first + cnt].tolist()
        assert (dst[:first] == 0xA5A5).all() and (dst[first + cnt:] == 0xA5A5).all()


@pytest.mark.parametrize("n", [1, 64, 65, 4097])
def test_short_capacity_is_refused_and_nothing_is_written(n):
    rec = M.random_valid(np.random.default_rng(n), n)
    for cap in (M.nbytes(n) - 1, M.nbytes(n) - 80, 0):
        buf = np.full(M.nbytes(n) + 16, 0x5E, np.uint8)
        with pytest.raises(capi.CabacHipError) as e:
            capi.rec10_pack_host(rec, packed=buf, packed_capacity=cap)
        assert e.value.status == -2 and e.value.first_bad == M.NO_BAD
        assert (buf == 0x5E).all()                                   # the canary behind the capacity, and everything in front of it


@pytest.mark.parametrize("bit", [9, 14])
@pytest.mark.parametrize("n", [65, 4097])
def test_reserved_bits_are_refused_with_the_smallest_index(bit, n):
    rng = np.random.default_rng(bit * 10000 + n)
    rec = M.random_valid(rng, n)
    spots = [0, 63, 64, n - 1]
    for at in spots:
        bad = rec.copy()
        bad[at] |= 1 << bit
        with pytest.raises(capi.CabacHipError) as e:
            capi.rec10_pack_host(bad)
        assert e.value.status == -2 and e.value.first_bad == at == M.first_bad(bad)
    for a in spots:
        for b in spots:
            if a < b:
                bad = rec.copy()
                bad[a] |= 1 << bit
                bad[b] |= 1 << (23 - bit)
                with pytest.raises(capi.CabacHipError) as e:
                    capi.rec10_pack_host(bad)
                assert e.value.first_bad == a
    assert capi.rec10_pack_host(rec).tolist() == M.pack(rec).tolist()   # and without them it packs


def test_null_pointers_are_refused():
    L = capi.load_library()
    assert L.cabac_hip_rec10_bytes(5, None) == -2
    assert L.cabac_hip_rec10_pack_host(None, 1, None, 80, None) == -2
    assert L.cabac_hip_rec10_unpack_host(None, 0, 1, None) == -2
    assert L.cabac_hip_rec10_pack_host(None, 0, None, 0, None) == 0 and L.cabac_hip_rec10_unpack_host(None, 5, 0, None) == 0
