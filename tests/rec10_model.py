"""A numpy model of the packed bin records of include/cabac_hip_rec10.h ("rec10"), written from the header's DEFINITION OF THE
RESULT alone: block b holds records 64 b .. 64 b + 63 in 80 bytes — 64 id bytes (bits 7..0 of the ids), a little-endian uint64 of
the ids' bit 8 and a little-endian uint64 of the bins (bit 15 of the record).  Records behind n in the last block are zero."""
import numpy as np

BLOCK_RECORDS, BLOCK_BYTES = 64, 80
RESERVED_BITS = 0x7E00                   # bits 14..9 of a record
NO_BAD = 0xFFFFFFFFFFFFFFFF


def nbytes(n):
    return (int(n) + 63) // 64 * 80


def first_bad(records):
    """The smallest index of a record with reserved bits set, else NO_BAD."""
    bad = np.flatnonzero(np.asarray(records, np.uint16) & RESERVED_BITS)
    return int(bad[0]) if len(bad) else NO_BAD


def pack(records):
    """uint16 records -> uint8[nbytes(n)]; reserved bits are dropped."""
    records = np.asarray(records, np.uint16)
    n_blocks = (len(records) + 63) // 64
    r = np.zeros(n_blocks * 64, np.uint16)
    r[: len(records)] = records
    r = r.reshape(n_blocks, 64)
    out = np.zeros((n_blocks, BLOCK_BYTES), np.uint8)
    out[:, :64] = (r & 0xFF).astype(np.uint8)
    out[:, 64:72] = np.packbits(((r >> 8) & 1).astype(np.uint8), axis=1, bitorder="little")
    out[:, 72:80] = np.packbits((r >> 15).astype(np.uint8), axis=1, bitorder="little")
    return out.reshape(-1)


def unpack(packed, n):
    """The first n records of a packed buffer (any bytes are valid) as uint16."""
    n_blocks = (int(n) + 63) // 64
    p = np.asarray(packed, np.uint8)[: n_blocks * BLOCK_BYTES].reshape(n_blocks, BLOCK_BYTES)
    hi = np.unpackbits(p[:, 64:72], axis=1, bitorder="little").astype(np.uint16)
    bins = np.unpackbits(p[:, 72:80], axis=1, bitorder="little").astype(np.uint16)
    return (p[:, :64].astype(np.uint16) | hi << 8 | bins << 15).reshape(-1)[: int(n)]


def put(packed, r, record):
    """cabac_rec10_put: read-modify-write on the three places of record r."""
    blk, i = packed[(r >> 6) * 80: (r >> 6) * 80 + 80], r & 63
    blk[i] = record & 0xFF
    for plane, bit in ((64, (record >> 8) & 1), (72, (record >> 15) & 1)):
        blk[plane + (i >> 3)] = (int(blk[plane + (i >> 3)]) & ~(1 << (i & 7)) & 0xFF) | bit << (i & 7)


def get(packed, r):
    """cabac_rec10_get."""
    blk, i = packed[(r >> 6) * 80: (r >> 6) * 80 + 80], r & 63
    return int(blk[i]) | ((int(blk[64 + (i >> 3)]) >> (i & 7)) & 1) << 8 | ((int(blk[72 + (i >> 3)]) >> (i & 7)) & 1) << 15


def random_valid(rng, n):
    """n random records with clear reserved bits: every 9-bit id (379 .. 0x1FF included) and both bins."""
    return (rng.integers(0, 512, size=n).astype(np.uint16) | (rng.integers(0, 2, size=n).astype(np.uint16) << 15)).astype(np.uint16)
