"""Payload assembly in plain numpy / Python, from the words of include/cabac_hip.h ("substream assembly on the device", the
gather, cabac_hip_decode_batch_packed) and of the reference's bit_stream.cpp:139-181 — not from the kernels of
csrc/cabac_assemble.hip, which the GPU tests compare with this file byte for byte.  Every function returns new arrays and
leaves its arguments alone.  The second half builds the crafted batches that tests/test_assemble_model.py (CPU: the model
against the oracle and sharding.py, and the checks that the batches reach the branches they are made for) and
tests/test_gpu_assemble.py (the kernels against the model) share."""
import numpy as np

import helpers as H

PAY_SENTINEL, SLOT_SENTINEL = 0xC3, 0x5A       # what a payload and the slack of a slot hold before a call


# ------------------------------------------------------------------------------------------------ the model
def sizes(desc, results, clamp=True):
    """Bytes of every substream that take part: all the bytes its bits touch, but no more than its slot holds"""
    n = (results["n_bits"].astype(np.uint64) + np.uint64(7)) // np.uint64(8)
    return np.minimum(n, desc["byte_capacity"].astype(np.uint64)) if clamp else n


def offsets(desc, results):
    """n_sub + 1 entry points: where each substream starts in the payload, and the total"""
    out = np.zeros(len(desc) + 1, np.uint64)
    out[1:] = np.cumsum(sizes(desc, results), dtype=np.uint64)
    return out


def assemble(desc, results, slots, capacity, payload_init):
    """The payload after cabac_hip_assemble_device: the substreams back to back in descriptor order, what does not fit into
    `capacity` bytes dropped, every other byte of payload_init as it was"""
    sz = sizes(desc, results)
    parts = [slots[int(o): int(o) + int(n)] for o, n in zip(desc["byte_offset"], sz)]
    whole = np.concatenate(parts + [np.zeros(0, np.uint8)]).astype(np.uint8)[: int(capacity)]
    out = np.array(payload_init, np.uint8)
    out[: len(whole)] = whole
    return out


def split(desc, offs, payload, slots_init):
    """The slots after cabac_hip_split_device: payload[offs[s] .. offs[s + 1]) at the head of slot s, no more of it than the slot
    holds, every other byte of slots_init as it was"""
    out = np.array(slots_init, np.uint8)
    for s in range(len(desc)):
        lo, n = int(offs[s]), min(int(offs[s + 1]) - int(offs[s]), int(desc["byte_capacity"][s]))
        at = int(desc["byte_offset"][s])
        out[at: at + n] = payload[lo: lo + n]
    return out


def count_bytes(b):
    """Start code emulations in a byte string as bit_stream.cpp:157-181 counts them: 00 00 followed by a byte 00..03, searched
    from the front, the search going on AT the third byte of a match (so that it may be the first zero of the next one)"""
    b = np.asarray(b, np.uint8).tobytes()
    n, i, cnt = len(b), 0, 0
    while i + 2 < n:
        if b[i] == 0 and b[i + 1] == 0:
            cnt += b[i + 2] <= 3
            i += 2
        else:
            i += 1
    return cnt


def fifo_bytes(desc, results, clamp=True, partial=False):
    """Bytes of every substream that the count runs over: the whole bytes of its bits — a trailing partial byte is the
    reference's held bits, not part of its FIFO — and no more than the slot holds.  clamp / partial: the two rules switched off
    (for the tests' self-checks only)"""
    nb = results["n_bits"].astype(np.int64)
    n = (nb + 7) // 8 if partial else nb // 8
    return np.minimum(n, desc["byte_capacity"].astype(np.int64)) if clamp else n


def count(desc, results, slots, clamp=True, partial=False):
    n = fifo_bytes(desc, results, clamp, partial)
    return np.array([count_bytes(slots[int(o): int(o) + int(k)]) for o, k in zip(desc["byte_offset"], n)], np.uint32).reshape(-1)


def counts_of(batch):
    """count() of one of the batches below, computed once"""
    if "counts" not in batch:
        batch["counts"] = count(batch["desc"], batch["results"], batch["slots"])
    return batch["counts"]


def gather(src_off, dst_off, length, src, dst_init):
    """dst after cabac_hip_gather_records_device: run k = src[src_off[k] .. + length[k]) at dst[dst_off[k] ..), offsets in records"""
    out = np.array(dst_init, np.uint16)
    for so, do, n in zip(src_off, dst_off, length):
        out[int(do): int(do) + int(n)] = src[int(so): int(so) + int(n)]
    return out


def pack_bins(bins):
    """Bins eight to a byte: bit r & 7 of byte r >> 3 is bin r, the bits behind the last bin zero"""
    bins = np.asarray(bins, np.uint8) & 1
    out = np.zeros((len(bins) + 7) // 8, np.uint8)
    for r in np.nonzero(bins)[0]:
        out[r >> 3] |= 1 << (r & 7)
    return out


# ------------------------------------------------------------------------------------------------ the shared batch
N_SUBS = (0, 1, 2, 3, 5, 1023, 1024, 1025, 2049, 3073)
# 1019..1032: 255 / 256 / 257 dwords for a workgroup of 256 that takes a dword per thread and pass, with every tail length
SPECIAL_SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65] + list(range(1019, 1033))
WHOLE, PARTIAL, OVERFLOWED = 0, 1, 2

_batches = {}


def _layout(caps):
    """Slots back to back at 16-byte boundaries: (byte_offset of each, bytes in all)"""
    pitch = (np.asarray(caps, np.int64) + 15) // 16 * 16
    return np.concatenate([[0], np.cumsum(pitch)[:-1]]).astype(np.uint64)[: len(caps)], int(pitch.sum())


def shared_batch(n_sub):
    """dict(desc, results, slots, kind, size): descriptors, results and slot bytes written directly (no encoder run).  Substream s
    holds size[s] bytes of its own, the rest of its slot and the padding behind it SLOT_SENTINEL.  Every third one ends in a
    partial byte; every ninth one overflowed its slot: flag set, n_bits beyond 8 * byte_capacity, and right behind its
    capacity the sentinel or the head of the next slot, which a copy that believed n_bits would carry into the payload.  The
    result is cached and must not be written to."""
    if n_sub in _batches:
        return _batches[n_sub]
    rng = np.random.default_rng(0xA55E + n_sub)
    size = np.array([SPECIAL_SIZES[int(rng.integers(0, len(SPECIAL_SIZES)))] if k % 2 == 0 else int(rng.integers(0, 1500))
                     for k in range(n_sub)], np.int64)
    kind = np.array([OVERFLOWED if k % 9 == 2 else PARTIAL if k % 3 == 1 else WHOLE for k in range(n_sub)], np.int64)
    for k, n in ((0, 1029), (1, 700), (2, 48), (3, 1022), (4, 9), (1024, 1030)):   # the substreams the clipping capacities name
        if k < n_sub:
            size[k] = n
    if n_sub > 1024:
        kind[1024] = WHOLE
    kind[(kind == PARTIAL) & (size == 0)] = WHOLE
    over = kind == OVERFLOWED
    size[over & (np.arange(n_sub) % 2 == 0)] = (size[over & (np.arange(n_sub) % 2 == 0)] + 15) // 16 * 16   # the next slot follows at once
    cap = np.where(over, size, size + rng.choice([0, 1, 5, 16, 40], size=n_sub)).astype(np.int64)
    desc = np.zeros(n_sub, H.DESC_DTYPE)
    desc["byte_capacity"] = cap
    desc["byte_offset"], total = _layout(cap)
    res = np.zeros(n_sub, H.RESULT_DTYPE)
    res["n_bits"] = 8 * size
    part = kind == PARTIAL
    res["n_bits"][part] -= rng.integers(1, 8, size=int(part.sum())).astype(np.uint32)
    res["n_bits"][over] += rng.integers(1, 5000, size=int(over.sum())).astype(np.uint32)
    res["flags"][over] = H.RES_OVERFLOW
    slots = np.full(total, SLOT_SENTINEL, np.uint8)
    for s in range(n_sub):
        o, n = int(desc["byte_offset"][s]), int(size[s])
        slots[o: o + n] = rng.integers(0, 256, size=n)
        slots[o: o + min(n, 2)] = [s & 0x7F, (s >> 7) | 0x80][: min(n, 2)]          # no two alike, no first byte a sentinel
    _batches[n_sub] = dict(desc=desc, results=res, slots=slots, kind=kind, size=size)
    return _batches[n_sub]


def clip_capacities(offs):
    """{name: payload_capacity} for a batch with the entry points offs: the total, and the capacities that cut — before anything,
    in the first substream (a dword boundary of its slot), on a boundary between two, one to three bytes into a substream, a
    byte short, a byte over, and in the second tile of the size scan (behind substream 1024)"""
    n_sub, total = len(offs) - 1, int(offs[-1])
    caps = {"total": total, "0": 0, "1": 1, "total+1": total + 1}
    if n_sub:
        k = min(3, n_sub - 1)                                     # (sizes 1029, 700, 48, 1022: see shared_batch)
        caps.update({"in_first": 516, "boundary": int(offs[(n_sub + 1) // 2]), "total-1": total - 1})
        caps.update({"into+%d" % j: int(offs[k]) + j for j in (1, 2, 3)})
    if n_sub > 1024:
        caps["tile_1"] = int(offs[1024]) + 6
    return caps


def cut_at(offs, capacity):
    """Where `capacity` cuts: None if it drops nothing, else (the first substream that loses bytes, how many of its bytes are left:
    0 if the cut falls on its start)"""
    if capacity >= int(offs[-1]):
        return None
    s = max(k for k in range(len(offs) - 1) if int(offs[k]) <= capacity and int(offs[k + 1]) > capacity)
    return s, int(capacity) - int(offs[s])


def wide_offsets(batch, seed=3):
    """Hand-made entry points for the split: every other span larger than the slot it goes to (by 1 .. 40 bytes, or by a whole
    slot), the rest as the batch's sizes; and a payload of that length"""
    rng = np.random.default_rng(seed)
    cap = batch["desc"]["byte_capacity"].astype(np.int64)
    span = np.minimum((batch["results"]["n_bits"].astype(np.int64) + 7) // 8, cap)
    wide = np.arange(len(cap)) % 2 == 1
    span[wide] = cap[wide] + rng.choice([1, 2, 3, 4, 15, 16, 17, 40, 2000], size=int(wide.sum()))
    offs = np.concatenate([[0], np.cumsum(span)]).astype(np.uint64)
    return offs, rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ streams for the count
COUNT_N_SUBS = (1, 2, 3, 5, 1023, 1025)
LONG_RUNS = (65535, 65536, 65537, 100000)


def _place(streams, caps, n_bits, behind):
    """desc / results / slots for byte strings lying at the heads of their slots; behind[k]: what follows stream k's capacity
    inside the memory of its own slot (descriptors never describe more than is there: the slot's pitch covers it)"""
    n = len(streams)
    pitch = [max(len(b), int(c)) + len(x) for b, c, x in zip(streams, caps, behind)]
    desc = np.zeros(n, H.DESC_DTYPE)
    desc["byte_offset"], total = _layout(pitch)
    desc["byte_capacity"] = caps
    res = np.zeros(n, H.RESULT_DTYPE)
    res["n_bits"] = n_bits
    slots = np.full(total, 0x77, np.uint8)
    for k, (b, c, x) in enumerate(zip(streams, caps, behind)):
        o = int(desc["byte_offset"][k])
        slots[o: o + len(b)] = b
        slots[o + int(c): o + int(c) + len(x)] = x
    return desc, res, slots


def count_batch(n_sub):
    """dict(desc, results, slots, kind): byte strings rich in zeros, written as substreams of three kinds in turn.  WHOLE:
    whole bytes.  PARTIAL: n_bits ends 1..7 bits into the last byte, which is chosen so that it would complete a match.
    OVERFLOWED: n_bits says more than byte_capacity, and what lies behind the capacity would add matches."""
    key = ("count", n_sub)
    if key in _batches:
        return _batches[key]
    rng = np.random.default_rng(0xC0DE + n_sub)
    streams, caps, n_bits, behind, kind = [], [], [], [], []
    for k in range(n_sub):
        n = int(rng.integers(4, 400))
        p0 = float(rng.choice([0.3, 0.6, 0.9, 0.98]))
        b = rng.choice(np.array([0, 1, 2, 3, 4, 255], np.uint8), size=n, p=[p0] + [(1 - p0) / 5] * 5).astype(np.uint8)
        kd = (WHOLE, PARTIAL, OVERFLOWED)[k % 3] if n_sub > 2 else (PARTIAL, OVERFLOWED)[k % 2]
        if kd == PARTIAL:
            b[-3:] = [0, 0, int(rng.integers(0, 4))]               # ... 00 00 | 0x: a match only if the partial byte counted
            streams.append(b), caps.append(n + int(rng.integers(0, 20))), behind.append(np.zeros(0, np.uint8))
            n_bits.append(8 * n - int(rng.integers(1, 8)))
        elif kd == OVERFLOWED:
            c = int(rng.integers(2, n))
            b[c - 2: c] = 0                                        # the slot ends in 00 00; 01 00 00 01 ... follow it
            tail = np.tile(np.array([1, 0, 0], np.uint8), 8)
            streams.append(b[:c]), caps.append(c), behind.append(tail)
            n_bits.append(8 * c + int(rng.integers(1, 200)))
        else:
            streams.append(b), caps.append(n + int(rng.integers(0, 20))), behind.append(np.zeros(0, np.uint8))
            n_bits.append(8 * n)
        kind.append(kd)
    desc, res, slots = _place(streams, caps, n_bits, behind)
    _batches[key] = dict(desc=desc, results=res, slots=slots, kind=np.array(kind))
    return _batches[key]


def long_run_batch():
    """Zero runs long enough for any narrow run-length counter to wrap, each ending 0..3 bytes before a partial byte; and one
    string of each run length in whole bytes"""
    if "long" in _batches:
        return _batches["long"]
    streams, n_bits, kind = [], [], []
    for run in LONG_RUNS:
        for j in range(4):
            b = np.concatenate([np.full(5 + j, 9, np.uint8), np.zeros(run, np.uint8), np.array([1, 0, 0][:j], np.uint8),
                                np.array([2], np.uint8)]).astype(np.uint8)
            streams += [b, b][: 2 if j == 3 else 1]
            n_bits += [8 * len(b) - 1 - j, 8 * len(b)][: 2 if j == 3 else 1]
            kind += [PARTIAL, WHOLE][: 2 if j == 3 else 1]
    caps = [len(b) + 3 for b in streams]
    desc, res, slots = _place(streams, caps, n_bits, [np.zeros(0, np.uint8)] * len(streams))
    _batches["long"] = dict(desc=desc, results=res, slots=slots, kind=np.array(kind))
    return _batches["long"]


# ------------------------------------------------------------------------------------------------ segments for the gather
GATHER_LENGTHS = (0, 1, 7, 8, 9, 511, 512, 513)


def gather_case(n_seg, first=0, seed=11):
    """dict(src_off, dst_off, length, src, n_dst): segment k has length GATHER_LENGTHS[(first + k) % 8] and the parities of its
    source and destination offsets run through all four combinations; the destination segments lie in ascending order with gaps
    of 1 .. 4 records between them"""
    rng = np.random.default_rng(seed + n_seg)
    src_off, dst_off, length = [], [], []
    s_at, d_at = 0, 0
    for k in range(n_seg):
        q = first + k
        n = GATHER_LENGTHS[q % 8]
        s_at += 1 + int(rng.integers(0, 2)) * 2
        d_at += 1 + int(rng.integers(0, 2)) * 2
        s_at += (s_at ^ (q >> 3)) & 1                               # source parity: bit 3 of q; destination parity: bit 4
        d_at += (d_at ^ (q >> 4)) & 1
        src_off.append(s_at), dst_off.append(d_at), length.append(n)
        s_at += n
        d_at += n
    src = rng.integers(0, 1 << 16, size=s_at + 8, dtype=np.uint16)
    return dict(src_off=np.array(src_off, np.uint64), dst_off=np.array(dst_off, np.uint64), length=np.array(length, np.uint32),
                src=src, n_dst=d_at + 8)
