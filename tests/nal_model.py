"""Plain Python restatement of the two walks that include/cabac_hip_nal.h defines (emulation prevention of a segmented byte
string and its inverse).  Not a test file: tests/test_nal_model.py pins it to the oracle's countStartCodeEmulations, and
tests/test_gpu_nal.py takes every expectation from it."""
import numpy as np

NAL_OVERFLOW, NAL_TRAILING_ZERO, NAL_FORBIDDEN, NAL_BAD_ESCAPE, NAL_LOC_OVERFLOW, NAL_INPUT_CLIPPED = 1, 2, 4, 8, 16, 32


def escape_bound(n):
    return n + n // 2


def _clip(offsets, data, bytes_max):
    """What the device forms do with a length above the bound the host gave: (offsets, data, flags) of the clipped input."""
    data = np.asarray(data, np.uint8)
    offsets = [int(o) for o in offsets]
    n = offsets[-1] if offsets else 0
    flags = 0
    if bytes_max is not None and n > bytes_max:
        n, flags = int(bytes_max), NAL_INPUT_CLIPPED
    return [min(o, n) for o in offsets], data[:n], flags


def escape(offsets, payload, capacity=None, bytes_max=None):
    """(nal bytes of the full result, nal_offsets, status) with status = dict(out_bytes, n_changed, flags).  `capacity` only
    sets NAL_OVERFLOW: the caller compares the first `capacity` bytes."""
    offsets, payload, flags = _clip(offsets, payload, bytes_max)
    out = bytearray()
    ins_before = np.zeros(len(payload) + 1, np.int64)   # insertions in front of raw positions < i
    z = n_ins = 0
    for i, b in enumerate(payload.tolist()):
        ins_before[i] = n_ins
        if z == 2 and b <= 3:
            out.append(3)
            n_ins += 1
            z = 0
        out.append(b)
        z = z + 1 if b == 0 else 0
    ins_before[len(payload)] = n_ins
    if len(payload) and payload[-1] == 0:
        flags |= NAL_TRAILING_ZERO
    if capacity is not None and len(out) > capacity:
        flags |= NAL_OVERFLOW
    nal_offsets = np.array([o + int(ins_before[o]) for o in offsets], np.uint64)
    return np.frombuffer(bytes(out), np.uint8), nal_offsets, dict(out_bytes=len(out), n_changed=n_ins, flags=flags)


def unescape(nal_offsets, nal, capacity=None, loc_capacity=None, loc_base=0, bytes_max=None):
    """(payload bytes of the full result, offsets, all locations, status).  `loc_capacity` None: no location list is asked
    for (no NAL_LOC_OVERFLOW)."""
    nal_offsets, nal, flags = _clip(nal_offsets, nal, bytes_max)
    out = bytearray()
    loc = []
    rem_before = np.zeros(len(nal) + 1, np.int64)
    z = 0
    dropped = False            # the previous byte was a removed 03
    for i, b in enumerate(nal.tolist()):
        rem_before[i] = len(loc)
        if dropped and b > 3:
            flags |= NAL_BAD_ESCAPE
        dropped = False
        if z == 2 and b == 3:
            loc.append((i + loc_base) & 0xFFFFFFFF)
            z = 0
            dropped = True
            continue
        if z >= 2 and b <= 2:
            flags |= NAL_FORBIDDEN
        out.append(b)
        z = z + 1 if b == 0 else 0
    rem_before[len(nal)] = len(loc)
    if capacity is not None and len(out) > capacity:
        flags |= NAL_OVERFLOW
    if loc_capacity is not None and len(loc) > loc_capacity:
        flags |= NAL_LOC_OVERFLOW
    offsets = np.array([o - int(rem_before[o]) for o in nal_offsets], np.uint64)
    return (np.frombuffer(bytes(out), np.uint8), offsets, np.array(loc, np.uint32),
            dict(out_bytes=len(out), n_changed=len(loc), flags=flags))


def has_forbidden(data):
    """True if `data` holds 00 00 {00, 01, 02}."""
    d = np.asarray(data, np.uint8)
    if len(d) < 3:
        return False
    return bool(np.any((d[:-2] == 0) & (d[1:-1] == 0) & (d[2:] <= 2)))
