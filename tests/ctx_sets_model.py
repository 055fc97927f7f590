"""The expectation of include/cabac_hip_ctx_sets.h, on the CPU: the oracle's record coder started from given contexts
(tests/csrc/ctx_sets_ref.c, which includes oracle/cabac_oracle.c unchanged and adds the two `_from` drivers), the batch
semantics of the sets calls on top of it, and the WPP loop level by level.  tests/test_ctx_sets_model.py pins all of it to the
oracle's own entry points; the GPU tests compare the device with it.

A context set here is (s0 uint16[379], s1 uint16[379], rate uint8[379]), as tests/test_gpu_residual_estimate.py::make_sets
builds them."""
import ctypes
import os
import subprocess

import numpy as np

import helpers as H

NO_SET = 0xFFFFFFFF
RES_BAD_SET = 0x40
CSRC = os.path.join(H.ROOT, "tests", "csrc")

_lib = None


def load():
    """tests/csrc/libctx_sets_ref.so, compiled with plain cc when ctx_sets_ref.c or the oracle is newer."""
    global _lib
    if _lib is not None:
        return _lib
    src = os.path.join(CSRC, "ctx_sets_ref.c")
    orc = os.path.join(H.ORACLE_DIR, "cabac_oracle.c")
    so = os.path.join(CSRC, "libctx_sets_ref.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(orc)):
        subprocess.check_call(["cc", "-O2", "-fPIC", "-std=c11", "-pthread", "-D_POSIX_C_SOURCE=200809L", "-Wno-unused-function",
                               "-I" + os.path.join(H.ROOT, "include"), "-I" + H.ORACLE_DIR, "-shared", src, "-o", so + ".tmp"])
        os.replace(so + ".tmp", so)
    L = ctypes.CDLL(so)
    L.csr_encode_records_from.restype = ctypes.c_long
    L.csr_encode_records_from.argtypes = [H.u16p, ctypes.c_long, H.u16p, H.u16p, H.u8p, ctypes.c_int, H.u8p, ctypes.c_long, H.u32p,
                                          H.u16p, H.u16p, H.u8p]
    L.csr_decode_records_from.restype = ctypes.c_int
    L.csr_decode_records_from.argtypes = [H.u16p, ctypes.c_long, H.u16p, H.u16p, H.u8p, ctypes.c_int, H.u8p, ctypes.c_long, H.u8p,
                                          H.u32p, H.u16p, H.u16p, H.u8p]
    _lib = L
    return L


def _set_in(ctx):
    return [np.ascontiguousarray(ctx[0], np.uint16), np.ascontiguousarray(ctx[1], np.uint16), np.ascontiguousarray(ctx[2], np.uint8)]


def _set_out():
    return np.zeros(H.NUM_CTX, np.uint16), np.zeros(H.NUM_CTX, np.uint16), np.zeros(H.NUM_CTX, np.uint8)


def encode_from(rec, ctx, flags=1, cap=None):
    """(rc, bytes, n_bits, contexts left): orc_encode_records from `ctx`.  flags: 1 finish, 2 RBSP alignment, 4 probe.
    rc < 0: -2 bad record (no contexts), -3 overflow of `cap`."""
    L = load()
    rec = np.ascontiguousarray(rec, np.uint16)
    cap = 64 + len(rec) if cap is None else int(cap)
    out = np.zeros(max(cap, 1), np.uint8)
    nbits = ctypes.c_uint32(0)
    s0, s1, rt = _set_in(ctx)
    o = _set_out()
    n = L.csr_encode_records_from(H._ptr(rec, H.u16p), len(rec), H._ptr(s0, H.u16p), H._ptr(s1, H.u16p), H._ptr(rt, H.u8p), flags,
                                  H._ptr(out, H.u8p), cap, ctypes.byref(nbits), H._ptr(o[0], H.u16p), H._ptr(o[1], H.u16p),
                                  H._ptr(o[2], H.u8p))
    return int(n), out[:max(n, 0)].copy(), nbits.value, o


def decode_from(rec, ctx, data, flags=0):
    """(rc, bins, n_bits_read, contexts left): orc_decode_records from `ctx`; rc -2 bad record, -4 underrun, -5 bad stop."""
    L = load()
    rec = np.ascontiguousarray(rec, np.uint16)
    data = np.ascontiguousarray(data, np.uint8)
    bins = np.zeros(max(len(rec), 1), np.uint8)
    nread = ctypes.c_uint32(0)
    s0, s1, rt = _set_in(ctx)
    o = _set_out()
    rc = L.csr_decode_records_from(H._ptr(rec, H.u16p), len(rec), H._ptr(s0, H.u16p), H._ptr(s1, H.u16p), H._ptr(rt, H.u8p), flags,
                                   H._ptr(data, H.u8p), len(data), H._ptr(bins, H.u8p), ctypes.byref(nread), H._ptr(o[0], H.u16p),
                                   H._ptr(o[1], H.u16p), H._ptr(o[2], H.u8p))
    return int(rc), bins[:len(rec)], nread.value, o


def advance_from(rec, ctx):
    """The contexts after update() for every context-coded record of `rec` (tests/test_gpu_residual_estimate.py::advance)."""
    from test_gpu_residual_estimate import advance
    s0, s1 = np.asarray(ctx[0]).astype(np.int64), np.asarray(ctx[1]).astype(np.int64)
    advance(s0, s1, ctx[2], rec)
    return s0.astype(np.uint16), s1.astype(np.uint16), np.asarray(ctx[2], np.uint8).copy()


def init_set(qp, init_id):
    return H.load_oracle().ctx_init(min(max(int(qp), 0), 63), int(init_id) & 3)


def pack(ctx):
    """(state uint32[379], rate uint8[379]) in the format of cabac_hip_ctx_init_device."""
    return ctx[0].astype(np.uint32) | (ctx[1].astype(np.uint32) << 16), np.asarray(ctx[2], np.uint8)


def _start_of(d, sets, start, s):
    if start is None or int(start[s]) == NO_SET:
        return init_set(int(d["qp"]), int(d["init_id"]))
    return sets[int(start[s])]


def _enc_flags(init_id):
    return (1 if init_id & H.SUB_FINISH else 0) | (2 if init_id & H.SUB_ALIGN_RBSP else 0) | (4 if init_id & 0x400 else 0)


def encode_sets(desc, records, bytes_total, sets, start=None):
    """cabac_hip_encode_sets_device on host arrays: (bytes, results, [contexts left per substream or None]).  A start index
    >= len(sets) gives {0, RES_BAD_SET} and None."""
    out = np.zeros(max(int(bytes_total), 1), np.uint8)
    res = np.zeros(len(desc), H.RESULT_DTYPE)
    left = []
    for s, d in enumerate(desc):
        if start is not None and int(start[s]) != NO_SET and int(start[s]) >= len(sets):
            res[s] = (0, RES_BAD_SET)
            left.append(None)
            continue
        rec = records[int(d["rec_offset"]):int(d["rec_offset"]) + int(d["n_records"])]
        n, data, nbits, o = encode_from(rec, _start_of(d, sets, start, s), _enc_flags(int(d["init_id"])), int(d["byte_capacity"]))
        if n == -2:
            res[s] = (0, H.RES_BAD_RECORD)
            left.append(None)
            continue
        assert n >= 0, "the model's batches fit their byte slots"
        out[int(d["byte_offset"]):int(d["byte_offset"]) + n] = data
        res[s] = (nbits, 0)
        left.append(o)
    return out, res, left


def decode_sets(desc, records, data, sets, start=None):
    """cabac_hip_decode_sets_device on host arrays: (bins, results, [contexts left or None])."""
    bins = np.zeros(max(len(records), 1), np.uint8)
    res = np.zeros(len(desc), H.RESULT_DTYPE)
    left = []
    for s, d in enumerate(desc):
        if start is not None and int(start[s]) != NO_SET and int(start[s]) >= len(sets):
            res[s] = (0, RES_BAD_SET)
            left.append(None)
            continue
        a, n = int(d["rec_offset"]), int(d["n_records"])
        src = data[int(d["byte_offset"]):int(d["byte_offset"]) + int(d["byte_capacity"])]
        rc, b, nread, o = decode_from(records[a:a + n], _start_of(d, sets, start, s), src, 1 if int(d["init_id"]) & H.SUB_FINISH else 0)
        assert rc in (0, -5), "the model's batches decode without a bad record or an underrun"
        bins[a:a + n] = b
        res[s] = (nread, H.RES_BAD_STOP if rc == -5 else 0)
        left.append(o)
    return bins[:len(records)], res, left


# ---------------------------------------------------------------------------------------------- WPP, level by level
def wpp_starts(desc, records, level_first, sync_from, sync_at):
    """The contexts every substream starts from under the links: level by level, slot p = the contexts p has after its first
    min(sync_at[p], n_records) records from its own start (update() only: the hand-over does not depend on the coder).  A link
    that does not point into an earlier level gives None (CABAC_RES_BAD_SET), and so does a link to such a substream."""
    n_sub = len(desc)
    start = [None] * n_sub
    slot = [None] * n_sub
    ok = [False] * n_sub
    for l in range(len(level_first) - 1):
        first = int(level_first[l])
        for s in range(first, int(level_first[l + 1])):
            f = int(sync_from[s])
            if f == NO_SET:
                start[s] = init_set(int(desc[s]["qp"]), int(desc[s]["init_id"]))
            elif f < first and slot[f] is not None:
                start[s] = slot[f]
            else:
                ok[s] = f < first     # a link to a refused substream: unspecified contexts, not refused itself
                continue
            ok[s] = True
            a = int(desc[s]["rec_offset"])
            n = min(int(sync_at[s]), int(desc[s]["n_records"]))
            slot[s] = advance_from(records[a:a + n], start[s])
    return start, ok


def encode_wpp(desc, records, bytes_total, level_first, sync_from, sync_at):
    """cabac_hip_encode_wpp_* on host arrays: (bytes, results).  Substreams whose contexts are unspecified (they link to a
    refused substream) are left out: result {0, 0}, no bytes — callers compare the others."""
    start, ok = wpp_starts(desc, records, level_first, sync_from, sync_at)
    out = np.zeros(max(int(bytes_total), 1), np.uint8)
    res = np.zeros(len(desc), H.RESULT_DTYPE)
    for s, d in enumerate(desc):
        if start[s] is None:
            if not ok[s]:
                res[s] = (0, RES_BAD_SET)
            continue
        rec = records[int(d["rec_offset"]):int(d["rec_offset"]) + int(d["n_records"])]
        n, data, nbits, _ = encode_from(rec, start[s], _enc_flags(int(d["init_id"])), int(d["byte_capacity"]))
        assert n >= 0
        out[int(d["byte_offset"]):int(d["byte_offset"]) + n] = data
        res[s] = (nbits, 0)
    return out, res


def decode_wpp(desc, records, data, level_first, sync_from, sync_at):
    """cabac_hip_decode_wpp_* on host arrays: (bins, results).  The hand-over contexts come from the DECODED bins, level by
    level, as a decoder has them."""
    n_sub = len(desc)
    bins = np.zeros(max(len(records), 1), np.uint8)
    res = np.zeros(n_sub, H.RESULT_DTYPE)
    slot = [None] * n_sub
    for l in range(len(level_first) - 1):
        first = int(level_first[l])
        for s in range(first, int(level_first[l + 1])):
            d = desc[s]
            f = int(sync_from[s])
            if f == NO_SET:
                ctx = init_set(int(d["qp"]), int(d["init_id"]))
            elif f < first and slot[f] is not None:
                ctx = slot[f]
            else:
                if f >= first:
                    res[s] = (0, RES_BAD_SET)
                continue
            a, n = int(d["rec_offset"]), int(d["n_records"])
            src = data[int(d["byte_offset"]):int(d["byte_offset"]) + int(d["byte_capacity"])]
            rc, b, nread, _ = decode_from(records[a:a + n], ctx, src, 1 if int(d["init_id"]) & H.SUB_FINISH else 0)
            assert rc in (0, -5)
            bins[a:a + n] = b
            res[s] = (nread, H.RES_BAD_STOP if rc == -5 else 0)
            k = min(int(sync_at[s]), n)
            decoded = (records[a:a + k] & 0x7FFF) | (b[:k].astype(np.uint16) << 15)
            slot[s] = advance_from(decoded, ctx)
    return bins[:len(records)], res


# ---------------------------------------------------------------------------------------------- the batches of the tests
def wpp_batch(seed, n_pic=3, n_row=4, lengths=None, sync_ats=(0, 21, None, 10 ** 6), unlinked_row=(1, 2)):
    """n_pic pictures x n_row rows in LEVEL ORDER (level r = row r of every picture): ragged rows, row r of a picture linked to
    its row r - 1, sync_at cycling through `sync_ats` (None: exactly n_records); picture unlinked_row[0]'s row unlinked_row[1]
    links to nothing.  Returns (desc, records, bytes_total, level_first, sync_from, sync_at)."""
    rng = np.random.default_rng(seed)
    n_sub = n_pic * n_row
    if lengths is None:
        lengths = [int(rng.integers(30, 400)) for _ in range(n_sub)]
    recs = [H.random_records(rng, n - 1, ctx_frac=0.8, ctx_pool=np.arange(86, 292)) for n in lengths]
    desc, total = H.make_desc([len(r) for r in recs], [int(rng.integers(20, 45)) for _ in range(n_sub)],
                              [int(rng.integers(0, 3)) for _ in range(n_sub)], flags=H.SUB_FINISH | H.SUB_ALIGN_RBSP)
    records = np.concatenate(recs).astype(np.uint16)
    level_first = np.arange(0, n_sub + 1, n_pic, dtype=np.uint32)
    sync_from = np.full(n_sub, NO_SET, np.uint32)
    sync_at = np.zeros(n_sub, np.uint32)
    for r in range(n_row):
        for p in range(n_pic):
            s = r * n_pic + p
            if r > 0 and (p, r) != tuple(unlinked_row):
                sync_from[s] = (r - 1) * n_pic + p
            at = sync_ats[s % len(sync_ats)]
            sync_at[s] = len(recs[s]) if at is None else at
    return desc, records, total, level_first, sync_from, sync_at
