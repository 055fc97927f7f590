"""Shared test plumbing: ctypes loaders for the oracle (oracle/libcabac_oracle.so), the compiled
reference (oracle/_ref/libcabac_ref.so, build container only) and random op/record generators.

The oracle and the reference harness are TEST INFRASTRUCTURE; product code never loads them."""
import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
GOLDEN = os.path.join(ROOT, "tests", "golden")

NUM_CTX = 379
REC_BIN = 0x8000
REC_ALIGN, REC_EP, REC_TRM = 0x1FD, 0x1FE, 0x1FF
SUB_FINISH, SUB_ALIGN_RBSP = 0x100, 0x200
RES_OVERFLOW, RES_BAD_RECORD, RES_UNDERRUN, RES_BAD_STOP, RES_RANGE = 1, 2, 4, 8, 16   # cabac_substream_result.flags

OP_BIN, OP_EP, OP_BINS_EP, OP_REM_ABS, OP_TRM, OP_ALIGN = 0, 1, 2, 3, 4, 5
OP_UNARY_MAX, OP_UNARY_EP, OP_EXP_GOLOMB, OP_TRUNC_BIN = 6, 7, 8, 9

u8p = ctypes.POINTER(ctypes.c_uint8)
u16p = ctypes.POINTER(ctypes.c_uint16)
u32p = ctypes.POINTER(ctypes.c_uint32)

DESC_DTYPE = np.dtype(
    [
        ("rec_offset", "<u8"),
        ("byte_offset", "<u8"),
        ("n_records", "<u4"),
        ("byte_capacity", "<u4"),
        ("qp", "<i4"),
        ("init_id", "<u4"),
    ]
)
RESULT_DTYPE = np.dtype([("n_bits", "<u4"), ("flags", "<u4")])

# cabac_tu_desc and friends (include/cabac_hip.h)
TU_DTYPE = np.dtype([("coeff_offset", "<u8"), ("log2_width", "u1"), ("log2_height", "u1"), ("channel", "u1"),
                     ("flags", "u1"), ("max_log2_tr_range", "u1"), ("reserved", "u1", (3,))])
TU_DEP_QUANT, TU_SIGN_HIDING, TU_TS_FLAG, TU_TRANSFORM_SKIP, TU_BDPCM, TU_SBT_ZERO_OUT = 1, 2, 4, 8, 16, 32
TU_INFO_MTS_VIOLATION, TU_INFO_EMPTY, TU_INFO_BAD_DESC = 0x10000, 0x80000000, 0x40000000
TU_INFO_TS = 0x20000


def TU_MAX_RECORDS(n):
    return 33 + 38 * n


def _ptr(a, ty):
    return a.ctypes.data_as(ty)


class CodecLib:
    """Uniform wrapper over the `orc_*` (oracle) or `ref_*` (compiled reference) entry points."""

    def __init__(self, lib, prefix):
        self.lib = lib
        self.p = prefix
        L = lib
        g = lambda n: getattr(L, prefix + n)
        g("encode_ops").restype = ctypes.c_long
        g("encode_ops").argtypes = [u32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, u8p,
                                    ctypes.c_long, u32p, u32p]
        g("encode_records").restype = ctypes.c_long
        g("encode_records").argtypes = [u16p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, u8p,
                                        ctypes.c_long, u32p]
        g("decode_records").restype = ctypes.c_int
        g("decode_records").argtypes = [u16p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, u8p,
                                        ctypes.c_long, u8p, u32p]
        g("decode_ops").restype = ctypes.c_int
        g("decode_ops").argtypes = [u32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, u8p,
                                    ctypes.c_long, u32p]
        g("ctx_init").argtypes = [ctypes.c_int, ctypes.c_int, u16p, u16p, u8p]
        g("ctx_trace").argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, u8p, ctypes.c_int, ctypes.c_uint,
                                   u8p, u8p, u16p, u16p]
        u64p = ctypes.POINTER(ctypes.c_uint64)
        g("estimate_ops").restype = ctypes.c_int
        g("estimate_ops").argtypes = [u32p, ctypes.c_long, ctypes.c_int, ctypes.c_int, u64p]
        g("estimate_records").restype = ctypes.c_int
        g("estimate_records").argtypes = [u16p, ctypes.c_long, ctypes.c_int, ctypes.c_int, u64p]
        if prefix == "orc_":
            L.orc_estimate_records_from.restype = ctypes.c_int
            L.orc_estimate_records_from.argtypes = [u16p, ctypes.c_long, u16p, u16p, u8p, u64p]
        else:
            L.ref_estimate_from_history.restype = ctypes.c_int
            L.ref_estimate_from_history.argtypes = [u16p, ctypes.c_long, u16p, ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                                    u64p, u16p, u16p, u8p]
        if prefix == "orc_":
            L.orc_estimate_batch.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, u16p, u64p, u32p]
            L.orc_ops_to_records.restype = ctypes.c_long
            L.orc_ops_to_records.argtypes = [u32p, ctypes.c_long, u16p, ctypes.c_long]
            L.orc_encode_batch.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, u16p, u8p, u32p]
            L.orc_decode_batch.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, u16p, u8p, u8p, u32p]

    # -- encode ---------------------------------------------------------------
    def encode_ops(self, ops, qp, init_id, flags=1):
        ops = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 4)
        cap = 64 + 8 * len(ops) * 5
        out = np.zeros(cap, np.uint8)
        nbits = ctypes.c_uint32(0)
        nbins = np.zeros(3, np.uint32)
        n = getattr(self.lib, self.p + "encode_ops")(_ptr(ops, u32p), len(ops), qp, init_id, flags,
                                                     _ptr(out, u8p), cap, ctypes.byref(nbits), _ptr(nbins, u32p))
        if n < 0:
            raise RuntimeError("%sencode_ops failed: %d" % (self.p, n))
        return out[:n].copy(), nbits.value, nbins

    def encode_records(self, rec, qp, init_id, flags=1):
        rec = np.ascontiguousarray(rec, dtype=np.uint16)
        cap = 64 + len(rec)
        out = np.zeros(cap, np.uint8)
        nbits = ctypes.c_uint32(0)
        n = getattr(self.lib, self.p + "encode_records")(_ptr(rec, u16p), len(rec), qp, init_id, flags,
                                                         _ptr(out, u8p), cap, ctypes.byref(nbits))
        if n < 0:
            raise RuntimeError("%sencode_records failed: %d" % (self.p, n))
        return out[:n].copy(), nbits.value

    # -- decode ---------------------------------------------------------------
    def decode_records(self, rec, qp, init_id, data, flags=0):
        rec = np.ascontiguousarray(rec, dtype=np.uint16)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        bins = np.zeros(max(len(rec), 1), np.uint8)
        nread = ctypes.c_uint32(0)
        rc = getattr(self.lib, self.p + "decode_records")(_ptr(rec, u16p), len(rec), qp, init_id, flags,
                                                          _ptr(data, u8p), len(data), _ptr(bins, u8p),
                                                          ctypes.byref(nread))
        return rc, bins[: len(rec)], nread.value

    def decode_ops(self, ops, qp, init_id, data, flags=0):
        ops = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 4)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        vals = np.zeros(max(len(ops), 1), np.uint32)
        rc = getattr(self.lib, self.p + "decode_ops")(_ptr(ops, u32p), len(ops), qp, init_id, flags,
                                                      _ptr(data, u8p), len(data), _ptr(vals, u32p))
        return rc, vals[: len(ops)]

    # -- context model --------------------------------------------------------
    def ctx_init(self, qp, init_id):
        s0 = np.zeros(NUM_CTX, np.uint16)
        s1 = np.zeros(NUM_CTX, np.uint16)
        rate = np.zeros(NUM_CTX, np.uint8)
        getattr(self.lib, self.p + "ctx_init")(qp, init_id, _ptr(s0, u16p), _ptr(s1, u16p), _ptr(rate, u8p))
        return s0, s1, rate

    def ctx_trace(self, qp, init_id, ctx_id, bins, rng):
        bins = np.ascontiguousarray(bins, dtype=np.uint8)
        n = len(bins)
        st = np.zeros(n, np.uint8)
        lps = np.zeros(n, np.uint8)
        a = np.zeros(n, np.uint16)
        b = np.zeros(n, np.uint16)
        getattr(self.lib, self.p + "ctx_trace")(qp, init_id, ctx_id, _ptr(bins, u8p), n, rng, _ptr(st, u8p),
                                                _ptr(lps, u8p), _ptr(a, u16p), _ptr(b, u16p))
        return st, lps, a, b

    # -- oracle only ----------------------------------------------------------
    def ops_to_records(self, ops):
        ops = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 4)
        n = self.lib.orc_ops_to_records(_ptr(ops, u32p), len(ops), None, 0)
        if n < 0:
            raise RuntimeError("ops_to_records failed")
        rec = np.zeros(max(n, 1), np.uint16)
        self.lib.orc_ops_to_records(_ptr(ops, u32p), len(ops), _ptr(rec, u16p), n)
        return rec[:n]

    # -- bit estimator (BitEstimator_Std) --------------------------------------
    def estimate_ops(self, ops, qp, init_id):
        """(rc, fractional bits in 1/32768 bit) of an op stream after reset(qp, init_id)."""
        ops = np.ascontiguousarray(ops, np.uint32).reshape(-1, 4)
        out = ctypes.c_uint64(0)
        rc = getattr(self.lib, self.p + "estimate_ops")(_ptr(ops, u32p), len(ops), qp, init_id, ctypes.byref(out))
        return rc, out.value

    def estimate_records(self, rec, qp, init_id):
        rec = np.ascontiguousarray(rec, np.uint16)
        out = ctypes.c_uint64(0)
        rc = getattr(self.lib, self.p + "estimate_records")(_ptr(rec, u16p), len(rec), qp, init_id, ctypes.byref(out))
        return rc, out.value

    def estimate_records_from(self, rec, s0, s1, rate):
        """oracle: cost of `rec` started from the given context states."""
        rec = np.ascontiguousarray(rec, np.uint16)
        out = ctypes.c_uint64(0)
        rc = self.lib.orc_estimate_records_from(_ptr(rec, u16p), len(rec), _ptr(np.ascontiguousarray(s0, np.uint16), u16p),
                                                _ptr(np.ascontiguousarray(s1, np.uint16), u16p),
                                                _ptr(np.ascontiguousarray(rate, np.uint8), u8p), ctypes.byref(out))
        return rc, out.value

    def estimate_from_history(self, hist, rec, qp, init_id):
        """reference: code `hist` after reset(qp, init_id), assign the contexts reached to a fresh estimator,
        resetBits(), cost `rec`.  Returns (rc, bits, s0, s1, rate) — the states the estimator started from."""
        hist = np.ascontiguousarray(hist, np.uint16)
        rec = np.ascontiguousarray(rec, np.uint16)
        s0, s1, rate = np.zeros(NUM_CTX, np.uint16), np.zeros(NUM_CTX, np.uint16), np.zeros(NUM_CTX, np.uint8)
        out = ctypes.c_uint64(0)
        rc = self.lib.ref_estimate_from_history(_ptr(hist, u16p), len(hist), _ptr(rec, u16p), len(rec), qp, init_id,
                                                ctypes.byref(out), _ptr(s0, u16p), _ptr(s1, u16p), _ptr(rate, u8p))
        return rc, out.value, s0, s1, rate

    def estimate_batch(self, desc, records):
        bits = np.zeros(len(desc), np.uint64)
        flags = np.zeros(len(desc), np.uint32)
        self.lib.orc_estimate_batch(desc.ctypes.data, 0, len(desc), _ptr(records, u16p),
                                    bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _ptr(flags, u32p))
        return bits, flags

    # -- residual coding ---------------------------------------
    def residual_records(self, coeff, chroma=0, flags=0, max_log2_range=15, with_cuctx=True):
        """coeff: (h, w) int32 block -> (records, scanPosLast, mts_violation).  Raises ValueError on an all-zero block."""
        coeff = np.ascontiguousarray(coeff, dtype=np.int32)
        h, w = coeff.shape
        cap = TU_MAX_RECORDS(min(w, 32) * min(h, 32))
        out = np.zeros(cap, np.uint16)
        i32p = ctypes.POINTER(ctypes.c_int32)
        if self.p == "orc_":
            f = self.lib.orc_residual_records
            f.restype = ctypes.c_long
            f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_int, i32p, u16p,
                          ctypes.c_long, u32p]
            info = ctypes.c_uint32(0)
            n = f(int(np.log2(w)), int(np.log2(h)), chroma, flags, max_log2_range, _ptr(coeff, i32p), _ptr(out, u16p),
                  cap, ctypes.byref(info))
            if n == -1:
                raise ValueError("empty block")
            assert 0 <= n <= cap, n
            return out[:n].copy(), info.value & 0xFFFF, bool(info.value & TU_INFO_MTS_VIOLATION)
        f = self.lib.ref_residual_records
        f.restype = ctypes.c_long
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, i32p, u16p, ctypes.c_long, i32p]
        info = np.zeros(8, np.int32)
        assert max_log2_range == 15 or 17 <= max_log2_range <= 20   # min(20, bit depth + 6) under extended precision
        depth = 0 if max_log2_range == 15 else max_log2_range - 6
        rig = (flags & 7) | (8 if with_cuctx else 0) | (0x10 if flags & TU_TRANSFORM_SKIP else 0) | (0x20 if flags & TU_BDPCM else 0) | \
              (0x40 if flags & TU_SBT_ZERO_OUT else 0)
        n = f(w, h, 1 if chroma else 0, rig | depth << 8, _ptr(coeff, i32p), _ptr(out, u16p), cap,
              _ptr(info, i32p))
        if n == -1:
            self.lib.ref_last_error.restype = ctypes.c_char_p
            raise ValueError(self.lib.ref_last_error().decode(errors="replace"))
        assert 0 <= n <= cap, n
        return out[:n].copy(), info

    def residual_decode(self, data, qp, blocks_meta, finish=True, with_info=False):
        """blocks_meta: [(w, h, chroma, flags[, max_log2_tr_range])] -> (rc, [coefficient blocks (h, w)], n_bits_read[, info]).
        max_log2_tr_range (0 or absent: 15) goes into the block's descriptor; the compiled reference's rig has no such knob and
        refuses anything but 15.
        info: per block CABAC_TU_INFO_* as the device parser reports it (scanPosLast | MTS violation, or TS); for the
        compiled reference it is put together from the TransformUnit / CUCtx the reader leaves behind."""
        data = np.ascontiguousarray(data, np.uint8)
        i32p = ctypes.POINTER(ctypes.c_int32)
        blocks_meta = [tuple(m) for m in blocks_meta]
        ranges = [m[4] if len(m) > 4 else 0 for m in blocks_meta]
        blocks_meta = [m[:4] for m in blocks_meta]
        total = sum(w * h for w, h, _, _ in blocks_meta)
        out = np.full(max(total, 1), 0x5A5A5A5A, np.int32)
        nbits = ctypes.c_uint32(0)
        n = len(blocks_meta)
        if self.p == "orc_":
            tus = np.zeros(n, TU_DTYPE)
            off = 0
            for i, (w, h, ch, fl) in enumerate(blocks_meta):
                tus[i]["coeff_offset"], tus[i]["log2_width"], tus[i]["log2_height"] = off, int(np.log2(w)), int(np.log2(h))
                tus[i]["channel"], tus[i]["flags"], tus[i]["max_log2_tr_range"] = ch, fl, ranges[i]
                off += w * h
            info = np.zeros(max(n, 1), np.uint32)
            f = self.lib.orc_residual_decode
            f.restype = ctypes.c_int
            f.argtypes = [u8p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, i32p, u32p,
                          u32p]
            rc = f(_ptr(data, u8p), len(data), qp, 2, tus.ctypes.data, len(tus), 1 if finish else 0, _ptr(out, i32p),
                   ctypes.byref(nbits), _ptr(info, u32p))
            info = info[:n]
        else:
            assert all(r in (0, 15) for r in ranges), "the reference rig parses with max_log2_tr_range 15 only"
            # rig flags (oracle/ref_rig.hpp): bit0 dep_quant, bit1 sign hiding, bit2 transform skip enabled (flag coded),
            # bit4 the block is transform-skip coded, bit5 BDPCM
            rig = np.array([(fl & 3) | (4 if fl & TU_TS_FLAG else 0) | (0x10 if fl & TU_TRANSFORM_SKIP else 0) |
                            (0x20 if fl & TU_BDPCM else 0) | (0x40 if fl & TU_SBT_ZERO_OUT else 0) for _, _, _, fl in blocks_meta], np.int32)
            assert not any((fl & TU_TS_FLAG) and (fl & TU_BDPCM) for _, _, _, fl in blocks_meta), \
                "with BDPCM the reference does not code transform_skip_flag"
            wh = np.array([[w, h] for w, h, _, _ in blocks_meta], np.int32).ravel()
            comp = np.array([1 if ch else 0 for _, _, ch, _ in blocks_meta], np.int32)
            rinfo = np.zeros(5 * max(n, 1), np.int32)
            ip = ctypes.POINTER(ctypes.c_int)
            f = self.lib.ref_residual_decode
            f.restype = ctypes.c_long
            f.argtypes = [ctypes.c_int, ip, ip, ctypes.c_int, u8p, ctypes.c_long, ctypes.c_int, ctypes.c_int, i32p, u32p, ip, i32p]
            rc = f(n, wh.ctypes.data_as(ip), comp.ctypes.data_as(ip), 0, _ptr(data, u8p), len(data), qp,
                   1 if finish else 0, _ptr(out, i32p), ctypes.byref(nbits), rig.ctypes.data_as(ip), _ptr(rinfo, i32p))
            info = rinfo.reshape(-1, 5)[:n]
        blocks, off = [], 0
        for w, h, _, _ in blocks_meta:
            blocks.append(out[off:off + w * h].reshape(h, w).copy())
            off += w * h
        if with_info:
            return int(rc), blocks, nbits.value, info
        return int(rc), blocks, nbits.value

    def scan_order(self, w, h):
        out = np.zeros(w * h, np.uint32)
        if self.p == "orc_":
            f = self.lib.orc_scan_order
            args = (int(np.log2(w)), int(np.log2(h)))
        else:
            f = self.lib.ref_scan_order
            args = (w, h)
        f.restype = ctypes.c_long
        f.argtypes = [ctypes.c_int, ctypes.c_int, u32p]
        assert f(*args, _ptr(out, u32p)) == w * h
        return out

    def encode_batch(self, desc, records, bytes_total):
        out = np.zeros(max(bytes_total, 1), np.uint8)
        res = np.zeros(len(desc), RESULT_DTYPE)
        self.lib.orc_encode_batch(desc.ctypes.data, 0, len(desc), _ptr(records, u16p), _ptr(out, u8p),
                                  res.ctypes.data_as(u32p))
        return out, res

    def decode_batch(self, desc, records, data):
        bins = np.zeros(max(len(records), 1), np.uint8)
        res = np.zeros(len(desc), RESULT_DTYPE)
        self.lib.orc_decode_batch(desc.ctypes.data, 0, len(desc), _ptr(records, u16p), _ptr(data, u8p),
                                  _ptr(bins, u8p), res.ctypes.data_as(u32p))
        return bins[: len(records)], res


def build_oracle():
    so = os.path.join(ORACLE_DIR, "libcabac_oracle.so")
    src = os.path.join(ORACLE_DIR, "cabac_oracle.c")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "libcabac_oracle.so"], stdout=subprocess.DEVNULL)
    return so


_oracle = None
_ref = None


def load_oracle():
    global _oracle
    if _oracle is None:
        _oracle = CodecLib(ctypes.CDLL(build_oracle()), "orc_")
    return _oracle


def ref_available():
    return os.path.exists(os.path.join(ORACLE_DIR, "_ref", "libcabac_ref.so"))


def load_ref():
    """The reference's own sources compiled by oracle/Makefile (build container only)."""
    global _ref
    if _ref is None:
        so = ref_test_library("libcabac_ref.so")
        cwd = os.getcwd()
        tmp = tempfile.mkdtemp(prefix="cabac_ref_")  # reference log.cpp:3-4 creates two files in CWD at load
        os.chdir(tmp)
        try:
            lib = ctypes.CDLL(so)
        finally:
            os.chdir(cwd)
        _ref = CodecLib(lib, "ref_")
    return _ref


def ref_library_current(so):
    """True when every file of this repository that oracle/Makefile compiled `so` against still has the content it had then
    (the `sha256sum` list written beside the library when it was linked)."""
    try:
        lines = open(so + ".sha256").read().splitlines()
    except OSError:
        return False
    for line in lines:
        digest, path = line.split(None, 1)
        path = os.path.join(ORACLE_DIR, path.lstrip("*"))
        if not os.path.exists(path) or hashlib.sha256(open(path, "rb").read()).hexdigest() != digest:
            return False
    return bool(lines)


def ref_test_library(name):
    """Path of oracle/_ref/<name>, built by oracle/Makefile from the reference's sources and this repo's host headers.  A copy
    compiled against other host headers lays the shim's classes out differently from libcabac_hip.so and corrupts memory
    without a diagnostic (the SIGABRT of round 2, a segfault in round 3): where the reference's sources
    are present it is rebuilt; where only the prebuilt file is, a stale one fails the test instead of running."""
    import pytest
    so = os.path.join(ORACLE_DIR, "_ref", name)
    if not os.path.exists(so):
        pytest.skip("oracle/_ref/%s not built" % name)
    if not ref_library_current(so):
        if subprocess.run(["make", "-s", "-C", ORACLE_DIR, "has-ref"], stderr=subprocess.DEVNULL).returncode == 0:
            os.remove(so)
            subprocess.check_call(["make", "-C", ORACLE_DIR, "-j8", "all"], stdout=subprocess.DEVNULL)
        if not ref_library_current(so):
            pytest.fail("oracle/_ref/%s was compiled against other host headers than this tree's: run `make -C oracle` where "
                        "the reference's sources are" % name)
    return so


def gpu_ctx(device=0):
    """A codec context for tests that hand torch tensors to the device-pointer entry points: it runs on torch's current
    stream, so the library's launches are ordered after torch's fills of those tensors and torch's reads after the launches
    (cabac_hip.h, stream ordering contract, form (a)).  tests/test_gpu_two_contexts.py covers form (b), the ctx's own stream
    ordered with events."""
    import torch
    from entropy_coding_amd import capi
    return capi.CabacHip(device, stream=torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ generators
def random_ops(rng, n, ctx_frac=0.6, p_one=None, with_helpers=True, with_align=False, end_trm=True):
    """Random operation stream exercising every BinEncIf entry point and binarisation helper."""
    ops = np.zeros((n + (1 if end_trm else 0), 4), np.uint32)
    if p_one is None:
        p_one = rng.choice([0.03, 0.1, 0.25, 0.5, 0.75, 0.9], size=NUM_CTX)
    i = 0
    while i < n:
        r = rng.random()
        if r < ctx_frac:
            c = int(rng.integers(0, NUM_CTX))
            ops[i] = (OP_BIN, int(rng.random() < p_one[c]), c, 0)
        elif r < ctx_frac + 0.12:
            ops[i] = (OP_EP, int(rng.integers(0, 2)), 0, 0)
        elif r < ctx_frac + 0.20:
            nb = int(rng.integers(0, 33))
            v = int(rng.integers(0, 1 << 32)) & ((1 << nb) - 1) if nb else 0
            ops[i] = (OP_BINS_EP, v, nb, 0)
        elif r < ctx_frac + 0.30:
            rice = int(rng.integers(0, 5))
            mode = rng.random()
            if mode < 0.7:
                v = int(rng.integers(0, 64))
            elif mode < 0.9:
                v = int(rng.integers(0, 1 << 12))
            else:
                # long escapes incl. maxPrefixLength saturation (arith_codec.cpp:440-442); values stay
                # inside the 15-bit transform dynamic range the callers guarantee — beyond it the
                # reference's suffix no longer fits suffixLength bits and its own output is undefined
                v = int(rng.integers(0, 1 << 15))
            ops[i] = (OP_REM_ABS, v, rice, 5 | (15 << 8))
        elif r < ctx_frac + 0.32:
            ops[i] = (OP_TRM, 0, 0, 0)
        elif with_align and r < ctx_frac + 0.33:
            ops[i] = (OP_ALIGN, 0, 0, 0)
        elif with_helpers:
            k = int(rng.integers(0, 4))
            if k == 0:
                mx = int(rng.integers(1, 12))
                sym = int(rng.integers(0, mx + 1))
                c0, cn = int(rng.integers(0, NUM_CTX)), int(rng.integers(0, NUM_CTX))
                ops[i] = (OP_UNARY_MAX, sym, c0 | (cn << 16), mx)
            elif k == 1:
                mx = int(rng.integers(0, 32))
                sym = int(rng.integers(0, mx + 1))
                ops[i] = (OP_UNARY_EP, sym, mx, 0)
            elif k == 2:
                cnt = int(rng.integers(0, 4))
                sym = int(rng.integers(0, 3000))
                ops[i] = (OP_EXP_GOLOMB, sym, cnt, 0)
            else:
                mx = int(rng.integers(1, 700))
                sym = int(rng.integers(0, mx))
                ops[i] = (OP_TRUNC_BIN, sym, mx, 0)
        else:
            ops[i] = (OP_EP, int(rng.integers(0, 2)), 0, 0)
        i += 1
    if end_trm:
        ops[n] = (OP_TRM, 1, 0, 0)
    return ops


def random_records(rng, n, ctx_frac=0.7, p_one=None, ctx_pool=None, end_trm=True, trm0_frac=0.002):
    """Flat bin-record stream (include/cabac_hip.h)."""
    if p_one is None:
        p_one = rng.choice([0.03, 0.1, 0.25, 0.5, 0.75, 0.9], size=NUM_CTX)
    if ctx_pool is None:
        ctx_pool = np.arange(NUM_CTX)
    r = rng.random(n)
    ids = rng.choice(ctx_pool, size=n).astype(np.uint32)
    bins = (rng.random(n) < np.asarray(p_one)[ids]).astype(np.uint32)
    is_ep = r >= ctx_frac
    is_trm = r >= 1.0 - trm0_frac
    ids[is_ep] = REC_EP
    bins[is_ep] = rng.integers(0, 2, size=int(is_ep.sum()))
    ids[is_trm] = REC_TRM
    bins[is_trm] = 0
    rec = (ids | (bins << 15)).astype(np.uint16)
    if end_trm:
        rec = np.concatenate([rec, np.array([REC_TRM | REC_BIN], np.uint16)])
    return rec


def make_desc(lengths, qps, init_ids, flags=SUB_FINISH, capacities=None):
    """Pack substreams back to back; capacity defaults to n/2 + 64 bytes (>= hard bound for the mixes used)."""
    n = len(lengths)
    d = np.zeros(n, DESC_DTYPE)
    lengths = np.asarray(lengths, np.uint64)
    d["n_records"] = lengths
    d["rec_offset"] = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    if capacities is None:
        capacities = (lengths * 3) // 4 + 64
    capacities = (np.asarray(capacities, np.uint64) + 15) // 16 * 16
    d["byte_capacity"] = capacities
    d["byte_offset"] = np.concatenate([[0], np.cumsum(capacities)[:-1]])
    d["qp"] = qps
    d["init_id"] = np.asarray(init_ids, np.uint32) | flags
    return d, int(capacities.sum())


def random_block(rng, w, h, density=0.3, big=0.05, huge=0.0, last_frac=1.0):
    """A (h, w) int32 coefficient block as a quantiser leaves it: mostly small levels with density falling off
    away from DC, some large ones, zero outside the top-left 32x32 (rom.cpp:218-226) and beyond a random
    'last' diagonal; never all-zero."""
    yy, xx = np.mgrid[0:h, 0:w]
    fall = np.exp(-(xx + yy) / max(2.0, (w + h) * 0.35))
    nz = rng.random((h, w)) < density * (0.25 + fall)
    mag = 1 + rng.geometric(0.55, (h, w)) - 1
    bigm = rng.random((h, w)) < big
    mag = np.where(bigm, mag + rng.integers(2, 40, (h, w)), mag)
    if huge:
        mag = np.where(rng.random((h, w)) < huge, rng.integers(1000, 32768, (h, w)), mag)
    sign = np.where(rng.random((h, w)) < 0.5, -1, 1)
    c = (nz * mag * sign).astype(np.int32)
    c[(xx + yy) > last_frac * (min(w, 32) + min(h, 32))] = 0
    c[:, 32:] = 0
    c[32:, :] = 0
    if not c.any():
        c[rng.integers(0, min(h, 32)), rng.integers(0, min(w, 32))] = int(rng.integers(1, 4)) * int(rng.choice([-1, 1]))
    return c
