"""ctypes binding of include/cabac_hip.h and its extension headers — test/bench plumbing; the product is the shared library."""
import ctypes
import sys
import os
import weakref

import numpy as np

from .build import build_library

NUM_CTX = 379
REC_BIN = 0x8000
REC_ALIGN, REC_EP, REC_TRM = 0x1FD, 0x1FE, 0x1FF
SUB_FINISH, SUB_ALIGN_RBSP = 0x100, 0x200
CABAC_INIT_B, CABAC_INIT_P, CABAC_INIT_I = 0, 1, 2
RES_OVERFLOW, RES_BAD_RECORD, RES_UNDERRUN, RES_BAD_STOP, RES_RANGE = 1, 2, 4, 8, 16

DESC_DTYPE = np.dtype([("rec_offset", "<u8"), ("byte_offset", "<u8"), ("n_records", "<u4"),
                       ("byte_capacity", "<u4"), ("qp", "<i4"), ("init_id", "<u4")])
RESULT_DTYPE = np.dtype([("n_bits", "<u4"), ("flags", "<u4")])
assert DESC_DTYPE.itemsize == 32 and RESULT_DTYPE.itemsize == 8
# cabac_tu_desc (include/cabac_hip.h): one transform block for the residual binariser
TU_DTYPE = np.dtype([("coeff_offset", "<u8"), ("log2_width", "u1"), ("log2_height", "u1"), ("channel", "u1"),
                     ("flags", "u1"), ("max_log2_tr_range", "u1"), ("reserved", "u1", (3,))])
assert TU_DTYPE.itemsize == 16
TU_DEP_QUANT, TU_SIGN_HIDING, TU_TS_FLAG, TU_TRANSFORM_SKIP, TU_BDPCM, TU_SBT_ZERO_OUT = 1, 2, 4, 8, 16, 32
TU_INFO_MTS_VIOLATION, TU_INFO_EMPTY, TU_INFO_BAD_DESC = 0x10000, 0x80000000, 0x40000000
TU_INFO_TS = 0x20000
SPLICE_DTYPE = np.dtype([("at", "<u4"), ("tu", "<u4")])          # cabac_splice
BIN_COUNT_WORDS = NUM_CTX + 2                                    # CABAC_BIN_COUNT_WORDS
SUB_PROBE = 0x400

EXPORTS = [
    "cabac_hip_encode_bound", "cabac_hip_init", "cabac_hip_destroy", "cabac_hip_strerror",
    "cabac_hip_last_error", "cabac_hip_set_stream", "cabac_hip_synchronize", "cabac_hip_set_variant",
    "cabac_hip_encode_device", "cabac_hip_decode_device", "cabac_hip_ctx_init_device",
    "cabac_hip_binarize_device", "cabac_hip_residual_device", "cabac_hip_residual_batch", "cabac_hip_residual_parse_device", "cabac_hip_residual_parse_batch", "cabac_hip_encode_batch", "cabac_hip_decode_batch",
    "cabac_hip_last_kernel_ms", "cabac_synth_records", "cabac_hip_profile_enable", "cabac_hip_profile_read",
    "cabac_hip_assemble_device", "cabac_hip_split_device", "cabac_hip_count_emulations_device",
    "cabac_hip_estimate_device", "cabac_hip_estimate_batch", "cabac_hip_estimate_from_device",
    "cabac_hip_host_alloc", "cabac_hip_host_free", "cabac_hip_host_register", "cabac_hip_host_unregister",
    "cabac_hip_host_is_pinned", "cabac_hip_encode_batch_payload", "cabac_hip_wait_event", "cabac_hip_record_event",
    "cabac_hip_encode_residual_device", "cabac_hip_encode_batch_residual", "cabac_hip_encode_residual16_device",
    "cabac_hip_encode_batch_residual16", "cabac_hip_decode_batch_packed", "cabac_hip_residual_parse16_device",
    "cabac_hip_residual_parse_batch16", "cabac_hip_gather_records_device",
]
# include/cabac_hip_estimate.h (the fused residual estimator; tests/test_residual_estimate_abi.py compares that header with this list)
EXPORTS_ESTIMATE = [
    "cabac_hip_estimate_residual_device", "cabac_hip_estimate_residual16_device", "cabac_hip_estimate_residual_batch",
]
# include/cabac_hip_nal.h (emulation prevention; tests/test_nal_abi.py compares that header with this list)
EXPORTS_NAL = [
    "cabac_hip_nal_escape_bound", "cabac_hip_nal_escape_device", "cabac_hip_nal_unescape_device", "cabac_hip_nal_escape_batch",
    "cabac_hip_nal_unescape_batch", "cabac_hip_encode_batch_nal",
]
# include/cabac_hip_search.h (search rounds; tests/test_search_abi.py compares that header with this list)
EXPORTS_SEARCH = [
    "cabac_hip_estimate_residual_ctx_device", "cabac_hip_estimate_residual_ctx16_device", "cabac_hip_search_select_device",
    "cabac_hip_search_round_device", "cabac_hip_search_round_batch",
]
# include/cabac_hip_search_unit.h (search rounds over candidates with side records; tests/test_search_unit_abi.py compares)
EXPORTS_SEARCH_UNIT = [
    "cabac_hip_estimate_unit_device", "cabac_hip_search_unit_round_device", "cabac_hip_search_unit_round_batch",
]
# include/cabac_hip_search_emit.h (the winner log; tests/test_search_emit_abi.py compares that header with this list)
EXPORTS_SEARCH_EMIT = [
    "cabac_hip_search_log_create", "cabac_hip_search_log_destroy", "cabac_hip_search_log_reset_device",
    "cabac_hip_search_log_append_device", "cabac_hip_search_log_view", "cabac_hip_search_log_encode_device",
]
# include/cabac_hip_parse_unit.h (spliced substreams read back; tests/test_parse_unit_abi.py compares that header with this list)
EXPORTS_PARSE_UNIT = [
    "cabac_hip_parse_unit_device", "cabac_hip_parse_unit_batch",
]
# include/cabac_hip_parse_elements.h (the unit parse over a plan of syntax elements; tests/test_parse_elements_abi.py compares)
EXPORTS_PARSE_ELEMENTS = [
    "cabac_hip_parse_elements_device", "cabac_hip_parse_elements_batch",
]
# include/cabac_hip_parse_plan.h (the element parse with computed entries; tests/test_parse_plan_abi.py compares)
EXPORTS_PARSE_PLAN = [
    "cabac_hip_parse_plan_device", "cabac_hip_parse_plan_batch",
]
# include/cabac_hip_write_plan.h (plan and values to coded substreams; tests/test_write_plan_abi.py compares)
EXPORTS_WRITE_PLAN = [
    "cabac_hip_write_plan_device", "cabac_hip_write_plan_batch",
]
# include/cabac_hip_search_plan.h (search rounds over plans; tests/test_search_plan_abi.py compares)
EXPORTS_SEARCH_PLAN = [
    "cabac_hip_resolve_plan_device", "cabac_hip_search_plan_round_device", "cabac_hip_search_plan_round_batch",
]
# include/cabac_hip_ctx_sets.h (the codec from and into context sets, WPP on top; tests/test_ctx_sets_abi.py compares)
EXPORTS_CTX_SETS = [
    "cabac_hip_encode_sets_device", "cabac_hip_decode_sets_device", "cabac_hip_ctx_advance_device", "cabac_hip_encode_wpp_device",
    "cabac_hip_decode_wpp_device", "cabac_hip_encode_wpp_batch", "cabac_hip_decode_wpp_batch",
]
# include/cabac_hip_plan_rows.h (the plan parse and the plan write from and into sets, and in WPP rows; tests/test_plan_rows_abi.py
# compares)
EXPORTS_PLAN_ROWS = [
    "cabac_hip_plan_parse_sets_device", "cabac_hip_plan_parse_rows_device", "cabac_hip_plan_parse_rows_batch",
    "cabac_hip_plan_write_sets_device", "cabac_hip_plan_write_rows_device", "cabac_hip_plan_write_rows_batch",
]
# include/cabac_hip_splice_rows.h (the splice pipeline and the winner log's emit from and into sets, and in WPP rows;
# tests/test_splice_rows_abi.py compares)
EXPORTS_SPLICE_ROWS = [
    "cabac_hip_encode_residual_sets_device", "cabac_hip_encode_residual_rows_device", "cabac_hip_encode_residual_rows_batch",
    "cabac_hip_search_log_mark_device", "cabac_hip_search_log_encode_sets_device", "cabac_hip_search_log_encode_rows_device",
]
# include/cabac_hip_workspace.h (the fixed workspace: the nine calls that code a slice to bytes without a host wait;
# tests/test_workspace_abi.py compares)
EXPORTS_WORKSPACE = [
    "cabac_hip_workspace_bound", "cabac_hip_workspace_fix", "cabac_hip_workspace_release", "cabac_hip_workspace_status_device",
    "cabac_hip_workspace_status", "cabac_hip_workspace_waits",
]
# include/cabac_hip_sparse.h (the sparse coefficient transport: blocks as lists of their non-zero coefficients;
# tests/test_sparse_abi.py compares)
EXPORTS_SPARSE = [
    "cabac_hip_sparse_pack_host", "cabac_hip_sparse_unpack_host", "cabac_hip_sparse_expand_device", "cabac_hip_sparse_compact_device",
    "cabac_hip_sparse_encode_batch", "cabac_hip_sparse_parse_batch",
]
SPARSE_STATUS_DTYPE = np.dtype([("n_entries", "<u8"), ("flags", "<u4"), ("first_bad", "<u4")])   # cabac_sparse_status
assert SPARSE_STATUS_DTYPE.itemsize == 16
SPARSE_OVERFLOW, SPARSE_RANGE, SPARSE_BAD_POS, SPARSE_BAD_FIRST, SPARSE_BAD_BLOCK = 1, 2, 4, 8, 16   # CABAC_SPARSE_*
SPARSE_NO_BAD = 0xFFFFFFFF                                       # CABAC_SPARSE_NO_BAD
# include/cabac_hip_rec10.h (the packed bin records: 64 records in 80 bytes; tests/test_rec10_abi.py compares)
EXPORTS_REC10 = [
    "cabac_hip_rec10_bytes", "cabac_hip_rec10_pack_host", "cabac_hip_rec10_unpack_host", "cabac_hip_rec10_unpack_device",
    "cabac_hip_rec10_pack_device", "cabac_hip_rec10_encode_batch", "cabac_hip_rec10_encode_batch_payload",
    "cabac_hip_rec10_decode_batch",
]
# include/cabac_hip_probe.h (probe points: written and estimated bits inside a substream; tests/test_probe_abi.py compares)
EXPORTS_PROBE = [
    "cabac_hip_written_bits_device", "cabac_hip_estimate_probes_device", "cabac_hip_encode_residual_probes_device",
    "cabac_hip_written_bits_batch", "cabac_hip_estimate_probes_batch", "cabac_hip_encode_residual_probes_batch",
]
# include/cabac_hip_pieces.h (the bin codec in pieces: the coder state handed from call to call; tests/test_pieces_abi.py compares)
EXPORTS_PIECES = ["cabac_hip_encode_pieces_device", "cabac_hip_decode_pieces_device"]
CODER_STATE_DTYPE = np.dtype([("kind", "<u4"), ("flags", "<u4"), ("bits", "<u4"), ("bytes_final", "<u4"), ("priv", "<u4", (4,))])  # cabac_coder_state
assert CODER_STATE_DTYPE.itemsize == 32
CODER_FRESH, CODER_ENC, CODER_DEC, CODER_CLOSED = 0, 1, 2, 3     # CABAC_CODER_*
RES_BAD_STATE = 0x80                                             # CABAC_RES_BAD_STATE
# include/cabac_hip_piece_encoder.h (which encoder codes the pieces: a per-ctx setting; tests/test_piece_encoder_abi.py compares)
EXPORTS_PIECE_ENCODER = ["cabac_hip_piece_encoder_set", "cabac_hip_piece_encoder_get"]
# include/cabac_hip_plan_resume.h (the plan parse in pieces: resumed from a coder state; tests/test_plan_resume_abi.py compares)
EXPORTS_PLAN_RESUME = ["cabac_hip_plan_resume_parse_device"]
# include/cabac_hip_plan_continue.h (the plan write in pieces: continued from a coder state; tests/test_plan_continue_abi.py compares)
EXPORTS_PLAN_CONTINUE = ["cabac_hip_plan_continue_write_device"]
REC10_STATUS_DTYPE = np.dtype([("first_bad", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])   # cabac_rec10_status
assert REC10_STATUS_DTYPE.itemsize == 16
REC10_BAD_BITS, REC10_OVERFLOW = 1, 2                            # CABAC_REC10_*
REC10_NO_BAD = 0xFFFFFFFFFFFFFFFF                                # first_bad with no bad record (UINT64_MAX)
REC10_BLOCK_RECORDS, REC10_BLOCK_BYTES = 64, 80                  # CABAC_REC10_BLOCK_*
WS_ROWS = 0x1                                                    # CABAC_WS_ROWS (cabac_workspace_sizes.flags)
WS_OVER_RECORDS, WS_OVER_SLOTS, WS_BAD_SPLICES, WS_RECORDS_32BIT, WS_LOG_OVERFLOW, WS_LOG_DAMAGED = 1, 2, 4, 8, 16, 32   # status flags
WS_NONE_VOIDED = 0xFFFFFFFF                                      # CABAC_WS_NONE_VOIDED
WORKSPACE_SIZES_DTYPE = np.dtype([("n_sub", "<u4"), ("n_tu", "<u4"), ("n_entries", "<u8"), ("expanded_records", "<u8"),
                                  ("slot_bytes", "<u8"), ("log_records", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])
WORKSPACE_STATUS_DTYPE = np.dtype([("records_needed", "<u8"), ("slot_bytes_needed", "<u8"), ("flags", "<u4"), ("n_calls", "<u4"),
                                   ("n_voided", "<u4"), ("first_voided", "<u4")])
assert WORKSPACE_SIZES_DTYPE.itemsize == 48 and WORKSPACE_STATUS_DTYPE.itemsize == 32
CTX_NO_SET = 0xFFFFFFFF                                          # CABAC_CTX_NO_SET
RES_BAD_SET = 0x40                                               # CABAC_RES_BAD_SET
PE_COND, PE_BLOCK_INFO = 9, 10                                   # CABAC_PE_COND, CABAC_PE_BLOCK_INFO
JOIN_NONE, JOIN_AND, JOIN_OR = range(3)                          # CABAC_JOIN_*
RES_BAD_VALUE = 0x20                                             # CABAC_RES_BAD_VALUE
TU_INFO_NOT_CODED = 0x40000                                      # CABAC_TU_INFO_NOT_CODED
SE_CTX_BIN, SE_EP_BINS, SE_REM_ABS, SE_TRM, SE_UNARY_MAX, SE_UNARY_EP, SE_EXP_GOLOMB, SE_TRUNC_BIN, SE_ALIGN = range(9)   # CABAC_SE_*
GUARD_NE, GUARD_EQ, GUARD_GE, GUARD_LT = range(4)                # CABAC_GUARD_*
SEARCH_NO_CHAIN = 0xFFFFFFFF                                     # CABAC_SEARCH_NO_CHAIN
SEARCH_LOG_OVERFLOW = 0x1                                        # CABAC_SEARCH_LOG_OVERFLOW and the capacity that was too small
SEARCH_LOG_OVER_ENTRIES, SEARCH_LOG_OVER_RECORDS, SEARCH_LOG_OVER_BLOCKS, SEARCH_LOG_OVER_COEFFS = 0x10, 0x20, 0x40, 0x80
SEARCH_LOG_OVER_CHAIN_RECORDS = 0x100
LOG_COUNTERS_DTYPE = np.dtype([("n_entry", "<u8"), ("n_record", "<u8"), ("n_tu", "<u8"), ("n_coeff", "<u8"), ("flags", "<u4"),
                               ("reserved", "<u4")])             # cabac_search_log_counters
LOG_ENTRY_DTYPE = np.dtype([("rec_first", "<u8"), ("chain", "<u4"), ("n_rec", "<u4"), ("n_tu", "<u4"), ("tu_first", "<u4"),
                            ("chain_rec_first", "<u4"), ("chain_tu_first", "<u4")])   # cabac_search_log_entry
assert LOG_COUNTERS_DTYPE.itemsize == 40 and LOG_ENTRY_DTYPE.itemsize == 32
SEARCH_NO_SET = SEARCH_NONE = 0xFFFFFFFF                        # CABAC_SEARCH_NO_SET, CABAC_SEARCH_NONE
NAL_STATUS_DTYPE = np.dtype([("out_bytes", "<u8"), ("n_changed", "<u4"), ("flags", "<u4")])   # cabac_nal_status
assert NAL_STATUS_DTYPE.itemsize == 16
NAL_OVERFLOW, NAL_TRAILING_ZERO, NAL_FORBIDDEN, NAL_BAD_ESCAPE, NAL_LOC_OVERFLOW, NAL_INPUT_CLIPPED = 1, 2, 4, 8, 16, 32

_lib = None
vp = ctypes.c_void_p


def _opt(p):
    """A device address as an optional pointer argument: 0 is NULL."""
    return vp(p) if p else None


def _ptr(a):
    """The address of an optional host array: None is NULL."""
    return a.ctypes.data if a is not None else None


def splices_to_tu_at(splices):
    """One substream's sorted cabac_splice list (SPLICE_DTYPE: at, tu) -> (block order, tu_at): the indices into tus[] in coded
    order and the position of each in the substream's side run — with the records and descriptors handed to
    encode_residual_device everything parse_unit_device needs to read that substream back."""
    splices = np.ascontiguousarray(splices, SPLICE_DTYPE)
    if len(splices) > 1 and (np.diff(splices["at"].astype(np.int64)) < 0).any():
        raise ValueError("the splice list is not sorted by `at`")
    return splices["tu"].astype(np.uint32), splices["at"].astype(np.uint32)


def element(kind, ctx=0, ctx_n=None, n=0, rice=0, cutoff=5, max_log2=15, max_symbol=0, count=0):
    """word0 of a syntax-element record (include/cabac_hip.h, "Syntax-element record"), the layout cabac_hip_binarize_device
    reads: kind in bits 3..0, then per kind — CTX_BIN ctx; EP_BINS n; REM_ABS rice, cutoff, max_log2; UNARY_MAX ctx, ctx_n
    (default ctx), max_symbol; UNARY_EP max_symbol; EXP_GOLOMB count; TRUNC_BIN max_symbol; TRM and ALIGN nothing.  Nothing is
    range-checked beyond the field widths: a plan with a bad entry is the callee's to refuse."""
    kind = int(kind)
    if not 0 <= kind <= 15:
        raise ValueError("kind must fit four bits")

    def field(v, bits, shift):
        v = int(v)
        if not 0 <= v < (1 << bits):
            raise ValueError("a parameter does not fit its field")
        return v << shift
    if kind == SE_CTX_BIN:
        return kind | field(ctx, 9, 4)
    if kind == SE_EP_BINS:
        return kind | field(n, 6, 4)
    if kind == SE_REM_ABS:
        return kind | field(rice, 5, 4) | field(cutoff, 5, 9) | field(max_log2, 6, 14)
    if kind == SE_UNARY_MAX:
        return kind | field(ctx, 9, 4) | field(ctx if ctx_n is None else ctx_n, 9, 13) | field(max_symbol, 8, 22)
    if kind == SE_UNARY_EP:
        return kind | field(max_symbol, 6, 4)
    if kind == SE_EXP_GOLOMB:
        return kind | field(count, 5, 4)
    if kind == SE_TRUNC_BIN:
        return kind | field(max_symbol, 28, 4)
    return kind


def guard(back, cmp=GUARD_NE, imm=0):
    """word1 of a plan element, or a block's guard word (include/cabac_hip_parse_elements.h, "GUARD WORD"): coded iff
    value(i - back) cmp imm; back 0 = unguarded."""
    back, cmp, imm = int(back), int(cmp), int(imm)
    if not (0 <= back <= 255 and 0 <= cmp <= 3 and 0 <= imm <= 0xFFFF):
        raise ValueError("back is 0..255, cmp 0..3, imm 0..65535")
    return back | (cmp << 8) | (imm << 16)


def cond(test_back, cmp=GUARD_NE, imm=0, join=JOIN_NONE, back2=0):
    """(word0, word1) of a CABAC_PE_COND entry (include/cabac_hip_parse_plan.h, "KIND 9"): value = value(i - test_back) cmp imm
    (test_back 0: 1), joined by AND / OR with value(i - back2) != 0."""
    join, back2 = int(join), int(back2)
    if not (0 <= join <= 2 and 0 <= back2 <= 255):
        raise ValueError("join is 0..2, back2 0..255")
    return PE_COND | (back2 << 4) | (join << 12), guard(test_back, cmp, imm)


def block_info(which=0, shift=0, width=16):
    """word0 of a CABAC_PE_BLOCK_INFO entry (include/cabac_hip_parse_plan.h, "KIND 10"): bits shift .. shift + width - 1 of the
    info word of the block `which` blocks in front of the last one walked."""
    which, shift, width = int(which), int(shift), int(width)
    if not (0 <= which <= 15 and 0 <= shift <= 31 and 1 <= width <= 32 and shift + width <= 32):
        raise ValueError("which is 0..15, shift 0..31, width 1..32, shift + width at most 32")
    return PE_BLOCK_INFO | (which << 4) | (shift << 8) | (width << 13)


class SearchLogView(ctypes.Structure):
    """cabac_search_log_view: const device pointers into a winner log and what it was created with."""
    _fields_ = [("d_counters", vp), ("d_entries", vp), ("d_records", vp), ("d_tu", vp), ("d_tu_at", vp), ("d_coeff", vp),
                ("record_capacity", ctypes.c_uint64), ("coeff_capacity", ctypes.c_uint64), ("n_chain", ctypes.c_uint32),
                ("entry_capacity", ctypes.c_uint32), ("tu_capacity", ctypes.c_uint32), ("coeff_bytes", ctypes.c_int32)]


# every CabacHip / PinnedArray that has not been closed yet: close_all() ends them in a defined order (contexts first, then
# the pinned buffers they may still have been copying from) while the HIP runtime is certainly alive
_live = weakref.WeakSet()


def close_all():
    """Close every live context, then every live pinned array.  Call before the process ends (a test session's last
    fixture, a server's shutdown hook): teardown then happens here, in this order, and not in whatever order the
    interpreter and the loaded libraries are finalized in."""
    objs = list(_live)
    for o in objs:
        if isinstance(o, CabacHip):
            o.close()
    for o in objs:
        if isinstance(o, PinnedArray):
            o.close()


def load_library():
    """Load libcabac_hip.so (building it first if the sources are newer). Loading does not need a GPU;
    cabac_hip_init does."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # torch bundles its own libamdhip64.so.7; whichever copy is loaded first serves the whole
        # process (same SONAME), and torch only works with its own.  Load it first so that this
        # library and torch share ONE HIP runtime (device memory, streams) in python processes.
        import torch  # noqa: F401
    except ImportError:
        pass
    # CABAC_HIP_LIBRARY: load this build of the library instead (experiments: the same sources under other compiler flags)
    L = ctypes.CDLL(os.environ.get("CABAC_HIP_LIBRARY") or build_library())
    L.cabac_hip_encode_bound.restype = ctypes.c_size_t
    L.cabac_hip_encode_bound.argtypes = [ctypes.c_uint64] * 3
    L.cabac_hip_init.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.cabac_hip_destroy.argtypes = [vp]
    L.cabac_hip_destroy.restype = None
    L.cabac_hip_strerror.restype = ctypes.c_char_p
    L.cabac_hip_strerror.argtypes = [ctypes.c_int]
    L.cabac_hip_last_error.restype = ctypes.c_char_p
    L.cabac_hip_last_error.argtypes = [vp]
    L.cabac_hip_set_stream.argtypes = [vp, vp]
    L.cabac_hip_synchronize.argtypes = [vp]
    L.cabac_hip_wait_event.argtypes = [vp, vp]
    L.cabac_hip_record_event.argtypes = [vp, vp]
    L.cabac_hip_set_variant.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.cabac_hip_encode_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp]
    L.cabac_hip_decode_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp]
    L.cabac_hip_ctx_init_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp]
    L.cabac_hip_binarize_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp]
    sets7 = [ctypes.c_uint32] + [vp] * 6   # n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate
    # (CABAC_HIP_LIBRARY may name a build from before cabac_hip_ctx_sets.h — tools/bench_ctx_sets.py --legs plain --label parent —:
    # everything else is bound all the same)
    if hasattr(L, "cabac_hip_encode_sets_device"):
        L.cabac_hip_encode_sets_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp] + sets7
        L.cabac_hip_decode_sets_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp] + sets7
        L.cabac_hip_ctx_advance_device.argtypes = [vp, ctypes.c_uint32, vp, vp] + sets7 + [vp]
        L.cabac_hip_encode_wpp_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32, vp, vp, vp]
        L.cabac_hip_decode_wpp_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp, ctypes.c_uint32, vp, vp, vp]
        L.cabac_hip_encode_wpp_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, ctypes.c_uint32,
                                                 vp, vp, vp]
        L.cabac_hip_decode_wpp_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp,
                                                 ctypes.c_uint32, vp, vp, vp]
    if hasattr(L, "cabac_hip_encode_pieces_device"):   # (a library from before cabac_hip_pieces.h: the calls then fail where they are made)
        L.cabac_hip_encode_pieces_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp] + sets7 + [vp, vp]
        L.cabac_hip_decode_pieces_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp] + sets7 + [vp, vp]
    if hasattr(L, "cabac_hip_piece_encoder_set"):      # (a library from before cabac_hip_piece_encoder.h: the calls then fail where they are made)
        L.cabac_hip_piece_encoder_set.argtypes = [vp, ctypes.c_int]
        L.cabac_hip_piece_encoder_get.argtypes = [vp]
    L.cabac_hip_residual_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    L.cabac_hip_residual_parse_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, vp]
    L.cabac_hip_residual_parse_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp, vp, ctypes.c_uint64, vp, vp]
    L.cabac_hip_residual_parse_batch16.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp, vp, ctypes.c_uint64, vp, vp]
    L.cabac_hip_residual_parse16_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, vp]
    L.cabac_hip_residual_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp, vp, ctypes.c_uint64]
    L.cabac_hip_encode_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp]
    L.cabac_hip_decode_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp]
    L.cabac_hip_decode_batch_packed.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp]
    L.cabac_hip_encode_batch_payload.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp]
    L.cabac_hip_encode_residual_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp,
                                                   vp, ctypes.c_uint64, vp, vp, vp, vp]
    L.cabac_hip_encode_residual16_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp,
                                                   vp, ctypes.c_uint64, vp, vp, vp, vp]
    L.cabac_hip_encode_batch_residual.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint32, vp, vp,
                                                  ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp, vp, vp]
    L.cabac_hip_encode_batch_residual16.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint32, vp, vp,
                                                  ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp, vp, vp]
    L.cabac_hip_gather_records_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp]
    L.cabac_hip_last_kernel_ms.restype = ctypes.c_float
    L.cabac_hip_last_kernel_ms.argtypes = [vp]
    L.cabac_hip_assemble_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint64, vp]
    L.cabac_hip_split_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp]
    L.cabac_hip_count_emulations_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp]
    L.cabac_hip_estimate_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp]
    L.cabac_hip_estimate_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp]
    L.cabac_hip_estimate_from_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, vp]
    L.cabac_hip_estimate_residual_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.cabac_hip_estimate_residual16_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.cabac_hip_estimate_residual_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_int, ctypes.c_uint64, vp, vp,
                                                    ctypes.c_uint32, vp, vp, vp, vp]
    L.cabac_hip_estimate_residual_ctx_device.argtypes = [vp, ctypes.c_uint32] + [vp] * 12
    L.cabac_hip_estimate_residual_ctx16_device.argtypes = [vp, ctypes.c_uint32] + [vp] * 12
    L.cabac_hip_search_select_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, vp]
    L.cabac_hip_search_round_device.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp,
                                                ctypes.c_uint64, vp, vp, vp, vp, vp]
    L.cabac_hip_search_round_batch.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_int, ctypes.c_uint64, vp,
                                               vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, vp]
    L.cabac_hip_estimate_unit_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_int] + [vp] * 13
    L.cabac_hip_search_unit_round_device.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_int] + [vp] * 8 + \
        [ctypes.c_uint64] + [vp] * 6
    L.cabac_hip_search_unit_round_batch.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_int, ctypes.c_uint64,
                                                    vp, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, ctypes.c_uint64,
                                                    vp, vp, vp, vp, vp]
    L.cabac_hip_parse_unit_device.argtypes = [vp, ctypes.c_uint32] + [vp] * 7 + [ctypes.c_int] + [vp] * 3
    L.cabac_hip_parse_unit_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, ctypes.c_uint64, vp,
                                             ctypes.c_int, ctypes.c_uint64, vp, vp, vp]
    L.cabac_hip_parse_elements_device.argtypes = [vp, ctypes.c_uint32] + [vp] * 8 + [ctypes.c_int] + [vp] * 3
    L.cabac_hip_parse_elements_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, vp, ctypes.c_uint64, vp,
                                                 ctypes.c_int, ctypes.c_uint64, vp, vp, vp]
    L.cabac_hip_parse_plan_device.argtypes = [vp, ctypes.c_uint32] + [vp] * 8 + [ctypes.c_int] + [vp] * 3
    L.cabac_hip_parse_plan_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, vp, ctypes.c_uint64, vp,
                                             ctypes.c_int, ctypes.c_uint64, vp, vp, vp]
    L.cabac_hip_write_plan_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_int, vp,
                                              ctypes.c_uint64, vp, vp, vp, vp]
    L.cabac_hip_write_plan_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, vp, ctypes.c_int,
                                             ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp, vp, vp]
    # (CABAC_HIP_LIBRARY may name a build from before cabac_hip_plan_rows.h — tools/bench_plan_rows.py --label parent)
    if hasattr(L, "cabac_hip_plan_parse_sets_device"):
        rows4 = [ctypes.c_uint32, vp, vp, vp]   # n_level, level_first, sync_from, sync_at
        L.cabac_hip_plan_parse_sets_device.argtypes = L.cabac_hip_parse_plan_device.argtypes + sets7 + [vp]
        L.cabac_hip_plan_parse_rows_device.argtypes = L.cabac_hip_parse_plan_device.argtypes + rows4
        L.cabac_hip_plan_parse_rows_batch.argtypes = L.cabac_hip_parse_plan_batch.argtypes + rows4
        L.cabac_hip_plan_write_sets_device.argtypes = L.cabac_hip_write_plan_device.argtypes + sets7
        L.cabac_hip_plan_write_rows_device.argtypes = L.cabac_hip_write_plan_device.argtypes + rows4
        L.cabac_hip_plan_write_rows_batch.argtypes = L.cabac_hip_write_plan_batch.argtypes + rows4
    # (... or from before cabac_hip_plan_resume.h — tools/bench_plan_resume.py --label parent)
    if hasattr(L, "cabac_hip_plan_resume_parse_device"):
        L.cabac_hip_plan_resume_parse_device.argtypes = L.cabac_hip_parse_plan_device.argtypes + sets7 + [vp, vp]
    # (... or from before cabac_hip_plan_continue.h — tools/bench_plan_continue.py --label parent)
    if hasattr(L, "cabac_hip_plan_continue_write_device"):
        L.cabac_hip_plan_continue_write_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_int,
                                                           vp, vp, vp, vp] + sets7 + [vp, vp]
    L.cabac_hip_resolve_plan_device.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_int, vp, vp,
                                                ctypes.c_uint64, vp, vp, vp, vp, vp, vp]
    L.cabac_hip_search_plan_round_device.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, ctypes.c_int] + \
        [vp] * 10 + [ctypes.c_uint64] + [vp] * 8 + [ctypes.c_uint64] + [vp] * 4
    L.cabac_hip_search_plan_round_batch.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_int, ctypes.c_uint64,
                                                    vp, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, vp,
                                                    ctypes.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    L.cabac_hip_search_log_create.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64,
                                              ctypes.c_int, ctypes.POINTER(vp)]
    L.cabac_hip_search_log_destroy.argtypes = [vp]
    L.cabac_hip_search_log_reset_device.argtypes = [vp]
    L.cabac_hip_search_log_append_device.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_int, vp, vp, vp]
    L.cabac_hip_search_log_view.argtypes = [vp, ctypes.POINTER(SearchLogView)]
    L.cabac_hip_search_log_encode_device.argtypes = [vp, vp, vp, ctypes.c_uint64, vp, vp, vp, vp]
    # (CABAC_HIP_LIBRARY may name a build from before cabac_hip_splice_rows.h)
    if hasattr(L, "cabac_hip_encode_residual_sets_device"):
        rows5 = [ctypes.c_uint32, vp, vp, vp, vp]   # n_level, level_first, sync_from, sync_at, sync_splice
        plain = L.cabac_hip_encode_residual_device.argtypes
        plain = plain[:10] + [ctypes.c_int] + plain[10:]                     # const void *d_coeff, int coeff_bytes
        plain_b = L.cabac_hip_encode_batch_residual.argtypes
        plain_b = plain_b[:10] + [ctypes.c_int] + plain_b[10:]
        L.cabac_hip_encode_residual_sets_device.argtypes = plain + sets7
        L.cabac_hip_encode_residual_rows_device.argtypes = plain + rows5
        L.cabac_hip_encode_residual_rows_batch.argtypes = plain_b + rows5
        L.cabac_hip_search_log_mark_device.argtypes = [vp, ctypes.c_uint32, vp]
        L.cabac_hip_search_log_encode_sets_device.argtypes = L.cabac_hip_search_log_encode_device.argtypes + sets7
        L.cabac_hip_search_log_encode_rows_device.argtypes = L.cabac_hip_search_log_encode_device.argtypes + [ctypes.c_uint32, vp, vp]
    # (CABAC_HIP_LIBRARY may name a build from before cabac_hip_workspace.h)
    if hasattr(L, "cabac_hip_workspace_fix"):
        L.cabac_hip_workspace_bound.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, vp, vp]
        L.cabac_hip_workspace_fix.argtypes = [vp, vp]
        L.cabac_hip_workspace_release.argtypes = [vp]
        L.cabac_hip_workspace_status_device.argtypes = [vp, vp]
        L.cabac_hip_workspace_status.argtypes = [vp, vp]
        L.cabac_hip_workspace_waits.argtypes = [vp, vp]
    L.cabac_hip_nal_escape_bound.restype = ctypes.c_size_t
    if hasattr(L, "cabac_hip_sparse_pack_host"):
        u32, u64 = ctypes.c_uint32, ctypes.c_uint64
        L.cabac_hip_sparse_pack_host.argtypes = [u32, vp, vp, ctypes.c_int, u64, vp, vp, u64, vp]
        L.cabac_hip_sparse_unpack_host.argtypes = [u32, vp, vp, vp, u64, vp, ctypes.c_int, u64, vp]
        L.cabac_hip_sparse_expand_device.argtypes = [vp, u32, vp, vp, vp, u64, vp, ctypes.c_int, u64, vp]
        L.cabac_hip_sparse_compact_device.argtypes = [vp, u32, vp, vp, ctypes.c_int, u64, vp, vp, u64, vp]
        L.cabac_hip_sparse_encode_batch.argtypes = [vp, u32, vp, vp, u64, vp, vp, u32, vp, vp, vp, u64, u64, vp, u64, vp, vp, vp, vp]
        L.cabac_hip_sparse_parse_batch.argtypes = [vp, u32, vp, vp, u64, vp, vp, vp, vp, u64, u64, vp, vp, vp]
    if hasattr(L, "cabac_hip_rec10_bytes"):
        u32, u64 = ctypes.c_uint32, ctypes.c_uint64
        L.cabac_hip_rec10_bytes.argtypes = [u64, vp]
        L.cabac_hip_rec10_pack_host.argtypes = [vp, u64, vp, u64, vp]
        L.cabac_hip_rec10_unpack_host.argtypes = [vp, u64, u64, vp]
        L.cabac_hip_rec10_unpack_device.argtypes = [vp, vp, u64, u64, vp]
        L.cabac_hip_rec10_pack_device.argtypes = [vp, vp, u64, vp, u64, vp]
        L.cabac_hip_rec10_encode_batch.argtypes = [vp, u32, vp, vp, u64, u64, vp, u64, vp]
        L.cabac_hip_rec10_encode_batch_payload.argtypes = [vp, u32, vp, vp, u64, u64, vp, u64, vp, vp]
        L.cabac_hip_rec10_decode_batch.argtypes = [vp, u32, vp, vp, u64, u64, vp, u64, vp, ctypes.c_int, vp]
    # (CABAC_HIP_LIBRARY may name a build from before cabac_hip_probe.h)
    if hasattr(L, "cabac_hip_written_bits_device"):
        u32, u64 = ctypes.c_uint32, ctypes.c_uint64
        probes = [vp, vp, u32]                      # probe_first, probe_at, n_probe
        sets4 = [u32, vp, vp, vp]                   # n_sets, state, rate, start_set
        L.cabac_hip_written_bits_device.argtypes = [vp, u32, vp, vp] + probes + sets4 + [vp, vp]
        L.cabac_hip_estimate_probes_device.argtypes = [vp, u32, vp, vp] + probes + sets4 + [vp, vp]
        L.cabac_hip_written_bits_batch.argtypes = [vp, u32, vp, vp, u64] + probes + sets4 + [vp, vp]
        L.cabac_hip_estimate_probes_batch.argtypes = [vp, u32, vp, vp, u64] + probes + sets4 + [vp, vp]
        plain = L.cabac_hip_encode_residual_device.argtypes
        plain_b = L.cabac_hip_encode_batch_residual.argtypes
        tail = [vp, vp, vp, u32, vp]                # probe_first, probe_at, probe_splice, n_probe, bits
        L.cabac_hip_encode_residual_probes_device.argtypes = plain[:10] + [ctypes.c_int] + plain[10:] + tail
        L.cabac_hip_encode_residual_probes_batch.argtypes = plain_b[:10] + [ctypes.c_int] + plain_b[10:] + tail
    L.cabac_hip_nal_escape_bound.argtypes = [ctypes.c_uint64]
    L.cabac_hip_nal_escape_device.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp]
    L.cabac_hip_nal_unescape_device.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp,
                                                ctypes.c_uint64, ctypes.c_uint32, vp]
    L.cabac_hip_nal_escape_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, vp]
    L.cabac_hip_nal_unescape_batch.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64,
                                               ctypes.c_uint32, vp]
    L.cabac_hip_encode_batch_nal.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp, vp, vp]
    L.cabac_hip_profile_enable.argtypes = [vp, ctypes.c_uint32]
    L.cabac_hip_profile_read.argtypes = [vp, vp, vp, ctypes.c_uint32]
    L.cabac_hip_host_alloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(vp)]
    L.cabac_hip_host_free.argtypes = [vp]
    L.cabac_hip_host_register.argtypes = [vp, ctypes.c_size_t]
    L.cabac_hip_host_unregister.argtypes = [vp]
    L.cabac_hip_host_is_pinned.argtypes = [vp, ctypes.c_size_t]
    L.cabac_synth_records.restype = None
    L.cabac_synth_records.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, vp]
    _lib = L
    return L


class CabacHipError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("cabac_hip status %d (%s): %s" % (status, load_library().cabac_hip_strerror(status).decode(), msg))
        self.status = status


def synth_records(seed, substream_index, n_bins, ctx_permille):
    L = load_library()
    out = np.empty(n_bins, np.uint16)
    L.cabac_synth_records(seed, substream_index, n_bins, ctx_permille, out.ctypes.data)
    return out


class PinnedArray:
    """A numpy array in page-locked host memory from cabac_hip_host_alloc (freed with close() / garbage collection):
    buffers the host-pointer entry points DMA without a staging copy."""

    def __init__(self, shape, dtype):
        L = load_library()
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = vp()
        rc = L.cabac_hip_host_alloc(max(n, 1), ctypes.byref(p))
        if rc != 0:
            raise CabacHipError(rc, "cabac_hip_host_alloc(%d)" % n)
        self._p = p
        _live.add(self)
        buf = (ctypes.c_uint8 * max(n, 1)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            load_library().cabac_hip_host_free(self._p)
            self._p = None
            _live.discard(self)

    def __del__(self):
        # not while the interpreter is shutting down: the HIP runtime (torch's, ours) may already be unloading then, and a
        # stream / event / pinned-memory release into a half-torn-down runtime can abort the process; the OS reclaims it all
        try:
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass


def host_is_pinned(a):
    a = np.asarray(a)
    return bool(load_library().cabac_hip_host_is_pinned(vp(a.ctypes.data), a.nbytes))


def encode_bound(n_ctx, n_ep, n_trm):
    return load_library().cabac_hip_encode_bound(n_ctx, n_ep, n_trm)


def nal_escape_bound(n_bytes):
    """cabac_hip_nal_escape_bound: the largest escape of n_bytes bytes."""
    return load_library().cabac_hip_nal_escape_bound(n_bytes)


def workspace_bound(n_sub, n_host_records, n_tu, n_coded_coeff):
    """cabac_hip_workspace_bound: (expanded_records, slot_bytes) that no call of that size can exceed.  Host arithmetic only."""
    out = np.zeros(2, np.uint64)
    rc = load_library().cabac_hip_workspace_bound(n_sub, n_host_records, n_tu, n_coded_coeff, vp(out.ctypes.data), vp(out.ctypes.data + 8))
    if rc != 0:
        raise CabacHipError(rc, "cabac_hip_workspace_bound")
    return int(out[0]), int(out[1])


def sparse_pack_host(tus, coeff, entry_capacity=None, entries=None, ent_first=None):
    """cabac_hip_sparse_pack_host (CPU, no GPU): dense blocks (int16 or int32 array) -> (ent_first uint32[n_tu + 1], entries, status
    record).  entry_capacity None: room for every element; `entries` / `ent_first` (optional): the caller's arrays, written in place."""
    tus = np.ascontiguousarray(tus, TU_DTYPE)
    assert coeff.dtype in (np.int16, np.int32) and coeff.flags.c_contiguous
    if entries is None:
        entries = np.zeros(max(len(coeff) if entry_capacity is None else int(entry_capacity), 1), np.uint32)
    cap = len(entries) if entry_capacity is None else int(entry_capacity)
    if ent_first is None:
        ent_first = np.zeros(len(tus) + 1, np.uint32)
    assert entries.dtype == np.uint32 and ent_first.dtype == np.uint32 and cap <= len(entries) and len(ent_first) >= len(tus) + 1
    status = np.zeros(1, SPARSE_STATUS_DTYPE)
    rc = load_library().cabac_hip_sparse_pack_host(len(tus), tus.ctypes.data, coeff.ctypes.data, coeff.itemsize, len(coeff),
                                                   ent_first.ctypes.data, entries.ctypes.data, cap, status.ctypes.data)
    if rc != 0:
        raise CabacHipError(rc, "cabac_hip_sparse_pack_host")
    return ent_first, entries[: min(int(status[0]["n_entries"]), cap)], status[0]


def sparse_unpack_host(tus, ent_first, entries, coeff, n_entries=None):
    """cabac_hip_sparse_unpack_host (CPU, no GPU): the lists written into the dense array `coeff` (int16 or int32, in place);
    returns the status record."""
    tus = np.ascontiguousarray(tus, TU_DTYPE)
    ent_first = np.ascontiguousarray(ent_first, np.uint32)
    entries = np.ascontiguousarray(entries, np.uint32)
    assert coeff.dtype in (np.int16, np.int32) and coeff.flags.c_contiguous and len(ent_first) >= len(tus) + 1
    status = np.zeros(1, SPARSE_STATUS_DTYPE)
    rc = load_library().cabac_hip_sparse_unpack_host(len(tus), tus.ctypes.data, ent_first.ctypes.data, entries.ctypes.data,
                                                     len(entries) if n_entries is None else int(n_entries), coeff.ctypes.data,
                                                     coeff.itemsize, len(coeff), status.ctypes.data)
    if rc != 0:
        raise CabacHipError(rc, "cabac_hip_sparse_unpack_host")
    return status[0]


def rec10_bytes(n_records):
    """cabac_hip_rec10_bytes: CABAC_REC10_BYTES(n_records), the size of n_records packed records."""
    out = ctypes.c_uint64(0)
    rc = load_library().cabac_hip_rec10_bytes(int(n_records), ctypes.byref(out))
    if rc != 0:
        raise CabacHipError(rc, "cabac_hip_rec10_bytes")
    return out.value


def rec10_pack_host(records, packed=None, packed_capacity=None):
    """cabac_hip_rec10_pack_host (CPU, no GPU): uint16 records -> packed uint8[rec10_bytes(n)].  `packed` (optional): the caller's
    array (e.g. pinned), written in place; packed_capacity defaults to its size.  A capacity that is too small or a record with
    reserved bits set raises with status CABAC_HIP_ERR_INVALID; the error's `first_bad` is then the smallest bad index
    (REC10_NO_BAD for the capacity)."""
    records = np.ascontiguousarray(records, np.uint16)
    if packed is None:
        packed = np.zeros(max(rec10_bytes(len(records)) if packed_capacity is None else int(packed_capacity), 1), np.uint8)
    cap = packed.nbytes if packed_capacity is None else int(packed_capacity)
    assert packed.dtype == np.uint8 and packed.flags.c_contiguous and cap <= packed.nbytes
    first_bad = ctypes.c_uint64(0)
    rc = load_library().cabac_hip_rec10_pack_host(records.ctypes.data, len(records), packed.ctypes.data, cap, ctypes.byref(first_bad))
    if rc != 0:
        e = CabacHipError(rc, "cabac_hip_rec10_pack_host")
        e.first_bad = first_bad.value
        raise e
    return packed[: rec10_bytes(len(records))]


def rec10_unpack_host(packed, first, n, records=None):
    """cabac_hip_rec10_unpack_host (CPU, no GPU): records first .. first + n - 1 of `packed` into records[first ..] (`records`:
    the caller's uint16 array of at least first + n, written in place, else a fresh zeroed one); returns `records`."""
    packed = np.ascontiguousarray(packed, np.uint8)
    first, n = int(first), int(n)
    assert n == 0 or rec10_bytes(first + n) <= packed.nbytes
    if records is None:
        records = np.zeros(first + n, np.uint16)
    assert records.dtype == np.uint16 and records.flags.c_contiguous and len(records) >= first + n
    rc = load_library().cabac_hip_rec10_unpack_host(packed.ctypes.data, first, n, records.ctypes.data)
    if rc != 0:
        raise CabacHipError(rc, "cabac_hip_rec10_unpack_host")
    return records


class CabacHip:
    """One codec context = one device + one HIP stream (stream=None: a non-blocking stream of the ctx's own; otherwise the
    caller's stream handle, 0 being the device's default stream).  Raises if there is no GPU (no CPU fallback)."""

    def __init__(self, device=0, stream=None):
        self.L = load_library()
        h = vp()
        rc = self.L.cabac_hip_init(device, ctypes.byref(h))
        if rc != 0:
            raise CabacHipError(rc, "cabac_hip_init(device=%d)" % device)
        self.h = h
        self.device = device
        _live.add(self)
        if stream is not None:
            # a HIP stream handle; 0 is the device's default stream (torch's current stream unless it was changed), which the
            # C ABI takes as CABAC_HIP_STREAM_DEFAULT — a null pointer there means "the ctx's own stream"
            self._check(self.L.cabac_hip_set_stream(self.h, vp(stream if stream else 1)))

    def close(self):
        if getattr(self, "h", None):
            for log in list(getattr(self, "_logs", ())):   # the winner logs of this ctx go first (close_all() closes them this way)
                log.close()
            self.L.cabac_hip_destroy(self.h)   # waits for the ctx's streams, then releases them
            self.h = None
            _live.discard(self)

    def __del__(self):
        # not while the interpreter is shutting down: the HIP runtime (torch's, ours) may already be unloading then, and a
        # stream / event / pinned-memory release into a half-torn-down runtime can abort the process; the OS reclaims it all
        try:
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass

    def _check(self, rc, allow_substream=False):
        if rc != 0 and not (allow_substream and rc == -5):
            raise CabacHipError(rc, self.L.cabac_hip_last_error(self.h).decode())
        return rc

    def set_variant(self, enc=0, dec=0):
        self._check(self.L.cabac_hip_set_variant(self.h, enc, dec))

    def piece_encoder_set(self, variant):
        """cabac_hip_piece_encoder.h: the encoder of encode_pieces_device and of plan_continue_write_device's encode leg —
        4 (the default), 7 or 0 = by the batch.  Any other value raises CabacHipError (status ERR_INVALID); the setting stays."""
        self._check(self.L.cabac_hip_piece_encoder_set(self.h, variant))

    def piece_encoder_get(self):
        return int(self.L.cabac_hip_piece_encoder_get(self.h))

    def synchronize(self):
        self._check(self.L.cabac_hip_synchronize(self.h))

    # ---- the fixed workspace (cabac_hip_workspace.h) ----
    workspace_bound = staticmethod(workspace_bound)

    def workspace_fix(self, n_sub, n_tu, expanded_records, slot_bytes, n_entries=0, log_records=0, rows=False):
        """Fix the workspace: the nine calls of cabac_hip_workspace.h then queue their work and return.  May block and allocate."""
        z = np.zeros(1, WORKSPACE_SIZES_DTYPE)
        z["n_sub"], z["n_tu"], z["n_entries"], z["expanded_records"] = n_sub, n_tu, n_entries, expanded_records
        z["slot_bytes"], z["log_records"], z["flags"] = slot_bytes, log_records, WS_ROWS if rows else 0
        self._check(self.L.cabac_hip_workspace_fix(self.h, vp(z.ctypes.data)))

    def workspace_release(self):
        self._check(self.L.cabac_hip_workspace_release(self.h))

    def workspace_status(self):
        """The status (one WORKSPACE_STATUS_DTYPE record) once the ctx's stream has drained."""
        st = np.zeros(1, WORKSPACE_STATUS_DTYPE)
        self._check(self.L.cabac_hip_workspace_status(self.h, vp(st.ctypes.data)))
        return st[0]

    def workspace_status_device(self, d_out):
        """Queue a copy of the status into d_out (device memory or pinned host memory): stream-ordered, no wait."""
        self._check(self.L.cabac_hip_workspace_status_device(self.h, vp(d_out)))

    def workspace_waits(self):
        """Blocking runtime calls the library has issued for this ctx so far (never decreases)."""
        n = ctypes.c_uint64(0)
        self._check(self.L.cabac_hip_workspace_waits(self.h, ctypes.byref(n)))
        return n.value

    def wait_event(self, hip_event):
        """The ctx's stream waits for `hip_event` (a hipEvent_t, e.g. torch.cuda.Event(...).cuda_event after record())."""
        self._check(self.L.cabac_hip_wait_event(self.h, vp(hip_event)))

    def record_event(self, hip_event):
        self._check(self.L.cabac_hip_record_event(self.h, vp(hip_event)))

    def last_kernel_ms(self):
        return float(self.L.cabac_hip_last_kernel_ms(self.h))

    def profile_enable(self, capacity):
        self._check(self.L.cabac_hip_profile_enable(self.h, capacity))
        self._prof_cap = capacity

    def profile_read(self):
        """[(kind, ms)] of the device calls since the last read; kind 0 encode, 1 decode, 2 binarize, ..., 12 residual estimate
        (the list is at cabac_hip_profile_read in include/cabac_hip.h; 12 in cabac_hip_estimate.h; 13 nal escape and 14 nal unescape in
        cabac_hip_nal.h; 15 residual estimate with contexts, 16 search select, 17 / 18 a round's estimate / commit in
        cabac_hip_search.h; 19 unit estimate, 20 / 21 / 22 a unit round's estimate / select / commit in cabac_hip_search_unit.h; 23 log append and
        24 log place in cabac_hip_search_emit.h; 25 unit parse in cabac_hip_parse_unit.h; 26 element parse in
        cabac_hip_parse_elements.h; 27 plan parse in cabac_hip_parse_plan.h; 28 plan write in cabac_hip_write_plan.h; 29 plan resolve in
        cabac_hip_search_plan.h; 30 encode with sets, 31 decode with sets, 32 context advance and 33 a WPP prefix pass in
        cabac_hip_ctx_sets.h; 34 plan parse with sets, 35 a level of a rows parse and 36 the encode launch of a plan write with sets
        in cabac_hip_plan_rows.h; 37 hand-over index, 38 log mark and 39 the encode launch of a spliced call with sets in
        cabac_hip_splice_rows.h; 40 the gate of a call on a fixed workspace in cabac_hip_workspace.h; 41 coefficient expand and
        42 coefficient compact in cabac_hip_sparse.h; 43 record unpack and 44 record pack in cabac_hip_rec10.h)."""
        cap = getattr(self, "_prof_cap", 0)
        kind = np.zeros(max(cap, 1), np.int32)
        ms = np.zeros(max(cap, 1), np.float32)
        n = self.L.cabac_hip_profile_read(self.h, kind.ctypes.data, ms.ctypes.data, cap)
        if n < 0:
            self._check(n)
        return list(zip(kind[:n].tolist(), ms[:n].tolist()))

    # ---- host-pointer entry points (numpy) --------------------------------------------------
    def encode_batch(self, desc, records, bytes_total, check=True, out=None):
        """`out` (optional): the caller's byte buffer (e.g. PinnedArray(...).array), else a fresh zeroed array."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        if out is None:
            out = np.zeros(max(int(bytes_total), 1), np.uint8)
        res = np.zeros(len(desc), RESULT_DTYPE)
        rc = self.L.cabac_hip_encode_batch(self.h, len(desc), desc.ctypes.data, records.ctypes.data, len(records),
                                           out.ctypes.data, int(bytes_total), res.ctypes.data)
        self._check(rc, allow_substream=not check)
        return out, res

    def encode_batch_payload(self, desc, records, payload, check=True):
        """cabac_hip_encode_batch_payload: the coded substreams back to back in `payload` (uint8 array, e.g. pinned);
        returns (offsets uint64[n + 1], results)."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        offsets = np.zeros(len(desc) + 1, np.uint64)
        res = np.zeros(len(desc), RESULT_DTYPE)
        rc = self.L.cabac_hip_encode_batch_payload(self.h, len(desc), desc.ctypes.data, records.ctypes.data, len(records),
                                                   payload.ctypes.data, payload.nbytes, offsets.ctypes.data, res.ctypes.data)
        self._check(rc, allow_substream=not check)
        return offsets, res

    def decode_batch(self, desc, records, data, check=True, bins=None):
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        data = np.ascontiguousarray(data, np.uint8)
        if bins is None:
            bins = np.zeros(max(len(records), 1), np.uint8)
        res = np.zeros(len(desc), RESULT_DTYPE)
        rc = self.L.cabac_hip_decode_batch(self.h, len(desc), desc.ctypes.data, records.ctypes.data, len(records),
                                           data.ctypes.data, len(data), bins.ctypes.data, res.ctypes.data)
        self._check(rc, allow_substream=not check)
        return bins[: len(records)], res

    def decode_batch_packed(self, desc, records, data, check=True, packed=None):
        """cabac_hip_decode_batch_packed: (packed uint8[(n + 7) // 8] — bit r & 7 of byte r >> 3 = the bin of record r —, results)."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        data = np.ascontiguousarray(data, np.uint8)
        if packed is None:
            packed = np.zeros((len(records) + 7) // 8 + 1, np.uint8)
        res = np.zeros(len(desc), RESULT_DTYPE)
        rc = self.L.cabac_hip_decode_batch_packed(self.h, len(desc), desc.ctypes.data, records.ctypes.data, len(records),
                                                  data.ctypes.data, len(data), packed.ctypes.data, res.ctypes.data)
        self._check(rc, allow_substream=not check)
        return packed[: (len(records) + 7) // 8], res

    # ---- device-pointer entry points (raw addresses, e.g. torch tensor .data_ptr()) ----------
    def encode_device(self, n_sub, d_desc, d_records, d_bytes, d_results):
        self._check(self.L.cabac_hip_encode_device(self.h, n_sub, vp(d_desc), vp(d_records), vp(d_bytes), vp(d_results)))

    def decode_device(self, n_sub, d_desc, d_records, d_bytes, d_bins, d_results):
        self._check(self.L.cabac_hip_decode_device(self.h, n_sub, vp(d_desc), vp(d_records), vp(d_bytes), vp(d_bins),
                                                   vp(d_results)))

    # ---- include/cabac_hip_ctx_sets.h: context sets in and out, WPP ------------------------------
    @staticmethod
    def _sets7(n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate):
        return [int(n_sets)] + [vp(p) if p else None for p in (d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate)]

    def encode_sets_device(self, n_sub, d_desc, d_records, d_bytes, d_results, n_sets=0, d_state=0, d_rate=0, d_start_set=0,
                           d_out_set=0, d_out_state=0, d_out_rate=0):
        """encode_device with substream s started from set d_start_set[s] (CTX_NO_SET: Ctx::init) and its final contexts written
        as set d_out_set[s]; 0 for a pointer = NULL."""
        self._check(self.L.cabac_hip_encode_sets_device(self.h, n_sub, vp(d_desc), vp(d_records), vp(d_bytes), vp(d_results),
                                                        *self._sets7(n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state,
                                                                     d_out_rate)))

    def decode_sets_device(self, n_sub, d_desc, d_records, d_bytes, d_bins, d_results, n_sets=0, d_state=0, d_rate=0, d_start_set=0,
                           d_out_set=0, d_out_state=0, d_out_rate=0):
        self._check(self.L.cabac_hip_decode_sets_device(self.h, n_sub, vp(d_desc), vp(d_records), vp(d_bytes), vp(d_bins),
                                                        vp(d_results), *self._sets7(n_sets, d_state, d_rate, d_start_set, d_out_set,
                                                                                    d_out_state, d_out_rate)))

    def encode_pieces_device(self, n_sub, d_desc, d_records, d_bytes, d_results, n_sets=0, d_state=0, d_rate=0, d_start_set=0,
                             d_out_set=0, d_out_state=0, d_out_rate=0, d_coder_in=0, d_coder_out=0):
        """One piece of every substream (include/cabac_hip_pieces.h): encode_sets_device continued from the coder states
        d_coder_in (CODER_STATE_DTYPE per substream; 0: all fresh) and leaving them in d_coder_out (0: not written; may be
        d_coder_in).  A descriptor without SUB_FINISH flushes nothing."""
        self._check(self.L.cabac_hip_encode_pieces_device(self.h, n_sub, vp(d_desc), vp(d_records), vp(d_bytes), vp(d_results),
                                                          *self._sets7(n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state,
                                                                       d_out_rate),
                                                          vp(d_coder_in) if d_coder_in else None,
                                                          vp(d_coder_out) if d_coder_out else None))

    def decode_pieces_device(self, n_sub, d_desc, d_records, d_bytes, d_bins, d_results, n_sets=0, d_state=0, d_rate=0, d_start_set=0,
                             d_out_set=0, d_out_state=0, d_out_rate=0, d_coder_in=0, d_coder_out=0):
        """decode_sets_device in pieces: the bins of this piece's records from the decoder states d_coder_in."""
        self._check(self.L.cabac_hip_decode_pieces_device(self.h, n_sub, vp(d_desc), vp(d_records), vp(d_bytes), vp(d_bins),
                                                          vp(d_results), *self._sets7(n_sets, d_state, d_rate, d_start_set, d_out_set,
                                                                                      d_out_state, d_out_rate),
                                                          vp(d_coder_in) if d_coder_in else None,
                                                          vp(d_coder_out) if d_coder_out else None))

    def ctx_advance_device(self, n_sub, d_desc, d_records, n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate,
                           d_flags=0):
        """update() for every context-coded record of the runs: sets in, sets out, nothing coded."""
        self._check(self.L.cabac_hip_ctx_advance_device(self.h, n_sub, vp(d_desc), vp(d_records),
                                                        *self._sets7(n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state,
                                                                     d_out_rate), vp(d_flags) if d_flags else None))

    def encode_wpp_device(self, n_sub, d_desc, d_records, d_bytes, d_results, level_first, d_sync_from, d_sync_at):
        """level_first: HOST, n_level + 1 entries."""
        lf = np.ascontiguousarray(level_first, np.uint32)
        self._check(self.L.cabac_hip_encode_wpp_device(self.h, n_sub, vp(d_desc), vp(d_records), vp(d_bytes), vp(d_results),
                                                       len(lf) - 1, lf.ctypes.data, vp(d_sync_from), vp(d_sync_at)))

    def decode_wpp_device(self, n_sub, d_desc, d_records, d_bytes, d_bins, d_results, level_first, d_sync_from, d_sync_at):
        lf = np.ascontiguousarray(level_first, np.uint32)
        self._check(self.L.cabac_hip_decode_wpp_device(self.h, n_sub, vp(d_desc), vp(d_records), vp(d_bytes), vp(d_bins),
                                                       vp(d_results), len(lf) - 1, lf.ctypes.data, vp(d_sync_from), vp(d_sync_at)))

    def encode_wpp_batch(self, desc, records, bytes_total, level_first, sync_from, sync_at, check=True):
        """Host arrays through cabac_hip_encode_wpp_batch: (bytes uint8[bytes_total], results)."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        lf = np.ascontiguousarray(level_first, np.uint32)
        sf, sa = np.ascontiguousarray(sync_from, np.uint32), np.ascontiguousarray(sync_at, np.uint32)
        out = np.zeros(max(int(bytes_total), 1), np.uint8)
        res = np.zeros(len(desc), RESULT_DTYPE)
        rc = self.L.cabac_hip_encode_wpp_batch(self.h, len(desc), desc.ctypes.data, records.ctypes.data, len(records), out.ctypes.data,
                                               int(bytes_total), res.ctypes.data, len(lf) - 1, lf.ctypes.data, sf.ctypes.data,
                                               sa.ctypes.data)
        self._check(rc, allow_substream=not check)
        return out, res

    def decode_wpp_batch(self, desc, records, data, level_first, sync_from, sync_at, check=True):
        """Host arrays through cabac_hip_decode_wpp_batch: (bins uint8[len(records)], results)."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        data = np.ascontiguousarray(data, np.uint8)
        lf = np.ascontiguousarray(level_first, np.uint32)
        sf, sa = np.ascontiguousarray(sync_from, np.uint32), np.ascontiguousarray(sync_at, np.uint32)
        bins = np.zeros(max(len(records), 1), np.uint8)
        res = np.zeros(len(desc), RESULT_DTYPE)
        rc = self.L.cabac_hip_decode_wpp_batch(self.h, len(desc), desc.ctypes.data, records.ctypes.data, len(records), data.ctypes.data,
                                               len(data), bins.ctypes.data, res.ctypes.data, len(lf) - 1, lf.ctypes.data,
                                               sf.ctypes.data, sa.ctypes.data)
        self._check(rc, allow_substream=not check)
        return bins[: len(records)], res

    def estimate_device(self, n_sub, d_desc, d_records, d_frac_bits, d_flags=0):
        """BitEstimator_Std over a batch of bin strings: d_frac_bits[s] (uint64) = cost in 1/32768 bit."""
        self._check(self.L.cabac_hip_estimate_device(self.h, n_sub, vp(d_desc), vp(d_records), vp(d_frac_bits),
                                                     vp(d_flags) if d_flags else None))

    def estimate_from_device(self, n_sub, d_desc, d_records, d_state, d_rate, d_set, d_frac_bits, d_flags=0):
        """estimate_device started from given context sets (format of ctx_init_device) instead of reset(qp, initId)."""
        self._check(self.L.cabac_hip_estimate_from_device(self.h, n_sub, vp(d_desc), vp(d_records), vp(d_state), vp(d_rate),
                                                          vp(d_set), vp(d_frac_bits), vp(d_flags) if d_flags else None))

    def estimate_batch(self, desc, records, check=False):
        """Host arrays through cabac_hip_estimate_batch: (frac_bits uint64[n], flags uint32[n])."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        bits = np.zeros(max(len(desc), 1), np.uint64)
        flags = np.zeros(max(len(desc), 1), np.uint32)
        rc = self.L.cabac_hip_estimate_batch(self.h, len(desc), desc.ctypes.data, records.ctypes.data, len(records),
                                             bits.ctypes.data, flags.ctypes.data)
        self._check(rc, allow_substream=not check)
        return bits[: len(desc)], flags[: len(desc)]

    def estimate_residual_device(self, n_cand, d_cand_first, d_tu, d_coeff, d_state, d_rate, d_set, d_frac_bits, d_tu_frac_bits=0,
                                 d_tu_info=0, int16=False):
        """cabac_hip_estimate_residual_device (int16: cabac_hip_estimate_residual16_device): coefficient blocks -> fractional
        bits.  Candidate c = blocks d_cand_first[c] .. d_cand_first[c + 1] - 1 costed in order from context set d_set[c];
        d_frac_bits[c] (uint64) = cost in 1/32768 bit, d_tu_frac_bits / d_tu_info (optional) per block."""
        self._check((self.L.cabac_hip_estimate_residual16_device if int16 else self.L.cabac_hip_estimate_residual_device)(
            self.h, n_cand, vp(d_cand_first), vp(d_tu), vp(d_coeff), vp(d_state), vp(d_rate), vp(d_set), vp(d_frac_bits),
            vp(d_tu_frac_bits) if d_tu_frac_bits else None, vp(d_tu_info) if d_tu_info else None))

    def estimate_residual_batch(self, cand_first, tus, coeff, state, rate, sets, int16=False, with_blocks=False, check=True):
        """Host arrays through cabac_hip_estimate_residual_batch (synchronous).  state / rate: (n_sets, 379) context sets in
        the format of ctx_init_device; sets[c]: the set candidate c starts from.  Returns frac_bits uint64[n_cand], with
        with_blocks also (tu_frac_bits uint64[n_tu], tu_info uint32[n_tu]).  check=False: an empty block or a bad
        descriptor does not raise (tu_info says which)."""
        cand_first = np.ascontiguousarray(cand_first, np.uint32)
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        coeff = np.ascontiguousarray(coeff, np.int16 if int16 else np.int32)
        state = np.ascontiguousarray(state, np.uint32).reshape(-1)
        rate = np.ascontiguousarray(rate, np.uint8).reshape(-1)
        sets = np.ascontiguousarray(sets, np.uint32)
        n_cand = len(cand_first) - 1
        assert n_cand >= 0 and len(sets) == n_cand and len(state) == len(rate) and len(state) % NUM_CTX == 0
        bits = np.zeros(max(n_cand, 1), np.uint64)
        tu_bits = np.zeros(max(len(tus), 1), np.uint64)
        info = np.zeros(max(len(tus), 1), np.uint32)
        rc = self.L.cabac_hip_estimate_residual_batch(self.h, n_cand, cand_first.ctypes.data, tus.ctypes.data, coeff.ctypes.data,
                                                      2 if int16 else 4, len(coeff), state.ctypes.data, rate.ctypes.data,
                                                      len(state) // NUM_CTX, sets.ctypes.data, bits.ctypes.data,
                                                      tu_bits.ctypes.data if with_blocks else None,
                                                      info.ctypes.data if with_blocks else None)
        self._check(rc, allow_substream=not check)
        if with_blocks:
            return bits[:n_cand], tu_bits[: len(tus)], info[: len(tus)]
        return bits[:n_cand]

    # ---- search rounds (include/cabac_hip_search.h) --------------------------------------------
    def estimate_residual_ctx_device(self, n_cand, d_cand_first, d_tu, d_coeff, d_state, d_rate, d_set, d_frac_bits, d_out_set,
                                     d_out_state, d_out_rate, d_tu_frac_bits=0, d_tu_info=0, int16=False):
        """cabac_hip_estimate_residual_ctx_device (int16: _ctx16_device): estimate_residual_device, and candidate c with
        d_out_set[c] != SEARCH_NO_SET writes the complete context set it leaves as set d_out_set[c] of d_out_state / d_out_rate
        (which may be d_state / d_rate under the in-place rule of the header)."""
        self._check((self.L.cabac_hip_estimate_residual_ctx16_device if int16 else self.L.cabac_hip_estimate_residual_ctx_device)(
            self.h, n_cand, vp(d_cand_first), vp(d_tu), vp(d_coeff), vp(d_state), vp(d_rate), vp(d_set), vp(d_frac_bits),
            vp(d_tu_frac_bits) if d_tu_frac_bits else None, vp(d_tu_info) if d_tu_info else None, vp(d_out_set), vp(d_out_state),
            vp(d_out_rate)))

    def search_select_device(self, n_group, d_group_first, d_frac_bits, d_dist, lambda_q16, d_pick, d_cost):
        """cabac_hip_search_select_device: per group the candidate with the smallest d_dist + ((lambda_q16 * d_frac_bits) >> 31)
        (d_dist = 0: no distortions) into d_pick (uint32, SEARCH_NONE for a group with nothing to pick) and d_cost (uint64)."""
        self._check(self.L.cabac_hip_search_select_device(self.h, n_group, vp(d_group_first), vp(d_frac_bits),
                                                          vp(d_dist) if d_dist else None, lambda_q16, vp(d_pick), vp(d_cost)))

    def search_round_device(self, n_group, d_group_first, n_cand, d_cand_first, d_tu, d_coeff, d_state, d_rate, d_set,
                            d_group_out_set, d_dist, lambda_q16, d_frac_bits, d_pick, d_cost, d_tu_frac_bits=0, d_tu_info=0,
                            int16=False):
        """cabac_hip_search_round_device: estimate, select, commit — the set the picked candidate of group g leaves is written
        as set d_group_out_set[g] of d_state / d_rate."""
        self._check(self.L.cabac_hip_search_round_device(
            self.h, n_group, vp(d_group_first), n_cand, vp(d_cand_first), vp(d_tu), vp(d_coeff), 2 if int16 else 4, vp(d_state),
            vp(d_rate), vp(d_set), vp(d_group_out_set) if d_group_out_set else None, vp(d_dist) if d_dist else None, lambda_q16,
            vp(d_frac_bits), vp(d_pick), vp(d_cost), vp(d_tu_frac_bits) if d_tu_frac_bits else None,
            vp(d_tu_info) if d_tu_info else None))

    def search_round_batch(self, group_first, cand_first, tus, coeff, state, rate, sets, group_out_set, dist, lambda_q16,
                           int16=False, with_blocks=False, check=True):
        """Host arrays through cabac_hip_search_round_batch (synchronous).  state / rate: (n_sets, 379) context sets, updated IN
        PLACE (they must be contiguous uint32 / uint8 arrays); group_out_set / dist may be None.  Returns (frac_bits uint64[n_cand],
        pick uint32[n_group], cost uint64[n_group]), with with_blocks also (tu_frac_bits, tu_info)."""
        group_first = np.ascontiguousarray(group_first, np.uint32)
        cand_first = np.ascontiguousarray(cand_first, np.uint32)
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        coeff = np.ascontiguousarray(coeff, np.int16 if int16 else np.int32)
        sets = np.ascontiguousarray(sets, np.uint32)
        assert state.dtype == np.uint32 and rate.dtype == np.uint8 and state.flags.c_contiguous and rate.flags.c_contiguous
        assert state.size == rate.size and state.size % NUM_CTX == 0
        n_group, n_cand = len(group_first) - 1, len(cand_first) - 1
        assert n_group >= 0 and n_cand >= 0 and len(sets) == n_cand
        out_set = None if group_out_set is None else np.ascontiguousarray(group_out_set, np.uint32)
        dist = None if dist is None else np.ascontiguousarray(dist, np.uint64)
        assert (out_set is None or len(out_set) == n_group) and (dist is None or len(dist) == n_cand)
        bits = np.zeros(max(n_cand, 1), np.uint64)
        pick = np.zeros(max(n_group, 1), np.uint32)
        cost = np.zeros(max(n_group, 1), np.uint64)
        tu_bits = np.zeros(max(len(tus), 1), np.uint64)
        info = np.zeros(max(len(tus), 1), np.uint32)
        rc = self.L.cabac_hip_search_round_batch(
            self.h, n_group, group_first.ctypes.data, n_cand, cand_first.ctypes.data, tus.ctypes.data, coeff.ctypes.data,
            2 if int16 else 4, len(coeff), state.ctypes.data, rate.ctypes.data, state.size // NUM_CTX, sets.ctypes.data,
            out_set.ctypes.data if out_set is not None else None, dist.ctypes.data if dist is not None else None, lambda_q16,
            bits.ctypes.data, pick.ctypes.data, cost.ctypes.data, tu_bits.ctypes.data if with_blocks else None,
            info.ctypes.data if with_blocks else None)
        self._check(rc, allow_substream=not check)
        out = (bits[:n_cand], pick[:n_group], cost[:n_group])
        if with_blocks:
            out += (tu_bits[: len(tus)], info[: len(tus)])
        return out

    # ---- search rounds over candidates with side records (include/cabac_hip_search_unit.h) ------
    def estimate_unit_device(self, n_cand, d_cand_first, d_tu, d_coeff, d_state, d_rate, d_set, d_rec_first, d_records, d_tu_at,
                             d_frac_bits, d_tu_frac_bits=0, d_tu_info=0, d_flags=0, d_out_set=0, d_out_state=0, d_out_rate=0,
                             int16=False):
        """cabac_hip_estimate_unit_device: candidate c = side records d_records[d_rec_first[c] .. d_rec_first[c + 1]) (d_rec_first
        uint64) with its blocks spliced in front of index d_tu_at[t] of that run (d_tu_at = 0: behind the run), costed in one walk;
        d_flags[c] = RES_BAD_RECORD for a side record that is none; d_out_set = 0 writes no set, else as
        estimate_residual_ctx_device with all 379 entries taken from the walk."""
        self._check(self.L.cabac_hip_estimate_unit_device(
            self.h, n_cand, vp(d_cand_first), vp(d_tu), vp(d_coeff), 2 if int16 else 4, vp(d_state), vp(d_rate), vp(d_set),
            vp(d_rec_first), _opt(d_records), _opt(d_tu_at), vp(d_frac_bits), _opt(d_tu_frac_bits), _opt(d_tu_info), _opt(d_flags),
            _opt(d_out_set), _opt(d_out_state), _opt(d_out_rate)))

    def search_unit_round_device(self, n_group, d_group_first, n_cand, d_cand_first, d_tu, d_coeff, d_state, d_rate, d_set,
                                 d_rec_first, d_records, d_tu_at, d_group_out_set, d_dist, lambda_q16, d_frac_bits, d_pick, d_cost,
                                 d_tu_frac_bits=0, d_tu_info=0, d_flags=0, int16=False):
        """cabac_hip_search_unit_round_device: search_round_device over candidates with side records (see estimate_unit_device)."""
        self._check(self.L.cabac_hip_search_unit_round_device(
            self.h, n_group, vp(d_group_first), n_cand, vp(d_cand_first), vp(d_tu), vp(d_coeff), 2 if int16 else 4, vp(d_state),
            vp(d_rate), vp(d_set), vp(d_rec_first), _opt(d_records), _opt(d_tu_at), _opt(d_group_out_set), _opt(d_dist), lambda_q16,
            vp(d_frac_bits), vp(d_pick), vp(d_cost), _opt(d_tu_frac_bits), _opt(d_tu_info), _opt(d_flags)))

    def search_unit_round_batch(self, group_first, cand_first, tus, coeff, state, rate, sets, records, rec_first, tu_at, group_out_set,
                                dist, lambda_q16, int16=False, with_blocks=False, check=True):
        """Host arrays through cabac_hip_search_unit_round_batch (synchronous): search_round_batch with the side records
        `records` (uint16), `rec_first` (uint64[n_cand + 1]) and `tu_at` (uint32 per block, or None).  state / rate are updated IN
        PLACE.  Returns (frac_bits, pick, cost), with with_blocks also (tu_frac_bits, tu_info)."""
        group_first = np.ascontiguousarray(group_first, np.uint32)
        cand_first = np.ascontiguousarray(cand_first, np.uint32)
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        coeff = np.ascontiguousarray(coeff, np.int16 if int16 else np.int32)
        sets = np.ascontiguousarray(sets, np.uint32)
        records = np.ascontiguousarray(records, np.uint16)
        rec_first = np.ascontiguousarray(rec_first, np.uint64)
        tu_at = None if tu_at is None else np.ascontiguousarray(tu_at, np.uint32)
        assert state.dtype == np.uint32 and rate.dtype == np.uint8 and state.flags.c_contiguous and rate.flags.c_contiguous
        assert state.size == rate.size and state.size % NUM_CTX == 0
        n_group, n_cand = len(group_first) - 1, len(cand_first) - 1
        assert n_group >= 0 and n_cand >= 0 and len(sets) == n_cand and len(rec_first) == n_cand + 1
        assert tu_at is None or len(tu_at) == len(tus)
        out_set = None if group_out_set is None else np.ascontiguousarray(group_out_set, np.uint32)
        dist = None if dist is None else np.ascontiguousarray(dist, np.uint64)
        assert (out_set is None or len(out_set) == n_group) and (dist is None or len(dist) == n_cand)
        bits = np.zeros(max(n_cand, 1), np.uint64)
        pick = np.zeros(max(n_group, 1), np.uint32)
        cost = np.zeros(max(n_group, 1), np.uint64)
        tu_bits = np.zeros(max(len(tus), 1), np.uint64)
        info = np.zeros(max(len(tus), 1), np.uint32)
        rc = self.L.cabac_hip_search_unit_round_batch(
            self.h, n_group, group_first.ctypes.data, n_cand, cand_first.ctypes.data, tus.ctypes.data, coeff.ctypes.data,
            2 if int16 else 4, len(coeff), state.ctypes.data, rate.ctypes.data, state.size // NUM_CTX, sets.ctypes.data,
            records.ctypes.data, len(records), rec_first.ctypes.data, tu_at.ctypes.data if tu_at is not None else None,
            out_set.ctypes.data if out_set is not None else None, dist.ctypes.data if dist is not None else None, lambda_q16,
            bits.ctypes.data, pick.ctypes.data, cost.ctypes.data, tu_bits.ctypes.data if with_blocks else None,
            info.ctypes.data if with_blocks else None)
        self._check(rc, allow_substream=not check)
        out = (bits[:n_cand], pick[:n_group], cost[:n_group])
        if with_blocks:
            out += (tu_bits[: len(tus)], info[: len(tus)])
        return out

    # ---- search rounds over plans (include/cabac_hip_search_plan.h) ------
    def resolve_plan_device(self, n_cand, d_cand_first, d_ent_first, d_plan, d_values_in, n_tu, d_tu, d_tu_at, d_tu_guard, d_coeff,
                            d_rec_first, d_records, record_capacity, d_tu_at_out, d_tu_out, d_flags, d_values_out=0, d_tu_info=0,
                            d_total=0, int16=False):
        """cabac_hip_resolve_plan_device: candidate c = the plan entries d_plan[2 * d_ent_first[c] ..) (d_ent_first uint64) with the
        values d_values_in and its blocks -> the candidate format of estimate_unit_device / search_unit_round_device /
        SearchLog.append_device: d_rec_first, d_records (record_capacity records), d_tu_at_out, d_tu_out; d_flags[c] = 0,
        RES_BAD_RECORD, RES_BAD_VALUE or RES_OVERFLOW (the call did not fit: d_total says what it needs)."""
        self._check(self.L.cabac_hip_resolve_plan_device(
            self.h, n_cand, vp(d_cand_first), vp(d_ent_first), _opt(d_plan), _opt(d_values_in), n_tu, _opt(d_tu), _opt(d_tu_at),
            _opt(d_tu_guard), _opt(d_coeff), 2 if int16 else 4, vp(d_rec_first), _opt(d_records), record_capacity, _opt(d_tu_at_out),
            _opt(d_tu_out), _opt(d_values_out), _opt(d_tu_info), vp(d_flags), _opt(d_total)))

    def search_plan_round_device(self, n_group, d_group_first, n_cand, d_cand_first, n_tu, d_tu, d_coeff, d_state, d_rate, d_set,
                                 d_ent_first, d_plan, d_values_in, d_tu_at, d_tu_guard, d_group_out_set, d_dist, lambda_q16, d_frac_bits,
                                 d_pick, d_cost, d_rec_first, d_records, record_capacity, d_tu_at_out, d_tu_out, d_tu_frac_bits=0,
                                 d_tu_info=0, d_flags=0, d_values_out=0, d_total=0, int16=False):
        """cabac_hip_search_plan_round_device: search_unit_round_device over candidates given as plans (see resolve_plan_device);
        the resolved form is left in d_rec_first / d_records / d_tu_at_out / d_tu_out for SearchLog.append_device."""
        self._check(self.L.cabac_hip_search_plan_round_device(
            self.h, n_group, vp(d_group_first), n_cand, vp(d_cand_first), n_tu, _opt(d_tu), _opt(d_coeff), 2 if int16 else 4, vp(d_state),
            vp(d_rate), vp(d_set), vp(d_ent_first), _opt(d_plan), _opt(d_values_in), _opt(d_tu_at), _opt(d_tu_guard), _opt(d_group_out_set),
            _opt(d_dist), lambda_q16, vp(d_frac_bits), vp(d_pick), vp(d_cost), _opt(d_tu_frac_bits), _opt(d_tu_info), _opt(d_flags),
            vp(d_rec_first), _opt(d_records), record_capacity, _opt(d_tu_at_out), _opt(d_tu_out), _opt(d_values_out), _opt(d_total)))

    def search_plan_round_batch(self, group_first, cand_first, tus, coeff, state, rate, sets, plan, values, ent_first, tu_at, tu_guard,
                                group_out_set, dist, lambda_q16, int16=False, with_blocks=False, check=True):
        """Host arrays through cabac_hip_search_plan_round_batch (synchronous): search_unit_round_batch with the plans `plan`
        (uint32 (n_entries, 2)), `values` (uint32 per entry), `ent_first` (uint64[n_cand + 1]), `tu_at` (in plan entries) and
        `tu_guard` (uint32 per block, or None) in place of the side records.  state / rate are updated IN PLACE.  Returns
        (frac_bits, pick, cost, flags, filled values), with with_blocks also (tu_frac_bits, tu_info)."""
        group_first = np.ascontiguousarray(group_first, np.uint32)
        cand_first = np.ascontiguousarray(cand_first, np.uint32)
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        coeff = np.ascontiguousarray(coeff, np.int16 if int16 else np.int32)
        sets = np.ascontiguousarray(sets, np.uint32)
        plan = np.ascontiguousarray(plan, np.uint32).reshape(-1, 2)
        values = np.ascontiguousarray(values, np.uint32)
        ent_first = np.ascontiguousarray(ent_first, np.uint64)
        tu_at = None if tu_at is None else np.ascontiguousarray(tu_at, np.uint32)
        tu_guard = None if tu_guard is None else np.ascontiguousarray(tu_guard, np.uint32)
        assert state.dtype == np.uint32 and rate.dtype == np.uint8 and state.flags.c_contiguous and rate.flags.c_contiguous
        assert state.size == rate.size and state.size % NUM_CTX == 0
        n_group, n_cand = len(group_first) - 1, len(cand_first) - 1
        assert n_group >= 0 and n_cand >= 0 and len(sets) == n_cand and len(ent_first) == n_cand + 1 and len(values) >= len(plan)
        assert (tu_at is None or len(tu_at) == len(tus)) and (tu_guard is None or len(tu_guard) == len(tus))
        out_set = None if group_out_set is None else np.ascontiguousarray(group_out_set, np.uint32)
        dist = None if dist is None else np.ascontiguousarray(dist, np.uint64)
        assert (out_set is None or len(out_set) == n_group) and (dist is None or len(dist) == n_cand)
        bits = np.zeros(max(n_cand, 1), np.uint64)
        pick = np.zeros(max(n_group, 1), np.uint32)
        cost = np.zeros(max(n_group, 1), np.uint64)
        flags = np.zeros(max(n_cand, 1), np.uint32)
        filled = np.zeros(max(len(plan), 1), np.uint32)
        tu_bits = np.zeros(max(len(tus), 1), np.uint64)
        info = np.zeros(max(len(tus), 1), np.uint32)
        ptr = lambda a: a.ctypes.data if a is not None else None
        rc = self.L.cabac_hip_search_plan_round_batch(
            self.h, n_group, group_first.ctypes.data, n_cand, cand_first.ctypes.data, tus.ctypes.data, coeff.ctypes.data,
            2 if int16 else 4, len(coeff), state.ctypes.data, rate.ctypes.data, state.size // NUM_CTX, sets.ctypes.data,
            plan.ctypes.data, values.ctypes.data, len(plan), ent_first.ctypes.data, ptr(tu_at), ptr(tu_guard), ptr(out_set), ptr(dist),
            lambda_q16, bits.ctypes.data, pick.ctypes.data, cost.ctypes.data, tu_bits.ctypes.data if with_blocks else None,
            info.ctypes.data if with_blocks else None, flags.ctypes.data, filled.ctypes.data)
        self._check(rc, allow_substream=not check)
        out = (bits[:n_cand], pick[:n_group], cost[:n_group], flags[:n_cand], filled[: len(plan)])
        if with_blocks:
            out += (tu_bits[: len(tus)], info[: len(tus)])
        return out

    # ---- the winner log (include/cabac_hip_search_emit.h) ------
    def search_log(self, n_chain, entry_capacity, record_capacity, tu_capacity, coeff_capacity, int16=False):
        """cabac_hip_search_log_create: a SearchLog of this ctx (closed with it at the latest)."""
        return SearchLog(self, n_chain, entry_capacity, record_capacity, tu_capacity, coeff_capacity, int16)

    def binarize_device(self, n_sub, d_se_offset, d_se, d_rec_offset, d_n_records, d_records):
        self._check(self.L.cabac_hip_binarize_device(self.h, n_sub, vp(d_se_offset), vp(d_se), vp(d_rec_offset),
                                                     vp(d_n_records), vp(d_records)))

    def residual_device(self, n_tu, d_tu, d_coeff, d_rec_offset, d_n_records, d_info, d_records):
        """cabac_hip_residual_device: coefficient blocks -> bin records (pass 1 when d_records == 0)."""
        self._check(self.L.cabac_hip_residual_device(self.h, n_tu, vp(d_tu), vp(d_coeff), vp(d_rec_offset),
                                                     vp(d_n_records), vp(d_info), vp(d_records)))

    def residual_parse_device(self, n_sub, d_desc, d_bytes, d_tile_first, d_tu, d_coeff, d_results, d_tu_info=0, int16=False):
        """cabac_hip_residual_parse_device (int16: cabac_hip_residual_parse16_device): bytes -> coefficient blocks, contexts
        derived on the device."""
        self._check((self.L.cabac_hip_residual_parse16_device if int16 else self.L.cabac_hip_residual_parse_device)(self.h, n_sub, vp(d_desc), vp(d_bytes), vp(d_tile_first), vp(d_tu),
                                                           vp(d_coeff), vp(d_tu_info) if d_tu_info else None, vp(d_results)))

    # ---- what the host-pointer forms of the parser family share ------
    @staticmethod
    def _parse_inputs(desc, data, tile_first, tus, n_coeff_total, int16, coeff):
        """The arrays every parser batch form takes, normalised; `coeff` (the caller's, else zeros); fresh results."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        data = np.ascontiguousarray(data, np.uint8)
        tile_first = np.ascontiguousarray(tile_first, np.uint32)
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        if coeff is None:
            coeff = np.zeros(max(int(n_coeff_total), 1), np.int16 if int16 else np.int32)
        return desc, data, tile_first, tus, coeff, np.zeros(max(len(desc), 1), RESULT_DTYPE)

    @staticmethod
    def _per_block(a, tus):
        """tu_at or tu_guard: None, or uint32 with one entry per block."""
        if a is not None:
            a = np.ascontiguousarray(a, np.uint32)
            assert len(a) == len(tus)
        return a

    @staticmethod
    def _rows(level_first, sync_from, sync_at, n):
        """The trailing arguments of a rows batch form as arrays (kept alive by the caller): level_first, and one link and one
        hand-over position per substream."""
        lf = np.ascontiguousarray(level_first, np.uint32)
        sf, sa = np.ascontiguousarray(sync_from, np.uint32), np.ascontiguousarray(sync_at, np.uint32)
        assert len(sf) == n and len(sa) == n
        return lf, sf, sa

    def _parse_plan_batch(self, fn, desc, data, tile_first, tus, tu_at, tu_guard, plan, n_coeff_total, check, int16, coeff, values,
                          info, rows=None):
        """parse_elements_batch, parse_plan_batch and plan_parse_rows_batch through the library function `fn`; rows: None, or
        (level_first, sync_from, sync_at) for the rows form."""
        desc, data, tile_first, tus, coeff, res = self._parse_inputs(desc, data, tile_first, tus, n_coeff_total, int16, coeff)
        plan = np.ascontiguousarray(plan, np.uint32).reshape(-1, 2)
        assert len(tile_first) == len(desc) + 1
        tu_at, tu_guard = self._per_block(tu_at, tus), self._per_block(tu_guard, tus)
        lf, sf, sa = self._rows(*rows, len(desc)) if rows else (None,) * 3
        if values is None:
            values = np.zeros(max(len(plan), 1), np.uint32)
        if info is None:
            info = np.zeros(max(len(tus), 1), np.uint32)
        assert coeff.dtype == (np.int16 if int16 else np.int32) and values.dtype == np.uint32 and info.dtype == np.uint32
        rc = fn(self.h, len(desc), desc.ctypes.data, data.ctypes.data, len(data), tile_first.ctypes.data, tus.ctypes.data, _ptr(tu_at),
                _ptr(tu_guard), plan.ctypes.data, len(plan), coeff.ctypes.data, 2 if int16 else 4, int(n_coeff_total), values.ctypes.data,
                info.ctypes.data, res.ctypes.data, *((len(lf) - 1, lf.ctypes.data, sf.ctypes.data, sa.ctypes.data) if rows else ()))
        self._check(rc, allow_substream=not check)
        return coeff[: int(n_coeff_total)], values[: len(plan)], res[: len(desc)], info[: len(tus)]

    def _write_plan_batch(self, fn, desc, plan, values, tile_first, tus, tu_at, tu_guard, coeff, payload, check, values_out, info,
                          rows=None):
        """write_plan_batch and plan_write_rows_batch through the library function `fn`; rows as in _parse_plan_batch."""
        narrow = isinstance(coeff, np.ndarray) and coeff.dtype == np.int16
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        plan = np.ascontiguousarray(plan, np.uint32).reshape(-1, 2)
        values = np.ascontiguousarray(values, np.uint32)
        tile_first = np.ascontiguousarray(tile_first, np.uint32)
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        coeff = np.ascontiguousarray(coeff, np.int16 if narrow else np.int32)
        n = len(desc)
        assert len(tile_first) == n + 1 and len(values) >= len(plan)
        tu_at, tu_guard = self._per_block(tu_at, tus), self._per_block(tu_guard, tus)
        lf, sf, sa = self._rows(*rows, n) if rows else (None,) * 3
        if values_out is None:
            values_out = np.zeros(max(len(plan), 1), np.uint32)
        if info is None:
            info = np.zeros(max(len(tus), 1), np.uint32)
        assert values_out.dtype == np.uint32 and len(values_out) >= len(plan) and info.dtype == np.uint32 and payload.dtype == np.uint8
        offsets = np.zeros(n + 1, np.uint64)
        res = np.zeros(max(n, 1), RESULT_DTYPE)
        rc = fn(self.h, n, desc.ctypes.data, plan.ctypes.data, values.ctypes.data, len(plan), tile_first.ctypes.data, tus.ctypes.data,
                _ptr(tu_at), _ptr(tu_guard), coeff.ctypes.data, 2 if narrow else 4, len(coeff), payload.ctypes.data, payload.nbytes,
                offsets.ctypes.data, res.ctypes.data, values_out.ctypes.data, info.ctypes.data,
                *((len(lf) - 1, lf.ctypes.data, sf.ctypes.data, sa.ctypes.data) if rows else ()))
        self._check(rc, allow_substream=not check)
        return payload[: int(offsets[n])], offsets, res[:n], values_out[: len(plan)], info[: len(tus)]

    def residual_parse_batch(self, desc, data, tile_first, tus, n_coeff_total, check=True, with_info=False, int16=False, coeff=None):
        """Host arrays in, (coeff, results[, info]) out (cabac_hip_residual_parse_batch, synchronous; int16:
        cabac_hip_residual_parse_batch16, the blocks as int16)."""
        desc, data, tile_first, tus, coeff, res = self._parse_inputs(desc, data, tile_first, tus, n_coeff_total, int16, coeff)
        info = np.zeros(max(len(tus), 1), np.uint32)
        rc = (self.L.cabac_hip_residual_parse_batch16 if int16 else self.L.cabac_hip_residual_parse_batch)(self.h, len(desc), desc.ctypes.data, data.ctypes.data, len(data),
                                                   tile_first.ctypes.data, tus.ctypes.data, coeff.ctypes.data, int(n_coeff_total),
                                                   info.ctypes.data, res.ctypes.data)
        self._check(rc, allow_substream=not check)
        if with_info:
            return coeff[: int(n_coeff_total)], res[: len(desc)], info[: len(tus)]
        return coeff[: int(n_coeff_total)], res[: len(desc)]

    # ---- spliced substreams read back (include/cabac_hip_parse_unit.h) ------
    def parse_unit_device(self, n_sub, d_desc, d_bytes, d_tile_first, d_tu, d_tu_at, d_records, d_coeff, d_side_bins, d_results,
                          d_tu_info=0, int16=False):
        """cabac_hip_parse_unit_device: substream s = its side run d_records[rec_offset .. + n_records) with the blocks
        d_tu[d_tile_first[s] .. d_tile_first[s + 1]) coded in front of index d_tu_at[t] of that run (d_tu_at = 0: behind it), read
        back in one walk on one context store: blocks to d_coeff, side bins to d_side_bins[rec_offset + i]."""
        self._check(self.L.cabac_hip_parse_unit_device(
            self.h, n_sub, vp(d_desc), vp(d_bytes), vp(d_tile_first), _opt(d_tu), _opt(d_tu_at), _opt(d_records), _opt(d_coeff),
            2 if int16 else 4, _opt(d_side_bins), _opt(d_tu_info), vp(d_results)))

    def parse_unit_batch(self, desc, data, tile_first, tus, tu_at, records, n_coeff_total, check=True, int16=False, coeff=None,
                         side_bins=None, with_info=False):
        """Host arrays through cabac_hip_parse_unit_batch (synchronous): (coeff, side_bins, results[, info]).  `coeff` /
        `side_bins` (optional): the caller's arrays, written in place; tu_at may be None."""
        desc, data, tile_first, tus, coeff, res = self._parse_inputs(desc, data, tile_first, tus, n_coeff_total, int16, coeff)
        records = np.ascontiguousarray(records, np.uint16)
        assert len(tile_first) == len(desc) + 1
        tu_at = self._per_block(tu_at, tus)
        if side_bins is None:
            side_bins = np.zeros(max(len(records), 1), np.uint8)
        assert coeff.dtype == (np.int16 if int16 else np.int32) and side_bins.dtype == np.uint8
        info = np.zeros(max(len(tus), 1), np.uint32)
        rc = self.L.cabac_hip_parse_unit_batch(
            self.h, len(desc), desc.ctypes.data, data.ctypes.data, len(data), tile_first.ctypes.data, tus.ctypes.data, _ptr(tu_at),
            records.ctypes.data, len(records), coeff.ctypes.data, 2 if int16 else 4, int(n_coeff_total), side_bins.ctypes.data,
            info.ctypes.data, res.ctypes.data)
        self._check(rc, allow_substream=not check)
        out = (coeff[: int(n_coeff_total)], side_bins[: len(records)], res[: len(desc)])
        return out + (info[: len(tus)],) if with_info else out

    # ---- spliced substreams read back element by element (include/cabac_hip_parse_elements.h) ------
    def parse_elements_device(self, n_sub, d_desc, d_bytes, d_tile_first, d_tu, d_tu_at, d_tu_guard, d_plan, d_coeff, d_values,
                              d_results, d_tu_info=0, int16=False):
        """cabac_hip_parse_elements_device: substream s = its plan d_plan[2 * rec_offset .. + 2 * n_records) of syntax elements
        (element() words, guard() words) with the blocks coded in front of element d_tu_at[t], each block behind the guard
        d_tu_guard[t] (0: none guarded): element values to d_values[rec_offset + i], blocks to d_coeff."""
        self._check(self.L.cabac_hip_parse_elements_device(
            self.h, n_sub, vp(d_desc), vp(d_bytes), vp(d_tile_first), _opt(d_tu), _opt(d_tu_at), _opt(d_tu_guard), _opt(d_plan),
            _opt(d_coeff), 2 if int16 else 4, _opt(d_values), _opt(d_tu_info), vp(d_results)))

    def parse_elements_batch(self, desc, data, tile_first, tus, tu_at, tu_guard, plan, n_coeff_total, check=True, int16=False,
                             coeff=None, values=None, info=None):
        """Host arrays through cabac_hip_parse_elements_batch (synchronous): (coeff, values, results, info).  plan: uint32
        (n_elements, 2); `coeff` / `values` / `info` (optional): the caller's arrays, written in place; tu_at and tu_guard may be
        None."""
        return self._parse_plan_batch(self.L.cabac_hip_parse_elements_batch, desc, data, tile_first, tus, tu_at, tu_guard, plan,
                                      n_coeff_total, check, int16, coeff, values, info)

    # ---- a whole transform unit in one walk (include/cabac_hip_parse_plan.h) ------
    def parse_plan_device(self, n_sub, d_desc, d_bytes, d_tile_first, d_tu, d_tu_at, d_tu_guard, d_plan, d_coeff, d_values,
                          d_results, d_tu_info=0, int16=False):
        """cabac_hip_parse_plan_device: parse_elements_device on a plan that may hold cond() and block_info() entries."""
        self._check(self.L.cabac_hip_parse_plan_device(
            self.h, n_sub, vp(d_desc), vp(d_bytes), vp(d_tile_first), _opt(d_tu), _opt(d_tu_at), _opt(d_tu_guard), _opt(d_plan),
            _opt(d_coeff), 2 if int16 else 4, _opt(d_values), _opt(d_tu_info), vp(d_results)))

    def parse_plan_batch(self, desc, data, tile_first, tus, tu_at, tu_guard, plan, n_coeff_total, check=True, int16=False,
                         coeff=None, values=None, info=None):
        """Host arrays through cabac_hip_parse_plan_batch (synchronous): (coeff, values, results, info), as
        parse_elements_batch."""
        return self._parse_plan_batch(self.L.cabac_hip_parse_plan_batch, desc, data, tile_first, tus, tu_at, tu_guard, plan,
                                      n_coeff_total, check, int16, coeff, values, info)

    # ---- plan and values to coded substreams (include/cabac_hip_write_plan.h) ------
    def write_plan_device(self, n_sub, d_desc, d_plan, d_values_in, d_tile_first, n_tu, d_tu, d_tu_at, d_tu_guard, d_coeff, d_payload,
                          payload_capacity, d_payload_offsets, d_results, d_values_out=0, d_tu_info=0, int16=False):
        """cabac_hip_write_plan_device: the plan of parse_plan_device, the values of its real elements and the blocks' coefficients
        -> compacted coded substreams, the filled values (d_values_out, may be d_values_in) and the blocks' info words."""
        self._check(self.L.cabac_hip_write_plan_device(
            self.h, n_sub, vp(d_desc), _opt(d_plan), _opt(d_values_in), vp(d_tile_first), n_tu, _opt(d_tu), _opt(d_tu_at), _opt(d_tu_guard),
            _opt(d_coeff), 2 if int16 else 4, vp(d_payload), payload_capacity, vp(d_payload_offsets), vp(d_results), _opt(d_values_out),
            _opt(d_tu_info)))

    def write_plan_batch(self, desc, plan, values, tile_first, tus, tu_at, tu_guard, coeff, payload, check=True, values_out=None,
                         info=None):
        """Host arrays through cabac_hip_write_plan_batch (synchronous): (payload bytes, offsets uint64[n + 1], results, filled
        values, info words).  plan: uint32 (n_elements, 2); values: uint32 per element; coeff: int32 or int16; `payload`: the
        caller's uint8 array, written in place; `values_out` / `info` (optional): the caller's arrays, written in place (values_out
        may be `values`); tu_at and tu_guard may be None."""
        return self._write_plan_batch(self.L.cabac_hip_write_plan_batch, desc, plan, values, tile_first, tus, tu_at, tu_guard, coeff,
                                      payload, check, values_out, info)

    # ---- plans from and into context sets, and in WPP rows (include/cabac_hip_plan_rows.h) ------
    def plan_parse_sets_device(self, n_sub, d_desc, d_bytes, d_tile_first, d_tu, d_tu_at, d_tu_guard, d_plan, d_coeff, d_values,
                               d_results, d_tu_info=0, int16=False, n_sets=0, d_state=0, d_rate=0, d_start_set=0, d_out_set=0,
                               d_out_state=0, d_out_rate=0, d_out_at=0):
        """parse_plan_device with substream s started from set d_start_set[s] (CTX_NO_SET: Ctx::init) and the contexts it holds
        when it arrives at plan entry d_out_at[s] (0: the end) written as set d_out_set[s]; 0 for a pointer = NULL."""
        self._check(self.L.cabac_hip_plan_parse_sets_device(
            self.h, n_sub, vp(d_desc), vp(d_bytes), vp(d_tile_first), _opt(d_tu), _opt(d_tu_at), _opt(d_tu_guard), _opt(d_plan),
            _opt(d_coeff), 2 if int16 else 4, _opt(d_values), _opt(d_tu_info), vp(d_results),
            *self._sets7(n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate), _opt(d_out_at)))

    # ---- the plan parse in pieces (include/cabac_hip_plan_resume.h) ------
    def plan_resume_parse_device(self, n_sub, d_desc, d_bytes, d_tile_first, d_tu, d_tu_at, d_tu_guard, d_plan, d_coeff, d_values,
                                 d_results, d_tu_info=0, int16=False, n_sets=0, d_state=0, d_rate=0, d_start_set=0, d_out_set=0,
                                 d_out_state=0, d_out_rate=0, d_coder_in=0, d_coder_out=0):
        """One piece of every substream's plan: plan_parse_sets_device (out set behind the piece) continued from the coder states
        d_coder_in (CODER_STATE_DTYPE per substream; 0: all fresh) and leaving them in d_coder_out (0: not written; may be
        d_coder_in).  A descriptor without SUB_FINISH runs no stop check."""
        self._check(self.L.cabac_hip_plan_resume_parse_device(
            self.h, n_sub, vp(d_desc), vp(d_bytes), vp(d_tile_first), _opt(d_tu), _opt(d_tu_at), _opt(d_tu_guard), _opt(d_plan),
            _opt(d_coeff), 2 if int16 else 4, _opt(d_values), _opt(d_tu_info), vp(d_results),
            *self._sets7(n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate), _opt(d_coder_in), _opt(d_coder_out)))

    def plan_parse_rows_device(self, n_sub, d_desc, d_bytes, d_tile_first, d_tu, d_tu_at, d_tu_guard, d_plan, d_coeff, d_values,
                               d_results, level_first, d_sync_from, d_sync_at, d_tu_info=0, int16=False):
        """parse_plan_device over WPP rows in level order; level_first: HOST, n_level + 1 entries; d_sync_at in plan entries."""
        lf = np.ascontiguousarray(level_first, np.uint32)
        self._check(self.L.cabac_hip_plan_parse_rows_device(
            self.h, n_sub, vp(d_desc), vp(d_bytes), vp(d_tile_first), _opt(d_tu), _opt(d_tu_at), _opt(d_tu_guard), _opt(d_plan),
            _opt(d_coeff), 2 if int16 else 4, _opt(d_values), _opt(d_tu_info), vp(d_results), len(lf) - 1, lf.ctypes.data,
            vp(d_sync_from), vp(d_sync_at)))

    def plan_parse_rows_batch(self, desc, data, tile_first, tus, tu_at, tu_guard, plan, n_coeff_total, level_first, sync_from, sync_at,
                              check=True, int16=False, coeff=None, values=None, info=None):
        """Host arrays through cabac_hip_plan_parse_rows_batch (synchronous): (coeff, values, results, info), as parse_plan_batch."""
        return self._parse_plan_batch(self.L.cabac_hip_plan_parse_rows_batch, desc, data, tile_first, tus, tu_at, tu_guard, plan,
                                      n_coeff_total, check, int16, coeff, values, info, rows=(level_first, sync_from, sync_at))

    def plan_write_sets_device(self, n_sub, d_desc, d_plan, d_values_in, d_tile_first, n_tu, d_tu, d_tu_at, d_tu_guard, d_coeff,
                               d_payload, payload_capacity, d_payload_offsets, d_results, d_values_out=0, d_tu_info=0, int16=False,
                               n_sets=0, d_state=0, d_rate=0, d_start_set=0, d_out_set=0, d_out_state=0, d_out_rate=0):
        """write_plan_device with substream s coded from set d_start_set[s] and its final contexts written as set d_out_set[s]."""
        self._check(self.L.cabac_hip_plan_write_sets_device(
            self.h, n_sub, vp(d_desc), _opt(d_plan), _opt(d_values_in), vp(d_tile_first), n_tu, _opt(d_tu), _opt(d_tu_at), _opt(d_tu_guard),
            _opt(d_coeff), 2 if int16 else 4, vp(d_payload), payload_capacity, vp(d_payload_offsets), vp(d_results), _opt(d_values_out),
            _opt(d_tu_info), *self._sets7(n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate)))

    # ---- the plan write in pieces (include/cabac_hip_plan_continue.h) ------
    def plan_continue_write_device(self, n_sub, d_desc, d_plan, d_values_in, d_tile_first, n_tu, d_tu, d_tu_at, d_tu_guard, d_coeff,
                                   d_bytes, d_results, d_values_out=0, d_tu_info=0, int16=False, n_sets=0, d_state=0, d_rate=0,
                                   d_start_set=0, d_out_set=0, d_out_state=0, d_out_rate=0, d_coder_in=0, d_coder_out=0):
        """One piece of every substream's plan: plan_write_sets_device into the caller's slots (d_bytes + the descriptor's
        byte_offset, byte_capacity bytes) continued from the coder states d_coder_in (CODER_STATE_DTYPE per substream; 0: all
        fresh) and leaving them in d_coder_out (0: not written; may be d_coder_in).  A descriptor without SUB_FINISH flushes
        nothing."""
        self._check(self.L.cabac_hip_plan_continue_write_device(
            self.h, n_sub, vp(d_desc), _opt(d_plan), _opt(d_values_in), vp(d_tile_first), n_tu, _opt(d_tu), _opt(d_tu_at), _opt(d_tu_guard),
            _opt(d_coeff), 2 if int16 else 4, vp(d_bytes), vp(d_results), _opt(d_values_out), _opt(d_tu_info),
            *self._sets7(n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate), _opt(d_coder_in), _opt(d_coder_out)))

    def plan_write_rows_device(self, n_sub, d_desc, d_plan, d_values_in, d_tile_first, n_tu, d_tu, d_tu_at, d_tu_guard, d_coeff,
                               d_payload, payload_capacity, d_payload_offsets, d_results, level_first, d_sync_from, d_sync_at,
                               d_values_out=0, d_tu_info=0, int16=False):
        """write_plan_device over WPP rows in level order; level_first: HOST, n_level + 1 entries; d_sync_at in plan entries."""
        lf = np.ascontiguousarray(level_first, np.uint32)
        self._check(self.L.cabac_hip_plan_write_rows_device(
            self.h, n_sub, vp(d_desc), _opt(d_plan), _opt(d_values_in), vp(d_tile_first), n_tu, _opt(d_tu), _opt(d_tu_at), _opt(d_tu_guard),
            _opt(d_coeff), 2 if int16 else 4, vp(d_payload), payload_capacity, vp(d_payload_offsets), vp(d_results), _opt(d_values_out),
            _opt(d_tu_info), len(lf) - 1, lf.ctypes.data, vp(d_sync_from), vp(d_sync_at)))

    def plan_write_rows_batch(self, desc, plan, values, tile_first, tus, tu_at, tu_guard, coeff, payload, level_first, sync_from,
                              sync_at, check=True, values_out=None, info=None):
        """Host arrays through cabac_hip_plan_write_rows_batch (synchronous): as write_plan_batch."""
        return self._write_plan_batch(self.L.cabac_hip_plan_write_rows_batch, desc, plan, values, tile_first, tus, tu_at, tu_guard,
                                      coeff, payload, check, values_out, info, rows=(level_first, sync_from, sync_at))

    def residual_batch(self, tus, coeff, check=True):
        """Host arrays in, (records, offsets, info) out (cabac_hip_residual_batch: both passes, synchronous)."""
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        coeff = np.ascontiguousarray(coeff, np.int32)
        n = len(tus)
        offsets = np.zeros(n + 1, np.uint64)
        info = np.zeros(max(n, 1), np.uint32)
        rc = self.L.cabac_hip_residual_batch(self.h, n, tus.ctypes.data, coeff.ctypes.data, len(coeff), offsets.ctypes.data,
                                             info.ctypes.data, None, 0)
        self._check(rc, allow_substream=not check)
        records = np.zeros(max(int(offsets[n]), 1), np.uint16)
        rc = self.L.cabac_hip_residual_batch(self.h, n, tus.ctypes.data, coeff.ctypes.data, len(coeff), offsets.ctypes.data,
                                             info.ctypes.data, records.ctypes.data, len(records))
        self._check(rc, allow_substream=not check)
        return records[: int(offsets[n])], offsets, info[:n]

    def encode_residual_device(self, n_sub, d_desc, d_records, d_splice_first, d_splices, n_splice, n_tu, d_tu, d_coeff,
                               d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info=0, d_bin_counts=0, int16=False):
        """cabac_hip_encode_residual_device (int16: cabac_hip_encode_residual16_device, d_coeff holds int16 coefficients): host
        records + spliced coefficient blocks -> compacted coded substreams."""
        self._check((self.L.cabac_hip_encode_residual16_device if int16 else self.L.cabac_hip_encode_residual_device)(
            self.h, n_sub, vp(d_desc), vp(d_records), vp(d_splice_first), vp(d_splices) if d_splices else None, n_splice, n_tu,
            vp(d_tu) if d_tu else None, vp(d_coeff) if d_coeff else None, vp(d_payload), payload_capacity, vp(d_payload_offsets),
            vp(d_results), vp(d_tu_info) if d_tu_info else None, vp(d_bin_counts) if d_bin_counts else None))

    def encode_batch_residual(self, desc, records, splice_first, splices, tus, coeff, payload, check=True, with_info=False,
                              with_counts=False):
        """cabac_hip_encode_batch_residual (host arrays, synchronous): (offsets uint64[n + 1], results[, tu_info][, counts]).
        int16 coefficients go through cabac_hip_encode_batch_residual16."""
        narrow = isinstance(coeff, np.ndarray) and coeff.dtype == np.int16
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        splice_first = np.ascontiguousarray(splice_first, np.uint32)
        splices = np.ascontiguousarray(splices, SPLICE_DTYPE)
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        coeff = np.ascontiguousarray(coeff, np.int16 if narrow else np.int32)
        n = len(desc)
        offsets = np.zeros(n + 1, np.uint64)
        res = np.zeros(max(n, 1), RESULT_DTYPE)
        info = np.zeros(max(len(tus), 1), np.uint32) if with_info else None
        counts = np.zeros((max(n, 1), BIN_COUNT_WORDS), np.uint32) if with_counts else None
        rc = (self.L.cabac_hip_encode_batch_residual16 if narrow else self.L.cabac_hip_encode_batch_residual)(
            self.h, n, desc.ctypes.data, records.ctypes.data, len(records), splice_first.ctypes.data, splices.ctypes.data,
            len(tus), tus.ctypes.data, coeff.ctypes.data, len(coeff), payload.ctypes.data, payload.nbytes, offsets.ctypes.data,
            res.ctypes.data, info.ctypes.data if with_info else None, counts.ctypes.data if with_counts else None)
        self._check(rc, allow_substream=not check)
        out = [offsets, res[:n]]
        if with_info:
            out.append(info[: len(tus)])
        if with_counts:
            out.append(counts[:n])
        return tuple(out)

    # ---- probe points: written and estimated bits inside a substream (include/cabac_hip_probe.h) ------
    def written_bits_device(self, n_sub, d_desc, d_records, d_probe_first, d_probe_at, n_probe, d_bits, d_flags=0, n_sets=0,
                            d_state=0, d_rate=0, d_start_set=0):
        """cabac_hip_written_bits_device: d_bits[p] (uint32) = getNumWrittenBits() after the first d_probe_at[p] records of the
        substream that owns probe p.  Asynchronous on the ctx stream."""
        self._check(self.L.cabac_hip_written_bits_device(self.h, n_sub, _opt(d_desc), _opt(d_records), _opt(d_probe_first), _opt(d_probe_at),
                                                         n_probe, n_sets, _opt(d_state), _opt(d_rate), _opt(d_start_set), _opt(d_bits),
                                                         _opt(d_flags)))

    def estimate_probes_device(self, n_sub, d_desc, d_records, d_probe_first, d_probe_at, n_probe, d_frac_bits, d_flags=0, n_sets=0,
                               d_state=0, d_rate=0, d_start_set=0):
        """cabac_hip_estimate_probes_device: d_frac_bits[p] (uint64, 1/32768 bit) = the estimator's total after the first
        d_probe_at[p] records.  Asynchronous on the ctx stream."""
        self._check(self.L.cabac_hip_estimate_probes_device(self.h, n_sub, _opt(d_desc), _opt(d_records), _opt(d_probe_first),
                                                            _opt(d_probe_at), n_probe, n_sets, _opt(d_state), _opt(d_rate),
                                                            _opt(d_start_set), _opt(d_frac_bits), _opt(d_flags)))

    def _probes_batch(self, fn, dtype, desc, records, probe_first, probe_at, state, rate, start_set, check, out):
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        probe_first = np.ascontiguousarray(probe_first, np.uint32)
        probe_at = np.ascontiguousarray(probe_at, np.uint32)
        n = len(desc)
        if len(probe_first) != n + 1:
            raise ValueError("probe_first holds n_sub + 1 entries")
        n_sets = 0
        if start_set is not None:
            state = np.ascontiguousarray(state, np.uint32).reshape(-1, NUM_CTX)
            rate = np.ascontiguousarray(rate, np.uint8).reshape(-1, NUM_CTX)
            start_set = np.ascontiguousarray(start_set, np.uint32)
            n_sets = len(state)
            if len(rate) != n_sets or len(start_set) != n:
                raise ValueError("state and rate hold the same sets; start_set holds n_sub entries")
        values = np.zeros(max(len(probe_at), 1), dtype) if out is None else out
        flags = np.zeros(max(n, 1), np.uint32)
        rc = fn(self.h, n, desc.ctypes.data, records.ctypes.data, len(records), probe_first.ctypes.data, probe_at.ctypes.data,
                len(probe_at), n_sets, state.ctypes.data if n_sets else None, rate.ctypes.data if n_sets else None,
                start_set.ctypes.data if start_set is not None else None, values.ctypes.data, flags.ctypes.data)
        self._check(rc, allow_substream=not check)
        return values[: len(probe_at)], flags[:n]

    def written_bits_batch(self, desc, records, probe_first, probe_at, state=None, rate=None, start_set=None, check=True, out=None):
        """cabac_hip_written_bits_batch (host arrays, synchronous): (bits uint32[n_probe], flags uint32[n_sub])."""
        return self._probes_batch(self.L.cabac_hip_written_bits_batch, np.uint32, desc, records, probe_first, probe_at, state, rate,
                                  start_set, check, out)

    def estimate_probes_batch(self, desc, records, probe_first, probe_at, state=None, rate=None, start_set=None, check=True, out=None):
        """cabac_hip_estimate_probes_batch (host arrays, synchronous): (frac_bits uint64[n_probe], flags uint32[n_sub])."""
        return self._probes_batch(self.L.cabac_hip_estimate_probes_batch, np.uint64, desc, records, probe_first, probe_at, state, rate,
                                  start_set, check, out)

    def encode_residual_probes_device(self, n_sub, d_desc, d_records, d_splice_first, d_splices, n_splice, n_tu, d_tu, d_coeff,
                                      d_payload, payload_capacity, d_payload_offsets, d_results, d_probe_first, d_probe_at, n_probe,
                                      d_bits, d_probe_splice=0, d_tu_info=0, d_bin_counts=0, int16=False):
        """cabac_hip_encode_residual_probes_device: encode_residual_device that also answers probes (k host records, m splices in
        front) with the written bits of the expanded string in front of each."""
        self._check(self.L.cabac_hip_encode_residual_probes_device(
            self.h, n_sub, _opt(d_desc), _opt(d_records), _opt(d_splice_first), _opt(d_splices), n_splice, n_tu, _opt(d_tu), _opt(d_coeff),
            2 if int16 else 4, _opt(d_payload), payload_capacity, _opt(d_payload_offsets), _opt(d_results), _opt(d_tu_info),
            _opt(d_bin_counts), _opt(d_probe_first), _opt(d_probe_at), _opt(d_probe_splice), n_probe, _opt(d_bits)))

    def encode_residual_probes_batch(self, desc, records, splice_first, splices, tus, coeff, payload, probe_first, probe_at,
                                     probe_splice=None, check=True, with_info=False, with_counts=False):
        """cabac_hip_encode_residual_probes_batch (host arrays, synchronous): (offsets, results, bits uint32[n_probe][, tu_info]
        [, counts]); int16 coefficients go through with coeff_bytes = 2."""
        narrow = isinstance(coeff, np.ndarray) and coeff.dtype == np.int16
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        splice_first = np.ascontiguousarray(splice_first, np.uint32)
        splices = np.ascontiguousarray(splices, SPLICE_DTYPE)
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        coeff = np.ascontiguousarray(coeff, np.int16 if narrow else np.int32)
        probe_first = np.ascontiguousarray(probe_first, np.uint32)
        probe_at = np.ascontiguousarray(probe_at, np.uint32)
        n = len(desc)
        if len(probe_first) != n + 1:
            raise ValueError("probe_first holds n_sub + 1 entries")
        if probe_splice is not None:
            probe_splice = np.ascontiguousarray(probe_splice, np.uint32)
            if len(probe_splice) != len(probe_at):
                raise ValueError("probe_splice holds one entry per probe")
        offsets = np.zeros(n + 1, np.uint64)
        res = np.zeros(max(n, 1), RESULT_DTYPE)
        bits = np.zeros(max(len(probe_at), 1), np.uint32)
        info = np.zeros(max(len(tus), 1), np.uint32) if with_info else None
        counts = np.zeros((max(n, 1), BIN_COUNT_WORDS), np.uint32) if with_counts else None
        rc = self.L.cabac_hip_encode_residual_probes_batch(
            self.h, n, desc.ctypes.data, records.ctypes.data, len(records), splice_first.ctypes.data, splices.ctypes.data, len(tus),
            tus.ctypes.data, coeff.ctypes.data, 2 if narrow else 4, len(coeff), payload.ctypes.data, payload.nbytes, offsets.ctypes.data,
            res.ctypes.data, info.ctypes.data if with_info else None, counts.ctypes.data if with_counts else None,
            probe_first.ctypes.data, probe_at.ctypes.data, probe_splice.ctypes.data if probe_splice is not None else None, len(probe_at),
            bits.ctypes.data)
        self._check(rc, allow_substream=not check)
        out = [offsets, res[:n], bits[: len(probe_at)]]
        if with_info:
            out.append(info[: len(tus)])
        if with_counts:
            out.append(counts[:n])
        return tuple(out)

    # ---- the splice pipeline from and into context sets, and in WPP rows (include/cabac_hip_splice_rows.h) ------
    def encode_residual_sets_device(self, n_sub, d_desc, d_records, d_splice_first, d_splices, n_splice, n_tu, d_tu, d_coeff,
                                    d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info=0, d_bin_counts=0, int16=False,
                                    n_sets=0, d_state=0, d_rate=0, d_start_set=0, d_out_set=0, d_out_state=0, d_out_rate=0):
        """encode_residual_device with substream s coded from set d_start_set[s] and the contexts after the last record of its
        expanded string written as set d_out_set[s]."""
        self._check(self.L.cabac_hip_encode_residual_sets_device(
            self.h, n_sub, _opt(d_desc), _opt(d_records), _opt(d_splice_first), _opt(d_splices), n_splice, n_tu, _opt(d_tu), _opt(d_coeff),
            2 if int16 else 4, _opt(d_payload), payload_capacity, vp(d_payload_offsets), _opt(d_results), _opt(d_tu_info),
            _opt(d_bin_counts), *self._sets7(n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate)))

    def encode_residual_rows_device(self, n_sub, d_desc, d_records, d_splice_first, d_splices, n_splice, n_tu, d_tu, d_coeff,
                                    d_payload, payload_capacity, d_payload_offsets, d_results, level_first, d_sync_from, d_sync_at,
                                    d_sync_splice=0, d_tu_info=0, d_bin_counts=0, int16=False):
        """encode_residual_device over WPP rows in level order; level_first: HOST, n_level + 1 entries; (d_sync_at, d_sync_splice):
        the hand-over pair of every substream (d_sync_splice 0: every block at the position goes in front)."""
        lf = np.ascontiguousarray(level_first, np.uint32)
        self._check(self.L.cabac_hip_encode_residual_rows_device(
            self.h, n_sub, _opt(d_desc), _opt(d_records), _opt(d_splice_first), _opt(d_splices), n_splice, n_tu, _opt(d_tu), _opt(d_coeff),
            2 if int16 else 4, _opt(d_payload), payload_capacity, vp(d_payload_offsets), _opt(d_results), _opt(d_tu_info),
            _opt(d_bin_counts), len(lf) - 1, lf.ctypes.data, _opt(d_sync_from), _opt(d_sync_at), _opt(d_sync_splice)))

    def encode_residual_rows_batch(self, desc, records, splice_first, splices, tus, coeff, payload, level_first, sync_from, sync_at,
                                   sync_splice=None, check=True, offsets=None, results=None, info=None, counts=None):
        """Host arrays through cabac_hip_encode_residual_rows_batch (synchronous): (offsets uint64[n + 1], results, tu_info, counts).
        offsets / results / info / counts: the caller's arrays (else fresh ones).  A sync_from, sync_at or sync_splice shorter than
        the batch is refused here as the library refuses a bad link: CabacHipError(-2), nothing run, no output touched."""
        narrow = isinstance(coeff, np.ndarray) and coeff.dtype == np.int16
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        splice_first = np.ascontiguousarray(splice_first, np.uint32)
        splices = np.ascontiguousarray(splices, SPLICE_DTYPE)
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        coeff = np.ascontiguousarray(coeff, np.int16 if narrow else np.int32)
        lf = np.ascontiguousarray(level_first, np.uint32)
        sf, sa = np.ascontiguousarray(sync_from, np.uint32), np.ascontiguousarray(sync_at, np.uint32)
        ss = None if sync_splice is None else np.ascontiguousarray(sync_splice, np.uint32)
        n = len(desc)
        for name, a in (("sync_from", sf), ("sync_at", sa), ("sync_splice", ss)):
            if a is not None and len(a) < n:
                raise CabacHipError(-2, "%s is shorter than the batch: substream %d has none" % (name, len(a)))
        assert len(splice_first) == n + 1 and payload.dtype == np.uint8
        offsets = np.zeros(n + 1, np.uint64) if offsets is None else offsets
        res = np.zeros(max(n, 1), RESULT_DTYPE) if results is None else results
        info = np.zeros(max(len(tus), 1), np.uint32) if info is None else info
        counts = np.zeros((max(n, 1), BIN_COUNT_WORDS), np.uint32) if counts is None else counts
        rc = self.L.cabac_hip_encode_residual_rows_batch(
            self.h, n, desc.ctypes.data, records.ctypes.data, len(records), splice_first.ctypes.data, splices.ctypes.data, len(tus),
            tus.ctypes.data, coeff.ctypes.data, 2 if narrow else 4, len(coeff), payload.ctypes.data, payload.nbytes,
            offsets.ctypes.data, res.ctypes.data, info.ctypes.data, counts.ctypes.data, len(lf) - 1, lf.ctypes.data, sf.ctypes.data,
            sa.ctypes.data, ss.ctypes.data if ss is not None else None)
        self._check(rc, allow_substream=not check)
        return offsets, res[:n], info[: len(tus)], counts[:n]

    def assemble_device(self, n_sub, d_desc, d_results, d_bytes, d_payload, payload_capacity, d_offsets):
        self._check(self.L.cabac_hip_assemble_device(self.h, n_sub, vp(d_desc), vp(d_results), vp(d_bytes), vp(d_payload),
                                                     payload_capacity, vp(d_offsets)))

    def gather_records_device(self, n_seg, d_src_off, d_dst_off, d_len, d_src, d_dst):
        self._check(self.L.cabac_hip_gather_records_device(self.h, n_seg, vp(d_src_off), vp(d_dst_off), vp(d_len), vp(d_src), vp(d_dst)))

    def split_device(self, n_sub, d_desc, d_offsets, d_payload, d_bytes):
        self._check(self.L.cabac_hip_split_device(self.h, n_sub, vp(d_desc), vp(d_offsets), vp(d_payload), vp(d_bytes)))

    def count_emulations_device(self, n_sub, d_desc, d_results, d_bytes, d_counts):
        self._check(self.L.cabac_hip_count_emulations_device(self.h, n_sub, vp(d_desc), vp(d_results), vp(d_bytes),
                                                             vp(d_counts)))

    def ctx_init_device(self, n_sub, d_qp, d_init_id, d_state, d_rate):
        self._check(self.L.cabac_hip_ctx_init_device(self.h, n_sub, vp(d_qp), vp(d_init_id), vp(d_state), vp(d_rate)))

    # ---- emulation prevention (include/cabac_hip_nal.h) ---------------------------------------
    def nal_escape_device(self, n_seg, d_offsets, d_payload, payload_bytes_max, d_nal, nal_capacity, d_nal_offsets, d_status):
        """cabac_hip_nal_escape_device: segmented payload -> NAL bytes (03 inserted), entry points and a cabac_nal_status, all in
        device memory; payload_bytes_max bounds the length d_offsets[n_seg] that only the device reads."""
        self._check(self.L.cabac_hip_nal_escape_device(self.h, n_seg, vp(d_offsets) if d_offsets else None,
                                                       vp(d_payload) if d_payload else None, payload_bytes_max,
                                                       vp(d_nal) if d_nal else None, nal_capacity,
                                                       vp(d_nal_offsets) if d_nal_offsets else None, vp(d_status)))

    def nal_unescape_device(self, n_seg, d_nal_offsets, d_nal, nal_bytes_max, d_payload, payload_capacity, d_offsets, d_status,
                            d_locations=0, loc_capacity=0, loc_base=0):
        """cabac_hip_nal_unescape_device: the inverse; d_locations (optional, uint32): the positions of the removed bytes."""
        self._check(self.L.cabac_hip_nal_unescape_device(self.h, n_seg, vp(d_nal_offsets) if d_nal_offsets else None,
                                                         vp(d_nal) if d_nal else None, nal_bytes_max,
                                                         vp(d_payload) if d_payload else None, payload_capacity,
                                                         vp(d_offsets) if d_offsets else None,
                                                         vp(d_locations) if d_locations else None, loc_capacity, loc_base,
                                                         vp(d_status)))

    def nal_escape_batch(self, offsets, payload, nal):
        """cabac_hip_nal_escape_batch (host arrays, synchronous): fills `nal` (uint8 array, its size is the capacity; e.g.
        pinned) and returns (nal_offsets uint64[n_seg + 1], status record of NAL_STATUS_DTYPE)."""
        offsets = np.ascontiguousarray(offsets, np.uint64)
        payload = np.ascontiguousarray(payload, np.uint8)
        nal_offsets = np.zeros(len(offsets), np.uint64)
        status = np.zeros(1, NAL_STATUS_DTYPE)
        self._check(self.L.cabac_hip_nal_escape_batch(self.h, len(offsets) - 1, offsets.ctypes.data, payload.ctypes.data,
                                                      nal.ctypes.data, nal.nbytes, nal_offsets.ctypes.data, status.ctypes.data))
        return nal_offsets, status[0]

    def nal_unescape_batch(self, nal_offsets, nal, payload, locations=None, loc_base=0):
        """cabac_hip_nal_unescape_batch: fills `payload` (and `locations`, a uint32 array, if given; their sizes are the
        capacities) and returns (offsets uint64[n_seg + 1], status record)."""
        nal_offsets = np.ascontiguousarray(nal_offsets, np.uint64)
        nal = np.ascontiguousarray(nal, np.uint8)
        offsets = np.zeros(len(nal_offsets), np.uint64)
        status = np.zeros(1, NAL_STATUS_DTYPE)
        self._check(self.L.cabac_hip_nal_unescape_batch(self.h, len(nal_offsets) - 1, nal_offsets.ctypes.data, nal.ctypes.data,
                                                        payload.ctypes.data, payload.nbytes, offsets.ctypes.data,
                                                        locations.ctypes.data if locations is not None else None,
                                                        len(locations) if locations is not None else 0, loc_base,
                                                        status.ctypes.data))
        return offsets, status[0]

    # ---- sparse coefficient transport (include/cabac_hip_sparse.h) ------
    sparse_pack_host = staticmethod(sparse_pack_host)
    sparse_unpack_host = staticmethod(sparse_unpack_host)

    def sparse_expand_device(self, n_tu, d_tu, d_ent_first, d_entries, n_entries_max, d_coeff, coeff_bytes, n_coeff_total, d_status):
        """cabac_hip_sparse_expand_device: lists -> dense blocks in d_coeff (coeff_bytes 2 or 4); asynchronous on the ctx's stream."""
        self._check(self.L.cabac_hip_sparse_expand_device(self.h, n_tu, _opt(d_tu), vp(d_ent_first), _opt(d_entries), n_entries_max,
                                                          _opt(d_coeff), coeff_bytes, n_coeff_total, vp(d_status)))

    def sparse_compact_device(self, n_tu, d_tu, d_coeff, coeff_bytes, n_coeff_total, d_ent_first, d_entries, entry_capacity, d_status):
        """cabac_hip_sparse_compact_device: dense blocks -> d_ent_first (n_tu + 1 words) and at most entry_capacity entries."""
        self._check(self.L.cabac_hip_sparse_compact_device(self.h, n_tu, _opt(d_tu), _opt(d_coeff), coeff_bytes, n_coeff_total,
                                                           vp(d_ent_first), _opt(d_entries), entry_capacity, vp(d_status)))

    def sparse_encode_batch(self, desc, records, splice_first, splices, tus, ent_first, entries, n_coeff_total, payload, check=True,
                            with_info=False, with_counts=False, offsets=None, results=None):
        """cabac_hip_sparse_encode_batch (host arrays, synchronous): encode_batch_residual with the int16 blocks given as their
        lists; (offsets uint64[n + 1], results[, tu_info][, counts]).  `offsets` / `results` (optional): the caller's arrays."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        splice_first = np.ascontiguousarray(splice_first, np.uint32)
        splices = np.ascontiguousarray(splices, SPLICE_DTYPE)
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        ent_first = np.ascontiguousarray(ent_first, np.uint32)
        entries = np.ascontiguousarray(entries, np.uint32)
        n = len(desc)
        assert len(ent_first) >= len(tus) + 1
        offsets = np.zeros(n + 1, np.uint64) if offsets is None else offsets
        res = np.zeros(max(n, 1), RESULT_DTYPE) if results is None else results
        info = np.zeros(max(len(tus), 1), np.uint32) if with_info else None
        counts = np.zeros((max(n, 1), BIN_COUNT_WORDS), np.uint32) if with_counts else None
        rc = self.L.cabac_hip_sparse_encode_batch(
            self.h, n, desc.ctypes.data, records.ctypes.data, len(records), splice_first.ctypes.data, splices.ctypes.data, len(tus),
            tus.ctypes.data, ent_first.ctypes.data, entries.ctypes.data, len(entries), int(n_coeff_total), payload.ctypes.data,
            payload.nbytes, offsets.ctypes.data, res.ctypes.data, _ptr(info), _ptr(counts))
        self._check(rc, allow_substream=not check)
        out = [offsets, res[:n]]
        if with_info:
            out.append(info[: len(tus)])
        if with_counts:
            out.append(counts[:n])
        return tuple(out)

    def sparse_parse_batch(self, desc, data, tile_first, tus, n_coeff_total, entries=None, entry_capacity=None, check=True,
                           ent_first=None):
        """cabac_hip_sparse_parse_batch (host arrays, synchronous): residual_parse_batch(int16=True) with the blocks coming back as
        their lists; (ent_first, entries, results, tu_info, status record).  `entries` / `ent_first` (optional): the caller's uint32
        arrays, e.g. pinned; entry_capacity defaults to the length of `entries` (n_coeff_total without it).  A capacity that is too small raises with status
        CABAC_HIP_ERR_INVALID; the error's `sparse_status["n_entries"]` then tells the need, and `sparse_outputs` holds
        (ent_first, results, tu_info)."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        data = np.ascontiguousarray(data, np.uint8)
        tile_first = np.ascontiguousarray(tile_first, np.uint32)
        tus = np.ascontiguousarray(tus, TU_DTYPE)
        assert len(tile_first) == len(desc) + 1
        if entries is None:
            entries = np.zeros(max(int(n_coeff_total) if entry_capacity is None else int(entry_capacity), 1), np.uint32)
        cap = len(entries) if entry_capacity is None else int(entry_capacity)
        assert entries.dtype == np.uint32 and cap <= len(entries)
        if ent_first is None:
            ent_first = np.zeros(len(tus) + 1, np.uint32)
        assert ent_first.dtype == np.uint32 and len(ent_first) >= len(tus) + 1
        res = np.zeros(max(len(desc), 1), RESULT_DTYPE)
        info = np.zeros(max(len(tus), 1), np.uint32)
        status = np.zeros(1, SPARSE_STATUS_DTYPE)
        rc = self.L.cabac_hip_sparse_parse_batch(self.h, len(desc), desc.ctypes.data, data.ctypes.data, len(data), tile_first.ctypes.data,
                                                 tus.ctypes.data, ent_first.ctypes.data, entries.ctypes.data, cap, int(n_coeff_total),
                                                 info.ctypes.data, res.ctypes.data, status.ctypes.data)
        try:
            self._check(rc, allow_substream=not check)
        except CabacHipError as e:
            e.sparse_status = status[0]
            e.sparse_outputs = (ent_first, res[: len(desc)], info[: len(tus)])
            raise
        return ent_first, entries[: int(status[0]["n_entries"])], res[: len(desc)], info[: len(tus)], status[0]

    # ---- packed bin records (include/cabac_hip_rec10.h) ------
    rec10_bytes = staticmethod(rec10_bytes)
    rec10_pack_host = staticmethod(rec10_pack_host)
    rec10_unpack_host = staticmethod(rec10_unpack_host)

    def rec10_unpack_device(self, d_packed, first, n, d_records):
        """cabac_hip_rec10_unpack_device: d_records[first .. first + n) from the packed blocks at d_packed (16-byte aligned);
        asynchronous on the ctx's stream."""
        self._check(self.L.cabac_hip_rec10_unpack_device(self.h, _opt(d_packed), int(first), int(n), _opt(d_records)))

    def rec10_pack_device(self, d_records, n_records, d_packed, packed_capacity, d_status):
        """cabac_hip_rec10_pack_device: n_records records -> rec10_bytes(n_records) bytes at d_packed (16-byte aligned); *d_status
        receives a REC10_STATUS_DTYPE record; asynchronous on the ctx's stream."""
        self._check(self.L.cabac_hip_rec10_pack_device(self.h, _opt(d_records), int(n_records), _opt(d_packed), int(packed_capacity),
                                                       _opt(d_status)))

    def rec10_encode_batch(self, desc, packed, n_records_total, bytes_total, check=True, out=None, packed_bytes=None):
        """cabac_hip_rec10_encode_batch: encode_batch with the records as packed blocks (uint8 array, e.g. pinned; packed_bytes
        defaults to its size)."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        assert packed is None or (packed.dtype == np.uint8 and packed.flags.c_contiguous)
        if out is None:
            out = np.zeros(max(int(bytes_total), 1), np.uint8)
        res = np.zeros(len(desc), RESULT_DTYPE)
        rc = self.L.cabac_hip_rec10_encode_batch(self.h, len(desc), desc.ctypes.data, _ptr(packed),
                                                 packed.nbytes if packed_bytes is None else int(packed_bytes), int(n_records_total),
                                                 out.ctypes.data, int(bytes_total), res.ctypes.data)
        self._check(rc, allow_substream=not check)
        return out, res

    def rec10_encode_batch_payload(self, desc, packed, n_records_total, payload, check=True, packed_bytes=None, payload_capacity=None):
        """cabac_hip_rec10_encode_batch_payload: encode_batch_payload with the records as packed blocks; (offsets uint64[n + 1],
        results)."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        assert packed is None or (packed.dtype == np.uint8 and packed.flags.c_contiguous)
        offsets = np.zeros(len(desc) + 1, np.uint64)
        res = np.zeros(len(desc), RESULT_DTYPE)
        rc = self.L.cabac_hip_rec10_encode_batch_payload(
            self.h, len(desc), desc.ctypes.data, _ptr(packed), packed.nbytes if packed_bytes is None else int(packed_bytes),
            int(n_records_total), _ptr(payload), payload.nbytes if payload_capacity is None else int(payload_capacity),
            offsets.ctypes.data, res.ctypes.data)
        self._check(rc, allow_substream=not check)
        return offsets, res

    def rec10_decode_batch(self, desc, packed, n_records_total, data, bins_packed=False, check=True, bins=None, packed_bytes=None):
        """cabac_hip_rec10_decode_batch: decode_batch (bins_packed False: one bin per byte) or decode_batch_packed (True: eight to
        a byte) with the records as packed blocks; (bins, results)."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        data = np.ascontiguousarray(data, np.uint8)
        assert packed is None or (packed.dtype == np.uint8 and packed.flags.c_contiguous)
        n = int(n_records_total)
        n_out = (n + 7) // 8 if bins_packed else n
        if bins is None:
            bins = np.zeros(n_out + 1, np.uint8)
        res = np.zeros(len(desc), RESULT_DTYPE)
        rc = self.L.cabac_hip_rec10_decode_batch(self.h, len(desc), desc.ctypes.data, _ptr(packed),
                                                 packed.nbytes if packed_bytes is None else int(packed_bytes), n, data.ctypes.data,
                                                 len(data), bins.ctypes.data, 1 if bins_packed else 0, res.ctypes.data)
        self._check(rc, allow_substream=not check)
        return bins[:n_out], res

    def encode_batch_nal(self, desc, records, nal, check=True):
        """cabac_hip_encode_batch_nal: records -> NAL-ready payload in `nal` (uint8 array, e.g. pinned); returns (nal_offsets
        uint64[n + 1] — the entry points —, results, status record).  A `nal` that is too small raises with status
        CABAC_HIP_ERR_INVALID; the size needed is then in the error's `nal_status["out_bytes"]`."""
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        records = np.ascontiguousarray(records, np.uint16)
        nal_offsets = np.zeros(len(desc) + 1, np.uint64)
        res = np.zeros(max(len(desc), 1), RESULT_DTYPE)
        status = np.zeros(1, NAL_STATUS_DTYPE)
        rc = self.L.cabac_hip_encode_batch_nal(self.h, len(desc), desc.ctypes.data, records.ctypes.data, len(records),
                                               nal.ctypes.data, nal.nbytes, nal_offsets.ctypes.data, res.ctypes.data,
                                               status.ctypes.data)
        try:
            self._check(rc, allow_substream=not check)
        except CabacHipError as e:
            e.nal_status = status[0]
            raise
        return nal_offsets, res[: len(desc)], status[0]


class SearchLog:
    """A winner log (include/cabac_hip_search_emit.h): the candidates the search rounds picked, copied on the device round by
    round, coded into one substream per chain by encode_device().  Owned by its CabacHip, which closes it when it is closed."""

    def __init__(self, hip, n_chain, entry_capacity, record_capacity, tu_capacity, coeff_capacity, int16=False):
        self.hip, self.L, self.n_chain, self.int16 = hip, hip.L, n_chain, bool(int16)
        h = vp()
        hip._check(self.L.cabac_hip_search_log_create(hip.h, n_chain, entry_capacity, record_capacity, tu_capacity, coeff_capacity,
                                                      2 if int16 else 4, ctypes.byref(h)))
        self.h = h
        if not hasattr(hip, "_logs"):
            hip._logs = []
        hip._logs.append(self)

    def close(self):
        if getattr(self, "h", None):
            self.L.cabac_hip_search_log_destroy(self.h)   # waits for the ctx's stream
            self.h = None
            self.hip._logs.remove(self)

    @staticmethod
    def validate(pick, group_chain, n_cand, n_chain):
        """What the device form cannot see: among the groups that append (a pick below n_cand, a chain below n_chain) no chain
        may be named twice in one call.  Raises ValueError."""
        pick, group_chain = np.asarray(pick, np.uint32), np.asarray(group_chain, np.uint32)
        if pick.shape != group_chain.shape or pick.ndim != 1:
            raise ValueError("pick and group_chain must be one word per group")
        chains = group_chain[(pick < n_cand) & (group_chain < n_chain)]
        uniq, count = np.unique(chains, return_counts=True)
        if (count > 1).any():
            raise ValueError("chain %d is named by %d appending groups of one call (one group per chain)"
                             % (int(uniq[count > 1][0]), int(count.max())))

    def append_device(self, n_group, d_pick, d_group_chain, n_cand, d_cand_first, d_tu, d_coeff, d_rec_first, d_records=0, d_tu_at=0,
                      int16=None, check=True, pick=None, group_chain=None):
        """cabac_hip_search_log_append_device (asynchronous): group g appends candidate d_pick[g] to chain d_group_chain[g].  An
        array-backed call — the host copies `pick` and `group_chain` of the two device arrays are passed too — is validated on
        the host first with check=True (see validate); what only exists on the device cannot be."""
        if check and pick is not None and group_chain is not None:
            self.validate(pick, group_chain, n_cand, self.n_chain)
        narrow = self.int16 if int16 is None else bool(int16)
        self.hip._check(self.L.cabac_hip_search_log_append_device(
            self.h, n_group, _opt(d_pick), _opt(d_group_chain), n_cand, _opt(d_cand_first), _opt(d_tu), _opt(d_coeff), 2 if narrow else 4,
            _opt(d_rec_first), _opt(d_records), _opt(d_tu_at)))

    def reset(self):
        """cabac_hip_search_log_reset_device (asynchronous): the log is empty again."""
        self.hip._check(self.L.cabac_hip_search_log_reset_device(self.h))

    def view(self):
        """cabac_hip_search_log_view: a SearchLogView of device pointers (counters, entries, records, descriptors, positions,
        coefficients) and the capacities."""
        v = SearchLogView()
        self.hip._check(self.L.cabac_hip_search_log_view(self.h, ctypes.byref(v)))
        return v

    def read(self):
        """The log's content on the host, after waiting for the ctx's stream: a dict of numpy arrays cut to the counters
        (counters, entries, records, tu, tu_at, coeff)."""
        v = self.view()
        self.hip.synchronize()
        copy = self.L.hipMemcpy          # the HIP runtime this library is linked with
        copy.argtypes, copy.restype = [vp, vp, ctypes.c_size_t, ctypes.c_int], ctypes.c_int

        def fetch(ptr, n, dtype):
            out = np.zeros(n, dtype)
            if out.nbytes and copy(out.ctypes.data, ptr, out.nbytes, 2) != 0:   # hipMemcpyDeviceToHost
                raise CabacHipError(-3, "hipMemcpy of the log failed")
            return out

        cnt = fetch(v.d_counters, 1, LOG_COUNTERS_DTYPE)[0]
        return {"counters": cnt, "entries": fetch(v.d_entries, int(cnt["n_entry"]), LOG_ENTRY_DTYPE),
                "records": fetch(v.d_records, int(cnt["n_record"]), np.uint16), "tu": fetch(v.d_tu, int(cnt["n_tu"]), TU_DTYPE),
                "tu_at": fetch(v.d_tu_at, int(cnt["n_tu"]), np.uint32),
                "coeff": fetch(v.d_coeff, int(cnt["n_coeff"]), np.int16 if v.coeff_bytes == 2 else np.int32)}

    def encode_device(self, d_desc, d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info=0, d_bin_counts=0):
        """cabac_hip_search_log_encode_device: every chain's entries coded into its substream (d_desc: n_chain descriptors, qp and
        init_id | SUB_* read); waits for the ctx's stream twice.  Raises CabacHipError(-2) for a log that overflowed."""
        self.hip._check(self.L.cabac_hip_search_log_encode_device(
            self.h, vp(d_desc), vp(d_payload), payload_capacity, vp(d_payload_offsets), vp(d_results),
            vp(d_tu_info) if d_tu_info else None, vp(d_bin_counts) if d_bin_counts else None))

    # ---- marks, and the emit from sets and in rows (include/cabac_hip_splice_rows.h) ------
    def search_log_mark_device(self, n, d_chain):
        """cabac_hip_search_log_mark_device (asynchronous): the present cursors of the n listed chains become their hand-over
        points; a later mark replaces an earlier one, reset() clears them all."""
        self.hip._check(self.L.cabac_hip_search_log_mark_device(self.h, n, vp(d_chain) if d_chain else None))

    def search_log_encode_sets_device(self, d_desc, d_payload, payload_capacity, d_payload_offsets, d_results, d_tu_info=0,
                                      d_bin_counts=0, n_sets=0, d_state=0, d_rate=0, d_start_set=0, d_out_set=0, d_out_state=0,
                                      d_out_rate=0):
        """encode_device with chain k coded from set d_start_set[k] and its final contexts written as set d_out_set[k]."""
        self.hip._check(self.L.cabac_hip_search_log_encode_sets_device(
            self.h, vp(d_desc), vp(d_payload), payload_capacity, vp(d_payload_offsets), vp(d_results), _opt(d_tu_info), _opt(d_bin_counts),
            *CabacHip._sets7(n_sets, d_state, d_rate, d_start_set, d_out_set, d_out_state, d_out_rate)))

    def search_log_encode_rows_device(self, d_desc, d_payload, payload_capacity, d_payload_offsets, d_results, level_first, d_sync_from,
                                      d_tu_info=0, d_bin_counts=0):
        """encode_device over WPP rows: the chains in level order (level_first: HOST, n_level + 1 entries), chain k coded from the
        contexts chain d_sync_from[k] holds at its mark."""
        lf = np.ascontiguousarray(level_first, np.uint32)
        self.hip._check(self.L.cabac_hip_search_log_encode_rows_device(
            self.h, vp(d_desc), vp(d_payload), payload_capacity, vp(d_payload_offsets), vp(d_results), _opt(d_tu_info), _opt(d_bin_counts),
            len(lf) - 1, lf.ctypes.data, _opt(d_sync_from)))
