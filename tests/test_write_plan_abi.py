"""CPU: the public surface of the plan write — include/cabac_hip_write_plan.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the two cabac_hip_write_plan_* entry points, none of it leaked into the lists the other headers are
compared with, and the header states the contract the GPU tests check."""
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_write_plan_device", "cabac_hip_write_plan_batch"]
HEADER = "cabac_hip_write_plan.h"


def _code(name):
    hdr = open(os.path.join(H.ROOT, "include", name)).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_library_exports_and_binding_lists_the_entry_points():
    hdr, code = _code(HEADER)
    L = capi.load_library()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
        assert hasattr(L, n), n
    declared = sorted(set(re.findall(r"\b(cabac_hip_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(capi.EXPORTS_WRITE_PLAN) == sorted(NAMES)
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip.h"]
    others = (set(capi.EXPORTS) | set(capi.EXPORTS_ESTIMATE) | set(capi.EXPORTS_NAL) | set(capi.EXPORTS_SEARCH) |
              set(capi.EXPORTS_SEARCH_UNIT) | set(capi.EXPORTS_SEARCH_EMIT) | set(capi.EXPORTS_PARSE_UNIT) |
              set(capi.EXPORTS_PARSE_ELEMENTS) | set(capi.EXPORTS_PARSE_PLAN))
    assert not set(NAMES) & others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "write_plan" not in _code(other)[1], other
    for word in ("parse_plan", "parse_unit", "parse_elements", "search_unit", "estimate_unit", "search_log", "search_emit",
                 "cabac_hip_search", "CABAC_SEARCH"):
        assert word not in code, word                              # what the other headers' tests forbid outside their own header
    for word in ("kind 23", "kind 24", "kind 25", "kind 26", "kind 27"):
        assert word not in hdr, word


def test_header_states_the_contract():
    hdr, _ = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for word in ("W1.", "W2.", "W3.", "kind 28", "CABAC_RES_BAD_VALUE", "CABAC_RES_BAD_RECORD", "STREAM ORDERING CONTRACT",
                 "INCLUDE THAT HEADER FIRST", "cabac_hip_parse_elements.h", "cabac_hip_parse_plan.h", "waits for the ctx's stream ONCE",
                 "CTX_BIN, TRM value <= 1", "EP_BINS value < 2^numBins", "UNARY_MAX, UNARY_EP value <= maxSymbol",
                 "TRUNC_BIN value < maxSymbol", "REM_ABS value within the code word's range", "EXP_GOLOMB count + prefix ones < 32",
                 "the set of values the element parse reads back unflagged", "A stop codes nothing", "exactly one flag",
                 "CABAC_TU_INFO_TS", "CABAC_TU_INFO_NOT_CODED", "CABAC_TU_INFO_EMPTY", "CABAC_TU_INFO_BAD_DESC",
                 "may equal d_values_in", "FILLED values", "byte_offset / byte_capacity are ignored"):
        assert word in flat, word
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "kind 28" not in _code(other)[0], other


def test_header_compiles_as_c_behind_the_two_parse_headers():
    src = ('#include <stdio.h>\n#include "cabac_hip_parse_elements.h"\n#include "cabac_hip_parse_plan.h"\n#include "%s"\n'
           "int main(void) { int (*f)(cabac_hip_ctx *, uint32_t, const cabac_substream_desc *, const uint32_t *, const uint32_t *,\n"
           "  const uint32_t *, uint32_t, const cabac_tu_desc *, const uint32_t *, const uint32_t *, const void *, int, uint8_t *,\n"
           "  uint64_t, uint64_t *, cabac_substream_result *, uint32_t *, uint32_t *) = cabac_hip_write_plan_device;\n"
           "  int (*g)(cabac_hip_ctx *, uint32_t, const cabac_substream_desc *, const uint32_t *, const uint32_t *, uint64_t,\n"
           "  const uint32_t *, const cabac_tu_desc *, const uint32_t *, const uint32_t *, const void *, int, uint64_t, uint8_t *,\n"
           "  uint64_t, uint64_t *, cabac_substream_result *, uint32_t *, uint32_t *) = cabac_hip_write_plan_batch;\n"
           '  printf("%%d %%d %%u %%u\\n", f != 0, g != 0, CABAC_RES_BAD_VALUE, CABAC_PE_COND_WORD0(CABAC_JOIN_AND, 1));\n'
           "  return 0; }\n" % HEADER)
    alone = '#include "%s"\nint main(void) { return cabac_hip_write_plan_device == 0; }\n' % HEADER
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in (("t.c", src), ("u.c", alone)):          # behind the parse headers, and on its own
            c = os.path.join(tmp, name)
            open(c, "w").write(text)
            subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-address", "-I" + os.path.join(H.ROOT, "include"), c, "-c",
                                   "-o", os.path.join(tmp, name + ".o")])


def test_declarations_have_as_many_parameters_as_the_bindings_pass():
    L = capi.load_library()
    _, code = _code(HEADER)
    want = {"cabac_hip_write_plan_device": 18, "cabac_hip_write_plan_batch": 19}
    for n in NAMES:
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(getattr(L, n).argtypes) == want[n], n
    p = inspect.signature(capi.CabacHip.write_plan_device).parameters
    assert list(p)[:15] == ["self", "n_sub", "d_desc", "d_plan", "d_values_in", "d_tile_first", "n_tu", "d_tu", "d_tu_at", "d_tu_guard",
                            "d_coeff", "d_payload", "payload_capacity", "d_payload_offsets", "d_results"]
    assert [p[k].default for k in ("d_values_out", "d_tu_info", "int16")] == [0, 0, False]
    q = inspect.signature(capi.CabacHip.write_plan_batch).parameters
    assert list(q)[:10] == ["self", "desc", "plan", "values", "tile_first", "tus", "tu_at", "tu_guard", "coeff", "payload"]


def test_profile_kind_is_listed_in_the_binding():
    assert "28 plan write in cabac_hip_write_plan.h" in " ".join(capi.CabacHip.profile_read.__doc__.split())


def test_without_a_gpu_the_context_refuses():
    """No GPU: the binding raises CabacHipError (CABAC_HIP_ERR_NO_DEVICE), it does not fall back to anything.  Where there is one
    the same call — no substream — returns an empty payload."""
    args = (np.zeros(0, capi.DESC_DTYPE), np.zeros((0, 2), np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.uint32),
            np.zeros(0, capi.TU_DTYPE), None, None, np.zeros(0, np.int32), np.zeros(16, np.uint8))
    try:
        hip = capi.CabacHip()
    except capi.CabacHipError as e:
        assert e.status == -1
        return
    try:
        payload, offsets, res, values, info = hip.write_plan_batch(*args)
        assert len(payload) == 0 and offsets.tolist() == [0] and len(res) == 0
    finally:
        hip.close()
