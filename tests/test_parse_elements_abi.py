"""CPU: the public surface of the element parse — include/cabac_hip_parse_elements.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the two cabac_hip_parse_elements_* entry points, none of it leaked into the lists the other headers
are compared with, and the packers put the bits where the header says."""
import inspect
import os
import re
import subprocess
import tempfile

import pytest

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_parse_elements_device", "cabac_hip_parse_elements_batch"]
HEADER = "cabac_hip_parse_elements.h"


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
    assert declared == sorted(capi.EXPORTS_PARSE_ELEMENTS) == sorted(NAMES)
    assert '#include "cabac_hip_parse.h"' in hdr
    others = (set(capi.EXPORTS) | set(capi.EXPORTS_ESTIMATE) | set(capi.EXPORTS_NAL) | set(capi.EXPORTS_SEARCH) |
              set(capi.EXPORTS_SEARCH_UNIT) | set(capi.EXPORTS_SEARCH_EMIT) | set(capi.EXPORTS_PARSE_UNIT))
    assert not set(NAMES) & others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "parse_elements" not in _code(other)[1], other
    for word in ("parse_unit", "search_unit", "estimate_unit", "search_log", "search_emit", "cabac_hip_search", "CABAC_SEARCH"):
        assert word not in code, word                              # what the other headers' tests forbid outside their own header
    for word in ("kind 23", "kind 24", "kind 25"):
        assert word not in hdr, word


def test_header_states_the_contract():
    hdr, _ = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for word in ("DEFINITION OF THE RESULT", "GUARD WORD", "bits 7..0 back 0 means unguarded", "bits 9..8 cmp 0 !=, 1 ==, 2 >=, 3 < (unsigned)",
                 "bits 15..10 - must be zero", "bits 31..16 imm comparison operand", "value() of a skipped element is 0", "TWO IDENTITIES",
                 "E1.", "E2.", "CABAC_RES_BAD_VALUE", "CABAC_TU_INFO_NOT_CODED", "kind 26", "STREAM ORDERING CONTRACT",
                 "A BAD PLAN ENTRY", "count + ones reaches 32", "ONE context store", "CABAC_RES_UNDERRUN is reported alone",
                 "arbitrary bytes terminate"):
        assert word in flat, word
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "kind 26" not in _code(other)[0], other


def test_header_compiles_as_c():
    src = ('#include <stdio.h>\n#include "%s"\n'
           "int main(void) { int (*f)(cabac_hip_ctx *, uint32_t, const cabac_substream_desc *, const uint8_t *, const uint32_t *,\n"
           "  const cabac_tu_desc *, const uint32_t *, const uint32_t *, const uint32_t *, void *, int, uint32_t *, uint32_t *,\n"
           "  cabac_substream_result *) = cabac_hip_parse_elements_device;\n"
           '  printf("%%d %%u %%u %%u\\n", f != 0, CABAC_RES_BAD_VALUE, CABAC_TU_INFO_NOT_CODED, CABAC_GUARD(255, CABAC_GUARD_LT, 7));\n'
           "  return 0; }\n" % HEADER)
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(H.ROOT, "include"), c, "-c", "-o", os.path.join(tmp, "t.o")])


def test_declarations_have_as_many_parameters_as_the_bindings_pass():
    L = capi.load_library()
    _, code = _code(HEADER)
    want = {"cabac_hip_parse_elements_device": 14, "cabac_hip_parse_elements_batch": 17}
    for n in NAMES:
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(getattr(L, n).argtypes) == want[n], n
    p = inspect.signature(capi.CabacHip.parse_elements_device).parameters
    assert [k for k in p][1:12] == ["n_sub", "d_desc", "d_bytes", "d_tile_first", "d_tu", "d_tu_at", "d_tu_guard", "d_plan", "d_coeff",
                                    "d_values", "d_results"]
    assert callable(capi.CabacHip.parse_elements_batch)


def test_flag_values_match_the_header_and_collide_with_nothing():
    hdr, _ = _code(HEADER)
    assert re.search(r"#define CABAC_RES_BAD_VALUE 0x20u\b", hdr) and capi.RES_BAD_VALUE == 0x20
    assert re.search(r"#define CABAC_TU_INFO_NOT_CODED 0x40000u\b", hdr) and capi.TU_INFO_NOT_CODED == 0x40000
    assert capi.RES_BAD_VALUE not in (capi.RES_OVERFLOW, capi.RES_BAD_RECORD, capi.RES_UNDERRUN, capi.RES_BAD_STOP, capi.RES_RANGE)
    assert not capi.TU_INFO_NOT_CODED & (0xFFFF | capi.TU_INFO_MTS_VIOLATION | capi.TU_INFO_TS | capi.TU_INFO_EMPTY | capi.TU_INFO_BAD_DESC)


def test_packers_put_the_bits_where_the_binariser_reads_them():
    """word0 as in include/cabac_hip.h, "Syntax-element record"; word1 as the header's guard table"""
    e = capi.element
    assert e(capi.SE_CTX_BIN, ctx=378) == 0 | 378 << 4
    assert e(capi.SE_EP_BINS, n=32) == 1 | 32 << 4
    assert e(capi.SE_REM_ABS, rice=14, cutoff=12, max_log2=20) == 2 | 14 << 4 | 12 << 9 | 20 << 14
    assert e(capi.SE_REM_ABS) == 2 | 5 << 9 | 15 << 14
    assert e(capi.SE_TRM) == 3 and e(capi.SE_ALIGN) == 8
    assert e(capi.SE_UNARY_MAX, ctx=3, ctx_n=377, max_symbol=255) == 4 | 3 << 4 | 377 << 13 | 255 << 22
    assert e(capi.SE_UNARY_MAX, ctx=3, max_symbol=1) == 4 | 3 << 4 | 3 << 13 | 1 << 22
    assert e(capi.SE_UNARY_EP, max_symbol=32) == 5 | 32 << 4
    assert e(capi.SE_EXP_GOLOMB, count=31) == 6 | 31 << 4
    assert e(capi.SE_TRUNC_BIN, max_symbol=(1 << 28) - 1) == 7 | ((1 << 28) - 1) << 4
    assert capi.guard(0) == 0 and capi.guard(255, capi.GUARD_LT, 0xFFFF) == 0xFFFF03FF
    assert capi.guard(1, capi.GUARD_EQ, 5) == 1 | 1 << 8 | 5 << 16 and capi.guard(64, capi.GUARD_GE, 2) == 64 | 2 << 8 | 2 << 16
    assert [capi.GUARD_NE, capi.GUARD_EQ, capi.GUARD_GE, capi.GUARD_LT] == [0, 1, 2, 3]
    for bad in (lambda: capi.guard(256), lambda: capi.guard(1, 4), lambda: capi.guard(1, 0, 1 << 16), lambda: e(capi.SE_CTX_BIN, ctx=512),
                lambda: e(capi.SE_EP_BINS, n=64), lambda: e(capi.SE_TRUNC_BIN, max_symbol=1 << 28)):
        with pytest.raises(ValueError):
            bad()
    # the binariser's own words: the oracle's record of the same element decodes to the same fields
    import parse_elements_model as E
    assert E.fields(e(capi.SE_UNARY_MAX, ctx=3, ctx_n=377, max_symbol=255)) == (4, dict(ctx=3, ctx_n=377, max_symbol=255))
    assert E.fields(e(capi.SE_REM_ABS, rice=14, cutoff=12, max_log2=20)) == (2, dict(rice=14, cutoff=12, max_log2=20))
