"""CPU: the public surface of the plan parse — include/cabac_hip_parse_plan.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the two cabac_hip_parse_plan_* entry points, none of it leaked into the lists the other headers are
compared with, and the packers put the bits where the header says."""
import inspect
import os
import re
import subprocess
import tempfile

import pytest

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_parse_plan_device", "cabac_hip_parse_plan_batch"]
HEADER = "cabac_hip_parse_plan.h"


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
    assert declared == sorted(capi.EXPORTS_PARSE_PLAN) == sorted(NAMES)
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip_parse.h"]
    others = (set(capi.EXPORTS) | set(capi.EXPORTS_ESTIMATE) | set(capi.EXPORTS_NAL) | set(capi.EXPORTS_SEARCH) |
              set(capi.EXPORTS_SEARCH_UNIT) | set(capi.EXPORTS_SEARCH_EMIT) | set(capi.EXPORTS_PARSE_UNIT) | set(capi.EXPORTS_PARSE_ELEMENTS))
    assert not set(NAMES) & others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "parse_plan" not in _code(other)[1], other
    for word in ("parse_unit", "parse_elements", "search_unit", "estimate_unit", "search_log", "search_emit", "cabac_hip_search", "CABAC_SEARCH"):
        assert word not in code, word                              # what the other headers' tests forbid outside their own header
    for word in ("kind 23", "kind 24", "kind 25", "kind 26"):
        assert word not in hdr, word


def test_header_states_the_contract():
    hdr, _ = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for word in ("CABAC_PE_COND", "CABAC_PE_BLOCK_INFO", "P1.", "P2.", "kind 27", "never skipped", "reads no bin", "nb(i)",
                 "INCLUDE THAT HEADER FIRST", "cabac_hip_parse_elements.h", "KINDS 11..15 are bad", "join 3", "which >= nb(i)",
                 "shift + width > 32", "STREAM ORDERING CONTRACT"):
        assert word in flat, word
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "kind 27" not in _code(other)[0], other


def test_header_compiles_as_c_behind_the_element_parse_s_header():
    src = ('#include <stdio.h>\n#include "cabac_hip_parse_elements.h"\n#include "%s"\n'
           "typedef char cond_word0[CABAC_PE_COND_WORD0(CABAC_JOIN_OR, 255) == 0x2FF9u ? 1 : -1];\n"
           "typedef char info_word0[CABAC_PE_BLOCK_INFO_WORD0(15, 0, 32) == 0x400FAu ? 1 : -1];\n"
           "int main(void) { int (*f)(cabac_hip_ctx *, uint32_t, const cabac_substream_desc *, const uint8_t *, const uint32_t *,\n"
           "  const cabac_tu_desc *, const uint32_t *, const uint32_t *, const uint32_t *, void *, int, uint32_t *, uint32_t *,\n"
           "  cabac_substream_result *) = cabac_hip_parse_plan_device;\n"
           '  printf("%%d %%u %%u %%u %%u\\n", f != 0, CABAC_PE_COND_WORD0(CABAC_JOIN_AND, 1), CABAC_PE_BLOCK_INFO_WORD0(0, 16, 1),\n'
           "         CABAC_GUARD(1, CABAC_GUARD_NE, 0), CABAC_TU_INFO_NOT_CODED);\n"
           "  return 0; }\n" % HEADER)
    assert (0x2FF9, 0x400FA) == (capi.cond(0, 0, 0, capi.JOIN_OR, 255)[0], capi.block_info(15, 0, 32))
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(H.ROOT, "include"), c, "-c", "-o", os.path.join(tmp, "t.o")])


def test_declarations_have_as_many_parameters_as_the_bindings_pass():
    L = capi.load_library()
    _, code = _code(HEADER)
    want = {"cabac_hip_parse_plan_device": 14, "cabac_hip_parse_plan_batch": 17}
    for n in NAMES:
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(getattr(L, n).argtypes) == want[n], n
        twin = n.replace("parse_plan", "parse_elements")           # the same parameter list as the element parse's form
        _, ecode = _code("cabac_hip_parse_elements.h")
        assert " ".join(args.split()) == " ".join(re.search(r"\b%s\s*\((.*?)\)\s*;" % twin, ecode, flags=re.S).group(1).split()), n
        assert [a for a in getattr(L, n).argtypes] == [a for a in getattr(L, twin).argtypes], n
    p, q = inspect.signature(capi.CabacHip.parse_plan_device).parameters, inspect.signature(capi.CabacHip.parse_elements_device).parameters
    assert list(p) == list(q)
    p, q = inspect.signature(capi.CabacHip.parse_plan_batch).parameters, inspect.signature(capi.CabacHip.parse_elements_batch).parameters
    assert list(p) == list(q)


def test_packers_put_the_bits_where_the_header_says():
    hdr, _ = _code(HEADER)
    assert re.search(r"#define CABAC_PE_COND 9u\b", hdr) and re.search(r"#define CABAC_PE_BLOCK_INFO 10u\b", hdr)
    assert (capi.PE_COND, capi.PE_BLOCK_INFO) == (9, 10) and [capi.JOIN_NONE, capi.JOIN_AND, capi.JOIN_OR] == [0, 1, 2]
    assert capi.cond(0, 0, 0) == (9, 0)
    assert capi.cond(255, capi.GUARD_LT, 0xFFFF, capi.JOIN_OR, 255) == (9 | 255 << 4 | 2 << 12, 0xFFFF03FF)
    assert capi.cond(64, capi.GUARD_GE, 2, capi.JOIN_AND, 1) == (9 | 1 << 4 | 1 << 12, capi.guard(64, capi.GUARD_GE, 2))
    assert capi.cond(3, capi.GUARD_EQ, 5, back2=7) == (9 | 7 << 4, capi.guard(3, capi.GUARD_EQ, 5))
    assert capi.block_info() == 10 | 16 << 13
    assert capi.block_info(15, 31, 1) == 10 | 15 << 4 | 31 << 8 | 1 << 13
    assert capi.block_info(2, 0, 32) == 10 | 2 << 4 | 32 << 13 and capi.block_info(0, 16, 16) == 10 | 16 << 8 | 16 << 13
    for bad in (lambda: capi.cond(256), lambda: capi.cond(1, 4), lambda: capi.cond(1, 0, 1 << 16), lambda: capi.cond(1, 0, 0, 3),
                lambda: capi.cond(1, 0, 0, 1, 256), lambda: capi.cond(1, 0, 0, -1), lambda: capi.block_info(16),
                lambda: capi.block_info(0, 32, 1), lambda: capi.block_info(0, 0, 0), lambda: capi.block_info(0, 0, 33),
                lambda: capi.block_info(0, 17, 16), lambda: capi.block_info(-1)):
        with pytest.raises(ValueError):
            bad()
    import parse_plan_model as PM
    assert PM.fields(capi.cond(1, 0, 0, capi.JOIN_OR, 200)[0]) == (9, dict(back2=200, join=2))
    assert PM.fields(capi.block_info(3, 17, 1)) == (10, dict(which=3, shift=17, width=1))
