"""CPU: the public surface of the plan rows — include/cabac_hip_plan_rows.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the six entry points, none of it leaked into the lists the other headers are compared with, the
header compiles as C99 behind the three headers it needs, states the contract the GPU tests check, and keeps out of the words the
other headers' tests reserve for their own."""
import inspect
import os
import re
import subprocess
import tempfile

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_plan_parse_sets_device", "cabac_hip_plan_parse_rows_device", "cabac_hip_plan_parse_rows_batch",
         "cabac_hip_plan_write_sets_device", "cabac_hip_plan_write_rows_device", "cabac_hip_plan_write_rows_batch"]
HEADER = "cabac_hip_plan_rows.h"
NEEDS = ["cabac_hip_parse_elements.h", "cabac_hip_parse_plan.h", "cabac_hip_ctx_sets.h"]
OTHER_LISTS = ["EXPORTS", "EXPORTS_ESTIMATE", "EXPORTS_NAL", "EXPORTS_SEARCH", "EXPORTS_SEARCH_UNIT", "EXPORTS_SEARCH_EMIT",
               "EXPORTS_PARSE_UNIT", "EXPORTS_PARSE_ELEMENTS", "EXPORTS_PARSE_PLAN", "EXPORTS_WRITE_PLAN", "EXPORTS_SEARCH_PLAN",
               "EXPORTS_CTX_SETS"]


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
    assert declared == sorted(capi.EXPORTS_PLAN_ROWS) == sorted(NAMES)
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip_parse.h"]
    others = set()
    for name in OTHER_LISTS:
        others |= set(getattr(capi, name))
    assert not set(NAMES) & others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            c = _code(other)[1]
            assert "plan_parse_" not in c and "plan_write_" not in c and "PLAN_ROWS" not in c, other


def test_the_lists_of_the_other_headers_are_untouched():
    sizes = {"EXPORTS": 44, "EXPORTS_ESTIMATE": 3, "EXPORTS_NAL": 6, "EXPORTS_SEARCH": 5, "EXPORTS_SEARCH_UNIT": 3,
             "EXPORTS_SEARCH_EMIT": 6, "EXPORTS_PARSE_UNIT": 2, "EXPORTS_PARSE_ELEMENTS": 2, "EXPORTS_PARSE_PLAN": 2,
             "EXPORTS_WRITE_PLAN": 2, "EXPORTS_SEARCH_PLAN": 3, "EXPORTS_CTX_SETS": 7}
    assert sorted(sizes) == sorted(OTHER_LISTS)
    for name, n in sizes.items():
        assert len(getattr(capi, name)) == n, name
    assert len(capi.EXPORTS_PLAN_ROWS) == 6


def test_header_keeps_out_of_the_words_the_other_headers_reserve():
    """Every tests/test_*_abi.py forbids its own header's words in every other header: outside comments none of the names below,
    and nowhere in the text a profile kind another header names."""
    hdr, code = _code(HEADER)
    for word in ("parse_plan", "write_plan", "search_plan", "resolve_plan", "parse_unit", "parse_elements", "search_unit",
                 "estimate_unit", "search_log", "search_emit", "ctx_sets", "ctx_advance", "_wpp_", "CABAC_CTX_NO_SET"):
        assert word not in code, word
    for kind in range(25, 34):
        assert "kind %d" % kind not in hdr, kind
    assert "0xFFFFFFFF" in hdr                                      # "no set", spelled out


def test_header_compiles_as_c99_behind_the_headers_it_needs():
    src = "".join('#include "%s"\n' % h for h in NEEDS + [HEADER]) + "int main(void) { return 0; }\n"
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(H.ROOT, "include"), c, "-o",
                               os.path.join(tmp, "t")])


def test_header_states_the_contract():
    hdr, _ = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for word in ("THE HAND-OVER POINT", "ARRIVES at entry k", "at(t) <= k", "k >= n", "k == 0 with no block at position 0",
                 "THE ZERO-BIN MARKER", "EP_BINS entry with numBins 0", "INCLUDE THOSE HEADERS FIRST", "DEFINITION OF THE RESULT",
                 "bit-identical", "IN-PLACE RULE", "LEVEL ORDER", "HOST memory", "EARLIER level", "all 379 entries",
                 "once per substream", "CABAC_RES_BAD_SET", "UNSPECIFIED", "CABAC_RES_UNDERRUN", "no host wait inside",
                 "ONE launch", "parsed exactly once", "ONCE in the middle", "CABAC_HIP_ERR_INVALID", "cabac_hip_last_error",
                 "kind 34", "kind 35", "kind 36"):
        assert word in flat, word
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            for kind in ("kind 34", "kind 35", "kind 36"):
                assert kind not in _code(other)[0], (other, kind)


def test_python_binding_has_the_methods():
    for m in NAMES:
        assert callable(getattr(capi.CabacHip, m[len("cabac_hip_"):])), m
    p = [k for k in inspect.signature(capi.CabacHip.plan_parse_sets_device).parameters]
    assert p[-8:] == ["n_sets", "d_state", "d_rate", "d_start_set", "d_out_set", "d_out_state", "d_out_rate", "d_out_at"]
    L = capi.load_library()
    n_parse, n_parse_b = len(L.cabac_hip_parse_plan_device.argtypes), len(L.cabac_hip_parse_plan_batch.argtypes)
    n_write, n_write_b = len(L.cabac_hip_write_plan_device.argtypes), len(L.cabac_hip_write_plan_batch.argtypes)
    assert (n_parse, n_parse_b, n_write, n_write_b) == (14, 17, 18, 19)
    assert len(L.cabac_hip_plan_parse_sets_device.argtypes) == n_parse + 8
    assert len(L.cabac_hip_plan_parse_rows_device.argtypes) == n_parse + 4
    assert len(L.cabac_hip_plan_parse_rows_batch.argtypes) == n_parse_b + 4
    assert len(L.cabac_hip_plan_write_sets_device.argtypes) == n_write + 7
    assert len(L.cabac_hip_plan_write_rows_device.argtypes) == n_write + 4
    assert len(L.cabac_hip_plan_write_rows_batch.argtypes) == n_write_b + 4
    # the header's own count of arguments
    _, code = _code("cabac_hip_plan_rows.h")
    for n in NAMES:
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(getattr(L, n).argtypes), n
