"""CPU: the public surface of the spliced rows — include/cabac_hip_splice_rows.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the six entry points, none of it leaked into the lists the other headers are compared with, the
header compiles as C99 behind the header it needs, states the contract the GPU tests check, keeps out of the words the other
headers' tests reserve for their own, and the log's three structs are the size they were."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_encode_residual_sets_device", "cabac_hip_encode_residual_rows_device", "cabac_hip_encode_residual_rows_batch",
         "cabac_hip_search_log_mark_device", "cabac_hip_search_log_encode_sets_device", "cabac_hip_search_log_encode_rows_device"]
HEADER = "cabac_hip_splice_rows.h"
NEEDS = ["cabac_hip_ctx_sets.h"]
OTHER_LISTS = ["EXPORTS", "EXPORTS_ESTIMATE", "EXPORTS_NAL", "EXPORTS_SEARCH", "EXPORTS_SEARCH_UNIT", "EXPORTS_SEARCH_EMIT",
               "EXPORTS_PARSE_UNIT", "EXPORTS_PARSE_ELEMENTS", "EXPORTS_PARSE_PLAN", "EXPORTS_WRITE_PLAN", "EXPORTS_SEARCH_PLAN",
               "EXPORTS_CTX_SETS", "EXPORTS_PLAN_ROWS"]


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
    assert declared == sorted(capi.EXPORTS_SPLICE_ROWS) == sorted(NAMES)
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip_search_emit.h"]
    others = set()
    for name in OTHER_LISTS:
        others |= set(getattr(capi, name))
    assert not set(NAMES) & others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            c = _code(other)[1]
            assert "residual_sets" not in c and "residual_rows" not in c and "log_mark" not in c and "log_encode_sets" not in c and \
                "log_encode_rows" not in c and "SPLICE_ROWS" not in c, other


def test_the_lists_of_the_other_headers_are_untouched():
    sizes = {"EXPORTS": 44, "EXPORTS_ESTIMATE": 3, "EXPORTS_NAL": 6, "EXPORTS_SEARCH": 5, "EXPORTS_SEARCH_UNIT": 3,
             "EXPORTS_SEARCH_EMIT": 6, "EXPORTS_PARSE_UNIT": 2, "EXPORTS_PARSE_ELEMENTS": 2, "EXPORTS_PARSE_PLAN": 2,
             "EXPORTS_WRITE_PLAN": 2, "EXPORTS_SEARCH_PLAN": 3, "EXPORTS_CTX_SETS": 7, "EXPORTS_PLAN_ROWS": 6}
    assert sorted(sizes) == sorted(OTHER_LISTS)
    for name, n in sizes.items():
        assert len(getattr(capi, name)) == n, name
    assert len(capi.EXPORTS_SPLICE_ROWS) == 6


def test_header_keeps_out_of_the_words_the_other_headers_reserve():
    """Every tests/test_*_abi.py forbids its own header's words in every other header: outside comments none of the names below,
    and nowhere in the text a profile kind another header names."""
    hdr, code = _code(HEADER)
    for word in ("ctx_sets", "_wpp_", "ctx_advance", "CABAC_CTX_NO_SET", "plan_parse_", "plan_write_", "PLAN_ROWS", "parse_unit",
                 "parse_elements", "parse_plan", "write_plan", "search_plan", "resolve_plan", "CABAC_RES_BAD_SET"):
        assert word not in code, word
    for kind in range(0, 37):
        assert not re.search(r"kind %d\b" % kind, hdr), kind
    assert "0xFFFFFFFF" in hdr and "CABAC_RES_BAD_SET" in hdr             # "no set", spelled out; the flag, in comments only


def test_header_compiles_as_c99_behind_the_header_it_needs():
    src = "".join('#include "%s"\n' % h for h in NEEDS + [HEADER]) + "int main(void) { return 0; }\n"
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(H.ROOT, "include"), c, "-o",
                               os.path.join(tmp, "t")])


def test_header_states_the_contract():
    hdr, _ = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for word in ("THE HAND-OVER POINT", "EXPANDED STRING", "clipped to n", "[#{at < k}, #{at <= k}]", "the upper end everywhere",
                 "LOWER END", "begins with a block", "contribute nothing", "INCLUDE THAT HEADER FIRST", "DEFINITION OF THE RESULT",
                 "bit-identical", "IN-PLACE RULE", "rate rule", "LEVEL ORDER", "HOST memory", "EARLIER level", "all 379 entries",
                 "a copy of its start set", "CABAC_RES_BAD_SET", "no payload byte", "ONCE in the middle", "NO SECOND HOST WAIT",
                 "no atomics", "ONE encode launch", "ONE chunk", "CABAC_HIP_ERR_INVALID", "cabac_hip_last_error", "REPLACES",
                 "end of chain", "skipped", "dropped for capacity", "hands over its final contexts", "WAIT FOR THE STREAM TWICE",
                 "not consumed", "kind 37", "kind 38", "kind 39"):
        assert word in flat, word
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            for kind in ("kind 37", "kind 38", "kind 39"):
                assert kind not in _code(other)[0], (other, kind)


def test_python_binding_has_the_methods_and_the_argument_counts():
    for m in NAMES[:3]:
        assert callable(getattr(capi.CabacHip, m[len("cabac_hip_"):])), m
    for m in NAMES[3:]:
        assert callable(getattr(capi.SearchLog, m[len("cabac_hip_"):])), m
    p = [k for k in inspect.signature(capi.CabacHip.encode_residual_sets_device).parameters]
    assert p[-7:] == ["n_sets", "d_state", "d_rate", "d_start_set", "d_out_set", "d_out_state", "d_out_rate"]
    p = [k for k in inspect.signature(capi.SearchLog.search_log_encode_sets_device).parameters]
    assert p[-7:] == ["n_sets", "d_state", "d_rate", "d_start_set", "d_out_set", "d_out_state", "d_out_rate"]
    L = capi.load_library()
    # the plain calls, in the const void * / coeff_bytes form (one argument more than the typed forms)
    n_plain, n_plain_b = len(L.cabac_hip_encode_residual_device.argtypes) + 1, len(L.cabac_hip_encode_batch_residual.argtypes) + 1
    n_log = len(L.cabac_hip_search_log_encode_device.argtypes)
    assert (n_plain, n_plain_b, n_log) == (17, 18, 8)
    assert len(L.cabac_hip_encode_residual_sets_device.argtypes) == n_plain + 7
    assert len(L.cabac_hip_encode_residual_rows_device.argtypes) == n_plain + 5
    assert len(L.cabac_hip_encode_residual_rows_batch.argtypes) == n_plain_b + 5
    assert len(L.cabac_hip_search_log_encode_sets_device.argtypes) == n_log + 7
    assert len(L.cabac_hip_search_log_encode_rows_device.argtypes) == n_log + 3
    assert len(L.cabac_hip_search_log_mark_device.argtypes) == 3
    assert L.cabac_hip_encode_residual_rows_device.argtypes[10] is ctypes.c_int          # coeff_bytes behind d_coeff
    _, code = _code(HEADER)
    for n in NAMES:                                                     # the header's own count of arguments
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(getattr(L, n).argtypes), n


def test_the_log_s_structs_are_the_size_they_were():
    """The marks are internal words of the log: the view and the two pinned structs do not change."""
    src = '#include <stdio.h>\n#include "cabac_hip_ctx_sets.h"\n#include "%s"\n' % HEADER + \
        'int main(void) { printf("%zu %zu %zu\\n", sizeof(cabac_search_log_counters), sizeof(cabac_search_log_entry), ' \
        'sizeof(cabac_search_log_view)); return 0; }\n'
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "t.c"), os.path.join(tmp, "t")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-I" + os.path.join(H.ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [40, 32, 80]
    assert capi.LOG_COUNTERS_DTYPE.itemsize == 40 and capi.LOG_ENTRY_DTYPE.itemsize == 32 and ctypes.sizeof(capi.SearchLogView) == 80
