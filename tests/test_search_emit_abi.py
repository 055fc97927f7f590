"""CPU: the public surface of the winner log — include/cabac_hip_search_emit.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the six cabac_hip_search_log_* entry points, and nothing of it leaked into the lists the other
five headers are compared with."""
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_search_log_create", "cabac_hip_search_log_destroy", "cabac_hip_search_log_reset_device",
         "cabac_hip_search_log_append_device", "cabac_hip_search_log_view", "cabac_hip_search_log_encode_device"]
OTHERS = ("cabac_hip.h", "cabac_hip_estimate.h", "cabac_hip_nal.h", "cabac_hip_search.h", "cabac_hip_search_unit.h")


def _code(name):
    hdr = open(os.path.join(H.ROOT, "include", name)).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_library_exports_and_binding_lists_the_entry_points():
    hdr, code = _code("cabac_hip_search_emit.h")
    L = capi.load_library()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
        assert hasattr(L, n), n
    declared = sorted(set(re.findall(r"\b(cabac_hip_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(capi.EXPORTS_SEARCH_EMIT) == sorted(NAMES)
    assert '#include "cabac_hip_search_unit.h"' in hdr
    others = set(capi.EXPORTS) | set(capi.EXPORTS_ESTIMATE) | set(capi.EXPORTS_NAL) | set(capi.EXPORTS_SEARCH) | set(capi.EXPORTS_SEARCH_UNIT)
    assert not set(NAMES) & others
    for other in OTHERS:
        _, c = _code(other)
        assert "search_log" not in c and "search_emit" not in c, other


def test_header_defines_the_result_and_names_its_profile_kinds():
    hdr, _ = _code("cabac_hip_search_emit.h")
    assert "DEFINITION OF THE RESULT" in hdr
    for word in ("A CALL IS ALL OR NOTHING", "NOTHING of the call is appended", "CABAC_SEARCH_LOG_OVERFLOW", "ONE GROUP PER CHAIN",
                 "at most one appending group", "CABAC_SEARCH_NO_CHAIN", "EXPANDED STRING", "HEAD AND TAIL SYNTAX", "WAITS FOR THE STREAM TWICE",
                 "2^32 - 1"):
        assert word in hdr, word
    for kind in ("kind 23", "kind 24"):
        assert kind in hdr, kind
    for other in OTHERS:                                                   # the next two free numbers: nobody else has them
        h, _ = _code(other)
        assert "kind 23" not in h and "kind 24" not in h, other


def test_header_compiles_as_c_and_the_structs_are_the_binding_s():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "cabac_hip_search_emit.h"\n'
           "int main(void) { int (*f)(cabac_search_log *, uint32_t, const uint32_t *, const uint32_t *, uint32_t, const uint32_t *,\n"
           "  const cabac_tu_desc *, const void *, int, const uint64_t *, const uint16_t *, const uint32_t *) = cabac_hip_search_log_append_device;\n"
           '  printf("%u %u %d %d %d %d %d %d\\n", CABAC_SEARCH_NO_CHAIN, CABAC_SEARCH_LOG_OVERFLOW, f != 0,\n'
           "         (int)sizeof(cabac_search_log_counters), (int)sizeof(cabac_search_log_entry), (int)sizeof(cabac_search_log_view),\n"
           "         (int)offsetof(cabac_search_log_entry, chain_tu_first), (int)offsetof(cabac_search_log_view, n_chain)); return 0; }\n")
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        obj = os.path.join(tmp, "t.o")
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(H.ROOT, "include"), "-c", c, "-o", obj])
    hdr, _ = _code("cabac_hip_search_emit.h")
    for name, dtype in (("cabac_search_log_counters", capi.LOG_COUNTERS_DTYPE), ("cabac_search_log_entry", capi.LOG_ENTRY_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
        fields = re.findall(r"\b(uint64_t|uint32_t)\s+(\w+);", body)
        assert [f for _, f in fields] == list(dtype.names), name
        assert [np.dtype("<u8" if t == "uint64_t" else "<u4") for t, _ in fields] == [dtype.fields[f][0] for f in dtype.names]
    body = re.search(r"typedef struct cabac_search_log_view \{(.*?)\} cabac_search_log_view;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f for f, _ in capi.SearchLogView._fields_]
    assert capi.SEARCH_NO_CHAIN == 0xFFFFFFFF and capi.SEARCH_LOG_OVERFLOW == 1
    for word, value in (("OVERFLOW", capi.SEARCH_LOG_OVERFLOW), ("OVER_ENTRIES", capi.SEARCH_LOG_OVER_ENTRIES),
                        ("OVER_RECORDS", capi.SEARCH_LOG_OVER_RECORDS), ("OVER_BLOCKS", capi.SEARCH_LOG_OVER_BLOCKS),
                        ("OVER_COEFFS", capi.SEARCH_LOG_OVER_COEFFS), ("OVER_CHAIN_RECORDS", capi.SEARCH_LOG_OVER_CHAIN_RECORDS)):
        assert int(re.search(r"#define CABAC_SEARCH_LOG_%s (0x[0-9a-fA-F]+)u" % word, hdr).group(1), 16) == value, word


def test_python_binding_has_the_methods():
    assert callable(capi.CabacHip.search_log)
    p = inspect.signature(capi.CabacHip.search_log).parameters
    assert [k for k in p][1:6] == ["n_chain", "entry_capacity", "record_capacity", "tu_capacity", "coeff_capacity"]
    for m in ("append_device", "reset", "view", "encode_device", "close", "read", "validate"):
        assert callable(getattr(capi.SearchLog, m)), m
    p = inspect.signature(capi.SearchLog.append_device).parameters
    assert [k for k in p][1:11] == ["n_group", "d_pick", "d_group_chain", "n_cand", "d_cand_first", "d_tu", "d_coeff", "d_rec_first",
                                    "d_records", "d_tu_at"]
    assert p["check"].default is True
    p = inspect.signature(capi.SearchLog.encode_device).parameters
    assert [k for k in p][1:8] == ["d_desc", "d_payload", "payload_capacity", "d_payload_offsets", "d_results", "d_tu_info", "d_bin_counts"]
    L = capi.load_library()
    want = {"cabac_hip_search_log_create": 8, "cabac_hip_search_log_destroy": 1, "cabac_hip_search_log_reset_device": 1,
            "cabac_hip_search_log_append_device": 12, "cabac_hip_search_log_view": 2, "cabac_hip_search_log_encode_device": 8}
    _, code = _code("cabac_hip_search_emit.h")
    for n in NAMES:                                                        # the declarations have as many parameters as the bindings pass
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(getattr(L, n).argtypes) == want[n], n
    # append_device passes the log, its ten arguments and coeff_bytes; encode_device the log and its seven
    assert len(inspect.signature(capi.SearchLog.append_device).parameters) - 1 - 4 + 2 == want["cabac_hip_search_log_append_device"]
    assert len(inspect.signature(capi.SearchLog.encode_device).parameters) == want["cabac_hip_search_log_encode_device"]


def test_the_host_side_validator_refuses_two_groups_on_one_chain():
    ok = capi.SearchLog.validate
    ok([0, 1, 2], [0, 1, 2], 3, 3)
    ok([0, capi.SEARCH_NONE, 2, 5], [1, 1, capi.SEARCH_NO_CHAIN, 1], 3, 3)   # only appending groups count
    ok([0, 1], [7, 7], 3, 3)                                                 # a chain >= n_chain appends nothing
    ok([], [], 3, 3)
    with pytest.raises(ValueError, match="chain 1 is named by 2"):
        ok([0, 1, 2], [1, 0, 1], 3, 3)
    with pytest.raises(ValueError):
        ok([0, 1], [0], 3, 3)
