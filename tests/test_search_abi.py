"""CPU: the public surface of the search rounds — include/cabac_hip_search.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds cabac_hip_estimate_residual_ctx_device / _ctx16_device, cabac_hip_search_select_device,
cabac_hip_search_round_device and cabac_hip_search_round_batch; the two pinned headers declare what they declared before."""
import inspect
import os
import re
import subprocess
import tempfile

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_estimate_residual_ctx_device", "cabac_hip_estimate_residual_ctx16_device", "cabac_hip_search_select_device",
         "cabac_hip_search_round_device", "cabac_hip_search_round_batch"]


def _code(name):
    hdr = open(os.path.join(H.ROOT, "include", name)).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_library_exports_and_binding_lists_the_entry_points():
    hdr, code = _code("cabac_hip_search.h")
    L = capi.load_library()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
        assert hasattr(L, n), n
    declared = sorted(set(re.findall(r"\b(cabac_hip_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(capi.EXPORTS_SEARCH) == sorted(NAMES)
    assert '#include "cabac_hip.h"' in hdr
    # the result and the in-place rule are defined in the header, and the profile kinds are listed
    assert "DEFINITION OF THE RESULT" in hdr and "IN-PLACE RULE" in hdr
    for kind in ("kind 15", "kind 16", "kind 17", "kind 18"):
        assert kind in hdr, kind
    # nothing of it leaked into the lists the other headers are compared with
    assert not set(NAMES) & (set(capi.EXPORTS) | set(capi.EXPORTS_ESTIMATE) | set(capi.EXPORTS_NAL))


def test_the_pinned_headers_declare_what_they_declared_before():
    _, code = _code("cabac_hip.h")
    declared = sorted(set(re.findall(r"\b(cabac_(?:hip|synth)_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(capi.EXPORTS) and len(declared) == 44
    _, code = _code("cabac_hip_estimate.h")
    declared = sorted(set(re.findall(r"\b(cabac_hip_[a-z0-9_]+)\s*\(", code)))
    assert declared == ["cabac_hip_estimate_residual16_device", "cabac_hip_estimate_residual_batch", "cabac_hip_estimate_residual_device"]
    assert declared == sorted(capi.EXPORTS_ESTIMATE)
    assert "cabac_hip_search" not in code and "CABAC_SEARCH" not in code


def test_header_compiles_as_c_and_the_sentinels_are_all_ones():
    src = ('#include <stdio.h>\n#include "cabac_hip_search.h"\nint main(void) { printf("%u %u\\n", CABAC_SEARCH_NO_SET, CABAC_SEARCH_NONE); '
           "return 0; }\n")
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(tmp, "t")
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(H.ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe], text=True).split()
    assert out == ["4294967295", "4294967295"]
    assert capi.SEARCH_NO_SET == capi.SEARCH_NONE == 0xFFFFFFFF


def test_python_binding_has_the_methods():
    for m in ("estimate_residual_ctx_device", "search_select_device", "search_round_device", "search_round_batch"):
        assert callable(getattr(capi.CabacHip, m)), m
    p = inspect.signature(capi.CabacHip.search_round_batch).parameters
    assert [k for k in p][1:11] == ["group_first", "cand_first", "tus", "coeff", "state", "rate", "sets", "group_out_set", "dist",
                                    "lambda_q16"]
    assert p["int16"].default is False and p["with_blocks"].default is False and p["check"].default is True
    p = inspect.signature(capi.CabacHip.estimate_residual_ctx_device).parameters
    assert [k for k in p][9:12] == ["d_out_set", "d_out_state", "d_out_rate"] and p["int16"].default is False
    L = capi.load_library()
    assert len(L.cabac_hip_search_round_device.argtypes) == 19 and len(L.cabac_hip_search_round_batch.argtypes) == 21
    assert len(L.cabac_hip_estimate_residual_ctx_device.argtypes) == 14 and len(L.cabac_hip_search_select_device.argtypes) == 8
