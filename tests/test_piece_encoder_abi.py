"""CPU: the public surface of the piece encoder setting — include/cabac_hip_piece_encoder.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the two entry points; the header compiles as C99 on its own, keeps to its own words, and states the
definitions the GPU tests check (tests/test_gpu_piece_encoder.py); without a context the calls fail loudly."""
import inspect
import os
import re
import subprocess
import tempfile

import pytest

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_piece_encoder_set", "cabac_hip_piece_encoder_get"]
HEADER = "cabac_hip_piece_encoder.h"


def _code(name):
    hdr = open(os.path.join(H.ROOT, "include", name)).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_library_exports_and_binding_lists_the_entry_points():
    _, code = _code(HEADER)
    L = capi.load_library()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
        assert hasattr(L, n), n
    declared = sorted(set(re.findall(r"\b(cabac_hip_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(capi.EXPORTS_PIECE_ENCODER) == sorted(NAMES)
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip.h"]
    others = set()
    for name in dir(capi):
        if name.startswith("EXPORTS") and name != "EXPORTS_PIECE_ENCODER":
            others |= set(getattr(capi, name))
    assert not set(NAMES) & others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "piece_encoder" not in _code(other)[1].lower(), other
    # the pieces header keeps declaring exactly its two calls
    assert sorted(set(re.findall(r"\b(cabac_hip_[a-z0-9_]+)\s*\(", _code("cabac_hip_pieces.h")[1]))) == sorted(capi.EXPORTS_PIECES)


def test_header_compiles_alone_as_c99():
    src = ('#include "%s"\nint main(void) { return cabac_hip_piece_encoder_get((const cabac_hip_ctx *)0) < 0 ? 0 : 1; }\n' % HEADER)
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(H.ROOT, "include"), "-c", c,
                               "-o", os.path.join(tmp, "t.o")])


def test_header_states_the_definitions():
    hdr, code = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for words in ("D1: under every setting the bytes in the slots, the results, the out sets and all 32 bytes of every out state are those of setting 4",
                  "for every way of cutting", "D2: therefore a state written under one setting continues under any other",
                  "THE DEFAULT IS 4", "ANY OTHER VALUE IS REFUSED with CABAC_HIP_ERR_INVALID and changes nothing",
                  "0 by the batch", "results never depend on it", "WHICH CALLS FOLLOW THE SETTING",
                  "cabac_hip_encode_pieces_device", "the encode leg of cabac_hip_plan_continue_write_device", "and nothing else",
                  "keep ignoring cabac_hip_set_variant", "cabac_hip_decode_pieces_device does not look at it",
                  "read before the first workgroup barrier", "written behind the last",
                  "NOT COVERED: the v6 encoder, the decoders", "the splice pipeline", "the winner log", "host-pointer forms", "the C++ shim"):
        assert words in flat, words
    # what the other headers' tests forbid outside their own header: their words in this one's code, their kinds anywhere in it
    for word in ("_pieces_", "cabac_coder_state", "CABAC_RES_BAD_STATE", "plan_continue", "plan_resume"):
        assert word not in code, word
    assert not re.search(r"kind \d", hdr)


def test_python_binding_has_the_methods_and_without_a_context_the_calls_fail():
    for m in ("piece_encoder_set", "piece_encoder_get"):
        assert callable(getattr(capi.CabacHip, m)), m
    assert [k for k in inspect.signature(capi.CabacHip.piece_encoder_set).parameters] == ["self", "variant"]
    L = capi.load_library()
    assert len(L.cabac_hip_piece_encoder_set.argtypes) == 2 and len(L.cabac_hip_piece_encoder_get.argtypes) == 1
    # no context, no call: an error code, never a quiet return
    for v in (4, 7, 0, 5):
        assert L.cabac_hip_piece_encoder_set(None, v) == -2      # CABAC_HIP_ERR_INVALID
    assert L.cabac_hip_piece_encoder_get(None) < 0
    import torch
    if not torch.cuda.is_available():       # and no context without a GPU: there is no CPU path behind these calls
        with pytest.raises(capi.CabacHipError):
            capi.CabacHip(0)
