"""CPU: the public surface of the pieces calls — include/cabac_hip_pieces.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the two entry points; the coder state is 32 bytes with its four documented words in front; the
header compiles as C99 on its own and states the definitions the GPU tests check; without a context the calls fail loudly."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_encode_pieces_device", "cabac_hip_decode_pieces_device"]
HEADER = "cabac_hip_pieces.h"


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
    assert declared == sorted(capi.EXPORTS_PIECES) == sorted(NAMES)
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip.h"]
    others = set()
    for name in dir(capi):
        if name.startswith("EXPORTS") and name != "EXPORTS_PIECES":
            others |= set(getattr(capi, name))
    assert not set(NAMES) & others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            c = _code(other)[1]
            assert "_pieces_" not in c and "cabac_coder_state" not in c and "CABAC_RES_BAD_STATE" not in c, other


def test_the_struct_is_32_bytes_with_the_documented_words_in_front():
    src = ('#include "%s"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) { printf("%%u %%u %%u %%u %%u %%u %%u %%u %%u %%u\\n", '
           "(unsigned)sizeof(cabac_coder_state), (unsigned)offsetof(cabac_coder_state, kind), (unsigned)offsetof(cabac_coder_state, flags), "
           "(unsigned)offsetof(cabac_coder_state, bits), (unsigned)offsetof(cabac_coder_state, bytes_final), CABAC_CODER_FRESH, "
           "CABAC_CODER_ENC, CABAC_CODER_DEC, CABAC_CODER_CLOSED, CABAC_RES_BAD_STATE); return 0; }\n" % HEADER)
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(tmp, "t")
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(H.ROOT, "include"), c, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert out == [32, 0, 4, 8, 12, 0, 1, 2, 3, 0x80]
    dt = capi.CODER_STATE_DTYPE
    assert dt.itemsize == 32
    assert [dt.fields[k][1] for k in ("kind", "flags", "bits", "bytes_final", "priv")] == [0, 4, 8, 12, 16]
    assert (capi.CODER_FRESH, capi.CODER_ENC, capi.CODER_DEC, capi.CODER_CLOSED) == (0, 1, 2, 3)
    assert not np.zeros(1, dt).tobytes().strip(b"\0"), "an all-zero struct is start()"
    # the flag is a bit of its own among the result flags: the next free one
    assert capi.RES_BAD_STATE == 0x80
    assert not capi.RES_BAD_STATE & (capi.RES_OVERFLOW | capi.RES_BAD_RECORD | capi.RES_UNDERRUN | capi.RES_BAD_STOP | capi.RES_RANGE |
                                     capi.RES_BAD_VALUE | capi.RES_BAD_SET)


def test_header_states_the_definitions():
    hdr, _ = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for words in ("DEFINITION OF THE RESULT", "consecutive runs of its records", "WITHOUT CABAC_SUB_FINISH", "Nothing is flushed",
                  "WITH CABAC_SUB_FINISH", "CABAC_CODER_CLOSED", "n_records == 0 is legal", "P1, encode", "P2, decode", "P3:",
                  "pieces of one record included", "FLAGS ARE STICKY", "returns {0, flags} and copies the state",
                  "bytes_final + 2 (buffered and outstanding units) > byte_capacity",
                  "unspecified inside its slot", "nothing outside the slot is ever written", "A STATE IS DATA FROM MEMORY",
                  "before any loop that depends on it", "{0, CABAC_RES_BAD_STATE}", "range outside 256..510", "pend > 15",
                  "low >= 2^(10 + pend)", "bits != 8 bytes_final + 16 nbuf + pend", "an odd bytes_final",
                  "a value not below range << 7", "ignore cabac_hip_set_variant", "They allocate nothing, wait for nothing",
                  "CABAC_SUB_PROBE itself is ignored", "kind 48", "kind 49", "d_coder_in", "May be d_coder_in", "Not covered"):
        assert words in flat, words
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            for kind in ("kind 48", "kind 49"):
                assert kind not in _code(other)[0], (other, kind)
    # the header says itself what CABAC_SUB_FINISH means here (cabac_hip.h is one of the files the prebuilt reference adapters
    # under oracle/_ref are pinned to by hash, oracle/Makefile ADAPTER_SRCS, and stays as it is)
    assert "one call" in flat and "cabac_hip.h" in flat


def test_python_binding_has_the_methods_and_without_a_context_the_calls_fail():
    for m in ("encode_pieces_device", "decode_pieces_device"):
        assert callable(getattr(capi.CabacHip, m)), m
    p = [k for k in inspect.signature(capi.CabacHip.encode_pieces_device).parameters]
    assert p[1:5] == ["n_sub", "d_desc", "d_records", "d_bytes"] and p[-2:] == ["d_coder_in", "d_coder_out"]
    p = [k for k in inspect.signature(capi.CabacHip.decode_pieces_device).parameters]
    assert p[5] == "d_bins" and p[-2:] == ["d_coder_in", "d_coder_out"]
    L = capi.load_library()
    assert len(L.cabac_hip_encode_pieces_device.argtypes) == 15 and len(L.cabac_hip_decode_pieces_device.argtypes) == 16
    # no context, no call: an error code, never a quiet return
    assert L.cabac_hip_encode_pieces_device(*([None, 1] + [None] * 4 + [0] + [None] * 8)) < 0
    assert L.cabac_hip_decode_pieces_device(*([None, 1] + [None] * 5 + [0] + [None] * 8)) < 0
    import torch
    if not torch.cuda.is_available():       # and no context without a GPU: there is no CPU path behind these calls
        with pytest.raises(capi.CabacHipError):
            capi.CabacHip(0)
