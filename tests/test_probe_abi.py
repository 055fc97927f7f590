"""CPU: the public surface of the probe points — include/cabac_hip_probe.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the six entry points, none of it leaked into the lists the other headers are compared with, the
header compiles as C99 on its own and states the definitions the GPU tests check."""
import inspect
import os
import re
import subprocess
import tempfile

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_written_bits_device", "cabac_hip_estimate_probes_device", "cabac_hip_encode_residual_probes_device",
         "cabac_hip_written_bits_batch", "cabac_hip_estimate_probes_batch", "cabac_hip_encode_residual_probes_batch"]
HEADER = "cabac_hip_probe.h"


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
    assert declared == sorted(capi.EXPORTS_PROBE) == sorted(NAMES)
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip.h"]
    others = set()
    for name in dir(capi):
        if name.startswith("EXPORTS") and name != "EXPORTS_PROBE":
            others |= set(getattr(capi, name))
    assert not set(NAMES) & others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            c = _code(other)[1]
            assert "probes" not in c and "written_bits" not in c and "PROBE_H" not in c, other


def test_cabac_hip_h_is_untouched_by_the_probes():
    _, code = _code("cabac_hip.h")
    declared = sorted(set(re.findall(r"\b(cabac_(?:hip|synth)_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(capi.EXPORTS) and len(capi.EXPORTS) == 44


def test_header_compiles_as_c99_alone():
    src = '#include "%s"\nint main(void) { return sizeof(&cabac_hip_written_bits_device) == 0; }\n' % HEADER
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(H.ROOT, "include"), c])


def test_header_states_the_definitions():
    hdr, _ = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for words in ("PROBE LISTS", "n_sub + 1 ascending uint32_t, starting at 0", "after the first k records", "k is clipped to n_records",
                  "non-decreasing", "duplicates are allowed", "n_probe == 0 is fine", "DEFINITION OF THE RESULT",
                  "results[s].n_bits of cabac_hip_encode_device with CABAC_SUB_PROBE on substream s cut to its first k records",
                  "cabac_hip_encode_sets_device", "getNumWrittenBits()", "k = 0 gives 0", "no byte is written",
                  "only rec_offset, n_records, qp and init_id & 3", "CABAC_CTX_NO_SET means Ctx::init", "CABAC_RES_BAD_RECORD",
                  "CABAC_RES_BAD_SET", "values are unspecified", "they are 0", "nothing outside the arguments is touched",
                  "what cabac_hip_estimate_device answers for substream s cut to its first k records",
                  "cabac_hip_estimate_from_device", "CABAC_REC_ALIGN, CABAC_REC_EST_RESETBITS and CABAC_REC_EST_RESTART act exactly as there",
                  "k host records in front, and m of the substream's splices in front", "[#{at < k}, #{at <= k}]",
                  "d_probe_splice == NULL means the upper end", "EXPANDED string", "bit-identical to the plain call's",
                  "no host wait is added", "CABAC_HIP_ERR_INVALID with nothing queued", "nothing run and no output touched",
                  "CABAC_HIP_ERR_SUBSTREAM", "kind 45", "kind 46", "kind 47", "needs no carry state"):
        assert words in flat, words
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            for kind in ("kind 45", "kind 46", "kind 47"):
                assert kind not in _code(other)[0], (other, kind)


def test_python_binding_has_the_methods():
    for m in ("written_bits_device", "estimate_probes_device", "encode_residual_probes_device", "written_bits_batch",
              "estimate_probes_batch", "encode_residual_probes_batch"):
        assert callable(getattr(capi.CabacHip, m)), m
    p = [k for k in inspect.signature(capi.CabacHip.written_bits_device).parameters]
    assert p[1:8] == ["n_sub", "d_desc", "d_records", "d_probe_first", "d_probe_at", "n_probe", "d_bits"]
    L = capi.load_library()
    assert len(L.cabac_hip_written_bits_device.argtypes) == 13 and len(L.cabac_hip_estimate_probes_device.argtypes) == 13
    assert len(L.cabac_hip_written_bits_batch.argtypes) == 14 and len(L.cabac_hip_estimate_probes_batch.argtypes) == 14
    assert len(L.cabac_hip_encode_residual_probes_device.argtypes) == 22
    assert len(L.cabac_hip_encode_residual_probes_batch.argtypes) == 23
