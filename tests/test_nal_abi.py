"""CPU: the public surface of the emulation prevention — include/cabac_hip_nal.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the five cabac_hip_nal_* calls and cabac_hip_encode_batch_nal."""
import ctypes
import os
import re
import subprocess
import tempfile

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_nal_escape_bound", "cabac_hip_nal_escape_device", "cabac_hip_nal_unescape_device",
         "cabac_hip_nal_escape_batch", "cabac_hip_nal_unescape_batch", "cabac_hip_encode_batch_nal"]


def _header():
    return open(os.path.join(H.ROOT, "include", "cabac_hip_nal.h")).read()


def test_header_declares_library_exports_and_binding_lists_the_entry_points():
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = capi.load_library()
    for n in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % n, code), n
        assert hasattr(L, n), n
    declared = sorted(set(re.findall(r"\b(cabac_hip_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(capi.EXPORTS_NAL) == sorted(NAMES)
    assert '#include "cabac_hip.h"' in hdr
    # the walks are the contract (VTM's NALread is not what is restated), and the profile kinds are listed
    assert "DEFINITION OF THE RESULT" in hdr and "not VTM" in hdr and "kind 13" in hdr and "kind 14" in hdr
    # nothing of it leaked into the list tests/test_cabi_exports.py compares with cabac_hip.h
    assert not set(NAMES) & set(capi.EXPORTS)


def test_status_struct_is_16_bytes_and_matches_the_dtype():
    d = capi.NAL_STATUS_DTYPE
    assert d.itemsize == 16 and [d.fields[k][1] for k in ("out_bytes", "n_changed", "flags")] == [0, 8, 12]
    # the compiler's view of the header
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "cabac_hip_nal.h"\nint main(void) { printf("%zu %zu %zu %zu %u %u\\n", '
           "sizeof(cabac_nal_status), offsetof(cabac_nal_status, out_bytes), offsetof(cabac_nal_status, n_changed), "
           "offsetof(cabac_nal_status, flags), CABAC_NAL_OVERFLOW | CABAC_NAL_TRAILING_ZERO | CABAC_NAL_FORBIDDEN | CABAC_NAL_BAD_ESCAPE, "
           "CABAC_NAL_LOC_OVERFLOW | CABAC_NAL_INPUT_CLIPPED); return 0; }\n")
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(tmp, "t")
        subprocess.check_call(["cc", "-std=c99", "-I" + os.path.join(H.ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe], text=True).split()
    assert out == ["16", "0", "8", "12", "15", "48"]
    assert (capi.NAL_OVERFLOW, capi.NAL_TRAILING_ZERO, capi.NAL_FORBIDDEN, capi.NAL_BAD_ESCAPE, capi.NAL_LOC_OVERFLOW,
            capi.NAL_INPUT_CLIPPED) == (1, 2, 4, 8, 16, 32)


def test_escape_bound():
    L = capi.load_library()
    assert L.cabac_hip_nal_escape_bound.restype is ctypes.c_size_t
    for n, want in ((0, 0), (1, 1), (2, 3), (3, 4), (5, 7), (10 ** 9, 1500000000)):
        assert capi.nal_escape_bound(n) == want


def test_python_binding_has_the_methods():
    import inspect
    for m in ("nal_escape_device", "nal_unescape_device", "nal_escape_batch", "nal_unescape_batch", "encode_batch_nal"):
        assert callable(getattr(capi.CabacHip, m)), m
    p = inspect.signature(capi.CabacHip.nal_unescape_device).parameters
    assert p["d_locations"].default == 0 and p["loc_capacity"].default == 0 and p["loc_base"].default == 0
