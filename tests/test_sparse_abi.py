"""CPU: the public surface of the sparse coefficient transport — include/cabac_hip_sparse.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the six entry points, none of it leaked into the lists the other headers are compared with; the
header includes cabac_hip.h alone, compiles as C99, states the format and the four identities the tests check, and keeps out of
the words the other headers' tests reserve; the status struct has the size of its dtype and the flags are the binding's."""
import os
import re
import subprocess
import tempfile

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_sparse_pack_host", "cabac_hip_sparse_unpack_host", "cabac_hip_sparse_expand_device",
         "cabac_hip_sparse_compact_device", "cabac_hip_sparse_encode_batch", "cabac_hip_sparse_parse_batch"]
HEADER = "cabac_hip_sparse.h"
OTHER_LISTS = {"EXPORTS": 44, "EXPORTS_ESTIMATE": 3, "EXPORTS_NAL": 6, "EXPORTS_SEARCH": 5, "EXPORTS_SEARCH_UNIT": 3,
               "EXPORTS_SEARCH_EMIT": 6, "EXPORTS_PARSE_UNIT": 2, "EXPORTS_PARSE_ELEMENTS": 2, "EXPORTS_PARSE_PLAN": 2,
               "EXPORTS_WRITE_PLAN": 2, "EXPORTS_SEARCH_PLAN": 3, "EXPORTS_CTX_SETS": 7, "EXPORTS_PLAN_ROWS": 6, "EXPORTS_SPLICE_ROWS": 6,
               "EXPORTS_WORKSPACE": 6}
# what the other headers' tests reserve for their own header (outside comments)
RESERVED = ("workspace", "CABAC_WS_", "cabac_hip_search", "CABAC_SEARCH", "parse_unit", "parse_elements", "parse_plan", "write_plan",
            "search_plan", "resolve_plan", "search_unit", "estimate_unit", "search_log", "search_emit", "ctx_sets", "_wpp_", "ctx_advance",
            "CABAC_CTX_NO_SET", "plan_parse_", "plan_write_", "PLAN_ROWS", "residual_sets", "residual_rows", "log_mark", "log_encode_sets",
            "log_encode_rows", "SPLICE_ROWS", "CABAC_RES_BAD_SET")


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
    assert declared == sorted(capi.EXPORTS_SPARSE) == sorted(NAMES)
    assert all(n.startswith("cabac_hip_sparse_") for n in declared)
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip.h"]
    others = set()
    for name in OTHER_LISTS:
        others |= set(getattr(capi, name))
    assert not set(NAMES) & others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            c = _code(other)[1]
            assert "cabac_hip_sparse" not in c and "CABAC_SPARSE_" not in c, other
    for n in NAMES:                                                 # the header's own count of arguments
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(getattr(L, n).argtypes), n


def test_the_lists_of_the_other_headers_are_untouched():
    for name, n in OTHER_LISTS.items():
        assert len(getattr(capi, name)) == n, name
    assert len(capi.EXPORTS_SPARSE) == 6


def test_header_keeps_out_of_the_words_the_other_headers_reserve():
    hdr, code = _code(HEADER)
    for word in RESERVED:
        assert word not in code, word
    for kind in range(0, 41):                                       # kinds up to 40 are the other headers'
        assert not re.search(r"kind %d\b" % kind, hdr), kind
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "kind 41" not in _code(other)[0] and "kind 42" not in _code(other)[0], other


def test_header_compiles_as_c99_on_its_own():
    src = '#include "%s"\nint main(void) { return 0; }\n' % HEADER
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(H.ROOT, "include"), c, "-o",
                               os.path.join(tmp, "t")])


def test_struct_size_matches_the_dtype_and_the_flags_the_binding():
    names = ["CABAC_SPARSE_OVERFLOW", "CABAC_SPARSE_RANGE", "CABAC_SPARSE_BAD_POS", "CABAC_SPARSE_BAD_FIRST", "CABAC_SPARSE_BAD_BLOCK",
             "CABAC_SPARSE_NO_BAD"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n' % HEADER + \
        'int main(void) { printf("%zu %zu %zu", sizeof(cabac_sparse_status), offsetof(cabac_sparse_status, flags), ' \
        'offsetof(cabac_sparse_status, first_bad));' + \
        "".join(' printf(" %%u", (unsigned)%s);' % n for n in names) + " return 0; }\n"
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "t.c"), os.path.join(tmp, "t")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-I" + os.path.join(H.ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    z = capi.SPARSE_STATUS_DTYPE
    assert got[:3] == [16, z.fields["flags"][1], z.fields["first_bad"][1]] and z.itemsize == 16
    assert list(z.names) == ["n_entries", "flags", "first_bad"]
    assert got[3:] == [capi.SPARSE_OVERFLOW, capi.SPARSE_RANGE, capi.SPARSE_BAD_POS, capi.SPARSE_BAD_FIRST, capi.SPARSE_BAD_BLOCK,
                       capi.SPARSE_NO_BAD]
    assert got[3:8] == [1, 2, 4, 8, 16]


def test_header_states_the_format_and_the_identities():
    hdr, code = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for word in ("DEFINITION OF THE RESULT", "S1.", "S2.", "S3.", "S4.", "kind 41", "kind 42", "coefficient expand", "coefficient compact",
                 "pos | (uint32_t)(uint16_t)level << 16", "ascending from 0", "max_log2_tr_range above 15", "0xFFFFFFFF", "EXPAND", "COMPACT",
                 "one is taken", "ascending pos", "are not read", "stored truncated", "nothing is written past the capacity",
                 "no host synchronisation", "no workgroup waits for another", "sized from n_tu alone", "must not overlap", "2^32",
                 "CABAC_TU_INFO_EMPTY", "status->n_entries telling the need", "cabac_hip_workspace_waits"):
        assert word in flat, word
    for n in ("cabac_hip_encode_batch_residual16", "cabac_hip_residual_parse_batch16"):   # named, in comments only
        assert n in hdr and n not in code, n


def test_python_binding_has_the_functions_and_the_methods():
    assert callable(capi.sparse_pack_host) and callable(capi.sparse_unpack_host)
    for m in ("sparse_expand_device", "sparse_compact_device", "sparse_encode_batch", "sparse_parse_batch"):
        assert callable(getattr(capi.CabacHip, m)), m
