"""CPU: the public surface of the fixed workspace — include/cabac_hip_workspace.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the six entry points, none of it leaked into the lists the other headers are compared with; the header
includes cabac_hip.h alone, compiles as C99, states the contract the GPU tests check and keeps out of the words the other headers'
tests reserve; the two structs are the size of their dtypes; and cabac_hip_workspace_bound — host arithmetic, no GPU — is never
below the totals the models under tests/ compute for the same input."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np

import helpers as H
import parse_corpus as PC
import plan_rows_model as R
import search_emit_model as E
import splice_rows_model as M
import write_plan_model as WP
from entropy_coding_amd import capi
from test_gpu_search_unit import Case

NAMES = ["cabac_hip_workspace_bound", "cabac_hip_workspace_fix", "cabac_hip_workspace_release", "cabac_hip_workspace_status_device",
         "cabac_hip_workspace_status", "cabac_hip_workspace_waits"]
HEADER = "cabac_hip_workspace.h"
OTHER_LISTS = {"EXPORTS": 44, "EXPORTS_ESTIMATE": 3, "EXPORTS_NAL": 6, "EXPORTS_SEARCH": 5, "EXPORTS_SEARCH_UNIT": 3,
               "EXPORTS_SEARCH_EMIT": 6, "EXPORTS_PARSE_UNIT": 2, "EXPORTS_PARSE_ELEMENTS": 2, "EXPORTS_PARSE_PLAN": 2,
               "EXPORTS_WRITE_PLAN": 2, "EXPORTS_SEARCH_PLAN": 3, "EXPORTS_CTX_SETS": 7, "EXPORTS_PLAN_ROWS": 6, "EXPORTS_SPLICE_ROWS": 6}
# what the other headers' tests reserve for their own header (outside comments)
RESERVED = ("parse_unit", "parse_elements", "parse_plan", "write_plan", "search_plan", "resolve_plan", "search_unit", "estimate_unit",
            "search_log", "search_emit", "ctx_sets", "_wpp_", "ctx_advance", "CABAC_CTX_NO_SET", "plan_parse_", "plan_write_", "PLAN_ROWS",
            "residual_sets", "residual_rows", "log_mark", "log_encode_sets", "log_encode_rows", "SPLICE_ROWS", "CABAC_RES_BAD_SET")
NINE = ["cabac_hip_encode_residual_device", "cabac_hip_encode_residual16_device", "cabac_hip_encode_residual_sets_device",
        "cabac_hip_encode_residual_rows_device", "cabac_hip_write_plan_device", "cabac_hip_plan_write_sets_device",
        "cabac_hip_plan_write_rows_device", "cabac_hip_search_log_encode_device", "cabac_hip_search_log_encode_sets_device",
        "cabac_hip_search_log_encode_rows_device"]                  # the splice pipeline's 16-bit form makes ten names for nine calls


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
    assert declared == sorted(capi.EXPORTS_WORKSPACE) == sorted(NAMES)
    assert all(n.startswith("cabac_hip_workspace_") for n in declared)
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip.h"]
    others = set()
    for name in OTHER_LISTS:
        others |= set(getattr(capi, name))
    assert not set(NAMES) & others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            c = _code(other)[1]
            assert "workspace" not in c and "CABAC_WS_" not in c, other
    for n in NAMES:                                                 # the header's own count of arguments
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(getattr(L, n).argtypes), n


def test_the_lists_of_the_other_headers_are_untouched():
    for name, n in OTHER_LISTS.items():
        assert len(getattr(capi, name)) == n, name
    assert len(capi.EXPORTS_WORKSPACE) == 6


def test_header_keeps_out_of_the_words_the_other_headers_reserve():
    hdr, code = _code(HEADER)
    for word in RESERVED:
        assert word not in code, word
    for kind in range(0, 40):                                       # kinds up to 39 are the other headers'
        assert not re.search(r"kind %d\b" % kind, hdr), kind
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "kind 40" not in _code(other)[0], other


def test_header_compiles_as_c99_on_its_own():
    src = '#include "%s"\nint main(void) { return 0; }\n' % HEADER
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(H.ROOT, "include"), c, "-o",
                               os.path.join(tmp, "t")])


def test_struct_sizes_match_the_dtypes_and_the_flags_the_binding():
    names = ["CABAC_WS_ROWS", "CABAC_WS_OVER_RECORDS", "CABAC_WS_OVER_SLOTS", "CABAC_WS_BAD_SPLICES", "CABAC_WS_RECORDS_32BIT",
             "CABAC_WS_LOG_OVERFLOW", "CABAC_WS_LOG_DAMAGED", "CABAC_WS_NONE_VOIDED"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n' % HEADER + \
        'int main(void) { printf("%zu %zu %zu %zu %zu", sizeof(cabac_workspace_sizes), sizeof(cabac_workspace_status), ' \
        'offsetof(cabac_workspace_sizes, slot_bytes), offsetof(cabac_workspace_sizes, flags), offsetof(cabac_workspace_status, n_voided));' + \
        "".join(' printf(" %%u", (unsigned)%s);' % n for n in names) + " return 0; }\n"
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "t.c"), os.path.join(tmp, "t")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-I" + os.path.join(H.ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    z, s = capi.WORKSPACE_SIZES_DTYPE, capi.WORKSPACE_STATUS_DTYPE
    assert got[:5] == [48, 32, z.fields["slot_bytes"][1], z.fields["flags"][1], s.fields["n_voided"][1]]
    assert (z.itemsize, s.itemsize) == (48, 32)
    assert list(z.names) == ["n_sub", "n_tu", "n_entries", "expanded_records", "slot_bytes", "log_records", "flags", "reserved"]
    assert list(s.names) == ["records_needed", "slot_bytes_needed", "flags", "n_calls", "n_voided", "first_voided"]
    assert got[5:] == [capi.WS_ROWS, capi.WS_OVER_RECORDS, capi.WS_OVER_SLOTS, capi.WS_BAD_SPLICES, capi.WS_RECORDS_32BIT,
                       capi.WS_LOG_OVERFLOW, capi.WS_LOG_DAMAGED, capi.WS_NONE_VOIDED]


def test_header_states_the_contract():
    hdr, code = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for word in ("FIXED WORKSPACE", "no host synchronisation", "no allocation", "no blocking copy", "THE NINE CALLS", "ONCE in the middle",
                 "WAIT FOR THE STREAM TWICE", "does not wait at all", "before anything is queued", "CABAC_HIP_ERR_INVALID",
                 "cabac_hip_last_error", "the waits counter does not move", "A GOOD CALL", "bit for bit", "A VOIDED CALL", "VOIDED",
                 "THE GATE", "tail of the scan kernel", "CABAC_RES_OVERFLOW", "d_payload_offsets[0 .. n_sub]", "no payload byte", "no out set",
                 "no values_out word", "d_values_out == d_values_in", "nothing to the log", "inside their arrays",
                 "THE STATUS IS THE AUTHORITY", "7 bits per record", "tu_capacity", "record_capacity", "descriptors it rejects",
                 "the number of logged blocks", "one word per LOGGED block", "THE HOST-POINTER FORMS", "cabac_hip_workspace_release",
                 "EVERY OTHER ENTRY POINT", "still grows on demand", "STREAM-ORDERED", "CABAC_TU_MAX_RECORDS", "33 n_tu + 38 n_coded_coeff",
                 "24 n_sub", "never decreases", "hipStreamSynchronize", "hipFree", "kind 40"):
        assert word in flat, word
    for n in NINE:                                                  # named, in comments only
        assert n in hdr and n not in code, n


def test_python_binding_has_the_methods_and_the_dtypes():
    for m in NAMES:
        assert callable(getattr(capi.CabacHip, m[len("cabac_hip_"):])), m
    p = [k for k in inspect.signature(capi.CabacHip.workspace_fix).parameters]
    assert p == ["self", "n_sub", "n_tu", "expanded_records", "slot_bytes", "n_entries", "log_records", "rows"]
    L = capi.load_library()
    assert L.cabac_hip_workspace_bound.argtypes[:4] == [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64]


# ---------------------------------------------------------------------------------------------- the bound against the models
def slot_bytes(n):
    """the device's rule (launch_splice_plan / launch_splice_scan): 7 bits per record, 8 bytes, rounded up to 16 per substream"""
    return ((7 * n + 7) // 8 + 8 + 15) // 16 * 16


def _totals(strings):
    return sum(len(s) for s in strings), sum(slot_bytes(len(s)) for s in strings)


def _splice_case(rng):
    """1 .. 4 substreams of helpers.random_records with blocks of every style of parse_corpus.random_tu spliced in"""
    case = Case()
    for s in range(int(rng.integers(1, 5))):
        n_host = int(rng.integers(0, 40))
        run = H.random_records(rng, n_host, ctx_frac=0.6, end_trm=False) if n_host else np.zeros(0, np.uint16)
        items = []
        for _ in range(int(rng.integers(0, 4))):
            (w, h, ch, fl), c = PC.random_tu(rng, PC.MIXED_STYLES[int(rng.integers(0, len(PC.MIXED_STYLES)))])
            items.append((c, ch, fl, int(rng.integers(0, n_host + 1))))
        case.add(run, items)
    case.finish()
    subs = M.subs_of(case)
    return len(subs), len(case.records), len(case.tus), len(case.coeff), [s.string for s in subs]


def _plan_case(rng):
    """1 .. 3 rows of plan_rows_model.tu_row: the expanded strings of write_plan_model's walk"""
    from test_parse_plan_model import TU_OUTCOMES
    rows = [R.tu_row(rng, [TU_OUTCOMES[int(rng.integers(0, len(TU_OUTCOMES)))] for _ in range(int(rng.integers(1, 4)))])
            for _ in range(int(rng.integers(1, 4)))]
    strings = []
    for r in rows:
        stopped = WP.stop_of(r["plan"], r["real"], r["metas"], r["blocks"], r["at"], r["guards"]) != 0
        strings.append(np.zeros(0, np.uint16) if stopped else R.filled(r)[3])
    # no element gives more than 255 context bins and a code word of 64 bypass bins (cabac_hip_parse_elements.h)
    n_bins = 320 * sum(len(r["plan"]) for r in rows)
    return len(rows), n_bins, sum(len(r["blocks"]) for r in rows), sum(b.size for r in rows for b in r["blocks"]), strings


def _log_case(rng):
    """2 .. 4 chains, 1 .. 2 positions of search_emit_model.search_round logged: the chains' expanded strings"""
    K = int(rng.integers(2, 5))
    model = M.MarkedLog(K)
    chain = np.arange(K, dtype=np.uint32)
    for _ in range(int(rng.integers(1, 3))):
        case, gf, _ = E.search_round(rng, K, 3)
        assert model.append(gf[:-1].copy(), chain, case.cand_first, case.tus, case.coeff, case.rec_first, case.records, case.tu_at)
    subs = model.subs()
    n_coeff = sum(E.block_size(d) for d in model.log.tu)
    return K, sum(len(s.side) for s in subs), len(model.log.tu), n_coeff, [s.string for s in subs]


def test_workspace_bound_is_never_below_the_models_totals():
    rng = np.random.default_rng(0xB0C1D)
    builders = [_splice_case, _plan_case, _log_case]

    for i in range(200):
        n_sub, n_host, n_tu, n_coeff, strings = builders[i % 3](rng)
        rec, slots = _totals(strings)
        b_rec, b_slots = capi.workspace_bound(n_sub, n_host, n_tu, n_coeff)
        assert b_rec >= rec and b_slots >= slots, (i, (rec, slots), (b_rec, b_slots))
        assert b_rec == n_host + 33 * n_tu + 38 * n_coeff and b_slots == (7 * b_rec + 7) // 8 + 24 * n_sub, i

    # no block: the record bound is exact; and the slot bound is above the rule for any split of the records over the substreams
    assert capi.workspace_bound(3, 100, 0, 0) == (100, (700 + 7) // 8 + 72)
    for split in ([100, 0, 0], [33, 33, 34], [1, 1, 98], [16, 16, 68]):
        assert sum(slot_bytes(n) for n in split) <= capi.workspace_bound(3, 100, 0, 0)[1]
    assert capi.workspace_bound(0, 0, 0, 0) == (0, 0)
