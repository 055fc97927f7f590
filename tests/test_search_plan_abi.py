"""CPU: the public surface of the search rounds over plans — include/cabac_hip_search_plan.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the three entry points, none of it leaked into the lists the other headers are compared with, and
the header states the contract the GPU tests check."""
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np

import helpers as H
from entropy_coding_amd import capi

NAMES = ["cabac_hip_resolve_plan_device", "cabac_hip_search_plan_round_device", "cabac_hip_search_plan_round_batch"]
HEADER = "cabac_hip_search_plan.h"


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
    assert declared == sorted(capi.EXPORTS_SEARCH_PLAN) == sorted(NAMES)
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip_search_unit.h"]
    others = (set(capi.EXPORTS) | set(capi.EXPORTS_ESTIMATE) | set(capi.EXPORTS_NAL) | set(capi.EXPORTS_SEARCH) |
              set(capi.EXPORTS_SEARCH_UNIT) | set(capi.EXPORTS_SEARCH_EMIT) | set(capi.EXPORTS_PARSE_UNIT) |
              set(capi.EXPORTS_PARSE_ELEMENTS) | set(capi.EXPORTS_PARSE_PLAN) | set(capi.EXPORTS_WRITE_PLAN))
    assert not set(NAMES) & others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            c = _code(other)[1]
            assert "search_plan" not in c and "resolve_plan" not in c, other
    for word in ("write_plan", "parse_plan", "parse_unit", "parse_elements"):
        assert word not in code, word                              # what the other headers' tests forbid outside their own header
    for word in ("kind 23", "kind 24", "kind 25", "kind 26", "kind 27", "kind 28"):
        assert word not in hdr, word


def test_header_states_the_contract():
    hdr, _ = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for word in ("kind 29", "plan resolve", "5, 29, 20, 21, 22", "CABAC_RES_BAD_VALUE", "CABAC_RES_BAD_RECORD", "CABAC_RES_OVERFLOW",
                 "STREAM ORDERING CONTRACT", "IN-PLACE RULE", "INCLUDE THAT HEADER FIRST", "cabac_hip_parse_elements.h",
                 "cabac_hip_parse_plan.h", "no host wait inside", "exactly one flag", "takes precedence over CABAC_RES_BAD_VALUE",
                 "CAPACITY IS ALL OR NOTHING PER CALL", "nothing is written to d_records", "every d_rec_first entry is 0",
                 "d_total still reports the need", "it cannot know", "EMPTY RUN", "log2_width = log2_height = 7", "coeff_offset is kept",
                 "may equal d_values_in", "FILLED values", "counted in RECORDS", "counts ENTRIES", "cabac_hip_binarize_device",
                 "cabac_hip_estimate_unit_device", "cabac_hip_search_unit_round_device", "cabac_hip_search_log_append_device",
                 "CABAC_TU_INFO_TS", "CABAC_TU_INFO_NOT_CODED", "CABAC_TU_INFO_EMPTY", "CABAC_TU_INFO_BAD_DESC",
                 "d_frac_bits = UINT64_MAX", "d_tu_frac_bits of a skipped block is 0", "THE MOST BINS", "CTX_BIN, TRM, ALIGN 1",
                 "EP_BINS numBins", "UNARY_MAX maxSymbol", "UNARY_EP maxSymbol", "TRUNC_BIN floor(log2(maxSymbol)) + 1",
                 "EXP_GOLOMB 63 - count", "REM_ABS max(32, cutoff + rice + max(0, 2 (32 - cutoff - maxLog2TrDR) - 1))",
                 "A CAPACITY THAT ALWAYS SUFFICES: 255 records per plan entry", "FROM THE BOUND", "names the candidate and the entry, or the block"):
        assert word in flat, word
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "kind 29" not in _code(other)[0], other


def test_header_compiles_as_c_behind_the_two_parse_headers_and_alone():
    src = ('#include <stdio.h>\n#include "cabac_hip_parse_elements.h"\n#include "cabac_hip_parse_plan.h"\n#include "%s"\n'
           "int main(void) { int (*f)(cabac_hip_ctx *, uint32_t, const uint32_t *, const uint64_t *, const uint32_t *, const uint32_t *,\n"
           "  uint32_t, const cabac_tu_desc *, const uint32_t *, const uint32_t *, const void *, int, uint64_t *, uint16_t *, uint64_t,\n"
           "  uint32_t *, cabac_tu_desc *, uint32_t *, uint32_t *, uint32_t *, uint64_t *) = cabac_hip_resolve_plan_device;\n"
           "  int (*g)(cabac_hip_ctx *, uint32_t, const uint32_t *, uint32_t, const uint32_t *, uint32_t, const cabac_tu_desc *,\n"
           "  const void *, int, uint32_t *, uint8_t *, const uint32_t *, const uint64_t *, const uint32_t *, const uint32_t *,\n"
           "  const uint32_t *, const uint32_t *, const uint32_t *, const uint64_t *, uint64_t, uint64_t *, uint32_t *, uint64_t *,\n"
           "  uint64_t *, uint32_t *, uint32_t *, uint64_t *, uint16_t *, uint64_t, uint32_t *, cabac_tu_desc *, uint32_t *,\n"
           "  uint64_t *) = cabac_hip_search_plan_round_device;\n"
           '  printf("%%d %%d %%u %%u %%u\\n", f != 0, g != 0, CABAC_RES_BAD_VALUE, CABAC_PE_COND_WORD0(CABAC_JOIN_AND, 1), CABAC_SEARCH_NONE);\n'
           "  return 0; }\n" % HEADER)
    alone = '#include "%s"\nint main(void) { return cabac_hip_search_plan_round_batch == 0; }\n' % HEADER
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in (("t.c", src), ("u.c", alone)):          # behind the parse headers, and on its own
            c = os.path.join(tmp, name)
            open(c, "w").write(text)
            subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-address", "-I" + os.path.join(H.ROOT, "include"), c, "-c",
                                   "-o", os.path.join(tmp, name + ".o")])


def test_declarations_have_as_many_parameters_as_the_bindings_pass():
    L = capi.load_library()
    _, code = _code(HEADER)
    want = {"cabac_hip_resolve_plan_device": 21, "cabac_hip_search_plan_round_device": 33, "cabac_hip_search_plan_round_batch": 29}
    for n in NAMES:
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(getattr(L, n).argtypes) == want[n], n
    p = inspect.signature(capi.CabacHip.resolve_plan_device).parameters
    assert list(p)[:17] == ["self", "n_cand", "d_cand_first", "d_ent_first", "d_plan", "d_values_in", "n_tu", "d_tu", "d_tu_at",
                            "d_tu_guard", "d_coeff", "d_rec_first", "d_records", "record_capacity", "d_tu_at_out", "d_tu_out", "d_flags"]
    assert [p[k].default for k in ("d_values_out", "d_tu_info", "d_total", "int16")] == [0, 0, 0, False]
    q = inspect.signature(capi.CabacHip.search_plan_round_device).parameters
    assert list(q)[:11] == ["self", "n_group", "d_group_first", "n_cand", "d_cand_first", "n_tu", "d_tu", "d_coeff", "d_state", "d_rate",
                            "d_set"]
    assert [q[k].default for k in ("d_tu_frac_bits", "d_tu_info", "d_flags", "d_values_out", "d_total", "int16")] == [0] * 5 + [False]
    r = inspect.signature(capi.CabacHip.search_plan_round_batch).parameters
    assert list(r)[:13] == ["self", "group_first", "cand_first", "tus", "coeff", "state", "rate", "sets", "plan", "values", "ent_first",
                            "tu_at", "tu_guard"]


def test_profile_kind_is_listed_in_the_binding():
    assert "29 plan resolve in cabac_hip_search_plan.h" in " ".join(capi.CabacHip.profile_read.__doc__.split())


def test_without_a_gpu_the_context_refuses():
    """No GPU: the binding raises CabacHipError (CABAC_HIP_ERR_NO_DEVICE), it does not fall back to anything.  Where there is one
    the same call — no group, no candidate — answers nothing, and the batch form's refusals that need no kernel are checked: each
    returns CABAC_HIP_ERR_INVALID and names what it refuses."""
    el, gd = capi.element, capi.guard
    state, rate = np.zeros(capi.NUM_CTX, np.uint32), np.zeros(capi.NUM_CTX, np.uint8)
    empty = ([0], [0], np.zeros(0, capi.TU_DTYPE), np.zeros(0, np.int32), state, rate, [], np.zeros((0, 2), np.uint32), [], [0], None, None,
             None, None, 1 << 16)
    try:
        hip = capi.CabacHip()
    except capi.CabacHipError as e:
        assert e.status == -1
        return
    try:
        bits, pick, cost, flags, filled = hip.search_plan_round_batch(*empty)
        assert len(bits) == len(pick) == len(cost) == len(flags) == len(filled) == 0
        tus = np.zeros(1, capi.TU_DTYPE)
        tus["log2_width"] = tus["log2_height"] = 2
        coeff = np.ones(16, np.int32)
        ok = dict(group_first=[0, 1], cand_first=[0, 1], tus=tus, coeff=coeff, state=state, rate=rate, sets=[0],
                  plan=np.array([[el(0, ctx=5), 0], [el(0, ctx=6), gd(1)]], np.uint32), values=[1, 0], ent_first=[0, 2], tu_at=[1],
                  tu_guard=[gd(1)], group_out_set=None, dist=None, lambda_q16=1 << 16)
        for change, word in ((dict(ent_first=[2, 0]), "ent_first is not non-decreasing"),
                             (dict(ent_first=[0, 3]), "ent_first ends past n_entries_total"),
                             (dict(tu_at=[3]), "tu_at exceeds the candidate's plan length"),
                             (dict(tu_guard=[gd(2)]), "bad block guard: candidate 0, block 0"),
                             (dict(plan=np.array([[el(0, ctx=5), 0], [15, 0]], np.uint32)), "bad plan entry: candidate 0, element 1"),
                             (dict(plan=np.array([[el(0, ctx=5), gd(1)], [el(0, ctx=6), 0]], np.uint32)), "bad plan entry: candidate 0, element 0"),
                             (dict(sets=[1]), "set out of range"),
                             (dict(group_first=[0, 0]), "group_first[n_group] must be n_cand"),
                             (dict(coeff=coeff[:15]), "coefficients out of range")):
            try:
                hip.search_plan_round_batch(**dict(ok, **change))
            except capi.CabacHipError as e:
                assert e.status == -2 and word in str(e), (word, str(e))
            else:
                raise AssertionError("not refused: " + word)
    finally:
        hip.close()
