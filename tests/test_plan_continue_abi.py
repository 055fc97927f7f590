"""CPU: the public surface of the plan write in pieces — include/cabac_hip_plan_continue.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the one entry point; the header compiles as C99 behind the headers it names and alone, states the
definitions the GPU tests check, and keeps clear of the words the other headers' tests look for; without a context the call fails
loudly."""
import inspect
import os
import re
import subprocess
import tempfile

import pytest

import helpers as H
from entropy_coding_amd import capi

NAME = "cabac_hip_plan_continue_write_device"
HEADER = "cabac_hip_plan_continue.h"
# "INCLUDE THOSE HEADERS FIRST (the element parse's, the plan parse's, the plan write's, the context sets', the plan rows' and the
# pieces', in this order)"
FIRST = ["cabac_hip_parse_elements.h", "cabac_hip_parse_plan.h", "cabac_hip_write_plan.h", "cabac_hip_ctx_sets.h", "cabac_hip_plan_rows.h",
         "cabac_hip_pieces.h"]
# what the tests of the other headers look for outside comments, and (the last two) anywhere
NOT_IN_CODE = ["_pieces_", "cabac_coder_state", "CABAC_RES_BAD_STATE", "plan_write_", "plan_parse_", "PLAN_ROWS", "plan_resume", "write_plan",
               "parse_plan", "parse_unit", "parse_elements", "search_plan", "resolve_plan", "workspace", "CABAC_WS_", "ctx_sets", "_wpp_",
               "ctx_advance", "CABAC_CTX_NO_SET", "probes", "written_bits", "cabac_hip_sparse", "CABAC_SPARSE_"]


def _code(name):
    hdr = open(os.path.join(H.ROOT, "include", name)).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_library_exports_and_binding_lists_the_entry_point():
    _, code = _code(HEADER)
    L = capi.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, code)
    assert hasattr(L, NAME)
    declared = sorted(set(re.findall(r"\b(cabac_hip_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(capi.EXPORTS_PLAN_CONTINUE) == [NAME]
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip.h"]
    assert "#ifndef CABAC_HIP_PLAN_CONTINUE_H" in code
    others = set()
    for name in dir(capi):
        if name.startswith("EXPORTS") and name != "EXPORTS_PLAN_CONTINUE":
            others |= set(getattr(capi, name))
    assert NAME not in others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "plan_continue" not in _code(other)[1], other
    # the prototype is the sets form's with d_bytes in place of the payload's three, and the two state arrays as void pointers last
    proto = lambda name, text: [a.split()[-1].lstrip("*") for a in
                                re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text, flags=re.S).group(1).split(",")]
    sets_form = proto("cabac_hip_plan_write_sets_device", _code("cabac_hip_plan_rows.h")[1])
    k = sets_form.index("d_payload")
    assert sets_form[k:k + 3] == ["d_payload", "payload_capacity", "d_payload_offsets"]
    assert proto(NAME, code) == sets_form[:k] + ["d_bytes"] + sets_form[k + 3:] + ["d_coder_in", "d_coder_out"]
    assert re.search(r"const\s+void\s*\*\s*d_coder_in\s*,\s*void\s*\*\s*d_coder_out", code)
    assert re.search(r"uint8_t\s*\*\s*d_bytes", code)


def test_header_compiles_as_c99_behind_the_headers_it_names_and_alone():
    src = "".join('#include "%s"\n' % h for h in FIRST + [HEADER]) + \
          "int main(void) { cabac_coder_state s; s.kind = CABAC_CODER_ENC; return (int)s.kind - 1 + (&%s == 0); }\n" % NAME
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-Wno-address", "-I" + os.path.join(H.ROOT, "include"),
                               "-c", c, "-o", os.path.join(tmp, "t.o")])
        alone = os.path.join(tmp, "a.c")                            # and on its own: it needs nothing of them to be declared
        open(alone, "w").write('#include "%s"\nint main(void) { return 0; }\n' % HEADER)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(H.ROOT, "include"), "-c", alone,
                               "-o", os.path.join(tmp, "a.o")])


def test_header_states_the_definitions():
    hdr, _ = _code(HEADER)
    flat = " ".join(hdr.replace("*", " ").split())
    for words in ("DEFINITION OF THE RESULT", "INCLUDE THOSE HEADERS FIRST", "consecutive runs of its plan entries", "is_cut, spans_of",
                  "the same byte_offset, byte_capacity, qp and init_id & 3", "tu_at relative to the piece", "start empty in every piece",
                  "a reference in front of the piece is CABAC_RES_BAD_RECORD", "USES the descriptor's byte_offset", "a multiple of 16",
                  "WITHOUT CABAC_SUB_FINISH", "Nothing is flushed", "as a CABAC_CODER_ENC state", "byte for byte",
                  "results[s].n_bits == state.bits", "getNumWrittenBits()", "WITH CABAC_SUB_FINISH", "CABAC_SUB_ALIGN_RBSP as usual",
                  "the result is the whole substream's", "CABAC_CODER_CLOSED", "n_records == 0 with no block is legal",
                  "passes the state through", "end the slice here", "CABAC_SUB_PROBE is ignored", "C1.", "C2, one state format", "C3.",
                  "pieces of one entry, of one block and no entry, and of nothing", "ONE cabac_hip_plan_write_sets_device call",
                  "the first bytes_final bytes", "All of this is exact", "as 32 bytes", "either call continues from the other's state",
                  "With all states fresh and every descriptor final", "a bad entry, a value outside its element's code or a coded block without a coefficient",
                  "CABAC_RES_BAD_RECORD / CABAC_RES_BAD_VALUE", "codes nothing of itself", "is not finished", "writes no out set",
                  "returns {0, flag}", "the in state with the flag added", "the CABAC_CODER_ENC state of start(), flagged",
                  "FLAGS ARE STICKY", "CABAC_RES_OVERFLOW and CABAC_RES_BAD_SET as the encoder in pieces raises them",
                  "returns {0, flags} and copies the state", "It writes no value, info word, byte or set", "A STATE IS DATA FROM MEMORY",
                  "before the walk writes anything", "{0, CABAC_RES_BAD_STATE}", "range outside 256..510", "pend > 15",
                  "low >= 2^(10 + pend)", "bits != 8 bytes_final + 16 nbuf + pend", "an odd bytes_final",
                  "bytes_final + 2 nbuf > byte_capacity", "d_coder_out may be d_coder_in", "d_values_out may be d_values_in",
                  "The IN-PLACE RULE of the sets applies", "waits for the ctx's stream once in the middle", "allocates only library scratch",
                  "returns CABAC_HIP_ERR_INVALID before anything is queued", "no host-pointer form, no rows form and nothing in the C++ shim",
                  "array of cabac_coder_state", "kind 51", "plan write continued"):
        assert words in flat, words
    assert re.findall(r"kind \d+", hdr) == ["kind 51"]             # it names no profile kind of another header
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "kind 51" not in _code(other)[0], other


def test_the_words_the_other_headers_tests_look_for_are_absent():
    hdr, code = _code(HEADER)
    for word in NOT_IN_CODE:
        assert word not in code, word
    assert "rec10" not in hdr.lower()
    assert all(not 12 <= int(k) <= 50 for k in re.findall(r"kind (\d+)", hdr))


def test_python_binding_has_the_method_and_without_a_context_the_call_fails():
    assert callable(capi.CabacHip.plan_continue_write_device)
    p = [k for k in inspect.signature(capi.CabacHip.plan_continue_write_device).parameters]
    q = [k for k in inspect.signature(capi.CabacHip.plan_write_sets_device).parameters]
    k = q.index("d_payload")
    assert p == q[:k] + ["d_bytes"] + q[k + 3:] + ["d_coder_in", "d_coder_out"]
    L = capi.load_library()
    assert len(L.cabac_hip_plan_continue_write_device.argtypes) == len(L.cabac_hip_plan_write_sets_device.argtypes) == 25
    # no context, no call: an error code, never a quiet return
    assert L.cabac_hip_plan_continue_write_device(*([None, 1] + [None] * 4 + [0] + [None] * 4 + [4] + [None] * 4 + [0] + [None] * 8)) < 0
    import torch
    if not torch.cuda.is_available():       # and no context without a GPU: there is no CPU path behind this call
        with pytest.raises(capi.CabacHipError):
            capi.CabacHip(0)
