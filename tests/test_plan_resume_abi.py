"""CPU: the public surface of the plan parse in pieces — include/cabac_hip_plan_resume.h declares, libcabac_hip.so exports and
entropy_coding_amd.capi binds the one entry point; the header compiles as C99 behind the headers it names and states the
definitions the GPU tests check; without a context the call fails loudly."""
import inspect
import os
import re
import subprocess
import tempfile

import pytest

import helpers as H
from entropy_coding_amd import capi

NAME = "cabac_hip_plan_resume_parse_device"
HEADER = "cabac_hip_plan_resume.h"
# "INCLUDE THOSE HEADERS FIRST (the element parse's, the plan parse's, the context sets', the plan rows' and the pieces', in this order)"
FIRST = ["cabac_hip_parse_elements.h", "cabac_hip_parse_plan.h", "cabac_hip_ctx_sets.h", "cabac_hip_plan_rows.h", "cabac_hip_pieces.h"]


def _code(name):
    hdr = open(os.path.join(H.ROOT, "include", name)).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_library_exports_and_binding_lists_the_entry_point():
    _, code = _code(HEADER)
    L = capi.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, code)
    assert hasattr(L, NAME)
    declared = sorted(set(re.findall(r"\b(cabac_hip_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(capi.EXPORTS_PLAN_RESUME) == [NAME]
    assert re.findall(r'#include\s+"([^"]+)"', code) == ["cabac_hip_parse.h"]
    others = set()
    for name in dir(capi):
        if name.startswith("EXPORTS") and name != "EXPORTS_PLAN_RESUME":
            others |= set(getattr(capi, name))
    assert NAME not in others
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "plan_resume" not in _code(other)[1], other
    # the prototype is the sets form's without d_out_at, with the two state arrays as void pointers behind it
    proto = lambda name, text: [a.split()[-1].lstrip("*") for a in
                                re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text, flags=re.S).group(1).split(",")]
    sets_form = proto("cabac_hip_plan_parse_sets_device", _code("cabac_hip_plan_rows.h")[1])
    assert sets_form[-1] == "d_out_at" and proto(NAME, code) == sets_form[:-1] + ["d_coder_in", "d_coder_out"]
    assert re.search(r"const\s+void\s*\*\s*d_coder_in\s*,\s*void\s*\*\s*d_coder_out", code)


def test_header_compiles_as_c99_behind_the_headers_it_names():
    src = "".join('#include "%s"\n' % h for h in FIRST + [HEADER]) + \
          "int main(void) { cabac_coder_state s; s.kind = CABAC_CODER_DEC; return (int)s.kind - 2 + (&%s == 0); }\n" % NAME
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
    for words in ("DEFINITION OF THE RESULT", "INCLUDE THOSE HEADERS FIRST", "consecutive runs of its plan entries", "tu_at relative to the piece",
                  "start empty in every piece", "WITHOUT CABAC_SUB_FINISH", "no stop check", "(S + 8)", "WITH CABAC_SUB_FINISH",
                  "the cumulative S", "CABAC_CODER_CLOSED", "n_records == 0 with no block is legal", "The out set is behind the piece, always",
                  "There is no d_out_at", "R1.", "R2.", "R3, one state format", "pieces of one entry, of one block and no entry, and of nothing",
                  "bit-identical to cabac_hip_plan_parse_sets_device", "as 32 bytes", "Nothing but finish() may follow a marked state",
                  "value below (range + 2) << 7", "are sticky in state.flags", "returns {0, flags} and copies the state",
                  "it is not stored and stops nothing", "reported by the final piece only", "A STATE IS DATA FROM MEMORY",
                  "before anything depends on its values", "{0, CABAC_RES_BAD_STATE}", "range outside 256..510 (511 when marked)",
                  "a value not below range << 7", "a mark above 1", "2 + (bits >> 3) > byte_capacity", "allocates nothing and waits for nothing",
                  "d_coder_out may be d_coder_in", "The IN-PLACE RULE of the sets applies", "array of cabac_coder_state", "byte for byte",
                  "no host-pointer form", "kind 50"):
        assert words in flat, words
    assert len(re.findall(r"kind \d+", hdr)) == 1                  # it names no profile kind of another header
    for other in os.listdir(os.path.join(H.ROOT, "include")):
        if other != HEADER:
            assert "kind 50" not in _code(other)[0], other


def test_python_binding_has_the_method_and_without_a_context_the_call_fails():
    assert callable(capi.CabacHip.plan_resume_parse_device)
    p = [k for k in inspect.signature(capi.CabacHip.plan_resume_parse_device).parameters]
    q = [k for k in inspect.signature(capi.CabacHip.plan_parse_sets_device).parameters]
    assert q[-1] == "d_out_at" and p == q[:-1] + ["d_coder_in", "d_coder_out"]
    L = capi.load_library()
    assert len(L.cabac_hip_plan_resume_parse_device.argtypes) == len(L.cabac_hip_plan_parse_sets_device.argtypes) + 1 == 23
    # no context, no call: an error code, never a quiet return
    assert L.cabac_hip_plan_resume_parse_device(*([None, 1] + [None] * 8 + [4] + [None] * 3 + [0] + [None] * 8)) < 0
    import torch
    if not torch.cuda.is_available():       # and no context without a GPU: there is no CPU path behind this call
        with pytest.raises(capi.CabacHipError):
            capi.CabacHip(0)
