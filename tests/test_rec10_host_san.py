"""CPU: entropy_coding_amd/csrc/cabac_rec10_host.cpp under AddressSanitizer and UBSan.  The translation unit has no HIP include, so
g++ alone builds it together with the stand-alone driver tests/csrc/rec10_host_main.cpp (its own main, tight heap buffers, the
edge cases of tests/test_rec10_model.py); the program runs as a child process.  Nothing is preloaded and nothing is loaded into
the interpreter."""
import os
import subprocess

import helpers as H

CSRC = os.path.join(H.ROOT, "tests", "csrc")
SAN_DIR = os.path.join(CSRC, "_san")
# the runtimes linked into the program itself: it then runs the same whatever the environment preloads
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
             "-fno-omit-frame-pointer", "-g", "-O1"]


def test_host_translation_unit_has_no_hip_include():
    src = open(os.path.join(H.ROOT, "entropy_coding_amd", "csrc", "cabac_rec10_host.cpp")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert includes and not [i for i in includes if "hip/" in i or "kernels" in i], includes
    assert '"cabac_hip_rec10.h"' in includes


def test_pack_and_unpack_run_clean_under_asan_and_ubsan():
    os.makedirs(SAN_DIR, exist_ok=True)
    exe = os.path.join(SAN_DIR, "rec10_host_main_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN_FLAGS + ["-I" + os.path.join(H.ROOT, "include"),
                           os.path.join(H.ROOT, "entropy_coding_amd", "csrc", "cabac_rec10_host.cpp"),
                           os.path.join(CSRC, "rec10_host_main.cpp"), "-o", exe])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rec10 host ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
