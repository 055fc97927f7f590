"""CPU: tests/nal_model.py (the Python restatement of the escape / unescape walks of include/cabac_hip_nal.h, from which
tests/test_gpu_nal.py takes every expectation) pinned to the oracle's countStartCodeEmulations, which
tests/test_oracle_vs_reference.py pins to the compiled reference."""
import ctypes

import numpy as np

import helpers as H
import nal_model as M
from entropy_coding_amd import capi


def _strings():
    """The generator of test_count_emulations_on_crafted_zero_runs (bytes over {0,1,2,3,4,255}, P(0) in {.3,.6,.9,.98}), 2 400
    strings, plus all-zero strings of length 0..130."""
    rng = np.random.default_rng(5)
    out = [np.zeros(n, np.uint8) for n in range(131)]
    for k in range(2400):
        n = int(rng.integers(1, 400))
        p0 = float(rng.choice([0.3, 0.6, 0.9, 0.98]))
        out.append(rng.choice(np.array([0, 1, 2, 3, 4, 255], np.uint8), size=n, p=[p0] + [(1 - p0) / 5] * 5).astype(np.uint8))
    return out


def test_model_against_the_oracle_count_and_its_own_inverse():
    orc = H.load_oracle()
    orc.lib.orc_count_emulations.argtypes = [H.u8p, ctypes.c_long]
    total = 0
    for b in _strings():
        n = len(b)
        cut = sorted({0, n // 3, n // 2, n})          # a few segment boundaries, to follow the offsets through
        nal, nal_off, st = M.escape(cut, b)
        want = orc.lib.orc_count_emulations(H._ptr(np.ascontiguousarray(b), H.u8p), n)
        assert st["n_changed"] == want and st["out_bytes"] == n + want == len(nal)
        total += want
        assert not M.has_forbidden(nal)
        assert len(nal) <= M.escape_bound(n) == capi.nal_escape_bound(n)
        if n and not b.any():
            assert (len(nal) == M.escape_bound(n)) == (n % 2 == 1)
            assert st["flags"] == M.NAL_TRAILING_ZERO
        # the inserted bytes are 03 at the recorded locations, and taking them out gives the input back
        back, off, loc, st2 = M.unescape(nal_off, nal, loc_capacity=len(nal))
        assert np.array_equal(back, b) and [int(o) for o in off] == cut and st2["flags"] == 0
        assert st2["n_changed"] == want and np.all(nal[loc.astype(np.int64)] == 3)
        keep = np.ones(len(nal), bool)
        keep[loc.astype(np.int64)] = False
        assert np.array_equal(nal[keep], b)
        # an inserted byte belongs to the segment of the byte it precedes
        for o, no in zip(cut, nal_off):
            assert int(no) == o + int(np.sum(loc.astype(np.int64) < int(no)))
    assert total > 100000


def test_model_flags_of_invalid_nal_input():
    cases = [([0, 0, 0], M.NAL_FORBIDDEN, [0, 0, 0]), ([0, 0, 1], M.NAL_FORBIDDEN, [0, 0, 1]), ([0, 0, 2], M.NAL_FORBIDDEN, [0, 0, 2]),
             ([0, 0, 3, 4], M.NAL_BAD_ESCAPE, [0, 0, 4]), ([0, 0, 0, 3], M.NAL_FORBIDDEN, [0, 0, 0, 3]), ([9, 0, 0, 3], 0, [9, 0, 0]),
             ([0, 0, 3, 0, 0, 3, 1], 0, [0, 0, 0, 0, 1])]
    for nal, flags, want in cases:
        out, off, loc, st = M.unescape([0, len(nal)], np.array(nal, np.uint8), loc_capacity=8)
        assert out.tolist() == want and st["flags"] == flags, nal
        assert int(off[1]) == len(want) == st["out_bytes"]
