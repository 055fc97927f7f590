"""The expectation of include/cabac_hip_probe.h, on the CPU, in ONE pass per substream: the shifts of every record (written
bits) and the cost of every record (estimated bits), summed as they go, so that the value of a probe "after the first k
records" is entry k of an array.  tests/test_probe_model.py pins both walks to the oracle's answers for every prefix; the GPU
tests of big batches compare the device with this model, and with the oracle itself on samples.

A context set is (s0 uint16[379], s1 uint16[379], rate uint8[379]) as everywhere in the tests."""
import os

import numpy as np

import helpers as H

REC_EST_RESETBITS, REC_EST_RESTART = 0x1FC, 0x1FB
_frac = None


def frac_table():
    global _frac
    if _frac is None:
        _frac = np.fromfile(os.path.join(H.GOLDEN, "frac_bits_table.bin"), "<u4").reshape(256, 2).astype(np.int64)
    return _frac


def _walk(rec, ctx, estimate):
    """[value after the first k records for k = 0 .. n], or None for a record id the walk does not know."""
    s0 = [int(v) for v in ctx[0]]
    s1 = [int(v) for v in ctx[1]]
    rate = [int(v) for v in ctx[2]]
    frac = frac_table()
    out = [0] * (len(rec) + 1)
    rng, total = 510, 0                                           # start(), arith_codec.cpp:329-337
    for k, r in enumerate(rec):
        i, b = int(r) & 0x1FF, int(r) >> 15
        if i < H.NUM_CTX:
            q8 = ((s0[i] + s1[i]) >> 8) & 0xFF                    # state(), contexts.cpp:939-941
            if estimate:
                total += int(frac[q8][b])                         # estFracBitsUpdate, contexts.cpp:922-925
            else:
                mps = q8 >> 7
                q = q8 ^ 0xFF if mps else q8
                lps = (((q >> 2) * (rng >> 5)) >> 1) + 4          # getLPS, contexts.cpp:945-949
                if b == mps:
                    rng -= lps
                    if rng < 256:
                        rng <<= 1
                        total += 1
                else:
                    nb = 8 - (lps.bit_length() - 1)               # getRenormBitsLPS, contexts.cpp:952-954
                    rng = lps << nb
                    total += nb
            r0, r1 = rate[i] >> 4, rate[i] & 15                   # update(), contexts.cpp:903-913
            s0[i] -= (s0[i] >> r0) & 0x7FE0
            s1[i] -= (s1[i] >> r1) & 0x7FFE
            if b:
                s0[i] += (0x7FFF >> r0) & 0x7FE0
                s1[i] += (0x7FFF >> r1) & 0x7FFE
        elif i == H.REC_EP:
            total += 32768 if estimate else 1                     # estFracBitsEP / one shift (arith_codec.cpp:389-399)
        elif i == H.REC_TRM:
            if estimate:
                total += 0x3BFBB if b else 0x0010C                # estFracBitsTrm, contexts.cpp:931-933
            else:                                                 # encodeBinTrm, arith_codec.cpp:460-478
                rng -= 2
                if b:
                    rng = 2 << 7
                    total += 7
                elif rng < 256:
                    rng <<= 1
                    total += 1
        elif i == H.REC_ALIGN:
            if estimate:
                total = (total + 0x7FFF) & ~0x7FFF                # align(), arith_codec.cpp:679-684
            else:
                rng = 256                                         # align(), arith_codec.cpp:401-404: no shift
        elif estimate and i == REC_EST_RESETBITS:
            total = 0                                             # resetBits() / start()
        elif estimate and i == REC_EST_RESTART:
            total &= ~0x7FFF                                      # restart()
        else:
            return None
        out[k + 1] = total
    return out


def written_bits(rec, ctx):
    """getNumWrittenBits() after the first k records, k = 0 .. len(rec): the sum of the shifts (a carry moves no bit)."""
    return _walk(rec, ctx, False)


def estimated_bits(rec, ctx):
    """BitEstimator_Std's total (1/32768 bit) after the first k records, k = 0 .. len(rec)."""
    return _walk(rec, ctx, True)


def probe_values(desc, records, probe_first, probe_at, sets, start, estimate):
    """The device calls on host arrays: (values per probe, flags per substream).  A start index >= len(sets): flag 0x40, values
    0.  A bad record: flag RES_BAD_RECORD, values None (unspecified)."""
    vals = [0] * len(probe_at)
    flags = np.zeros(len(desc), np.uint32)
    for s, d in enumerate(desc):
        a, n = int(d["rec_offset"]), int(d["n_records"])
        p0, p1 = int(probe_first[s]), int(probe_first[s + 1])
        if start is not None and int(start[s]) != 0xFFFFFFFF and int(start[s]) >= len(sets):
            flags[s] = 0x40
            continue
        if start is None or int(start[s]) == 0xFFFFFFFF:
            ctx = H.load_oracle().ctx_init(min(max(int(d["qp"]), 0), 63), int(d["init_id"]) & 3)
        else:
            ctx = sets[int(start[s])]
        run = _walk(records[a:a + n], ctx, estimate)
        if run is None:
            flags[s] = H.RES_BAD_RECORD
            for p in range(p0, p1):
                vals[p] = None
            continue
        for p in range(p0, p1):
            vals[p] = run[min(int(probe_at[p]), n)]
    return vals, flags
