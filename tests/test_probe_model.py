"""CPU: tests/probe_model.py — the one-pass model of the probe values — against the oracle's answers for EVERY prefix: the
written bits of orc_encode_records with the probe flag (flags=4: getNumWrittenBits(), nothing flushed) and the totals of
orc_estimate_records / orc_estimate_records_from, from Ctx::init and from given contexts.  The strings hold every record kind:
context bins over all 379 contexts, bypass bins, terminate bins of both values mid-string, align records, and for the estimator
its two pseudo-records."""
import numpy as np
import pytest

import ctx_sets_model as M
import helpers as H
import probe_model as P
from test_gpu_residual_estimate import make_sets


def strings(rng, n, estimate):
    rec = H.random_records(rng, n, ctx_frac=float(rng.choice([0.3, 0.7, 0.95])), end_trm=False, trm0_frac=0.02)
    if n:
        pos = rng.integers(0, n, size=max(n // 12, 3))
        rec[pos[0::3]] = H.REC_TRM | H.REC_BIN          # a terminate bin 1 in the middle: seven shifts, range 256
        rec[pos[1::3]] = H.REC_ALIGN
        rec[pos[2::3]] = H.REC_TRM
        if estimate:
            more = rng.integers(0, n, size=4)
            rec[more[:2]] = P.REC_EST_RESETBITS
            rec[more[2:]] = P.REC_EST_RESTART
    return rec


@pytest.mark.parametrize("seed", range(4))
def test_written_bits_of_every_prefix(seed):
    rng = np.random.default_rng(4500 + seed)
    orc = H.load_oracle()
    for n in (0, 1, 17, 150):
        rec = strings(rng, n, False)
        qp, iid = int(rng.integers(0, 64)), int(rng.integers(0, 3))
        got = P.written_bits(rec, orc.ctx_init(qp, iid))
        assert got[0] == 0 and len(got) == n + 1
        for k in range(n + 1):
            assert got[k] == orc.encode_records(rec[:k], qp, iid, flags=4)[1], (n, k)


def test_written_bits_from_given_contexts():
    rng = np.random.default_rng(4510)
    sets = make_sets(rng, 2)
    for ctx in sets:
        rec = strings(rng, 120, False)
        got = P.written_bits(rec, ctx)
        for k in range(len(rec) + 1):
            rc, _, nbits, _ = M.encode_from(rec[:k], ctx, flags=4)
            assert rc >= 0 and got[k] == nbits, k


@pytest.mark.parametrize("seed", range(4))
def test_estimated_bits_of_every_prefix(seed):
    rng = np.random.default_rng(4520 + seed)
    orc = H.load_oracle()
    for n in (0, 1, 17, 150):
        rec = strings(rng, n, True)
        qp, iid = int(rng.integers(0, 64)), int(rng.integers(0, 3))
        got = P.estimated_bits(rec, orc.ctx_init(qp, iid))
        for k in range(n + 1):
            assert (0, got[k]) == orc.estimate_records(rec[:k], qp, iid), (n, k)


def test_estimated_bits_from_given_contexts():
    rng = np.random.default_rng(4530)
    orc = H.load_oracle()
    for ctx in make_sets(rng, 2):
        rec = strings(rng, 120, True)
        got = P.estimated_bits(rec, ctx)
        for k in range(len(rec) + 1):
            assert (0, got[k]) == orc.estimate_records_from(rec[:k], *ctx), k


def test_bad_records_and_the_batch_form_of_the_model():
    orc = H.load_oracle()
    ctx = orc.ctx_init(30, 1)
    assert P.written_bits(np.array([3, 0x1F0, 4], np.uint16), ctx) is None
    assert P.written_bits(np.array([3, P.REC_EST_RESETBITS], np.uint16), ctx) is None   # the estimator's alone
    assert P.estimated_bits(np.array([3, 0x1F0, 4], np.uint16), ctx) is None
    rng = np.random.default_rng(4540)
    recs = [strings(rng, n, False) for n in (20, 0, 33)]
    desc, _ = H.make_desc([len(r) for r in recs], [30, 31, 32], [0, 1, 2])
    records = np.concatenate(recs).astype(np.uint16)
    first = np.array([0, 3, 3, 5], np.uint32)
    at = np.array([0, 7, 0xFFFFFFFF, 33, 40], np.uint32)
    vals, flags = P.probe_values(desc, records, first, at, [], None, False)
    w0, w2 = P.written_bits(recs[0], orc.ctx_init(30, 0)), P.written_bits(recs[2], orc.ctx_init(32, 2))
    assert vals == [0, w0[7], w0[20], w2[33], w2[33]] and not flags.any()
    vals, flags = P.probe_values(desc, records, first, at, [], np.array([0xFFFFFFFF, 0, 5], np.uint32), False)
    assert vals[3:] == [0, 0] and list(flags) == [0, 0x40, 0x40]
