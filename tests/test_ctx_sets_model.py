"""CPU: tests/ctx_sets_model.py — the expectation the GPU tests of include/cabac_hip_ctx_sets.h compare the device with — pinned
to the oracle's own entry points: from init sets it is orc.encode_records / orc.decode_records bit for bit, the sets it leaves
are advance() (update(), contexts.cpp:903-913), a WPP batch decodes back to its bins, and for the seeds the GPU tests use the
links really change the bytes (so that no GPU test can pass with the links ignored)."""
import numpy as np
import pytest

import ctx_sets_model as M
import helpers as H
from test_gpu_residual_estimate import advance, make_sets

WPP_SEEDS = (7101, 7102)    # tests/test_gpu_wpp.py uses these


def _same_set(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _carry_records(n, end=True):
    """A run that drives the encoder into 0xFF bytes and carries into them: a long stretch of bypass ones, then a bin that
    carries (the 0xFF / carry cases of H.random_records come with its long bypass runs; this one is forced)."""
    rec = [H.REC_EP | H.REC_BIN] * n + [10 | H.REC_BIN, H.REC_EP, 10] + ([H.REC_TRM | H.REC_BIN] if end else [])
    return np.array(rec, np.uint16)


@pytest.mark.parametrize("seed", range(6))
def test_from_init_sets_it_is_the_oracle(seed):
    orc = H.load_oracle()
    rng = np.random.default_rng(4000 + seed)
    for n in (0, 1, 15, 16, 17, 33, 64, 65, 300, 2000):
        qp, iid = int(rng.integers(0, 64)), int(rng.integers(0, 3))
        rec = H.random_records(rng, n, ctx_frac=float(rng.choice([0.3, 0.7, 0.95])))
        if n == 300:
            rec = np.concatenate([_carry_records(40 + seed, end=False), rec])
        for flags in (1, 3):
            want, want_bits = orc.encode_records(rec, qp, iid, flags)
            rc, got, bits, left = M.encode_from(rec, M.init_set(qp, iid), flags)
            assert rc == len(want) and np.array_equal(got, want) and bits == want_bits
        rc0, bins0, read0 = orc.decode_records(rec, qp, iid, want, 1)
        rc, bins, read, left_d = M.decode_from(rec, M.init_set(qp, iid), want, 1)
        assert (rc, read) == (rc0, read0) and rc == 0 and np.array_equal(bins, bins0)
        assert np.array_equal(bins, rec >> 15)
        # the sets left are advance(): encoder and decoder agree with it
        s0, s1, rate = M.init_set(qp, iid)
        s0, s1 = s0.astype(np.int64), s1.astype(np.int64)
        advance(s0, s1, rate, rec)
        assert _same_set(left, (s0.astype(np.uint16), s1.astype(np.uint16), rate))
        assert _same_set(left_d, left) and _same_set(M.advance_from(rec, M.init_set(qp, iid)), left)


def test_output_has_ff_bytes_and_the_probe_counts_bits():
    orc = H.load_oracle()
    rec = _carry_records(64)
    want, _ = orc.encode_records(rec, 30, 1, 1)
    assert (want == 0xFF).any()
    rc, got, bits, _ = M.encode_from(rec, M.init_set(30, 1), 1)
    assert np.array_equal(got, want)
    _, probe = orc.encode_records(rec, 30, 1, 4)
    assert M.encode_from(rec, M.init_set(30, 1), 4)[2] == probe


def test_from_given_sets_round_trips_and_differs_from_init():
    rng = np.random.default_rng(4100)
    sets = make_sets(rng, 3)
    differ = 0
    for k, ctx in enumerate(sets):
        rec = H.random_records(rng, 500, ctx_frac=0.9, ctx_pool=np.arange(86, 292))
        rc, data, bits, left = M.encode_from(rec, ctx, 3)   # finish() and the RBSP stop bit the decoder's finish() checks
        assert rc == len(data) > 0
        rc, bins, read, left_d = M.decode_from(rec, ctx, data, 1)
        assert rc == 0 and np.array_equal(bins, rec >> 15) and _same_set(left, left_d)
        assert _same_set(left, M.advance_from(rec, ctx))
        init = M.encode_from(rec, M.init_set(32, 0), 3)[1]
        differ += not np.array_equal(init, data)
    assert differ == 3


def test_batch_forms_mix_starts_and_flag_a_bad_set():
    rng = np.random.default_rng(4200)
    sets = make_sets(rng, 2)
    recs = [H.random_records(rng, n, ctx_frac=0.8) for n in (40, 0, 77, 16)]
    desc, total = H.make_desc([len(r) for r in recs], [30, 31, 32, 33], [0, 1, 2, 0], flags=H.SUB_FINISH | H.SUB_ALIGN_RBSP)
    records = np.concatenate(recs)
    start = np.array([0, M.NO_SET, 1, 2], np.uint32)
    out, res, left = M.encode_sets(desc, records, total, sets, start)
    assert tuple(res[3]) == (0, M.RES_BAD_SET) and left[3] is None and not res["flags"][:3].any()
    bins, dres, dleft = M.decode_sets(desc, records, out, sets, start)
    for s in range(3):
        a, n = int(desc[s]["rec_offset"]), int(desc[s]["n_records"])
        assert np.array_equal(bins[a:a + n], records[a:a + n] >> 15) and dres[s]["flags"] == 0 and _same_set(left[s], dleft[s])
    assert tuple(dres[3]) == (0, M.RES_BAD_SET)
    want, bits = H.load_oracle().encode_records(recs[1], 31, 1, 3)
    o = int(desc[1]["byte_offset"])
    assert np.array_equal(out[o:o + len(want)], want) and res[1]["n_bits"] == bits


@pytest.mark.parametrize("seed", WPP_SEEDS)
def test_wpp_batch_decodes_back_and_the_links_change_the_bytes(seed):
    desc, records, total, level_first, sync_from, sync_at = M.wpp_batch(seed)
    n_pic = int(level_first[1])
    # the cases the GPU test is about are in the batch
    parents = sorted({int(f) for f in sync_from if f != M.NO_SET})
    ats = {min(int(sync_at[p]), 10 ** 6) for p in parents}
    assert 0 in ats and 21 in ats and 10 ** 6 in ats and any(int(sync_at[p]) == int(desc[p]["n_records"]) for p in parents)
    assert sync_from[2 * n_pic + 1] == M.NO_SET and len(set(desc["n_records"].tolist())) > 6
    out, res = M.encode_wpp(desc, records, total, level_first, sync_from, sync_at)
    assert not res["flags"].any()
    bins, dres = M.decode_wpp(desc, records, out, level_first, sync_from, sync_at)
    assert not dres["flags"].any() and np.array_equal(bins, records >> 15)
    assert np.array_equal(dres["n_bits"] > 0, np.ones(len(desc), bool))
    # without links the same batch codes to other bytes in at least one row of every picture
    plain, pres, _ = M.encode_sets(desc, records, total, [], None)
    for p in range(n_pic):
        rows = [r * n_pic + p for r in range(1, len(level_first) - 1)]
        changed = 0
        for s in rows:
            o, c = int(desc[s]["byte_offset"]), int(desc[s]["byte_capacity"])
            changed += not np.array_equal(out[o:o + c], plain[o:o + c])
        assert changed >= 1, p
    # row 0 and the unlinked row are the plain coding
    for s in list(range(n_pic)) + [2 * n_pic + 1]:
        o, c = int(desc[s]["byte_offset"]), int(desc[s]["byte_capacity"])
        assert np.array_equal(out[o:o + c], plain[o:o + c]) and res[s]["n_bits"] == pres[s]["n_bits"]


def test_wpp_same_level_link_is_refused_and_its_dependents_left_out():
    desc, records, total, level_first, sync_from, sync_at = M.wpp_batch(WPP_SEEDS[0])
    n_pic = int(level_first[1])
    sync_from = sync_from.copy()
    sync_from[n_pic] = n_pic + 1          # picture 0, row 1 -> a substream of its own level
    out, res = M.encode_wpp(desc, records, total, level_first, sync_from, sync_at)
    assert tuple(res[n_pic]) == (0, M.RES_BAD_SET)
    good, gres = M.encode_wpp(*M.wpp_batch(WPP_SEEDS[0]))
    for s in range(len(desc)):
        if s % n_pic != 0:                # the other pictures are intact
            o, c = int(desc[s]["byte_offset"]), int(desc[s]["byte_capacity"])
            assert np.array_equal(out[o:o + c], good[o:o + c]) and tuple(res[s]) == tuple(gres[s])
