"""GPU: probe points (include/cabac_hip_probe.h, parts 1 and 2) — cabac_hip_written_bits_device and
cabac_hip_estimate_probes_device against the oracle's answer for the prefix every probe names (flags=4 of orc_encode_records;
orc_estimate_records / _from), from Ctx::init and from start sets; the batch of 4 100 substreams against tests/probe_model.py
(pinned to the oracle by tests/test_probe_model.py) and sampled against the oracle.  Every comparison is exact integer equality."""
import functools

import numpy as np
import pytest
import torch

import ctx_sets_model as M
import helpers as H
import probe_model as P
from entropy_coding_amd import capi
from test_gpu_residual_estimate import make_sets, pack_sets
from test_probe_model import strings

pytestmark = pytest.mark.gpu

NO_SET = 0xFFFFFFFF
SENT32 = 0x5A5A5A5A
SENT64 = 0x5A5A5A5A5A5A5A5A
LENGTHS = {1: [33], 3: [17, 0, 100], 5: [16, 1, 1000, 15, 33], 8: [1000, 0, 100, 16, 33, 1, 17, 15]}
GUARD = 8   # words in front of and behind the values


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def ptr(t):
    return t.data_ptr() if t is not None else 0


@functools.lru_cache(None)
def start_sets():
    sets = make_sets(np.random.default_rng(4600), 3)
    state, rate = pack_sets(sets)
    return sets, state.astype(np.uint32), rate.astype(np.uint8)


def probe_list(lengths):
    """Per substream: 0, 1, 15, 16, 17, n - 1, n, n + 5 (clipped) and 0xFFFFFFFF in ascending order; the substream of length 100 has
    a probe behind every record, the one of length 33 forty more at position 17, and the second substream of a batch has none."""
    first, at = [0], []
    for s, n in enumerate(lengths):
        mine = sorted([0, 1, 15, 16, 17, n, n + 5, NO_SET] + ([n - 1] if n else []))
        if n == 100:
            mine = sorted(mine + list(range(n + 1)))
        if n == 33:
            mine = sorted(mine + [17] * 40)
        if s == 1:
            mine = []
        at += mine
        first.append(len(at))
    return np.array(first, np.uint32), np.array(at, np.uint32)


@functools.lru_cache(None)
def batch(n_sub, estimate):
    rng = np.random.default_rng(4610 + 7 * n_sub + int(estimate))
    lengths = LENGTHS[n_sub]
    recs = [strings(rng, n, estimate) for n in lengths]
    desc, _ = H.make_desc(lengths, [int(rng.integers(0, 64)) for _ in lengths], [int(rng.integers(0, 3)) for _ in lengths])
    first, at = probe_list(lengths)
    return desc, np.concatenate(recs + [np.zeros(0, np.uint16)]).astype(np.uint16), first, at


def mixed_starts(n_sub):
    """Ctx::init and set starts in the rows of one wave; set 1 is shared by two substreams."""
    return np.array([[1, NO_SET, 1, 2, 0][s % 5] for s in range(n_sub)], np.uint32)


def oracle_values(desc, records, first, at, estimate, start=None):
    """What the header defines: the oracle's answer for the substream cut to the probe's first k records."""
    orc = H.load_oracle()
    sets = start_sets()[0]
    vals = []
    for s, d in enumerate(desc):
        a, n, qp, iid = int(d["rec_offset"]), int(d["n_records"]), int(d["qp"]), int(d["init_id"]) & 3
        seen = {}
        for p in range(int(first[s]), int(first[s + 1])):
            k = min(int(at[p]), n)
            if k not in seen:
                rec = records[a:a + k]
                if start is None or int(start[s]) == NO_SET:
                    seen[k] = orc.estimate_records(rec, qp, iid)[1] if estimate else orc.encode_records(rec, qp, iid, flags=4)[1]
                else:
                    ctx = sets[int(start[s])]
                    seen[k] = orc.estimate_records_from(rec, *ctx)[1] if estimate else M.encode_from(rec, ctx, flags=4)[2]
            vals.append(seen[k])
    return np.array(vals, np.uint64)


def run_device(hip, desc, records, first, at, estimate, start=None, n_sets=None, with_flags=True, n_probe=None):
    """One device call on fresh buffers with guard words around the values: (values, flags)."""
    dtype, sent = (np.uint64, SENT64) if estimate else (np.uint32, SENT32)
    n_probe = len(at) if n_probe is None else n_probe
    d_desc, d_rec = dev(desc), dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    d_first, d_at = dev(first), dev(np.concatenate([at, np.zeros(4, np.uint32)]))
    d_out = dev(np.full(len(at) + 2 * GUARD, sent, dtype))
    d_flags = dev(np.full(len(desc) + 2, SENT32, np.uint32)) if with_flags else None
    _, state, rate = start_sets()
    t = [dev(state), dev(rate), dev(start)] if start is not None else [None, None, None]
    ns = (len(state) // H.NUM_CTX if n_sets is None else n_sets) if start is not None else 0
    call = hip.estimate_probes_device if estimate else hip.written_bits_device
    call(len(desc), ptr(d_desc), ptr(d_rec), ptr(d_first), ptr(d_at), n_probe, ptr(d_out) + GUARD * dtype().itemsize, ptr(d_flags),
         ns, ptr(t[0]), ptr(t[1]), ptr(t[2]))
    hip.synchronize()
    out = host(d_out, dtype)
    assert (out[:GUARD] == sent).all() and (out[GUARD + len(at):] == sent).all(), "guard words"
    flags = host(d_flags, np.uint32) if with_flags else None
    if with_flags:
        assert (flags[len(desc):] == SENT32).all()
        flags = flags[:len(desc)]
    return out[GUARD:GUARD + len(at)].astype(np.uint64), flags


# ---------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("estimate", [False, True], ids=["written", "estimated"])
@pytest.mark.parametrize("n_sub", [1, 3, 5, 8])
def test_probes_from_ctx_init(hip, n_sub, estimate):
    desc, records, first, at = batch(n_sub, estimate)
    want = oracle_values(desc, records, first, at, estimate)
    for start in (None, np.full(n_sub, NO_SET, np.uint32)):
        got, flags = run_device(hip, desc, records, first, at, estimate, start=start)
        assert not flags.any()
        assert np.array_equal(got, want)
    got, _ = run_device(hip, desc, records, first, at, estimate, with_flags=False)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("estimate", [False, True], ids=["written", "estimated"])
@pytest.mark.parametrize("n_sub", [3, 5, 8])
def test_probes_from_start_sets(hip, n_sub, estimate):
    desc, records, first, at = batch(n_sub, estimate)
    start = mixed_starts(n_sub)
    want = oracle_values(desc, records, first, at, estimate, start)
    got, flags = run_device(hip, desc, records, first, at, estimate, start=start)
    assert not flags.any()
    assert np.array_equal(got, want)
    assert not np.array_equal(want, oracle_values(desc, records, first, at, estimate))   # the sets matter


def test_last_probe_is_the_gpus_own_end_of_substream_answer(hip):
    for estimate in (False, True):
        desc, records, first, at = batch(8, estimate)
        got, _ = run_device(hip, desc, records, first, at, estimate)
        ends = [int(first[s + 1]) - 1 for s in range(8) if first[s + 1] > first[s]]      # the 0xFFFFFFFF probe of each list
        subs = [s for s in range(8) if first[s + 1] > first[s]]
        d_desc, d_rec = dev(desc), dev(np.concatenate([records, np.zeros(8, np.uint16)]))
        if estimate:
            d_bits = dev(np.zeros(8, np.uint64))
            hip.estimate_device(8, ptr(d_desc), ptr(d_rec), ptr(d_bits))
            hip.synchronize()
            own = host(d_bits, np.uint64)
        else:
            probe_desc = desc.copy()
            probe_desc["init_id"] = (probe_desc["init_id"] & 3) | capi.SUB_PROBE
            d_desc = dev(probe_desc)
            d_bytes = torch.zeros(int(desc["byte_offset"][-1] + desc["byte_capacity"][-1]) + 16, dtype=torch.uint8, device="cuda")
            d_res = dev(np.zeros(8, H.RESULT_DTYPE))
            hip.encode_device(8, ptr(d_desc), ptr(d_rec), ptr(d_bytes), ptr(d_res))
            hip.synchronize()
            res = host(d_res, H.RESULT_DTYPE)
            assert not res["flags"].any()
            own = res["n_bits"].astype(np.uint64)
        assert np.array_equal(got[ends], own[subs])


# ---------------------------------------------------------------------------------------------- 2. the big-batch geometry
@functools.lru_cache(None)
def big_batch():
    n_sub, n = 4100, 64
    rng = np.random.default_rng(4700)
    pool = strings(rng, 20000, True)
    pool_w = pool.copy()
    pool_w[(pool_w & 0x1FF) == P.REC_EST_RESETBITS] = H.REC_EP                      # the written-bits walk has no pseudo-records
    pool_w[(pool_w & 0x1FF) == P.REC_EST_RESTART] = H.REC_EP | H.REC_BIN
    offs = rng.integers(0, len(pool) - n, size=n_sub)
    idx = (offs[:, None] + np.arange(n)[None, :]).reshape(-1)
    desc, _ = H.make_desc([n] * n_sub, rng.integers(0, 64, size=n_sub), rng.integers(0, 3, size=n_sub))
    first = np.arange(0, 4 * n_sub + 1, 4, dtype=np.uint32)
    at = np.sort(rng.integers(0, n + 2, size=(n_sub, 4)), axis=1).reshape(-1).astype(np.uint32)
    start = np.where(rng.random(n_sub) < 0.5, NO_SET, rng.integers(0, 3, size=n_sub)).astype(np.uint32)
    return desc, pool[idx].astype(np.uint16), pool_w[idx].astype(np.uint16), first, at, start


@pytest.mark.parametrize("estimate", [False, True], ids=["written", "estimated"])
def test_4100_substreams_against_the_model_and_sampled_against_the_oracle(hip, estimate):
    desc, rec_e, rec_w, first, at, start = big_batch()
    records = rec_e if estimate else rec_w
    want, wflags = P.probe_values(desc, records, first, at, start_sets()[0], start, estimate)
    got, flags = run_device(hip, desc, records, first, at, estimate, start=start)
    assert not wflags.any() and not flags.any()
    assert np.array_equal(got, np.array(want, np.uint64))
    pick = np.sort(np.random.default_rng(4701).choice(len(desc), size=64, replace=False))
    sub_first = np.arange(0, 4 * 64 + 1, 4, dtype=np.uint32)
    sub_at = np.concatenate([at[4 * s:4 * s + 4] for s in pick])
    orc = oracle_values(desc[pick], records, sub_first, sub_at, estimate, start[pick])
    assert np.array_equal(np.concatenate([got[4 * s:4 * s + 4] for s in pick]), orc)


# ---------------------------------------------------------------------------------------------- 3. flags, empty calls
@pytest.mark.parametrize("estimate", [False, True], ids=["written", "estimated"])
def test_bad_record_flags_its_substream_only(hip, estimate):
    desc, records, first, at = batch(8, estimate)
    records = records.copy()
    records[int(desc["rec_offset"][2]) + 40] = 0x1F0      # neither a context nor EP / TRM / align, in the substream of length 100
    want = oracle_values(desc, batch(8, estimate)[1], first, at, estimate)
    got, flags = run_device(hip, desc, records, first, at, estimate)
    assert list(flags) == [0, 0, capi.RES_BAD_RECORD, 0, 0, 0, 0, 0]
    keep = np.ones(len(at), bool)
    keep[int(first[2]):int(first[3])] = False
    assert np.array_equal(got[keep], want[keep])


@pytest.mark.parametrize("estimate", [False, True], ids=["written", "estimated"])
def test_bad_set_gives_zeros_and_the_flag(hip, estimate):
    desc, records, first, at = batch(5, estimate)
    start = mixed_starts(5)
    want = oracle_values(desc, records, first, at, estimate, start)
    start = start.copy()
    start[2], start[4] = 3, 0xFFFFFFFE                    # n_sets is 3
    got, flags = run_device(hip, desc, records, first, at, estimate, start=start)
    assert list(flags) == [0, 0, capi.RES_BAD_SET, 0, capi.RES_BAD_SET]
    for s in range(5):
        a, b = int(first[s]), int(first[s + 1])
        assert np.array_equal(got[a:b], np.zeros(b - a, np.uint64) if s in (2, 4) else want[a:b]), s
    got, flags = run_device(hip, desc, records, first, at, estimate, start=mixed_starts(5), n_sets=0)   # no set at all
    assert [int(f) for f in flags] == [capi.RES_BAD_SET if v != NO_SET else 0 for v in mixed_starts(5)]


def test_no_probe_and_no_substream_are_ok(hip):
    for estimate in (False, True):
        desc, records, first, at = batch(5, estimate)
        got, flags = run_device(hip, desc, records, np.zeros(6, np.uint32), np.zeros(0, np.uint32), estimate)
        assert len(got) == 0 and not flags.any()
        call = hip.estimate_probes_device if estimate else hip.written_bits_device
        call(0, 0, 0, 0, 0, 0, 0)
        call(0, 0, 0, 0, 0, 7, 0)
        bits, flags = (hip.estimate_probes_batch if estimate else hip.written_bits_batch)(desc, records, np.zeros(6, np.uint32), [])
        assert len(bits) == 0 and not flags.any()
    hip.synchronize()


# ---------------------------------------------------------------------------------------------- 4. the host-pointer forms
@pytest.mark.parametrize("estimate", [False, True], ids=["written", "estimated"])
def test_batch_forms_agree_refuse_and_leave_outputs_alone(hip, estimate):
    desc, records, first, at = batch(8, estimate)
    form = hip.estimate_probes_batch if estimate else hip.written_bits_batch
    dtype, sent = (np.uint64, SENT64) if estimate else (np.uint32, SENT32)
    got, flags = form(desc, records, first, at)
    assert not flags.any() and np.array_equal(got.astype(np.uint64), oracle_values(desc, records, first, at, estimate))
    _, state, rate = start_sets()
    start = mixed_starts(8)
    got, flags = form(desc, records, first, at, state, rate, start)
    assert not flags.any() and np.array_equal(got.astype(np.uint64), oracle_values(desc, records, first, at, estimate, start))

    def refused(first, at, start=None):
        out = np.full(len(at) + 4, sent, dtype)
        with pytest.raises(capi.CabacHipError) as e:
            form(desc, records, first, at, state if start is not None else None, rate if start is not None else None, start, out=out)
        assert e.value.status == -2
        assert (out == sent).all()

    f = first.copy()
    f[0] = 1
    refused(f, at)                                        # does not start at 0
    f = first.copy()
    f[3], f[4] = f[4], f[3]
    assert f[3] > f[4]
    refused(f, at)                                        # does not ascend
    a = at.copy()
    p = int(first[2])
    a[p + 5], a[p + 6] = 50, 49
    refused(first, a)                                     # positions go backwards inside a substream
    s = start.copy()
    s[5] = 3
    refused(first, at, s)                                 # a set index >= n_sets
    bad = records.copy()
    bad[int(desc["rec_offset"][0]) + 3] = 0x1F0
    with pytest.raises(capi.CabacHipError) as e:
        form(desc, bad, first, at)
    assert e.value.status == -5
    got, flags = form(desc, bad, first, at, check=False)
    assert flags[0] == capi.RES_BAD_RECORD and not flags[1:].any()


# ---------------------------------------------------------------------------------------------- 5. nothing else changes
def test_plain_calls_are_unchanged_by_a_preceding_probe_call(hip):
    desc, records, first, at = batch(8, False)
    d_desc, d_rec = dev(desc), dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    total = int(desc["byte_offset"][-1] + desc["byte_capacity"][-1])

    def plain():
        d_bytes = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        d_res, d_bits, d_fl = dev(np.zeros(8, H.RESULT_DTYPE)), dev(np.zeros(8, np.uint64)), dev(np.zeros(8, np.uint32))
        hip.encode_device(8, ptr(d_desc), ptr(d_rec), ptr(d_bytes), ptr(d_res))
        hip.estimate_device(8, ptr(d_desc), ptr(d_rec), ptr(d_bits), ptr(d_fl))
        hip.synchronize()
        return host(d_bytes, np.uint8).copy(), host(d_res, np.uint32).copy(), host(d_bits, np.uint64).copy(), host(d_fl, np.uint32).copy()

    before = plain()
    run_device(hip, desc, records, first, at, False)
    run_device(hip, desc, records, first, at, True, start=mixed_starts(8))
    after = plain()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    want_bytes, want_res = H.load_oracle().encode_batch(desc, records, total)
    assert np.array_equal(after[1].view(H.RESULT_DTYPE)["n_bits"], want_res["n_bits"])
