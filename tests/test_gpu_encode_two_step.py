"""The lane-serial encoder (encode_kernel_v7) over every loop length, ragged workgroups, every record kind at every place of
a PAIR of 16-bin steps, repeated contexts across step boundaries, every record id, and the context-sets entry point.

The context waves of encode_kernel_v7<4> read what a record id means from a 16-byte table row per id (quad_resolve<..,
kKindTab>; <1> derives it with compares, as variants 6 and 4 do): the "every id" case is that table, exhaustively.  The loop
itself passes one workgroup barrier per step; the cases are laid out by pairs of steps (32 places, both parities of the step
count, repeats across the middle of a pair and across two pairs) so that they judge a loop of two steps per barrier as they
stand.

Every GPU case is coded by the device and by the oracle and compared exactly: the coded bytes up to ceil(n_bits / 8), n_bits
and flags.  A substream with a bad record has unspecified n_bits and bytes (cabac_hip.h), so there only the flag is compared.
The cases run under encode variant 7 with fewer than 1 024 substreams (encode_kernel_v7<1>, workgroups of four), padded past
1 024 (encode_kernel_v7<4>, workgroups of sixteen, the last one with ONE live substream), and under variants 6 and 4 as
controls.  test_batches_reach_what_they_claim counts, on the CPU, what each batch holds."""
import functools

import numpy as np
import pytest

import helpers as H

FIN = H.SUB_FINISH | H.SUB_ALIGN_RBSP
ALIGN = np.uint16(H.REC_ALIGN)
TRM1 = np.uint16(H.REC_TRM | H.REC_BIN)
TRM0 = np.uint16(H.REC_TRM)
EP0, EP1 = np.uint16(H.REC_EP), np.uint16(H.REC_EP | H.REC_BIN)
QUIET = 200                        # a context the random records never use
CTX0, CTX1 = np.uint16(QUIET), np.uint16(QUIET | H.REC_BIN)   # one is the MPS and one the LPS path of its initial state
POOL = np.array([c for c in range(H.NUM_CTX) if c != QUIET])
KINDS = {"trm1": TRM1, "trm0": TRM0, "align": ALIGN, "ep0": EP0, "ep1": EP1, "ctx0": CTX0, "ctx1": CTX1}
MAX_LEN = 100
BIG_MIN = 1024                     # from here the dispatch takes encode_kernel_v7<4>
GEOMETRIES = {"v7x1": (7, 4, False), "v7x4": (7, 16, True), "v6": (6, 4, False), "v4": (4, 4, False)}   # variant, workgroup, padded


def _plain(rng, n):
    return H.random_records(rng, n, ctx_pool=POOL, end_trm=False, trm0_frac=0.0)


def _steps(n):
    return (n + 15) // 16


# ------------------------------------------------------------------ batches
@functools.lru_cache(None)
def _filler():
    rng = np.random.default_rng(5100)
    return [np.concatenate([_plain(rng, int(rng.integers(0, 40))), [TRM1]]).astype(np.uint16) for _ in range(BIG_MIN + 32)]


def _padded(recs, group, big):
    """The cases (whole workgroups of `group`), filler up to a whole number of workgroups (past 1 024 substreams if big), and
    the first case once more: alone in the last workgroup."""
    recs = [np.asarray(r, np.uint16) for r in recs]
    assert len(recs) % group == 0
    n = max(len(recs), BIG_MIN) if big else len(recs)
    n = (n + group - 1) // group * group
    recs = recs + _filler()[:n - len(recs)] + [recs[0]]
    assert (len(recs) >= BIG_MIN) == big and len(recs) % group == 1
    return recs


def _batch(recs):
    lens = [len(r) for r in recs]
    assert max(lens) <= MAX_LEN
    records = np.concatenate(recs + [np.zeros(0, np.uint16)]).astype(np.uint16)
    rng = np.random.default_rng(len(recs))
    desc, total = H.make_desc(lens, rng.integers(20, 45, len(recs)), rng.integers(0, 3, len(recs)), FIN, capacities=[n + 64 for n in lens])
    want_b, want_r = H.load_oracle().encode_batch(desc, records, total)
    return desc, records, total, want_b, want_r


def _whole_groups(recs, group):
    """Pad a list of cases with short substreams to whole workgroups."""
    recs = list(recs)
    while len(recs) % group:
        recs.append(np.array([TRM1], np.uint16))
    return recs


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _compare(desc, got_b, got_r, want_b, want_r):
    assert np.array_equal(got_r["flags"], want_r["flags"]), np.flatnonzero(got_r["flags"] != want_r["flags"])
    ok = (want_r["flags"] & H.RES_BAD_RECORD) == 0
    assert np.array_equal(got_r["n_bits"][ok], want_r["n_bits"][ok]), np.flatnonzero(ok & (got_r["n_bits"] != want_r["n_bits"]))
    for s in np.flatnonzero(ok):
        o, n = int(desc[s]["byte_offset"]), (int(want_r[s]["n_bits"]) + 7) // 8
        assert np.array_equal(got_b[o:o + n], want_b[o:o + n]), s


def _check(hip, case):
    import torch
    desc, records, total, want_b, want_r = case
    d_desc, d_rec = _dev(desc), _dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    d_bytes = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    d_res = _dev(np.full(2 * len(desc), 0x5A5A5A5A, np.uint32))
    hip.encode_device(len(desc), d_desc.data_ptr(), d_rec.data_ptr(), d_bytes.data_ptr(), d_res.data_ptr())
    hip.synchronize()
    _compare(desc, d_bytes.cpu().numpy(), d_res.cpu().numpy().view(H.RESULT_DTYPE), want_b, want_r)


@pytest.fixture(scope="module", params=list(GEOMETRIES), ids=list(GEOMETRIES))
def enc(request):
    variant, group, big = GEOMETRIES[request.param]
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    c.set_variant(variant, 0)
    yield c, group, big
    c.close()


# ------------------------------------------------------------------ every loop length
def _loop_length_recs(group):
    """For every L in 0 .. 97 one workgroup whose longest substream has L records, at a place that moves through the workgroup;
    the others are shorter by anything."""
    rng = np.random.default_rng(5101)
    recs = []
    for L in range(98):
        lens = [int(rng.integers(0, L + 1)) for _ in range(group)]
        lens[L % group] = L
        for n in lens:
            recs.append(np.concatenate([_plain(rng, n - 1), [TRM1]]).astype(np.uint16) if n else np.zeros(0, np.uint16))
    return recs


@functools.lru_cache(None)
def _loop_length_case(group, big):
    return _batch(_padded(_loop_length_recs(group), group, big))


@pytest.mark.gpu
def test_every_loop_length(enc):
    hip, group, big = enc
    _check(hip, _loop_length_case(group, big))


# ------------------------------------------------------------------ ragged workgroups
def _ragged_lens(group):
    """One workgroup per rotation: substream (k + rot) % group has 5k % 6 whole steps and a tail of its own (0 .. 5 steps apart)."""
    base = [16 * ((5 * k) % 6) + 1 + (7 * k) % 16 for k in range(group)]
    return [[base[(k - rot) % group] for k in range(group)] for rot in range(group)]


def _ragged_recs(group):
    rng = np.random.default_rng(5102)
    return [np.concatenate([_plain(rng, n - 1), [TRM1]]).astype(np.uint16) for lens in _ragged_lens(group) for n in lens]


@functools.lru_cache(None)
def _ragged_case(group, big):
    return _batch(_padded(_ragged_recs(group), group, big))


@pytest.mark.gpu
def test_ragged_workgroups(enc):
    """Lengths inside one workgroup up to five steps apart, in every rotation over its rows and units; the batch ends in a
    workgroup with a single live substream."""
    hip, group, big = enc
    _check(hip, _ragged_case(group, big))


# ------------------------------------------------------------------ record kinds at every place of a pair
N_PAIRS = 3                        # substreams of three pairs of steps: the first and the last pair carry the special record


def _kind_recs():
    rng = np.random.default_rng(5103)
    recs, where = [], []
    for name, rec in KINDS.items():
        for place in range(32):
            for pair in (0, N_PAIRS - 1):
                r = _plain(rng, 32 * N_PAIRS)
                at = 32 * pair + place
                r[at] = rec
                recs.append(np.concatenate([r, [TRM1]]).astype(np.uint16))
                where.append((name, pair, place))
    return recs, where


@functools.lru_cache(None)
def _kind_case(group, big):
    return _batch(_padded(_whole_groups(_kind_recs()[0], group), group, big))


@pytest.mark.gpu
def test_record_kinds_at_every_place_of_a_pair(enc):
    hip, group, big = enc
    case = _kind_case(group, big)
    assert not case[4]["flags"].any()
    _check(hip, case)


# ------------------------------------------------------------------ context repeats
REPEATS = {                        # name: the places of one context in a substream of three pairs
    "twice in a step": (3, 9),
    "three times in a step": (1, 2, 14),
    "five times in a step": (0, 4, 5, 11, 15),
    "a whole step": tuple(range(16, 32)),
    "across the middle of a pair": (15, 16),
    "across the middle, often": (12, 14, 15, 16, 17, 20),
    "across two pairs": (31, 32),
    "across two pairs, often": (29, 30, 31, 32, 33, 40),
    "every step": (5, 21, 37, 53, 69, 85),
    "everywhere": tuple(range(0, 96)),
}


def _repeat_recs():
    rng = np.random.default_rng(5104)
    recs = []
    for places in REPEATS.values():
        for bins in ("random", "ones", "zeros"):
            r = _plain(rng, 32 * N_PAIRS)
            for p in places:
                b = int(rng.integers(0, 2)) if bins == "random" else int(bins == "ones")
                r[p] = QUIET | (b << 15)
            recs.append(np.concatenate([r, [TRM1]]).astype(np.uint16))
    return recs


@functools.lru_cache(None)
def _repeat_case(group, big):
    return _batch(_padded(_whole_groups(_repeat_recs(), group), group, big))


@pytest.mark.gpu
def test_context_repeats(enc):
    hip, group, big = enc
    case = _repeat_case(group, big)
    assert not case[4]["flags"].any()
    _check(hip, case)


# ------------------------------------------------------------------ every id
def _every_id_recs():
    return [np.array([i | (b << 15)], np.uint16) for i in range(512) for b in (0, 1)]


@functools.lru_cache(None)
def _every_id_cases(group, big):
    """1 024 substreams of one record; under 1 024 substreams per call they go in two halves."""
    recs = _every_id_recs()
    parts = [recs] if big else [recs[:512], recs[512:]]
    return [_batch(_padded(p, group, big)) for p in parts]


@pytest.mark.gpu
def test_every_id(enc):
    """Every id 0 .. 511 with both bin values, each the one record of its substream: CABAC_RES_BAD_RECORD exactly where the
    oracle reports it, and n_bits and the bytes of every other."""
    hip, group, big = enc
    cases = _every_id_cases(group, big)
    bad = np.concatenate([c[4]["flags"][:len(_every_id_recs()) // len(cases)] for c in cases]).reshape(512, 2)
    good_ids = list(range(H.NUM_CTX)) + [H.REC_ALIGN, H.REC_EP, H.REC_TRM]
    assert (bad[good_ids] == 0).all() and (np.delete(bad, good_ids, axis=0) == H.RES_BAD_RECORD).all()
    for c in cases:
        _check(hip, c)


# ------------------------------------------------------------------ context sets
SET_LENS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)      # 1, 2, 3 and 4 steps, their first and their last record


@pytest.mark.gpu
def test_context_sets_after_one_to_four_steps(enc):
    """cabac_hip_encode_sets_device from start sets into out sets, one workgroup per length (the others of it shorter): the
    coded bytes and the exported set are the model's."""
    import ctx_sets_model as M
    import test_gpu_ctx_sets as CS
    hip, group, big = enc
    rng = np.random.default_rng(5105)
    recs = []
    for n in SET_LENS:
        for k in range(group):
            m = n if k == n % group else int(rng.integers(0, n + 1))
            recs.append(np.concatenate([H.random_records(rng, m - 1, ctx_frac=0.9, ctx_pool=np.arange(86, 292), end_trm=False), [TRM1]]).astype(np.uint16)
                        if m else np.zeros(0, np.uint16))
    recs = _padded(recs, group, big)
    lens = [len(r) for r in recs]
    assert {_steps(n) for n in SET_LENS} == {1, 2, 3, 4}
    records = np.concatenate(recs).astype(np.uint16)
    desc, total = H.make_desc(lens, rng.integers(20, 45, len(recs)), rng.integers(0, 3, len(recs)), FIN, capacities=[n + 64 for n in lens])
    sets, _, _ = CS.start_sets()
    n_sub = len(desc)
    start = np.array([M.NO_SET if s % 4 == 0 else s % CS.N_SETS for s in range(n_sub)], np.uint32)
    want_b, want_r, left = M.encode_sets(desc, records, total, sets, start)
    assert not want_r["flags"].any()
    n_out = n_sub + 1
    state, rate = CS.padded(n_out)
    out_set = np.array([M.NO_SET if s % 5 == 4 else s + 1 for s in range(n_sub)], np.uint32)
    os_, or_ = CS.sentinel_sets(n_out)
    got_b, got_r = CS.run_encode(hip, desc, records, total, state, rate, start, out_set, os_, or_)
    assert np.array_equal(got_r, want_r), np.flatnonzero(got_r != want_r)
    CS.same_coded_bytes(desc, got_b, want_b, want_r)
    CS.check_out_sets(os_, or_, n_out, {s + 1: left[s] for s in range(n_sub) if s % 5 != 4})


# ------------------------------------------------------------------ what the batches hold (CPU)
def _group_steps(recs, group):
    lens = np.array([len(r) for r in recs] + [0] * (-len(recs) % group)).reshape(-1, group)
    return lens, _steps(lens.max(axis=1))


@pytest.mark.parametrize("group,big", [(4, False), (16, True)])
def test_batches_reach_what_they_claim(group, big):
    # every loop length: the longest substream of a workgroup is L for every L in 0 .. 97 — 0 to 7 steps, every residue of a
    # step and both parities of the step count — and it stands at every place of a workgroup
    recs = _padded(_loop_length_recs(group), group, big)
    lens, steps = _group_steps(recs, group)
    assert set(range(98)) <= set(lens.max(axis=1).tolist()) and set(steps.tolist()) >= set(range(8))
    assert all(lens[L][L % group] == L for L in range(98))
    assert (len(recs) >= BIG_MIN) == big and len(recs) % group == 1          # the geometry, and one live substream at the end
    # ragged: every rotation, five steps between the shortest and the longest of a workgroup
    rag = _ragged_lens(group)
    assert len(rag) == group and all(_steps(max(l)) - _steps(min(l)) == 5 for l in rag)
    for k in range(group):
        assert {l[k] for l in rag} == set(rag[0])
    # record kinds: each kind at each of the 32 places of the first and of the last pair, nowhere else
    recs, where = _kind_recs()
    assert sorted(where) == sorted((n, p, q) for n in KINDS for p in (0, N_PAIRS - 1) for q in range(32))
    for r, (name, pair, place) in zip(recs, where):
        assert len(r) == 32 * N_PAIRS + 1 and r[32 * pair + place] == KINDS[name]
        if name.startswith("ctx") or name in ("align", "trm1"):
            assert list(np.flatnonzero((r[:-1] & 0x1FF) == (int(KINDS[name]) & 0x1FF))) == [32 * pair + place]
    # repeats: inside a step (twice, more than twice, all sixteen), over the middle of a pair, over two pairs
    in_step = [len(p) for p in REPEATS.values() if len({q // 16 for q in p}) == 1]
    assert 2 in in_step and 16 in in_step and any(2 < n < 16 for n in in_step)
    assert any({q // 16 for q in p} == {0, 1} for p in REPEATS.values())       # steps 0 and 1: one pair
    assert any({q // 16 for q in p} == {1, 2} for p in REPEATS.values())       # steps 1 and 2: two pairs
    for r, places in zip(_repeat_recs()[::3], REPEATS.values()):
        assert tuple(np.flatnonzero((r & 0x1FF) == QUIET)) == places
    # every id, both bins
    assert sorted(int(r[0]) for r in _every_id_recs()) == sorted(i | b << 15 for i in range(512) for b in (0, 1))
