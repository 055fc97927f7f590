"""The lane groups of the lane-serial encoder (encode_kernel_v7): its low wave gives a substream FOUR lanes, a quarter of a
step's sixteen bins each, and joins the quarters over the DPP quad; its one output wave gives a substream four lanes, a post
each, stores at most four units of a step with the lanes and sends a step of more through the serial path; a workgroup of
sixteen substreams is seven waves.

Every GPU case is coded by the device into a buffer full of a sentinel and compared with the oracle's coding (emit_model.Slots:
bytes up to ceil(n_bits / 8), n_bits, flags, and nothing written outside a slot), under variant 7 with fewer than 1 024
substreams (encode_kernel_v7<1>, workgroups of four) and padded past 1 024 with short filler (encode_kernel_v7<4>, workgroups of
sixteen, the last one with ONE live substream).  Substreams have at most about 100 records.

The cases are built from context-free records (bypass, terminate, align), whose arithmetic emit_model.Coder restates exactly, so
that the CPU tests below can say which quarter of which step does what (walk) and fail when a batch stops reaching a branch.
What the device must produce always comes from the oracle.

Units of a step: a bin shifts by at most seven bits, so a step carries at most 16 * 7 + 15 = 127 bits: SEVEN units, not eight."""
import functools

import numpy as np
import pytest

import emit_model as M
import helpers as H

EP0, EP1, TRM0, TRM1, ALIGN = M.EP0, M.EP1, M.TRM0, M.TRM1, M.ALIGN
BIG_MIN = 1024
GEOMETRIES = {"v7x1": False, "v7x4": True}
MAX_LEN = 110


# ------------------------------------------------------------------ what a substream does, quarter by quarter (CPU)
def walk(records):
    """-> [step][quarter] dicts for a context-free substream, as the low wave and the output stage see it:
    bins (records of the substream in the quarter), shifts, pend_in, pend_out (before the cut), units, carry (the post holds
    a carry above its units), cross_inside / cross_at_end (pend passes 16 before / reaches exactly 16 with the quarter's last
    bin), run_carry (the carry goes through a 0xFFFF run), and per step: m, plain (the step can take the output wave's lane
    path: one unit buffered, no run, no new 0xFFFF unit; room is the caller's business)."""
    c, low, pend = M.Coder(), 0, 0
    buf_n, steps = 0, []
    n = len(records)
    for base in range(0, max(n, 1), 16):
        quarters, leads = [], []
        for q in range(4):
            info = {"bins": 0, "shifts": 0, "pend_in": pend, "cross_inside": False, "cross_at_end": False}
            for i in range(4 * q, 4 * q + 4):
                if base + i < n:
                    before = c.low
                    sh = c.put(records[base + i])
                    low = (low << sh) + (c.low - (before << sh))
                    was = pend
                    pend += sh
                    info["bins"] += 1
                    info["shifts"] += sh
                    if was < 16 <= pend:
                        if i & 3 != 3:
                            info["cross_inside"] = True
                        elif pend == 16:
                            info["cross_at_end"] = True
            info["pend_out"] = pend
            info["units"], info["carry"] = pend >> 4, False
            if pend >= 16:
                keep, nun = pend & 15, pend >> 4
                v = low >> (9 + keep)
                info["carry"] = bool(v >> (16 * nun))
                leads += [(v >> 16, q), (v & 0xFFFF, q)] if nun == 2 else [(v, q)]
                low &= (1 << (9 + keep)) - 1
                pend = keep
            info["run_carry"] = False
            quarters.append(info)
        m = len(leads)
        plain = m == 0 or buf_n == 1
        for lead, q in leads:
            if lead >> 16 and buf_n >= 2:
                quarters[q]["run_carry"] = True
            if lead == 0xFFFF:
                plain = False
                buf_n += 1
            else:
                buf_n = 1
        steps.append({"quarters": quarters, "m": m, "plain": plain})
    return steps


# ------------------------------------------------------------------ batches
@functools.lru_cache(None)
def _filler():
    rng = np.random.default_rng(6200)
    return [H.random_records(rng, int(rng.integers(0, 40))) for _ in range(BIG_MIN + 64)]


def _padded(recs, caps, big):
    """Whole workgroups of sixteen as given; with `big`, filler past 1 024 substreams and the first case once more, alone in
    the last workgroup.  caps: None (roomy: N + 1 bytes) or the capacity per case."""
    recs = [np.asarray(r, np.uint16) for r in recs]
    caps = [None] * len(recs) if caps is None else list(caps)
    assert len(recs) % 16 == 0 and max(len(r) for r in recs) <= MAX_LEN
    if big:
        n = max(len(recs), BIG_MIN)
        n = (n + 15) // 16 * 16
        fill = _filler()[:n - len(recs)]
        recs, caps = recs + fill + [recs[0]], caps + [None] * (len(fill) + 1)
        assert len(recs) >= BIG_MIN and len(recs) % 16 == 1
    else:
        assert len(recs) < BIG_MIN
    return recs, caps


def _slots(recs, caps, seed):
    rng = np.random.default_rng(seed)
    qps, inits = rng.integers(20, 45, len(recs)), rng.integers(0, 3, len(recs))
    caps = [len(M.roomy(r, qps[s], inits[s])[0]) + 1 if caps[s] is None else caps[s] for s, r in enumerate(recs)]
    return M.Slots(recs, caps, qps, inits)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _check(hip, slots):
    n = len(slots.desc)
    d_desc, d_rec = _dev(slots.desc), _dev(np.concatenate([slots.records, np.zeros(8, np.uint16)]))
    d_bytes = _dev(slots.fresh())
    d_res = _dev(np.full(2 * n + 16, 0x5A5A5A5A, np.uint32))
    hip.encode_device(n, d_desc.data_ptr(), d_rec.data_ptr(), d_bytes.data_ptr(), d_res.data_ptr())
    hip.synchronize()
    res = d_res.cpu().numpy().view(np.uint32)
    assert (res[2 * n:] == 0x5A5A5A5A).all()
    slots.check(d_bytes.cpu().numpy(), res[:2 * n].view(H.RESULT_DTYPE))


@pytest.fixture(scope="module", params=list(GEOMETRIES), ids=list(GEOMETRIES))
def enc(request):
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    c.set_variant(7, 0)
    yield c, GEOMETRIES[request.param]
    c.close()


# ------------------------------------------------------------------ 1. the quarters of the low wave
EVENTS = ("cross_inside", "cross_at_end", "two_units", "late_carry", "run_carry", "no_shift", "ends_inside")


def _quarter_events(r):
    """{(event, quarter)} of one context-free substream."""
    got = set()
    steps = walk(r)
    posted_before = False
    for st in steps:
        for q, info in enumerate(st["quarters"]):
            if info["cross_inside"]:
                got.add(("cross_inside", q))
            if info["cross_at_end"]:
                got.add(("cross_at_end", q))
            if info["units"] == 2:
                got.add(("two_units", q))
            # a carry that leaves this quarter's partial and lands in bits an earlier quarter posted (of this step, or for
            # quarter 0 of a step before)
            if info["carry"] and posted_before:
                got.add(("late_carry", q))
            posted_before = posted_before or info["units"] > 0
            if info["run_carry"]:
                got.add(("run_carry", q))
            if info["bins"] == 4 and info["shifts"] == 0:
                got.add(("no_shift", q))
    if len(r) % 16:
        got.add(("ends_inside", (len(r) % 16 - 1) // 4))
    return got


@functools.lru_cache(None)
def _quarter_pool():
    """Candidates: the constructed crossings of emit_model (carries into 0xFFFF runs, in every lane and post), bursts of TRM 1
    (posts of two units), random context-free substreams with align / TRM 0 stretches (quarters that shift nothing) of every
    length mod 16."""
    pool = []
    for K in (1, 2):
        for f in range(16):
            for e in range(16):
                seed = 6300 + (K * 16 + f) * 16 + e
                recs, _ = M.head(f, e, 16 * K + 8, seed)
                tail = M.free_records(np.random.default_rng(seed + 1), (f * 5 + e) % 19, trm1=False)
                pool.append(np.array(recs + tail + [TRM1], np.uint16))
    rng = np.random.default_rng(6301)
    for k in range(600):
        n = int(rng.integers(20, 100))
        r = M.free_records(rng, n)
        at, span = int(rng.integers(0, n)), int(rng.integers(4, 12))
        r[at:at + span] = [ALIGN] * len(r[at:at + span])
        if k % 3 == 0:
            at = int(rng.integers(0, n))
            r[at:at + 5] = [TRM1] * len(r[at:at + 5])
        pool.append(np.array(r, np.uint16))
    return [p for p in pool if len(p) <= MAX_LEN]


@functools.lru_cache(None)
def _quarter_cases():
    """For every (event, quarter) sixteen substreams that reach it, one per position of a workgroup (distinct ones as far as the
    pool has them).  -> (records list, [(event, quarter)] per workgroup)."""
    pool = _quarter_pool()
    events = [_quarter_events(p) for p in pool]
    recs, what = [], []
    for ev in EVENTS:
        for q in range(4):
            have = [i for i, e in enumerate(events) if (ev, q) in e]
            assert have, (ev, q)
            start = (len(recs) // 16) * 7                 # not the same sixteen for every event
            recs += [pool[have[(start + p) % len(have)]] for p in range(16)]
            what.append((ev, q))
    return recs, what


@functools.lru_cache(None)
def _quarter_slots(big):
    recs, caps = _padded(_quarter_cases()[0], None, big)
    return _slots(recs, caps, 6302)


def test_quarter_cases_reach_what_they_claim():
    """The census: every event in every quarter 0 .. 3 at every substream position mod 16 (and so mod 4)."""
    recs, what = _quarter_cases()
    assert sorted(what) == sorted((ev, q) for ev in EVENTS for q in range(4))
    for g, (ev, q) in enumerate(what):
        for p in range(16):
            assert (ev, q) in _quarter_events(recs[16 * g + p]), (ev, q, p)
    for big in (False, True):
        padded = _padded(recs, None, big)[0]
        assert [len(a) for a in padded[:len(recs)]] == [len(a) for a in recs]      # positions mod 16 as built
        assert (len(padded) >= BIG_MIN) == big
    # the model agrees with the replay of emit_model on what leaves a substream
    for r in recs[::37]:
        assert max(st["m"] for st in walk(r)) == M.Replay(r).max_units


@pytest.mark.gpu
def test_quarters_of_the_low_wave(enc):
    hip, big = enc
    _check(hip, _quarter_slots(big))


# ------------------------------------------------------------------ 2. units per step
def _unit_step(m, rng):
    """A substream whose step 2 produces exactly m units from a pend of 15, with one unit buffered in front of it: step 0 sixteen
    bypass bins (the first unit), step 1 fifteen and an align (pend 15), step 2 a TRM 1 and b bypass bins in random order
    with 16 m <= 15 + 7 a + b <= 16 m + 15, the rest align; then a short tail.  Searched until step 2 is plain in everything
    but its unit count; six and seven units need twelve and more TRM 1, which leave 0xFFFF units whatever stands between them,
    so those steps are not plain on that account as well."""
    plain_only = m <= 5
    for _ in range(400):
        ab = [(a, b) for a in range(17) for b in range(17 - a) if 16 * m <= 15 + 7 * a + b <= 16 * m + 15]
        a, b = ab[int(rng.integers(0, len(ab)))]
        step = [TRM1] * a + [EP1 if rng.integers(0, 2) else EP0 for _ in range(b)] + [ALIGN] * (16 - a - b)
        step = [step[i] for i in rng.permutation(16)]
        head = [EP1 if rng.integers(0, 2) else EP0 for _ in range(31)]
        head.insert(16 + int(rng.integers(0, 16)), ALIGN)
        r = np.array(head + step + M.free_records(rng, int(rng.integers(0, 20)), trm1=False) + [TRM1], np.uint16)
        steps = walk(r)
        if steps[2]["m"] == m and steps[0]["m"] == 1 and steps[1]["m"] == 0 and (steps[2]["plain"] or not plain_only):
            return r
    raise AssertionError("no step of %d units found" % m)


@functools.lru_cache(None)
def _unit_cases():
    """m = 0 .. 4: a workgroup of sixteen such substreams (every lane of the output wave on the lane path in step 2).
    m = 5 .. 7: per position p a workgroup whose substream p has the step of m units and the other fifteen one of 0 .. 4 — the
    step takes the serial path because of that one.  -> (records list, [(m, p or None)] per workgroup)."""
    rng = np.random.default_rng(6400)
    recs, what = [], []
    for m in range(5):
        recs += [_unit_step(m, rng) for _ in range(16)]
        what.append((m, None))
    for m in (5, 6, 7):
        for p in range(16):
            recs += [_unit_step(m if k == p else (k + p) % 5, rng) for k in range(16)]
            what.append((m, p))
    return recs, what


def _tight_caps(recs):
    """Capacities that end inside step 2: the m units of the step (the buffered one and m - 1 new ones stored, 2 m bytes) do not
    fit by one byte.  m = 0 stores nothing there: one byte."""
    return [max(2 * walk(r)[2]["m"] - 1, 1) for r in recs]


@functools.lru_cache(None)
def _unit_slots(big, tight):
    recs = _unit_cases()[0]
    recs, caps = _padded(recs, _tight_caps(recs) if tight else None, big)
    return _slots(recs, caps, 6401)


def test_unit_cases_reach_what_they_claim():
    recs, what = _unit_cases()
    assert len(recs) < BIG_MIN
    assert sorted(what) == sorted([(m, None) for m in range(5)] + [(m, p) for m in (5, 6, 7) for p in range(16)])
    for g, (m, p) in enumerate(what):
        group = [walk(r)[2] for r in recs[16 * g:16 * g + 16]]
        # nothing but the count sends the step to the serial path (six and seven units: 0xFFFF units too, see _unit_step)
        assert all(st["plain"] for k, st in enumerate(group) if k != p or m <= 5)
        if p is None:
            assert [st["m"] for st in group] == [m] * 16              # every position mod 16, all on the lane path
        else:
            assert group[p]["m"] == m and all(st["m"] <= 4 for k, st in enumerate(group) if k != p)
    # with the tight capacities the step's units end one byte outside the slot: room = cap - pos - 2 m = -1 at step 2
    for r, cap in zip(recs, _tight_caps(recs)):
        st = walk(r)
        assert st[0]["m"] == 1 and st[1]["m"] == 0                     # one unit buffered, nothing stored yet: pos = 0
        assert cap - 2 * st[2]["m"] == -1 or st[2]["m"] == 0
    assert max(st["m"] for r in recs for st in walk(r)) == 7           # 16 * 7 + 15 = 127 bits: never eight
    slots = _slots(*_padded(recs, _tight_caps(recs), False), 6401)
    over = slots.results["flags"] == H.RES_OVERFLOW
    assert over.sum() >= len(recs) - 16 * 17                            # all but the steps of no unit overflow


@pytest.mark.gpu
@pytest.mark.parametrize("tight", [False, True], ids=["room", "tight"])
def test_units_per_step(enc, tight):
    hip, big = enc
    _check(hip, _unit_slots(big, tight))


# ------------------------------------------------------------------ 3. the seven-wave geometry
def _geometry_recs(n_sub):
    """n_sub substreams of 0 .. 60 records; zero-length ones at lanes 0 and 15 of every third workgroup."""
    rng = np.random.default_rng(6500 + n_sub)
    recs = []
    for s in range(n_sub):
        empty = (s // 16) % 3 == 0 and s % 16 in (0, 15)
        recs.append(np.zeros(0, np.uint16) if empty else H.random_records(rng, int(rng.integers(1, 60))))
    return recs


@functools.lru_cache(None)
def _geometry_slots(n_sub):
    recs = _geometry_recs(n_sub)
    return _slots(recs, [None] * n_sub, 6501)


def test_geometry_batches_reach_what_they_claim():
    for r in (1, 15, 16, 17):
        recs = _geometry_recs(BIG_MIN + r)
        assert len(recs) % 16 == r % 16 and len(recs) >= BIG_MIN
        empty = [s for s, a in enumerate(recs) if len(a) == 0]
        assert {s % 16 for s in empty} == {0, 15} and len(empty) >= 40
        assert (len(recs) - 1) // 16 % 3 != 0 or len(recs[-1]) == 0 or (len(recs) - 1) % 16 not in (0, 15)


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 15, 16, 17])
def test_seven_wave_geometry(r):
    """1 024 + r substreams through encode_kernel_v7<4>: the last workgroup holds r % 16 live substreams (sixteen for r = 16);
    zero-length substreams at lanes 0 and 15 of a workgroup."""
    hip = H.gpu_ctx()
    try:
        hip.set_variant(7, 0)
        _check(hip, _geometry_slots(BIG_MIN + r))
    finally:
        hip.close()


@pytest.mark.gpu
def test_context_sets_entry_point():
    """encode_kernel_v7<4, CtxSets>, once: the context-sets case of tests/test_gpu_encode_two_step.py in the big geometry."""
    import test_gpu_encode_two_step as T
    hip = H.gpu_ctx()
    try:
        hip.set_variant(7, 0)
        T.test_context_sets_after_one_to_four_steps((hip, 16, True))
    finally:
        hip.close()
