"""GPU: the plan rows (include/cabac_hip_plan_rows.h) — the plan parse and the plan write from and into context sets and over
WPP rows — against tests/plan_rows_model.py (parse_plan_model's fill / expand, the oracle's coder from a start set, the level
loop of ctx_sets_model) and against the plain calls.  Everything is bit-exact: == on integers.  Expected values never come from
the code under test.  Outputs sit between guard words that are checked.

Rows are made of parse_plan_model.tu_case units: 24 entries and three blocks per unit, three units and the terminate bin make a
row of 73 entries, which crosses the walk's 64-entry group boundary."""
import functools

import numpy as np
import pytest

import ctx_sets_model as CS
import helpers as H
import parse_elements_model as E
import parse_plan_model as PM
import plan_rows_model as R
import write_plan_model as W
from entropy_coding_amd import capi
from test_gpu_parse_elements import VAL_GUARD, WORD_GUARD_U, Out
from test_gpu_parse_plan import _flip_middle
from test_gpu_parse_plan import run as run_plain
from test_gpu_parse_unit import coded, dev, sentinel, t_or_dummy
from test_gpu_residual_estimate import make_sets, pack_sets

pytestmark = pytest.mark.gpu

NO = R.NO_SET
G = 64
SET_GUARD, RATE_GUARD = 0x0BADC0DE, 0xC3
BYTE_GUARD, OFF_GUARD, RES_GUARD = 0xA5, -7, -0x11223345
N_SETS = 16
ROW3 = 3 * PM.TU_LEN + 1
# three units of a row: everything coded; tu_cbf_cr skipped by its guard and the Cr block skipped; transform skip, Cb skipped
OUTCOMES3 = [(1, 1, 1, 0, 0, 0), (1, 0, 1, 0, 0, 0), (0, 1, 1, 1, 0, 0)]


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def start_sets():
    return make_sets(np.random.default_rng(0x5E75), N_SETS)


def unit_of(row, w, data=None):
    """The parser's input of a written row (parse_plan_model's unit)"""
    return dict(plan=row["plan"], metas=row["metas"], blocks=row["blocks"], at=row["at"], guards=row["guards"], qp=row["qp"],
                finish=True, data=w["data"] if data is None else data, values=w["values"], infos=w["infos"], coded=w["coded"])


def no_skips(rows):
    """The model skips no case: every row is one the plan write codes"""
    skipped = [s for s, r in enumerate(rows) if W.stop_of(r["plan"], r["real"], r["metas"], r["blocks"], r["at"], r["guards"]) != 0]
    assert skipped == []


class SetsOut:
    """Out arrays of n_sets sets between guard sets"""

    def __init__(self, n_sets, init=None):
        import torch
        self.n = n_sets
        st = np.full((n_sets + 2) * H.NUM_CTX, SET_GUARD, np.uint32)
        rt = np.full((n_sets + 2) * H.NUM_CTX, RATE_GUARD, np.uint8)
        if init is not None:
            st[H.NUM_CTX:-H.NUM_CTX], rt[H.NUM_CTX:-H.NUM_CTX] = init
        self.st, self.rt = dev(st.view(np.int32)), dev(rt)
        self.p_state, self.p_rate = self.st.data_ptr() + 4 * H.NUM_CTX, self.rt.data_ptr() + H.NUM_CTX

    def read(self):
        st, rt = self.st.cpu().numpy().view(np.uint32), self.rt.cpu().numpy()
        n = H.NUM_CTX
        assert (st[:n] == SET_GUARD).all() and (st[-n:] == SET_GUARD).all() and (rt[:n] == RATE_GUARD).all() and (rt[-n:] == RATE_GUARD).all()
        return st[n:-n].reshape(self.n, n), rt[n:-n].reshape(self.n, n)


def parse(hip, units, int16=False, entry="sets", start=None, out_set=None, out_at=None, in_place=False, rows=None, n_sets=N_SETS):
    """cabac_hip_plan_parse_sets_device ("sets") or cabac_hip_plan_parse_rows_device ("rows", rows = (level_first, sync_from,
    sync_at)) over `units` -> test_gpu_parse_plan.run's dict plus sets = (state, rate) of the out arrays"""
    P = PM.pack(units)
    out = Out(P, int16)
    t_desc, t_buf = dev(P["desc"], np.uint8), dev(P["bytes"])
    t_first, t_tu = dev(P["tile_first"].view(np.int32)), t_or_dummy(P["tus"][:P["n_tu"]], np.uint8)
    t_at = None if P["tu_at"] is None else t_or_dummy(P["tu_at"].view(np.int32), None)
    t_guard = None if P["tu_guard"] is None else t_or_dummy(P["tu_guard"].view(np.int32), None)
    t_plan = t_or_dummy(P["plan"].view(np.int32), None)
    p_co, p_val, p_info, p_res = out.ptrs()
    n_el = len(P["plan"])
    args = (len(units), t_desc.data_ptr(), t_buf.data_ptr(), t_first.data_ptr(), t_tu.data_ptr() if P["n_tu"] else 0,
            t_at.data_ptr() if t_at is not None else 0, t_guard.data_ptr() if t_guard is not None else 0,
            t_plan.data_ptr() if n_el else 0, p_co if P["n_tu"] else 0, p_val if n_el else 0, p_res)
    sets = None
    if entry == "sets":
        packed = pack_sets(start_sets()[:n_sets])
        t_state, t_rate = dev(packed[0].view(np.int32)), dev(packed[1])
        so = SetsOut(n_sets, packed if in_place else None)
        u32 = lambda a: None if a is None else dev(np.asarray(a, np.uint32).view(np.int32))
        t_start, t_out, t_oat = u32(start), u32(out_set), u32(out_at)
        ptr = lambda t: t.data_ptr() if t is not None else 0
        hip.plan_parse_sets_device(*args, d_tu_info=p_info, int16=int16, n_sets=n_sets,
                                   d_state=so.p_state if in_place else t_state.data_ptr(), d_rate=so.p_rate if in_place else t_rate.data_ptr(),
                                   d_start_set=ptr(t_start), d_out_set=ptr(t_out), d_out_state=so.p_state, d_out_rate=so.p_rate,
                                   d_out_at=ptr(t_oat))
        hip.synchronize()
        sets = so.read()
        if not in_place:
            assert np.array_equal(t_state.cpu().numpy().view(np.uint32), packed[0]) and np.array_equal(t_rate.cpu().numpy(), packed[1])
    else:
        level_first, sync_from, sync_at = rows
        t_from, t_sat = dev(np.asarray(sync_from, np.uint32).view(np.int32)), dev(np.asarray(sync_at, np.uint32).view(np.int32))
        hip.plan_parse_rows_device(*args, level_first, t_from.data_ptr(), t_sat.data_ptr(), d_tu_info=p_info, int16=int16)
        hip.synchronize()
    co, val, info, res = out.read()
    blocks, per_val, per_info, t = [], [], [], 0
    for s, u in enumerate(units):
        bl = []
        for m in u["metas"]:
            bl.append(co[int(P["offsets"][t]): int(P["offsets"][t]) + m[0] * m[1]].reshape(m[1], m[0]))
            t += 1
        blocks.append(bl)
        per_info.append(info[t - len(bl):t])
        r0 = int(P["desc"]["rec_offset"][s])
        per_val.append(val[r0:r0 + len(u["plan"])])
    return dict(P=P, co=co, values=per_val, all_values=val, info=info, infos=per_info, res=res, blocks=blocks, sets=sets)


def assert_row(r, s, row, w, what=""):
    """Substream s came back as the model wrote it"""
    n_bits, flags, _ = R.read_row(row, w)
    assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (n_bits, flags), (what, s)
    assert r["values"][s].tolist() == w["values"], (what, s)
    assert r["infos"][s].tolist() == w["infos"], (what, s)
    for k, on in enumerate(w["coded"]):
        if on:
            assert np.array_equal(coded(r["blocks"][s][k]), coded(row["blocks"][k])), (what, s, k)
        else:
            assert (r["blocks"][s][k] == np.int32(np.int16(sentinel(True)) if r.get("int16") else sentinel(False))).all(), (what, s, k)


def assert_untouched(r, s, int16, what=""):
    """Substream s wrote no value, coefficient or info word"""
    assert (r["values"][s] == VAL_GUARD).all() and (r["infos"][s] == WORD_GUARD_U).all(), (what, s)
    want = np.int32(np.int16(sentinel(True))) if int16 else np.int32(sentinel(False))
    for b in r["blocks"][s]:
        assert (b == want).all(), (what, s)


def assert_set(sets, k, ctx, what=""):
    state, rate = CS.pack(ctx)
    assert np.array_equal(sets[0][k], state), what
    assert np.array_equal(sets[1][k], rate), what


def assert_set_guard(sets, k, what=""):
    assert (sets[0][k] == SET_GUARD).all() and (sets[1][k] == RATE_GUARD).all(), what


# ---------------------------------------------------------------------------------------------- the shared batch
@functools.lru_cache(maxsize=None)
def wpp():
    """Three pictures of four ragged rows in level order, and what the model makes of them"""
    rows, level_first, sync_from, sync_at = R.batch(0x9B01)
    no_skips(rows)
    written, ok = R.rows(rows, level_first, sync_from, sync_at)
    assert all(ok)
    assert len(rows[0]["plan"]) == ROW3 and {len(r["plan"]) for r in rows} == {PM.TU_LEN + 1, 2 * PM.TU_LEN + 1, ROW3}
    assert sorted(set(int(a) for a in sync_at) - {len(r["plan"]) for r in rows}) == [0, PM.TU_LEN, 10 ** 6]
    assert int(sync_from[2 * 3 + 1]) == NO and sum(int(f) != NO for f in sync_from) == 8
    return rows, level_first, sync_from, sync_at, written


@functools.lru_cache(maxsize=None)
def unlinked():
    """The same rows, each written from Ctx::init: the plan parse's own input"""
    rows = wpp()[0]
    n = len(rows)
    written, _ = R.rows(rows, [0, n], [NO] * n, [0] * n)
    return rows, written


# ---------------------------------------------------------------------------------------------- 1. no set: the plan parse
@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_sets_form_with_no_set_is_the_plan_parse(hip, int16):
    rows, written = unlinked()
    units = [unit_of(r, w) for r, w in zip(rows, written)]
    rng = np.random.default_rng(0x9B02)
    flipped = [_flip_middle(rng, u) for u in units]
    for what, us in (("valid", units), ("flipped", flipped)):
        a = run_plain(hip, us, int16)
        for start, out_set in ((None, None), ([NO] * len(us), None), ([NO] * len(us), [NO] * len(us))):
            b = parse(hip, us, int16, start=start, out_set=out_set, out_at=None if start is None else [5] * len(us))
            for key in ("co", "all_values", "info", "res"):
                assert np.array_equal(a[key], b[key]), (what, key, start is None)
            for k in range(N_SETS):
                assert_set_guard(b["sets"], k)
    assert any(int(f) != 0 for f in run_plain(hip, flipped, int16)["res"]["flags"]), "the flips change nothing"


# ---------------------------------------------------------------------------------------------- 2. start sets, hand-over point
@functools.lru_cache(maxsize=None)
def handover_cases():
    """[(row, k, start set index or NO)]: the hand-over indices of the issue on rows of three units"""
    rng = np.random.default_rng(0x9B03)
    base = lambda: R.tu_row(rng, OUTCOMES3)
    cases = []
    ks = [0, PM.TU_BLOCK_AT, 11, PM.TU_LEN, 63, 64, 65, ROW3, ROW3 + 5,
          PM.TU_LEN + 1,                       # tu_cbf_cr of the second unit on the context of cbf_cb == 0: skipped by its guard
          PM.TU_LEN + 3,                       # a computed entry (COND)
          PM.TU_LEN + PM.TU_BLOCK_AT,          # the position of the second unit's blocks, the Cr one skipped
          PM.TU_LEN + PM.TU_BLOCK_AT + 1]
    for j, k in enumerate(ks):
        cases.append((base(), k, NO if j % 4 == 3 else (5 * j) % N_SETS))
    # a unit that BEGINS WITH A BLOCK behind a zero-bin marker: the marker is entry TU_LEN, the block stands at TU_LEN + 1
    row = R.tu_row(rng, OUTCOMES3, marker=True)
    meta, c = PM.chroma_block(rng)
    row["metas"].insert(3, meta)
    row["blocks"].insert(3, np.asarray(c, np.int32))
    row["at"].insert(3, PM.TU_LEN + 1)
    row["guards"].insert(3, 0)
    for k in (PM.TU_LEN, PM.TU_LEN + 1):
        cases.append((row, k, 7))
    no_skips([c[0] for c in cases])
    out = []
    for row, k, st in cases:
        w = R.write_row(row, R.start_of(row, start_sets(), st), k)
        out.append((row, k, st, w))
    # the cases are what their comments say
    w = out[9][3]
    assert w["values"][PM.TU_LEN] == 1 and not PM.E.guard_holds(out[9][0]["plan"][PM.TU_LEN + 1, 1], w["values"], PM.TU_LEN + 1)
    assert PM.is_computed(out[10][0]["plan"][PM.TU_LEN + 3, 0]) and out[11][3]["coded"][3:6] == [True, False, True]
    a, b = out[-2][3], out[-1][3]
    assert np.array_equal(a["string"], b["string"]) and b["at_rec"] > a["at_rec"] and a["coded"][3]
    assert out[1][3]["at_rec"] > out[0][3]["at_rec"] == 0
    return out


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_start_sets_and_the_hand_over_point(hip, int16):
    cases = handover_cases()
    units = [unit_of(row, w) for row, _, _, w in cases]
    n = len(cases)
    assert n <= N_SETS
    out_set = [(s * 7) % N_SETS for s in range(n)]                  # a permutation: 7 and 16 are coprime
    out_set[2] = NO
    r = parse(hip, units, int16, start=[c[2] for c in cases], out_set=out_set, out_at=[c[1] for c in cases])
    r["int16"] = int16
    written = set()
    for s, (row, k, st, w) in enumerate(cases):
        assert_row(r, s, row, w, ("k", k))
        if out_set[s] != NO:
            assert_set(r["sets"], out_set[s], w["handed"], ("k", k))
            written.add(out_set[s])
    for k in set(range(N_SETS)) - written:
        assert_set_guard(r["sets"], k)


def test_out_at_null_hands_over_the_end_of_the_substream(hip):
    cases = handover_cases()[:3]
    units = [unit_of(row, w) for row, _, _, w in cases]
    r = parse(hip, units, start=[c[2] for c in cases], out_set=[0, 1, 2], out_at=None)
    for s, (row, k, st, w) in enumerate(cases):
        assert_row(r, s, row, w)
        assert_set(r["sets"], s, w["left"])


# ---------------------------------------------------------------------------------------------- 3. bad set
def test_a_bad_set_index_parses_nothing_and_touches_nothing(hip):
    cases = handover_cases()[:6]
    units = [unit_of(row, w) for row, _, _, w in cases]
    start = [c[2] for c in cases]
    out_set = [0, 1, 2, 3, 4, 5]
    start[1], out_set[3], out_set[4] = N_SETS, N_SETS + 3, 0xFFFFFFFE
    r = parse(hip, units, start=start, out_set=out_set, out_at=[c[1] for c in cases])
    for s, (row, k, st, w) in enumerate(cases):
        if s in (1, 3, 4):
            assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (0, capi.RES_BAD_SET), s
            assert_untouched(r, s, False)
            if out_set[s] < N_SETS:
                assert_set_guard(r["sets"], out_set[s])
        else:
            assert_row(r, s, row, w)
            assert_set(r["sets"], out_set[s], w["handed"])
    for k in range(6, N_SETS):
        assert_set_guard(r["sets"], k)


# ---------------------------------------------------------------------------------------------- 4. in place
def test_the_out_set_may_be_the_substreams_own_start_set(hip):
    cases = [c for c in handover_cases() if c[2] != NO]
    seen, pick = set(), []
    for c in cases:                                                 # no other substream of the call starts from it
        if c[2] not in seen:
            seen.add(c[2])
            pick.append(c)
    assert len(pick) >= 6
    units = [unit_of(row, w) for row, _, _, w in pick]
    r = parse(hip, units, start=[c[2] for c in pick], out_set=[c[2] for c in pick], out_at=[c[1] for c in pick], in_place=True)
    for s, (row, k, st, w) in enumerate(pick):
        assert_row(r, s, row, w)
        assert_set(r["sets"], st, w["handed"])
    for k in set(range(N_SETS)) - seen:
        assert_set(r["sets"], k, start_sets()[k])


# ---------------------------------------------------------------------------------------------- 5. rows parsed
@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_rows_parse_device_form(hip, int16):
    rows, level_first, sync_from, sync_at, written = wpp()
    units = [unit_of(r, w) for r, w in zip(rows, written)]
    r = parse(hip, units, int16, entry="rows", rows=(level_first, sync_from, sync_at))
    r["int16"] = int16
    for s, (row, w) in enumerate(zip(rows, written)):
        assert_row(r, s, row, w, "rows")
    # what the links are worth: read from Ctx::init a linked row is not what was written
    plain = run_plain(hip, units, int16)
    differ = [s for s in range(len(rows)) if int(sync_from[s]) != NO and int(sync_at[int(sync_from[s])]) != 0 and
              (plain["values"][s].tolist() != written[s]["values"] or int(plain["res"]["flags"][s]) != 0)]
    assert differ, "no linked row depends on its link"


def test_rows_parse_of_one_level_is_the_plain_call(hip):
    rows, written = unlinked()
    units = [unit_of(r, w) for r, w in zip(rows, written)]
    n = len(units)
    a = run_plain(hip, units)
    b = parse(hip, units, entry="rows", rows=([0, n], [NO] * n, [3] * n))
    for key in ("co", "all_values", "info", "res"):
        assert np.array_equal(a[key], b[key]), key


@functools.lru_cache(maxsize=None)
def wide_level():
    """1 027 rows of one transform unit each in level 0 — one launch of four-wave workgroups whose last one has three live waves —
    and five rows in level 1 that start from slots of level 0, the first and the last among them, and from Ctx::init.  Level 0
    repeats twelve rows (every row of it starts from Ctx::init, so the model codes each once); sync_at differs with the row."""
    rng = np.random.default_rng(0x9B04)
    n0, froms = 1027, [0, 511, 1026, NO, 1024]
    pool = [R.tu_row(rng, [(0, 0, 1, 0, 0, 0)]) for _ in range(12)]          # luma alone is coded: one small block per row
    ats = [5, 0, PM.TU_LEN, PM.TU_LEN + 1, 10 ** 6, 12]
    pool_w = [R.write_row(r, CS.init_set(r["qp"], 2), ats[k % len(ats)]) for k, r in enumerate(pool)]
    rows = [pool[s % 12] for s in range(n0)] + [R.tu_row(rng, [OUTCOMES3[k % 3]]) for k in range(len(froms))]
    sync_at = [ats[(s % 12) % len(ats)] for s in range(n0)] + [0] * len(froms)
    written = [pool_w[s % 12] for s in range(n0)]
    for k, f in enumerate(froms):
        row = rows[n0 + k]
        written.append(R.write_row(row, CS.init_set(row["qp"], 2) if f == NO else written[f]["handed"], 0))
    no_skips(pool + rows[n0:])
    return rows, [0, n0, n0 + len(froms)], [NO] * n0 + froms, sync_at, written


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_rows_parse_across_the_four_wave_switch(hip, int16):
    """Levels [0, 1027, 1032]: level 0 is at the parser's switch to four waves per workgroup (1 024 substreams in one launch), and
    level 1's pointers start 1 027 substreams into every per-substream array."""
    rows, level_first, sync_from, sync_at, written = wide_level()
    units = [unit_of(r, w) for r, w in zip(rows, written)]
    r = parse(hip, units, int16, entry="rows", rows=(level_first, sync_from, sync_at))
    r["int16"] = int16
    for s, (row, w) in enumerate(zip(rows, written)):
        assert_row(r, s, row, w, "wide level")
    # the links count: a linked row read from Ctx::init is not what was written
    linked = [s for s in range(level_first[1], level_first[2]) if sync_from[s] != NO and sync_at[sync_from[s]] != 0]
    plain = run_plain(hip, [units[s] for s in linked], int16)
    assert any(plain["values"][k].tolist() != written[s]["values"] or int(plain["res"]["flags"][k]) != 0 for k, s in enumerate(linked))


def _host_buffers(P, int16=False):
    return (np.full(P["total"], sentinel(int16), np.int16 if int16 else np.int32), np.full(len(P["plan"]), VAL_GUARD, np.uint32),
            np.full(P["n_tu"], WORD_GUARD_U, np.uint32))


def test_rows_parse_batch_form(hip):
    rows, level_first, sync_from, sync_at, written = wpp()
    units = [unit_of(r, w) for r, w in zip(rows, written)]
    r = parse(hip, units, entry="rows", rows=(level_first, sync_from, sync_at))
    P = r["P"]
    coeff, values, info = _host_buffers(P)
    host = capi.CabacHip(0)
    co, val, res, inf = host.plan_parse_rows_batch(P["desc"], P["bytes"], P["tile_first"], P["tus"][:P["n_tu"]], P["tu_at"], P["tu_guard"],
                                                   P["plan"], P["total"], level_first, sync_from, sync_at, coeff=coeff, values=values,
                                                   info=info)
    host.close()
    assert np.array_equal(res, r["res"]) and np.array_equal(inf, r["info"]) and np.array_equal(val, r["all_values"])
    assert np.array_equal(co, r["co"])


# ---------------------------------------------------------------------------------------------- 6. links and malformed input
def test_a_same_level_link_flags_that_substream_alone(hip):
    rows, level_first, sync_from, sync_at, written = wpp()
    units = [unit_of(r, w) for r, w in zip(rows, written)]
    bad = sync_from.copy()
    bad[3] = 4                                                      # picture 0, row 1 links into its own level
    r = parse(hip, units, entry="rows", rows=(level_first, bad, sync_at))
    assert (int(r["res"]["n_bits"][3]), int(r["res"]["flags"][3])) == (0, capi.RES_BAD_SET)
    assert_untouched(r, 3, False)
    for s, (row, w) in enumerate(zip(rows, written)):
        if s % 3 != 0:                                              # the other pictures stay exact
            assert_row(r, s, row, w, "other pictures")
        elif s > 3:                                                 # behind the refused row: unspecified contexts, no flag of its own kind
            assert not int(r["res"]["flags"][s]) & capi.RES_BAD_SET, s
    assert_row(r, 0, rows[0], written[0])
    # a link beyond the batch is refused in the same way
    bad = sync_from.copy()
    bad[5] = 0x7FFFFFFF
    r = parse(hip, units, entry="rows", rows=(level_first, bad, sync_at))
    assert (int(r["res"]["n_bits"][5]), int(r["res"]["flags"][5])) == (0, capi.RES_BAD_SET)
    for s in (0, 1, 3, 4, 6, 7, 9, 10):
        assert_row(r, s, rows[s], written[s])


def test_batch_forms_refuse_malformed_levels_and_links_with_nothing_touched(hip):
    rows, level_first, sync_from, sync_at, written = wpp()
    units = [unit_of(r, w) for r, w in zip(rows, written)]
    P = PM.pack(units)
    PW = R.pack(rows)
    host = capi.CabacHip(0)
    n = len(rows)
    same, later, beyond = sync_from.copy(), sync_from.copy(), sync_from.copy()
    same[3], later[3], beyond[3] = 4, 9, n
    for lf, sf in (([0, 3, 6, 9], sync_from), ([1, 3, 6, 9, n], sync_from), ([0, 6, 3, 9, n], sync_from), ([0, 3, 6, 9, n + 1], sync_from),
                   (level_first, same), (level_first, later), (level_first, beyond)):
        coeff, values, info = _host_buffers(P)
        with pytest.raises(capi.CabacHipError) as e:
            host.plan_parse_rows_batch(P["desc"], P["bytes"], P["tile_first"], P["tus"][:P["n_tu"]], P["tu_at"], P["tu_guard"], P["plan"],
                                       P["total"], lf, sf, sync_at, coeff=coeff, values=values, info=info)
        assert e.value.status == -2
        assert (coeff == sentinel(False)).all() and (values == VAL_GUARD).all() and (info == WORD_GUARD_U).all()
        payload = np.full(4096, BYTE_GUARD, np.uint8)
        values_out, info = np.full(len(PW["plan"]), VAL_GUARD, np.uint32), np.full(PW["n_tu"], WORD_GUARD_U, np.uint32)
        with pytest.raises(capi.CabacHipError) as e:
            host.plan_write_rows_batch(_write_desc(PW), PW["plan"], PW["values_in"], PW["tile_first"], PW["tus"][:PW["n_tu"]], PW["tu_at"],
                                       PW["tu_guard"], PW["coeff"], payload, lf, sf, sync_at, values_out=values_out, info=info)
        assert e.value.status == -2
        assert (payload == BYTE_GUARD).all() and (values_out == VAL_GUARD).all() and (info == WORD_GUARD_U).all()
    host.close()


# ---------------------------------------------------------------------------------------------- 7. damaged row 0
def _decoded_string(plan, values):
    return PM.expand(plan, values, [], [], None, None)[0]


def test_a_damaged_block_free_row_hands_over_what_it_decoded(hip):
    """Block-free plans: parse_plan_model.read_plan says what the damaged bytes decode to, and the hand-over contexts are the
    advance over the string of the DECODED values in front of the hand-over entry."""
    rng = np.random.default_rng(0x9B07)
    units, want, ks = [], [], []
    while len(units) < 6:
        plan, real = PM.random_cond_plan(rng, int(rng.integers(70, 140)), kinds=(E.CTX_BIN, E.EP_BINS, E.UNARY_MAX, E.UNARY_EP))
        plan, real = E.close(plan, real)
        u = PM.build(rng, plan, real)
        d = _flip_middle(rng, u)
        got = PM.read_plan(plan, d["data"], u["qp"], finish=True)
        if got["flags"] & ~H.RES_BAD_STOP or got["values"] == [v & 0xFFFFFFFF for v in u["values"]]:
            continue                                                # an underrun or a stop leaves the set unspecified; no change shows nothing
        if PM.dec_walk(plan, d["data"], u["qp"])[0] is not None:
            continue                                                # an element met OUT OF RANGE: unspecified from there on
        units.append(d)
        want.append(got)
        ks.append(int(rng.integers(1, len(plan) + 1)) if len(units) % 3 else len(plan) + 2)
    n = len(units)
    r = parse(hip, units, start=[NO] * n, out_set=list(range(n)), out_at=ks)
    for s, (u, got, k) in enumerate(zip(units, want, ks)):
        assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (got["n_bits"], got["flags"]), s
        assert r["values"][s].tolist() == got["values"], s
        head = _decoded_string(u["plan"][:k], got["values"])
        assert_set(r["sets"], s, CS.advance_from(head, CS.init_set(u["qp"], 2)), s)
    # ... and as row 0 of a picture: row 0 is exact, the row linked to it parses from those contexts within its own ranges
    pair = [units[0], units[1]]
    r = parse(hip, pair, entry="rows", rows=([0, 1, 2], [NO, 0], [ks[0], 0]))
    assert r["values"][0].tolist() == want[0]["values"] and int(r["res"]["flags"][0]) == want[0]["flags"]


def test_a_damaged_row_with_blocks_stays_inside_its_outputs_and_its_picture(hip):
    rows, level_first, sync_from, sync_at, written = wpp()
    rng = np.random.default_rng(0x9B08)
    units = [unit_of(r, w) for r, w in zip(rows, written)]
    units[0] = _flip_middle(rng, units[0], pad=False)              # picture 0, row 0
    assert not np.array_equal(units[0]["data"], written[0]["data"])
    r = parse(hip, units, entry="rows", rows=(level_first, sync_from, sync_at))   # Out.read checks every guard band
    for s, (row, w) in enumerate(zip(rows, written)):
        if s % 3 != 0:
            assert_row(r, s, row, w, "undamaged pictures")


# ---------------------------------------------------------------------------------------------- 8. rows written
def _write_desc(P):
    d = P["desc"].copy()
    d["init_id"] = W.SUB_FLAGS
    d["byte_offset"], d["byte_capacity"] = 0x7FFFFFF0, 0            # ignored by the contract
    return d


def write(hip, rows, entry="rows", int16=False, links=None, start=None, out_set=None, n_sets=N_SETS):
    """cabac_hip_write_plan_device ("plain"), cabac_hip_plan_write_sets_device ("sets") or cabac_hip_plan_write_rows_device ("rows",
    links = (level_first, sync_from, sync_at)) -> dict(payload [per row], raw, offsets, res, values [per row], infos [per row], sets)"""
    import torch
    P = R.pack(rows)
    n_sub, n_tu, n_el = len(rows), P["n_tu"], len(P["plan"])
    cap = 64 + sum(len(r["plan"]) * 8 + sum(4 * b.size for b in r["blocks"]) for r in rows)
    t_desc, t_first = dev(_write_desc(P), np.uint8), dev(P["tile_first"].view(np.int32))
    t_plan, t_vin = dev(P["plan"].reshape(-1).view(np.int32)), dev(P["values_in"].view(np.int32))
    t_co = dev(P["coeff"].astype(np.int16) if int16 else P["coeff"])
    t_tu = dev(P["tus"], np.uint8)
    t_at, t_gd = dev(P["tu_at"].view(np.int32)), dev(P["tu_guard"].view(np.int32))
    t_pay = torch.full((cap + 2 * G,), BYTE_GUARD, dtype=torch.uint8, device="cuda")
    t_off = torch.full((n_sub + 1 + 2 * G,), OFF_GUARD, dtype=torch.int64, device="cuda")
    t_res = torch.full((2 * n_sub + 2 * G,), RES_GUARD, dtype=torch.int32, device="cuda")
    t_val = torch.full((n_el + 2 * G,), VAL_GUARD - (1 << 32), dtype=torch.int32, device="cuda")
    t_info = torch.full((n_tu + 2 * G,), RES_GUARD, dtype=torch.int32, device="cuda")
    args = (n_sub, t_desc.data_ptr(), t_plan.data_ptr(), t_vin.data_ptr(), t_first.data_ptr(), n_tu, t_tu.data_ptr(), t_at.data_ptr(),
            t_gd.data_ptr(), t_co.data_ptr(), t_pay.data_ptr() + G, cap, t_off.data_ptr() + 8 * G, t_res.data_ptr() + 4 * G)
    kw = dict(d_values_out=t_val.data_ptr() + 4 * G, d_tu_info=t_info.data_ptr() + 4 * G, int16=int16)
    sets = None
    if entry == "plain":
        hip.write_plan_device(*args, **kw)
    elif entry == "sets":
        packed = pack_sets(start_sets()[:n_sets])
        t_state, t_rate = dev(packed[0].view(np.int32)), dev(packed[1])
        so = SetsOut(n_sets)
        u32 = lambda a: None if a is None else dev(np.asarray(a, np.uint32).view(np.int32))
        t_start, t_out = u32(start), u32(out_set)
        ptr = lambda t: t.data_ptr() if t is not None else 0
        hip.plan_write_sets_device(*args, **kw, n_sets=n_sets, d_state=t_state.data_ptr(), d_rate=t_rate.data_ptr(), d_start_set=ptr(t_start),
                                   d_out_set=ptr(t_out), d_out_state=so.p_state, d_out_rate=so.p_rate)
    else:
        level_first, sync_from, sync_at = links
        t_from, t_sat = dev(np.asarray(sync_from, np.uint32).view(np.int32)), dev(np.asarray(sync_at, np.uint32).view(np.int32))
        hip.plan_write_rows_device(*args, level_first, t_from.data_ptr(), t_sat.data_ptr(), **kw)
    hip.synchronize()
    if entry == "sets":
        sets = so.read()
    pay, off, res = t_pay.cpu().numpy(), t_off.cpu().numpy(), t_res.cpu().numpy()
    val, info = t_val.cpu().numpy(), t_info.cpu().numpy()
    for a, g, n in ((pay, BYTE_GUARD, cap), (off, OFF_GUARD, n_sub + 1), (res, RES_GUARD, 2 * n_sub), (val, VAL_GUARD - (1 << 32), n_el),
                    (info, RES_GUARD, n_tu)):
        assert (a[:G] == g).all() and (a[G + n:] == g).all(), "written outside an output's range"
    off = off[G:G + n_sub + 1]
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] <= cap
    assert (pay[G + int(off[-1]): G + cap] == BYTE_GUARD).all(), "written behind the reported payload"
    out = dict(P=P, offsets=off, res=res[G:G + 2 * n_sub].view(H.RESULT_DTYPE), raw=pay[G:G + int(off[-1])], payload=[], values=[],
               infos=[], sets=sets, all_values=val[G:G + n_el].view(np.uint32), info=info[G:G + n_tu].view(np.uint32))
    for s in range(n_sub):
        out["payload"].append(pay[G + int(off[s]): G + int(off[s + 1])])
        r0 = int(P["desc"]["rec_offset"][s])
        out["values"].append(out["all_values"][r0: r0 + len(rows[s]["plan"])])
        out["infos"].append(out["info"][int(P["tile_first"][s]): int(P["tile_first"][s + 1])])
    return out


def assert_written(r, s, w, what=""):
    assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (w["n_bits"], 0), (what, s)
    assert np.array_equal(r["payload"][s], w["data"]), (what, s)
    assert r["values"][s].tolist() == w["values"] and r["infos"][s].tolist() == w["infos"], (what, s)


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_rows_write_device_form(hip, int16):
    rows, level_first, sync_from, sync_at, written = wpp()
    r = write(hip, rows, int16=int16, links=(level_first, sync_from, sync_at))
    for s, w in enumerate(written):
        assert_written(r, s, w, "rows")
    plain = write(hip, rows, entry="plain")
    assert any(not np.array_equal(plain["payload"][s], written[s]["data"]) for s in range(len(rows))), "no row depends on its link"


def test_rows_write_batch_form(hip):
    rows, level_first, sync_from, sync_at, written = wpp()
    P = R.pack(rows)
    host = capi.CabacHip(0)
    payload = np.full(1 << 16, BYTE_GUARD, np.uint8)
    pay, off, res, val, info = host.plan_write_rows_batch(_write_desc(P), P["plan"], P["values_in"], P["tile_first"], P["tus"][:P["n_tu"]],
                                                          P["tu_at"], P["tu_guard"], P["coeff"], payload, level_first, sync_from, sync_at)
    host.close()
    for s, w in enumerate(written):
        assert (int(res["n_bits"][s]), int(res["flags"][s])) == (w["n_bits"], 0), s
        assert np.array_equal(pay[int(off[s]):int(off[s + 1])], w["data"]), s
        r0 = int(P["desc"]["rec_offset"][s])
        assert val[r0:r0 + len(w["values"])].tolist() == w["values"], s
        assert info[int(P["tile_first"][s]):int(P["tile_first"][s + 1])].tolist() == w["infos"], s
    assert (payload[int(off[-1]):] == BYTE_GUARD).all()


def test_write_sets_form(hip):
    rows = wpp()[0]
    n = len(rows)
    plain = write(hip, rows, entry="plain")
    for start, out_set in ((None, None), ([NO] * n, None)):
        r = write(hip, rows, entry="sets", start=start, out_set=out_set)
        for key in ("raw", "offsets", "res", "all_values", "info"):
            assert np.array_equal(plain[key], r[key]), key
        for k in range(N_SETS):
            assert_set_guard(r["sets"], k)
    # from start sets, every out set written: the contexts behind the last record
    start = [(3 * s) % N_SETS if s % 5 else NO for s in range(n)]
    out_set = [(s * 5) % N_SETS for s in range(n)]
    out_set[4] = NO
    start[7] = N_SETS + 1                                           # a bad index codes nothing
    # a stopped row (a value outside its element's domain) writes no set
    stopped = dict(rows[9], real=list(rows[9]["real"]))
    stopped["real"][0] = 2
    assert W.stop_of(stopped["plan"], stopped["real"], stopped["metas"], stopped["blocks"], stopped["at"], stopped["guards"]) == W.BAD_VALUE
    given = list(rows)
    given[9] = stopped
    r = write(hip, given, entry="sets", start=start, out_set=out_set)
    live = set()
    for s, row in enumerate(rows):
        if s == 7:
            assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (0, capi.RES_BAD_SET) and len(r["payload"][s]) == 0
        elif s == 9:
            assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (0, W.BAD_VALUE) and len(r["payload"][s]) == 0
        else:
            w = R.write_row(row, R.start_of(row, start_sets(), start[s]))
            assert_written(r, s, w, "sets")
            if out_set[s] != NO:
                assert_set(r["sets"], out_set[s], w["left"], s)
                live.add(out_set[s])
    for k in set(range(N_SETS)) - live:
        assert_set_guard(r["sets"], k)


# ---------------------------------------------------------------------------------------------- 9. round trip
def test_what_the_rows_writer_writes_the_rows_parser_reads_back(hip):
    rows, level_first, sync_from, sync_at, written = wpp()
    r = write(hip, rows, links=(level_first, sync_from, sync_at))
    units = [unit_of(row, w, data=r["payload"][s].copy()) for s, (row, w) in enumerate(zip(rows, written))]
    back = parse(hip, units, entry="rows", rows=(level_first, sync_from, sync_at))
    for s, row in enumerate(rows):
        assert int(back["res"]["flags"][s]) == 0, s
        assert np.array_equal(back["values"][s], r["values"][s]) and np.array_equal(back["infos"][s], r["infos"][s]), s
        for k, on in enumerate(written[s]["coded"]):
            if on:
                assert np.array_equal(coded(back["blocks"][s][k]), coded(row["blocks"][k])), (s, k)


def test_profile_reports_the_new_kinds(hip):
    rows, level_first, sync_from, sync_at, written = wpp()
    units = [unit_of(r, w) for r, w in zip(rows, written)]
    own = capi.CabacHip(0)
    own.profile_enable(16)
    parse(own, units, entry="rows", rows=(level_first, sync_from, sync_at))
    parse(own, units[:3], start=None, out_set=None)
    prof = own.profile_read()
    own.close()
    assert [k for k, _ in prof] == [35, 35, 35, 35, 34] and all(ms > 0 for _, ms in prof)   # one entry per level launch
