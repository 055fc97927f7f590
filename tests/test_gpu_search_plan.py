"""GPU: the search rounds over plans (include/cabac_hip_search_plan.h; csrc/cabac_plan_search.hip) — candidates given as a plan,
the values of its real elements and its blocks, resolved on the device into the unit-candidate form and costed, picked and
committed from there — against tests/search_plan_model.py, that is parse_plan_model's fill / expand, write_plan_model's stops and
search_unit_model's costs.  Everything is bit-exact: == on integers.  Expected values never come from the code under test.  Every
output sits between guard words that are checked, and the slots of d_values_in that the header says are not used (computed
entries, skipped elements) hold garbage."""
import numpy as np
import pytest

import helpers as H
import parse_elements_model as E
import parse_plan_model as PM
import search_plan_model as S
from entropy_coding_amd import capi
from test_gpu_residual_estimate import dev, make_sets, pack_sets
from test_gpu_search import assert_sets_equal, t_u32, t_u64
from test_parse_plan_model import TU_OUTCOMES

pytestmark = pytest.mark.gpu

G = 16                                                             # guard elements on either side of every output
G32, G64, G16, G8 = -0x11223345, -0x1122334455667789, 0x5A5A, 0xA5
NONE, U64 = 0xFFFFFFFF, (1 << 64) - 1
el, gd, cond, bi = capi.element, capi.guard, capi.cond, capi.block_info
NE, EQ, GE, LT = capi.GUARD_NE, capi.GUARD_EQ, capi.GUARD_GE, capi.GUARD_LT
CB = el(E.CTX_BIN, ctx=33)
TUB = capi.TU_DTYPE.itemsize


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


def guarded(n, fill, dtype):
    import torch
    return torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")


def inner(t, n, fill, view=None):
    """The n elements between the guards of a guarded tensor; asserts the guards"""
    a = t.cpu().numpy()
    assert (a[:G] == fill).all() and (a[G + n:] == fill).all(), "written outside an output's range"
    a = a[G:G + n].copy()
    return a if view is None else a.view(view)


class Call:
    """The device arrays of one call: inputs (values_in with garbage where the header says they are not used), outputs between guards"""

    def __init__(self, cands, int16=False, in_place=False, capacity=None, null=(), P=None, want=None):
        import torch
        self.cands, self.int16, self.null = cands, int16, set(null)
        P = self.P = S.pack(cands) if P is None else P
        self.want = S.resolve_all(cands, P, capacity) if want is None else want
        self.cap = self.want["total"] if capacity is None else capacity
        self.n_cand, self.n_tu, self.n_ent = len(cands), P["n_tu"], len(P["plan"])
        vin = P["values"].copy()
        for c, act in enumerate(self.want["active"]):
            for i, on in enumerate(act or ()):
                if not on:
                    vin[int(P["ent_first"][c]) + i] = 0xDEAD0000 + (i & 0xFFFF)
        self.vin = vin
        self.t_cf, self.t_ef = t_u32(P["cand_first"]), t_u64(P["ent_first"])
        self.t_plan, self.t_vin = t_u32(np.concatenate([P["plan"].reshape(-1), [0, 0]])), t_u32(np.concatenate([vin, [0]]))
        self.t_tu = dev(P["tus"], np.uint8) if self.n_tu else torch.zeros(16, dtype=torch.uint8, device="cuda")
        self.t_co = dev(np.concatenate([P["coeff"], [0]]).astype(np.int16 if int16 else np.int32))
        self.t_at = None if P["tu_at"] is None else t_u32(np.concatenate([P["tu_at"], [0]]))
        self.t_gd = None if P["tu_guard"] is None else t_u32(np.concatenate([P["tu_guard"], [0]]))
        self.t_rf = guarded(self.n_cand + 1, G64, torch.int64)
        self.t_rec = guarded(self.cap, G16, torch.int16)
        self.t_ato = guarded(self.n_tu, G32, torch.int32)
        self.t_tuo = guarded(self.n_tu * TUB, G8, torch.uint8)
        self.t_val = guarded(self.n_ent, G32, torch.int32)
        self.t_info = guarded(self.n_tu, G32, torch.int32)
        self.t_flags = guarded(self.n_cand, G32, torch.int32)
        self.t_total = guarded(1, G64, torch.int64)
        self.in_place = in_place
        if in_place:
            self.t_val[G:G + self.n_ent] = self.t_vin[:self.n_ent]

    def p(self, t, size, what=None):
        return 0 if what in self.null else t.data_ptr() + size * G

    def plan_args(self):
        p_vin = self.t_val.data_ptr() + 4 * G if self.in_place else self.t_vin.data_ptr()
        return (self.t_ef.data_ptr(), self.t_plan.data_ptr() if self.n_ent else 0, p_vin if self.n_ent else 0,
                self.t_at.data_ptr() if self.t_at is not None else 0, self.t_gd.data_ptr() if self.t_gd is not None else 0)

    def resolve(self, hip):
        ef, plan, vin, at, gd_ = self.plan_args()
        hip.resolve_plan_device(self.n_cand, self.t_cf.data_ptr(), ef, plan, vin, self.n_tu, self.t_tu.data_ptr() if self.n_tu else 0, at, gd_,
                                self.t_co.data_ptr() if self.n_tu else 0, self.p(self.t_rf, 8), self.p(self.t_rec, 2) if self.cap else 0,
                                self.cap, self.p(self.t_ato, 4) if self.n_tu else 0, self.p(self.t_tuo, 1) if self.n_tu else 0,
                                self.p(self.t_flags, 4), self.p(self.t_val, 4, "values_out"), self.p(self.t_info, 4, "tu_info"),
                                self.p(self.t_total, 8, "total"), int16=self.int16)

    def resolved(self):
        """What the call left, guards checked: dict(rec_first, records, tu_at_out, tus_out, values, infos, flags, total)"""
        out = dict(rec_first=inner(self.t_rf, self.n_cand + 1, G64, np.uint64), records=inner(self.t_rec, self.cap, G16, np.uint16),
                   tu_at_out=inner(self.t_ato, self.n_tu, G32, np.uint32), tus_out=inner(self.t_tuo, self.n_tu * TUB, G8, capi.TU_DTYPE),
                   values=inner(self.t_val, self.n_ent, G32, np.uint32), infos=inner(self.t_info, self.n_tu, G32, np.uint32),
                   flags=inner(self.t_flags, self.n_cand, G32, np.uint32), total=inner(self.t_total, 1, G64, np.uint64))
        P = self.P
        assert np.array_equal(self.t_co.cpu().numpy()[:-1], P["coeff"]) and np.array_equal(self.t_tu.cpu().numpy()[:self.n_tu * TUB].view(capi.TU_DTYPE), P["tus"][:self.n_tu])
        assert np.array_equal(self.t_plan.cpu().numpy().view(np.uint32)[:2 * self.n_ent], P["plan"].reshape(-1))
        if not self.in_place:
            assert np.array_equal(self.t_vin.cpu().numpy().view(np.uint32)[:self.n_ent], self.vin)
        return out

    def check(self, what=""):
        """P1: the resolved form is the model's"""
        got, want, P = self.resolved(), self.want, self.P
        assert got["flags"].tolist() == want["flags"].tolist(), (what, got["flags"].tolist(), want["flags"].tolist())
        assert got["rec_first"].tolist() == want["rec_first"].tolist(), what
        n = len(want["records"])
        assert np.array_equal(got["records"][:n], want["records"]), (what, np.nonzero(got["records"][:n] != want["records"])[0][:8])
        assert (got["records"][n:] == G16).all(), "written behind the runs"
        assert got["tu_at_out"].tolist() == want["tu_at_out"].tolist(), what
        assert got["tus_out"].tobytes() == want["tus_out"].tobytes(), what
        if "total" not in self.null:
            assert int(got["total"][0]) == want["total"], what
        else:
            assert int(got["total"].view(np.int64)[0]) == G64
        for c in range(self.n_cand):
            e0, e1, t0, t1 = int(P["ent_first"][c]), int(P["ent_first"][c + 1]), int(P["cand_first"][c]), int(P["cand_first"][c + 1])
            if want["values"][c] is None:
                continue                                           # a stopped candidate's ranges are unspecified
            if "values_out" not in self.null:
                assert got["values"][e0:e1].tolist() == want["values"][c], (what, c)
            if "tu_info" not in self.null:
                assert got["infos"][t0:t1].tolist() == want["infos"][c], (what, c)
        if "values_out" in self.null:
            assert (got["values"].view(np.int32) == G32).all()
        if "tu_info" in self.null:
            assert (got["infos"].view(np.int32) == G32).all()
        return got


def run(hip, cands, what="", **kw):
    call = Call(cands, **kw)
    call.resolve(hip)
    hip.synchronize()
    return call, call.check(what)


class Round(Call):
    """One cabac_hip_search_plan_round_device call on top of the resolve's arrays"""

    def __init__(self, cands, group_first, which, out_set, dist, lam, sets, **kw):
        import torch
        self.model = S.round_model(cands, group_first, sets, which, out_set, dist, lam, capacity=kw.get("capacity"))
        super().__init__(cands, want=self.model["resolved"], **kw)
        self.n_group, self.lam = len(group_first) - 1, lam
        self.t_gf, self.t_set = t_u32(group_first), t_u32(which)
        self.t_out = None if out_set is None else t_u32(out_set)
        self.t_dist = None if dist is None else t_u64(dist)
        self.t_bits = guarded(self.n_cand, G64, torch.int64)
        self.t_pick = guarded(self.n_group, G32, torch.int32)
        self.t_cost = guarded(self.n_group, G64, torch.int64)
        self.t_tub = guarded(self.n_tu, G64, torch.int64)

    def enqueue(self, hip, t_state, t_rate):
        ef, plan, vin, at, gd_ = self.plan_args()
        hip.search_plan_round_device(
            self.n_group, self.t_gf.data_ptr(), self.n_cand, self.t_cf.data_ptr(), self.n_tu, self.t_tu.data_ptr() if self.n_tu else 0,
            self.t_co.data_ptr() if self.n_tu else 0, t_state.data_ptr(), t_rate.data_ptr(), self.t_set.data_ptr(), ef, plan, vin, at, gd_,
            self.t_out.data_ptr() if self.t_out is not None else 0, self.t_dist.data_ptr() if self.t_dist is not None else 0, self.lam,
            self.p(self.t_bits, 8), self.p(self.t_pick, 4), self.p(self.t_cost, 8), self.p(self.t_rf, 8),
            self.p(self.t_rec, 2) if self.cap else 0, self.cap, self.p(self.t_ato, 4) if self.n_tu else 0,
            self.p(self.t_tuo, 1) if self.n_tu else 0, d_tu_frac_bits=self.p(self.t_tub, 8), d_tu_info=self.p(self.t_info, 4, "tu_info"),
            d_flags=self.p(self.t_flags, 4, "flags"), d_values_out=self.p(self.t_val, 4, "values_out"),
            d_total=self.p(self.t_total, 8, "total"), int16=self.int16)

    def results(self):
        return dict(bits=inner(self.t_bits, self.n_cand, G64, np.uint64), pick=inner(self.t_pick, self.n_group, G32, np.uint32),
                    cost=inner(self.t_cost, self.n_group, G64, np.uint64), tu_bits=inner(self.t_tub, self.n_tu, G64, np.uint64))

    def check_round(self, what=""):
        got, m = self.results(), self.model
        assert got["bits"].tolist() == m["bits"].tolist(), what
        assert got["pick"].tolist() == m["pick"].tolist(), (what, got["pick"].tolist(), m["pick"].tolist())
        assert got["cost"].tolist() == m["cost"].tolist(), what
        assert got["tu_bits"].tolist() == m["tu_bits"].tolist(), what
        if "flags" not in self.null:
            self.check(what)
        return got


def tu_cand(rng, outcome, close=False):
    p, v, m, b, a, g = PM.tu_case(rng, *outcome)
    if close:
        p, v = E.close(p, v)
    return S.cand(p, v, m, [np.clip(x, -32767, 32767) for x in b], a, g)


def small_block(rng, kind=0):
    """(meta, coefficients): 4 x 4 and 8 x 8, now and then a chroma one; kind 1: transform skip 8 x 8; kind 2: 32 x 32"""
    if kind == 1:
        return (8, 8, 0, H.TU_TRANSFORM_SKIP), np.clip(H.random_block(rng, 8, 8, density=0.5), -300, 300) | 1
    w = 32 if kind == 2 else int(rng.choice([4, 8]))
    c = H.random_block(rng, w, w, density=0.4 if w < 32 else 0.1, big=0.05)
    c[w - 1, w - 2] = 3
    return (w, w, int(rng.integers(0, 2)), int(rng.integers(0, 4))), np.clip(c, -32767, 32767)


def random_cand(rng, n, n_blocks, kinds=None):
    """A random plan of real elements and CONDs with n_blocks blocks at random positions behind random guards, a BLOCK_INFO entry
    on the last block behind each position"""
    plan, real = PM.random_cond_plan(rng, n)
    at = sorted(int(x) for x in rng.integers(0, n + 1, n_blocks))
    filled = PM.fill(plan, real)[0]
    guards = [E.random_guard(rng, a, filled, backs=(1, 2, 3, 5)) if rng.random() < 0.6 else 0 for a in at]
    pairs = [small_block(rng, (kinds or [0] * n_blocks)[k]) for k in range(n_blocks)]
    return S.cand(plan, real, [m for m, _ in pairs], [b for _, b in pairs], at, guards)


_TU = {}


def tu_cands():
    """Every outcome of the worked transform unit once, in a fixed shuffled order — built once, shared"""
    if not _TU:
        rng = np.random.default_rng(0x5EA7C4)
        _TU["order"] = [TU_OUTCOMES[k] for k in rng.permutation(len(TU_OUTCOMES))]
        _TU["cands"] = [tu_cand(rng, o) for o in _TU["order"]]
    return _TU["cands"], _TU["order"]


# ------------------------------------------------------------------------------------------------ P1: resolve = model
@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_p1_resolve_is_the_model_s(hip, int16):
    """Random plans with CONDs, guarded blocks (a 32 x 32 and a transform-skip one among them) and the worked unit, no stops"""
    rng = np.random.default_rng(0x5EA10 + int16)
    cands = [random_cand(rng, int(rng.integers(0, 90)), int(rng.integers(0, 4))) for _ in range(40)]
    cands += [random_cand(rng, 30, 3, kinds=[2, 1, 0]), random_cand(rng, 12, 2, kinds=[1, 1])] + tu_cands()[0][:16]
    call, got = run(hip, cands, "p1", int16=int16)
    assert call.want["coded"].any() and not call.want["coded"].all() and not call.want["flags"].any()


# ------------------------------------------------------------------------------------------------ P2: identity with the binariser
def test_p2_without_guards_it_is_the_binariser(hip):
    from test_gpu_binarize import binarize
    rng = np.random.default_rng(0x5EA20)
    cands = []
    for n in (0, 1, 17, 64, 65, 200):
        plan, values = E.random_plan(rng, n, guard_frac=0.0)
        pairs = [small_block(rng) for _ in range(int(rng.integers(0, 3)))]
        cands.append(S.cand(plan, values, [m for m, _ in pairs], [b for _, b in pairs], at=sorted(int(x) for x in rng.integers(0, n + 1, len(pairs)))))
    call, got = run(hip, cands, "p2")
    se = [np.stack([c["plan"][:, 0], np.array(c["values"], np.uint64).astype(np.uint32)], axis=1).astype(np.uint32) for c in cands]
    recs, cnt = binarize(hip, se)
    for c in range(len(cands)):
        a, b = int(got["rec_first"][c]), int(got["rec_first"][c + 1])
        assert np.array_equal(got["records"][a:b], recs[c]), c
    assert got["tus_out"].tobytes() == call.P["tus"].tobytes()


# ------------------------------------------------------------------------------------------------ P3: identity with the unit calls
@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_p3_the_resolved_arrays_fed_to_the_unit_calls(hip, int16):
    import torch
    rng = np.random.default_rng(0x5EA30)
    cands = [random_cand(rng, int(rng.integers(0, 50)), int(rng.integers(0, 3))) for _ in range(21)] + tu_cands()[0][16:27]
    n_cand, K = len(cands), 4
    group_first = np.arange(0, n_cand + 1, 8, dtype=np.uint32)
    which = (np.arange(n_cand) // 8).astype(np.uint32)
    sets = make_sets(rng, K)
    state, rate = pack_sets(sets)
    out_set = np.arange(K, dtype=np.uint32)
    dist = rng.integers(0, 3000, n_cand).astype(np.uint64)
    lam = int(1.9 * (1 << 16))
    rd = Round(cands, group_first, which, out_set, dist, lam, sets, int16=int16)
    t_state, t_rate = dev(state, np.int32), dev(rate)
    rd.enqueue(hip, t_state, t_rate)
    hip.synchronize()
    got = rd.check_round("plan round")
    assert_sets_equal(t_state.cpu().numpy().view(np.uint32), t_rate.cpu().numpy(), rd.model["sets"], "plan round")
    # the same through resolve + the unit round, and through the unit estimate
    u_state, u_rate = dev(state, np.int32), dev(rate)
    t_bits, t_pick, t_cost = guarded(n_cand, G64, torch.int64), guarded(K, G32, torch.int32), guarded(K, G64, torch.int64)
    hip.search_unit_round_device(K, rd.t_gf.data_ptr(), n_cand, rd.t_cf.data_ptr(), rd.p(rd.t_tuo, 1), rd.t_co.data_ptr(), u_state.data_ptr(),
                                 u_rate.data_ptr(), rd.t_set.data_ptr(), rd.p(rd.t_rf, 8), rd.p(rd.t_rec, 2), rd.p(rd.t_ato, 4),
                                 rd.t_out.data_ptr(), rd.t_dist.data_ptr(), lam, t_bits.data_ptr() + 8 * G, t_pick.data_ptr() + 4 * G,
                                 t_cost.data_ptr() + 8 * G, int16=int16)
    e_bits = guarded(n_cand, G64, torch.int64)
    s_state, s_rate = dev(state, np.int32), dev(rate)
    hip.estimate_unit_device(n_cand, rd.t_cf.data_ptr(), rd.p(rd.t_tuo, 1), rd.t_co.data_ptr(), s_state.data_ptr(), s_rate.data_ptr(),
                             rd.t_set.data_ptr(), rd.p(rd.t_rf, 8), rd.p(rd.t_rec, 2), rd.p(rd.t_ato, 4), e_bits.data_ptr() + 8 * G, int16=int16)
    hip.synchronize()
    assert inner(t_bits, n_cand, G64, np.uint64).tolist() == got["bits"].tolist() == inner(e_bits, n_cand, G64, np.uint64).tolist()
    assert inner(t_pick, K, G32, np.uint32).tolist() == got["pick"].tolist() and inner(t_cost, K, G64, np.uint64).tolist() == got["cost"].tolist()
    assert torch.equal(u_state, t_state) and torch.equal(u_rate, t_rate)


# ------------------------------------------------------------------------------------------------ P4: the worked unit
def test_p4_worked_unit_every_case_costed_as_the_model_says(hip):
    """cbf combinations x transform skip x scanPosLast == 0 x MTS violation, one candidate each, one group per start set: mts_idx is
    costed exactly when the model says it is coded (entry 17 of the filled values, and the cost is the model's)"""
    rng = np.random.default_rng(0x5EA40)
    cands, order = tu_cands()
    K = 6
    group_first = np.arange(0, len(cands) + 1, 8, dtype=np.uint32)
    which = (np.arange(len(cands)) // 8).astype(np.uint32)
    sets = make_sets(rng, K)
    state, rate = pack_sets(sets)
    rd = Round(cands, group_first, which, np.arange(K, dtype=np.uint32), None, 1 << 16, sets)
    t_state, t_rate = dev(state, np.int32), dev(rate)
    rd.enqueue(hip, t_state, t_rate)
    hip.synchronize()
    rd.check_round("worked unit")
    assert_sets_equal(t_state.cpu().numpy().view(np.uint32), t_rate.cpu().numpy(), rd.model["sets"], "worked unit")
    got, mts = rd.resolved(), 0
    for c, o in enumerate(order):
        v, info = got["values"][PM.TU_LEN * c: PM.TU_LEN * (c + 1)], got["infos"][3 * c: 3 * c + 3]
        exp = PM.tu_expected(dict(values=list(v), infos=list(info)), 0)
        luma = int(info[2])
        by_hand = bool(o[2]) and not o[3] and (luma & 0xFFFF) > 0 and not (luma & H.TU_INFO_MTS_VIOLATION)
        assert int(v[17]) == exp["mts_coded"] == int(by_hand), o
        assert [int(x) != capi.TU_INFO_NOT_CODED for x in info] == [bool(o[0]), bool(o[1]), bool(o[2])], o
        mts += by_hand
    assert 0 < mts < len(order)


# ------------------------------------------------------------------------------------------------ P5: a chain
def test_p5_three_rounds_in_place_on_one_stream(hip):
    rng = np.random.default_rng(0x5EA50)
    K, A, lam = 5, 4, int(2.3 * (1 << 16))
    sets = make_sets(rng, K)
    start = sets
    state, rate = pack_sets(sets)
    t_state, t_rate = dev(state, np.int32), dev(rate)
    pool, _ = tu_cands()
    rounds = []
    for r in range(3):
        cands = [pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.7 else random_cand(rng, int(rng.integers(0, 40)), 2)
                 for _ in range(K * A)]
        dist = rng.integers(0, 3000, K * A).astype(np.uint64)
        rd = Round(cands, np.arange(0, K * A + 1, A, dtype=np.uint32), np.repeat(np.arange(K, dtype=np.uint32), A),
                   np.arange(K, dtype=np.uint32), dist, lam, sets, in_place=bool(r & 1))
        sets = rd.model["sets"]
        rounds.append(rd)
    for rd in rounds:                                              # no host synchronisation between the rounds
        rd.enqueue(hip, t_state, t_rate)
    hip.synchronize()
    for r, rd in enumerate(rounds):
        rd.check_round("round %d" % r)
    assert_sets_equal(t_state.cpu().numpy().view(np.uint32), t_rate.cpu().numpy(), sets, "final sets")
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(sets, start))


# ------------------------------------------------------------------------------------------------ P6: search to bytes
@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_p6_winners_through_the_log_are_the_plan_write_s_bytes(hip, int16):
    import torch
    rng = np.random.default_rng(0x5EA60)
    K, A, lam = 7, 3, int(1.7 * (1 << 16))
    qp, init = rng.integers(18, 42, K), rng.integers(0, 3, K)
    orc = H.load_oracle()
    sets = [orc.ctx_init(int(q), int(i)) for q, i in zip(qp, init)]
    t_state = torch.zeros(K * 379, dtype=torch.int32, device="cuda")
    t_rate = torch.zeros(K * 379, dtype=torch.uint8, device="cuda")
    t_qp, t_init = dev(np.asarray(qp, np.int32)), t_u32(init)
    hip.ctx_init_device(K, t_qp.data_ptr(), t_init.data_ptr(), t_state.data_ptr(), t_rate.data_ptr())
    cands = [tu_cand(rng, TU_OUTCOMES[int(rng.integers(0, len(TU_OUTCOMES)))], close=True) for _ in range(K * A)]
    rd = Round(cands, np.arange(0, K * A + 1, A, dtype=np.uint32), np.repeat(np.arange(K, dtype=np.uint32), A), np.arange(K, dtype=np.uint32),
               rng.integers(0, 3000, K * A).astype(np.uint64), lam, sets, int16=int16)
    log = hip.search_log(K, K, rd.want["total"] + 8, rd.n_tu, len(rd.P["coeff"]) + 8, int16=int16)
    t_chain = t_u32(np.arange(K, dtype=np.uint32))
    rd.enqueue(hip, t_state, t_rate)
    log.append_device(K, rd.p(rd.t_pick, 4), t_chain.data_ptr(), rd.n_cand, rd.t_cf.data_ptr(), rd.p(rd.t_tuo, 1), rd.t_co.data_ptr(),
                      rd.p(rd.t_rf, 8), rd.p(rd.t_rec, 2), rd.p(rd.t_ato, 4), int16=int16)
    desc = np.zeros(K, H.DESC_DTYPE)
    desc["qp"], desc["init_id"] = qp, np.asarray(init, np.uint32) | H.SUB_FINISH
    t_desc = dev(desc, np.uint8)
    cap = 4096 * K
    t_pay = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
    t_off, t_res = torch.zeros(K + 1, dtype=torch.int64, device="cuda"), torch.zeros(2 * K, dtype=torch.int32, device="cuda")
    log.encode_device(t_desc.data_ptr(), t_pay.data_ptr(), cap, t_off.data_ptr(), t_res.data_ptr())
    hip.synchronize()
    pick = rd.check_round("p6")["pick"]
    assert int(log.read()["counters"]["flags"]) == 0
    # the plan write of the winners' plans, values and blocks
    winners = [cands[int(p)] for p in pick]
    W = S.pack(winners)
    wdesc = np.zeros(K, H.DESC_DTYPE)
    wdesc["qp"], wdesc["init_id"] = qp, np.asarray(init, np.uint32) | H.SUB_FINISH
    wdesc["rec_offset"], wdesc["n_records"] = W["ent_first"][:-1], np.diff(W["ent_first"].astype(np.int64))
    coeff = W["coeff"].astype(np.int16) if int16 else W["coeff"]
    w_pay, w_off, w_res, _, _ = hip.write_plan_batch(wdesc, W["plan"], W["values"], W["cand_first"], W["tus"], W["tu_at"], W["tu_guard"], coeff,
                                                    np.zeros(cap, np.uint8))
    off, res = t_off.cpu().numpy().view(np.uint64), t_res.cpu().numpy().view(H.RESULT_DTYPE)
    assert off.tolist() == w_off.tolist() and res["n_bits"].tolist() == w_res["n_bits"].tolist()
    assert not res["flags"].any() and not w_res["flags"].any() and int(off[-1]) > K
    assert np.array_equal(t_pay.cpu().numpy()[:int(off[-1])], w_pay)
    log.close()


# ------------------------------------------------------------------------------------------------ P7: shapes
def between(rng, n):
    """A block, n entries (a reference chain through all of them: entry i lives only if entry i - 1 does, CONDs on odd places),
    a block behind a guard on the last of them, a BLOCK_INFO on each"""
    plan, real = [(bi(0, 0, 16), 0)], [0]
    for i in range(n):
        if i == 0:
            plan.append((CB, 0))
        elif i % 3 == 2:
            plan.append(cond(1, NE, 0, capi.JOIN_AND, 2))
        else:
            plan.append((el(E.EP_BINS, n=2), gd(1, NE, 0)))
        real.append(int(rng.integers(1, 4)) if i else 1)
    plan += [(bi(0, 0, 16), 0), (bi(1, 16, 2), 0)]
    real += [0, 0]
    (m0, b0), (m1, b1) = small_block(rng), small_block(rng)
    return S.cand(np.array(plan, np.uint32), real, [m0, m1], [b0, b1], at=[0, n + 1], guards=[0, gd(1, NE, 0) if n else 0])


def many_blocks(rng, k):
    """k blocks at one position behind guards on the two elements in front, a BLOCK_INFO on the last and (from 16) on the 16th last"""
    plan = [(CB, 0), (CB, 0), (bi(0, 0, 16), 0)] + ([(bi(15, 0, 16), 0)] if k >= 16 else []) + [(el(E.EP_BINS, n=3), gd(1, NE, 0))]
    real = [1, 0, 0] + ([0] if k >= 16 else []) + [5]
    if k == 0:
        plan, real = [(CB, 0), (CB, 0), (el(E.EP_BINS, n=3), 0)], [1, 0, 5]
    pairs = [small_block(rng) for _ in range(k)]
    guards = [gd(int(rng.integers(1, 3)), NE, 0) if t != k - 16 else gd(2, NE, 0) for t in range(k)]
    return S.cand(np.array(plan, np.uint32), real, [m for m, _ in pairs], [b for _, b in pairs], at=[2] * k, guards=guards)


def shape_cands():
    if "shapes" not in _TU:
        rng = np.random.default_rng(0x5EA70)
        shapes = [("between %d" % n, between(rng, n)) for n in (0, 1, 63, 64, 65, 129, 300)]
        # a guard 255 back in a plan longer than 256, on the elements and on a block
        plan = np.array([(el(E.EP_BINS, n=3), gd(255, GE, 4) if i >= 255 else 0) for i in range(300)], np.uint32)
        m, b = small_block(rng)
        shapes.append(("255 back", S.cand(plan, [int(v) for v in rng.integers(0, 8, 300)], [m, m], [b, b], at=[280, 300],
                                          guards=[gd(255, GE, 4), gd(255, LT, 4)])))
        shapes += [("%d blocks" % k, many_blocks(rng, k)) for k in (0, 1, 16, 17, 64, 65)]
        pairs = [small_block(rng) for _ in range(2)]
        shapes.append(("no plan", S.cand(np.zeros((0, 2), np.uint32), [], [m for m, _ in pairs], [b for _, b in pairs])))
        shapes.append(("no block", S.cand(*PM.random_cond_plan(rng, 20))))
        shapes.append(("neither", S.cand(np.zeros((0, 2), np.uint32), [])))
        _TU["shapes"] = shapes
    return _TU["shapes"]


@pytest.mark.parametrize("k", range(17))
def test_p7_shapes_alone_and_among_ordinary_candidates(hip, k):
    name, c = shape_cands()[k]
    call, _ = run(hip, [c], name)
    assert not call.want["flags"].any(), name
    if name.endswith("blocks") and int(name.split()[0]) >= 16:
        assert call.want["coded"].any() and not call.want["coded"].all(), name
    pool = tu_cands()[0]
    mixed = [pool[3], c, pool[11], pool[20], c, pool[7], pool[30]]
    run(hip, mixed, name + ", mixed", in_place=True)


@pytest.mark.parametrize("n_cand", [1, 3, 4, 5, 257])
def test_p7_candidate_counts_around_the_workgroup(hip, n_cand):
    rng = np.random.default_rng(0x5EA71 + n_cand)
    pool = tu_cands()[0]
    cands = [pool[int(rng.integers(0, len(pool)))] for _ in range(n_cand)]
    sets = make_sets(rng, 2)
    state, rate = pack_sets(sets)
    gf = np.array([0, n_cand // 2, n_cand], np.uint32)
    which = (np.arange(n_cand) >= n_cand // 2).astype(np.uint32)
    rd = Round(cands, gf, which, np.array([0, 1], np.uint32), None, 1 << 16, sets)
    t_state, t_rate = dev(state, np.int32), dev(rate)
    rd.enqueue(hip, t_state, t_rate)
    hip.synchronize()
    rd.check_round("n_cand %d" % n_cand)
    want = [s if s is not None else sets[k] for k, s in enumerate(rd.model["sets"])]
    assert_sets_equal(t_state.cpu().numpy().view(np.uint32), t_rate.cpu().numpy(), want, "n_cand %d" % n_cand)


# ------------------------------------------------------------------------------------------------ P8: stops
def stop_cands():
    rng = np.random.default_rng(0x5EA80)
    good = tu_cands()[0]
    base = tu_cand(rng, (1, 1, 1, False, False, False))
    plan, vals = base["plan"], base["values"]
    zero = [np.zeros_like(base["blocks"][0])] + base["blocks"][1:]
    stops = [
        ("a bad entry behind a false guard", dict(base, plan=np.concatenate([plan, [[15, gd(1, EQ, 77)]]]).astype(np.uint32), values=vals + [0]), S.BAD_RECORD),
        ("a bad block guard", dict(base, guards=[gd(11, NE, 0)] + base["guards"][1:]), S.BAD_RECORD),
        ("an active value outside its domain", dict(base, values=[vals[0]] + [vals[1]] + [7] + vals[3:]), S.BAD_VALUE),   # tu_cbf_cr on ctx 1
        ("the same value behind a false guard", dict(base, values=[vals[0]] + [7] + vals[2:]), 0),
        ("a coded all-zero block", dict(base, blocks=zero), S.BAD_VALUE),
        ("the same block behind a false guard", dict(base, blocks=zero, values=[0] + vals[1:]), 0),
        ("a bad entry and a bad value", dict(base, plan=np.concatenate([plan, [[15, 0]]]).astype(np.uint32), values=[5] + vals[1:] + [0]), S.BAD_RECORD),
    ]
    return good, stops


@pytest.mark.parametrize("k", range(7))
def test_p8_a_stop_flags_its_candidate_and_nothing_else(hip, k):
    good, stops = stop_cands()
    name, c, flag = stops[k]
    around = [good[5], good[18], c, good[9], good[40]]
    call, got = run(hip, around, name)
    assert call.want["flags"].tolist() == [0, 0, flag, 0, 0], name
    if not flag:
        return
    # the neighbours are bit-identical to a run without it; the stopped candidate's ranges hold nothing but their own words
    _, alone = run(hip, around[:2] + around[3:], name + ", without it")
    assert got["rec_first"][2] == got["rec_first"][3] and got["tu_at_out"][6:9].tolist() == [0, 0, 0]
    assert (got["tus_out"]["log2_width"][6:9] == 7).all() and (got["tus_out"]["log2_height"][6:9] == 7).all()
    assert np.array_equal(got["records"], alone["records"]) and got["total"] == alone["total"]
    assert np.array_equal(np.delete(got["rec_first"], 3), alone["rec_first"])
    e0, e1 = int(call.P["ent_first"][2]), int(call.P["ent_first"][3])
    assert np.array_equal(np.delete(got["values"], np.arange(e0, e1)), alone["values"])
    assert np.array_equal(np.delete(got["infos"], [6, 7, 8]), alone["infos"])
    for f in ("log2_width", "log2_height", "channel", "flags"):
        assert np.array_equal(np.delete(got["tus_out"][f], [6, 7, 8]), alone["tus_out"][f]), f
    assert np.array_equal(np.delete(got["tu_at_out"], [6, 7, 8]), alone["tu_at_out"])


def test_p8_in_the_round_a_stopped_candidate_costs_the_maximum(hip):
    rng = np.random.default_rng(0x5EA81)
    good, stops = stop_cands()
    cands = [good[5], stops[2][1], good[9], stops[0][1], stops[4][1]]
    gf = np.array([0, 3, 4, 5], np.uint32)                         # the stopped ones of groups 1 and 2 have nothing beside them
    sets = make_sets(rng, 3)
    state, rate = pack_sets(sets)
    rd = Round(cands, gf, np.array([0, 0, 0, 1, 2], np.uint32), None, np.array([9000, 0, 9000, 0, 0], np.uint64), 1 << 16, sets)
    t_state, t_rate = dev(state, np.int32), dev(rate)
    rd.enqueue(hip, t_state, t_rate)
    hip.synchronize()
    got = rd.check_round("stops in a round")
    assert got["bits"][[1, 3, 4]].tolist() == [U64] * 3 and got["pick"].tolist()[1:] == [3, 4] and int(got["pick"][0]) in (0, 2)
    assert rd.resolved()["flags"].tolist() == [0, S.BAD_VALUE, 0, S.BAD_RECORD, S.BAD_VALUE]
    assert np.array_equal(t_state.cpu().numpy().view(np.uint32), state)     # no out set: nothing committed


# ------------------------------------------------------------------------------------------------ P9: capacity
def test_p9_capacity_is_all_or_nothing(hip):
    good, stops = stop_cands()
    cands = good[:9] + [stops[2][1]] + good[9:14]
    call, got = run(hip, cands, "capacity = need")                 # Call sizes d_records to the need exactly
    need = call.want["total"]
    assert need > 0 and call.cap == need and call.want["flags"].tolist() == [0] * 9 + [S.BAD_VALUE] + [0] * 5
    short, got = run(hip, cands, "one record less", capacity=need - 1)
    assert got["flags"].tolist() == [S.OVERFLOW] * 9 + [S.BAD_VALUE] + [S.OVERFLOW] * 5 and not got["rec_first"].any()
    assert int(got["total"][0]) == need and (got["records"] == G16).all()
    assert (got["tus_out"]["log2_width"] == 7).all() and not got["tu_at_out"].any()
    # the host-pointer form sizes the buffer itself
    rng = np.random.default_rng(0x5EA90)
    sets = make_sets(rng, 1)
    state, rate = pack_sets(sets)
    P = call.P
    gf = np.array([0, len(cands)], np.uint32)
    m = S.round_model(cands, gf, sets, np.zeros(len(cands), np.uint32), np.array([0], np.uint32), None, 1 << 16, P=P)
    bits, pick, cost, flags, filled, tu_bits, info = hip.search_plan_round_batch(
        gf, P["cand_first"], P["tus"], P["coeff"], state, rate, np.zeros(len(cands), np.uint32), P["plan"], P["values"], P["ent_first"],
        P["tu_at"], P["tu_guard"], np.array([0], np.uint32), None, 1 << 16, with_blocks=True, check=False)
    assert bits.tolist() == m["bits"].tolist() and pick.tolist() == m["pick"].tolist() and cost.tolist() == m["cost"].tolist()
    assert flags.tolist() == m["flags"].tolist() and tu_bits.tolist() == m["tu_bits"].tolist()
    assert_sets_equal(state, rate, m["sets"], "host form")
    for c in range(len(cands)):
        if m["resolved"]["values"][c] is not None:
            assert filled[int(P["ent_first"][c]): int(P["ent_first"][c + 1])].tolist() == m["resolved"]["values"][c], c
            assert info[int(P["cand_first"][c]): int(P["cand_first"][c + 1])].tolist() == m["resolved"]["infos"][c], c


# ------------------------------------------------------------------------------------------------ P10: in place, optional outputs
@pytest.mark.parametrize("null", ["in_place", "values_out", "tu_info", "total", "tu_at", "tu_guard", "flags"])
def test_p10_in_place_and_optional_outputs(hip, null):
    rng = np.random.default_rng(0x5EA95)
    cands = tu_cands()[0][:6] + [random_cand(rng, 40, 3) for _ in range(4)]
    if null == "tu_at":                                            # every block behind its plan (no BLOCK_INFO entry in these plans)
        cands = [dict(random_cand(rng, int(rng.integers(0, 70)), 2), at=None, guards=None) for _ in range(9)]
    if null == "tu_guard":
        cands = [dict(c, guards=None) for c in cands]
    if null == "flags":                                            # optional in the round alone
        sets = make_sets(rng, 1)
        state, rate = pack_sets(sets)
        rd = Round(cands, np.array([0, len(cands)], np.uint32), np.zeros(len(cands), np.uint32), None, None, 1 << 16, sets, null=("flags",))
        rd.enqueue(hip, dev(state, np.int32), dev(rate))
        hip.synchronize()
        rd.check_round("no flags")
        assert (inner(rd.t_flags, rd.n_cand, G32) == G32).all()
        return
    call, _ = run(hip, cands, null, in_place=null == "in_place", null=() if null in ("in_place", "tu_at", "tu_guard") else (null,))
    assert (call.P["tu_at"] is None) == (null == "tu_at") and (call.P["tu_guard"] is None) == (null in ("tu_at", "tu_guard"))


# ------------------------------------------------------------------------------------------------ P11: profile
def test_p11_a_round_reports_its_parts_in_order():
    rng = np.random.default_rng(0x5EA99)
    hip = H.gpu_ctx()
    try:
        hip.profile_enable(16)
        cands = tu_cands()[0][:8]
        sets = make_sets(rng, 1)
        state, rate = pack_sets(sets)
        rd = Round(cands, np.array([0, 8], np.uint32), np.zeros(8, np.uint32), np.array([0], np.uint32), None, 1 << 16, sets)
        rd.enqueue(hip, dev(state, np.int32), dev(rate))
        hip.synchronize()
        kinds = [k for k, _ in hip.profile_read()]
        assert kinds == [5, 29, 20, 21, 22], kinds
        rd.check_round("profiled")
        call = Call(cands)
        call.resolve(hip)
        hip.synchronize()
        assert [k for k, _ in hip.profile_read()] == [5, 29]
    finally:
        hip.close()
