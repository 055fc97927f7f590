"""GPU: the element parse (include/cabac_hip_parse_elements.h; the element-walking instantiation of csrc/cabac_residual_parse.hip)
against the unit parse (identity E1), the oracle's reader (identity E2, through tests/parse_elements_model.py's exact reader), the
library's own writer, and the model's consistency check where blocks are involved.  Everything is bit-exact: == on integers.
Every output sits between guard words that are checked, what the header says is not written is checked untouched, every test has
its own bounded input, and nothing is run again after a failure."""
import functools

import numpy as np
import pytest

import helpers as H
import parse_elements_model as E
import parse_unit_model as M
import search_unit_model as U
from entropy_coding_amd import capi
from test_gpu_parse_unit import (BIN_GUARD, G, WORD_GUARD, _i1_units, _roundtrip_units, coded, dev, device_encode, run_unit, sentinel,
                                 t_or_dummy, want_info, with_)

pytestmark = pytest.mark.gpu

VAL_GUARD = 0xEEEEEEEE
WORD_GUARD_U = WORD_GUARD & 0xFFFFFFFF
el, gd = capi.element, capi.guard


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


class Out:
    """The four outputs of a call, each between G guard elements."""

    def __init__(self, P, int16):
        import torch
        self.int16 = int16
        self.co = torch.full((P["total"] + 2 * G,), sentinel(int16), dtype=torch.int16 if int16 else torch.int32, device="cuda")
        self.val = torch.full((len(P["plan"]) + 2 * G,), VAL_GUARD - (1 << 32), dtype=torch.int32, device="cuda")
        self.info = torch.full((P["n_tu"] + 2 * G,), WORD_GUARD, dtype=torch.int32, device="cuda")
        self.res = torch.full((2 * len(P["desc"]) + 2 * G,), WORD_GUARD, dtype=torch.int32, device="cuda")

    def ptrs(self):
        return (self.co.data_ptr() + G * (2 if self.int16 else 4), self.val.data_ptr() + 4 * G, self.info.data_ptr() + 4 * G,
                self.res.data_ptr() + 4 * G)

    def read(self):
        co, val, info, res = self.co.cpu().numpy(), self.val.cpu().numpy(), self.info.cpu().numpy(), self.res.cpu().numpy()
        for a, g in ((co, sentinel(self.int16)), (val, VAL_GUARD - (1 << 32)), (info, WORD_GUARD), (res, WORD_GUARD)):
            assert (a[:G] == g).all() and (a[len(a) - G:] == g).all(), "a guard word was written"
        return (co[G:len(co) - G].astype(np.int32), val[G:len(val) - G].view(np.uint32), info[G:len(info) - G].view(np.uint32),
                res[G:len(res) - G].view(H.RESULT_DTYPE))


def run_elements(hip, units, int16=False, capacities=None, mutate=None, null_at=False):
    """parse_elements_device over `units` (parse_elements_model.pack) -> dict(P, co, values [per unit], all_values, info, res,
    blocks [per unit])."""
    P = E.pack(units, capacities)
    if mutate:
        mutate(P)
    out = Out(P, int16)
    t_desc, t_buf = dev(P["desc"], np.uint8), dev(P["bytes"])
    t_first, t_tu = dev(P["tile_first"].view(np.int32)), t_or_dummy(P["tus"][:P["n_tu"]], np.uint8)
    t_at = None if (null_at or P["tu_at"] is None) else t_or_dummy(P["tu_at"].view(np.int32), None)
    t_guard = None if P["tu_guard"] is None else t_or_dummy(P["tu_guard"].view(np.int32), None)
    t_plan = t_or_dummy(P["plan"].view(np.int32), None)
    p_co, p_val, p_info, p_res = out.ptrs()
    n_el = len(P["plan"])
    hip.parse_elements_device(len(units), t_desc.data_ptr(), t_buf.data_ptr(), t_first.data_ptr(), t_tu.data_ptr() if P["n_tu"] else 0,
                              t_at.data_ptr() if t_at is not None else 0, t_guard.data_ptr() if t_guard is not None else 0,
                              t_plan.data_ptr() if n_el else 0, p_co if P["n_tu"] else 0, p_val if n_el else 0, p_res,
                              d_tu_info=p_info, int16=int16)
    hip.synchronize()
    co, val, info, res = out.read()
    blocks, per_val, t = [], [], 0
    for s, u in enumerate(units):
        bl = []
        for m in u["metas"]:
            w, h = m[0], m[1]
            bl.append(co[int(P["offsets"][t]): int(P["offsets"][t]) + w * h].reshape(h, w))
            t += 1
        blocks.append(bl)
        r0 = int(P["desc"]["rec_offset"][s])
        per_val.append(val[r0:r0 + len(u["plan"])])
    return dict(P=P, co=co, values=per_val, all_values=val, info=info, res=res, blocks=blocks)


def assert_blocks_untouched(r, units, int16, written):
    """Nothing but the coded top-left of the blocks with written[s][k] was written."""
    mask, t = np.zeros(len(r["co"]), bool), 0
    for s, u in enumerate(units):
        for k, m in enumerate(u["metas"]):
            w, h = m[0], m[1]
            if written[s][k]:
                blk = np.zeros((h, w), bool)
                blk[:min(h, 32), :min(w, 32)] = True
                mask[int(r["P"]["offsets"][t]): int(r["P"]["offsets"][t]) + w * h] = blk.ravel()
            t += 1
    want = np.int32(np.int16(sentinel(int16))) if int16 else np.int32(sentinel(int16))
    assert (r["co"][~mask] == want).all(), "a coefficient outside the coded regions of the parsed blocks was written"


def want_walk(u):
    """(n_bits, flags) of a valid unit: orc.decode_records of the string of its active elements and coded blocks"""
    orc = H.load_oracle()
    string, _, _, _ = E.expand(u["plan"], u["values"], u["metas"], u["blocks"], u["at"], u["guards"])
    rc, bins, nread = orc.decode_records(string, u["qp"], 2, u["data"], flags=1 if u["finish"] else 0)
    assert rc in (0, -5) and np.array_equal(bins, string >> 15)
    return nread, {0: 0, -5: H.RES_BAD_STOP}[rc]


def assert_valid(r, units, int16, what=""):
    """Every unit came back as it was coded: values (0 where skipped), the coded blocks, NOT_CODED for the skipped ones and their
    coefficients untouched, tu_info, n_bits and flags."""
    t = 0
    for s, u in enumerate(units):
        assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == want_walk(u), (what, s)
        assert r["values"][s].tolist() == [v & 0xFFFFFFFF for v in u["values"]], (what, s)
        info = want_info(u)
        for k, on in enumerate(u["coded"]):
            if on:
                assert np.array_equal(coded(r["blocks"][s][k]), coded(u["blocks"][k])), (what, s, k)
                assert int(r["info"][t + k]) == info[k], (what, s, k)
            else:
                assert int(r["info"][t + k]) == E.NOT_CODED, (what, s, k)
        t += len(info)
    assert_blocks_untouched(r, units, int16, [u["coded"] for u in units])


def small_block(rng):
    w, h = int(rng.choice([4, 8])), int(rng.choice([4, 8]))
    return (w, h, int(rng.integers(0, 2)), int(rng.integers(0, 2))), H.random_block(rng, w, h, density=float(rng.choice([0.3, 0.7])), big=0.1)


def as_elements(u):
    """A unit of the unit parse as the element unit of identity E1"""
    return dict(u, plan=E.plan_of_records(u["side"]), guards=None)


# ---------------------------------------------------------------------------------------------- 1. identity E1
@functools.lru_cache(maxsize=None)
def _e1_corpus(which):
    rng = np.random.default_rng(0xE10)
    if which == "roundtrip":
        return _roundtrip_units(rng)
    if which == "damaged":
        return M.damaged_units(7, 200)
    if which == "wide":                                                   # 1 030 substreams: four waves per workgroup
        return _i1_units(rng, 1030, True)
    if which == "i2":                                                     # the corpus of the unit parse's I2 test: block-free runs with
        orc, units = H.load_oracle(), []                                  # bypass, terminate and align records, intact and damaged
        for rep in range(2):
            for n in (0, 1, 63, 64, 65, 129, 1000):
                rec = H.random_records(rng, n - 1, ctx_frac=0.6, end_trm=True, trm0_frac=0.02) if n else np.zeros(0, np.uint16)
                if n >= 63:
                    rec[int(rng.integers(0, n - 1))] = H.REC_ALIGN
                    rec[int(rng.integers(0, n - 1))] = H.REC_TRM          # a terminate bin of 0 inside the run
                u = dict(metas=[], blocks=[], side=rec.astype(np.uint16), at=None, qp=int(rng.integers(0, 64)), finish=bool(n & 1))
                u["data"] = orc.encode_records(rec if n else M.TRM_END, u["qp"], 2, 3)[0]
                if rep:
                    d = u["data"].copy()
                    d[int(rng.integers(0, len(d)))] ^= 1 << int(rng.integers(0, 8))
                    u["data"] = d
                units.append(u)
        return units
    if which == "trm1":                                                   # a terminate bin of 1 in mid-run, bypass and context bins and an
        orc, units = H.load_oracle(), []                                  # align record behind it: the state OUT OF RANGE, where E1 still holds
        for s in range(8):
            head = H.random_records(rng, 5 + s, ctx_frac=0.6, end_trm=False)
            tail = H.random_records(rng, 40, ctx_frac=0.5, end_trm=False)
            tail[:3] = H.REC_EP
            tail[20] = H.REC_ALIGN
            rec = np.concatenate([head, M.TRM_END, tail]).astype(np.uint16)
            u = dict(metas=[], blocks=[], side=rec, at=None, qp=int(rng.integers(0, 64)), finish=False)
            u["data"] = np.concatenate([orc.encode_records(np.concatenate([head, M.TRM_END]), u["qp"], 2, 3)[0], rng.integers(0, 256, 48).astype(np.uint8)])
            units.append(u)
        return units
    units = [M.make_unit(rng, ["regular", "ts", "regular"], 12, at=[2, 6, 10]) for _ in range(5)]
    units[3] = with_(units[3], side=units[3]["side"].copy())
    units[3]["side"][7] = 0x1FC | 0x8000                                  # a bad record behind block 1, in front of block 2
    return units


@pytest.mark.parametrize("int16", [False, True])
@pytest.mark.parametrize("which", ["roundtrip", "damaged", "wide", "bad_record", "i2", "trm1"])
def test_e1_single_bin_elements_are_the_unit_parse(hip, which, int16):
    """The corpora of the unit-parse tests as plans of unguarded CTX_BIN / EP_BINS(1) / TRM / ALIGN elements, d_tu_guard NULL:
    values = side bins widened (and untouched where those are), results, blocks and tu_info equal."""
    units = list(_e1_corpus(which))
    want = run_unit(hip, units, int16)
    r = run_elements(hip, [as_elements(u) for u in units], int16)
    assert np.array_equal(r["res"], want["res"]) and np.array_equal(r["co"], want["co"]) and np.array_equal(r["info"], want["info"])
    bins = want["all_bins"]
    assert np.array_equal(r["all_values"], np.where(bins == BIN_GUARD, VAL_GUARD, bins.astype(np.uint32)))
    if which == "bad_record":
        assert int(r["res"]["flags"][3]) == H.RES_BAD_RECORD and (r["values"][3][7:] == VAL_GUARD).all() and not r["res"]["flags"][[0, 1, 2, 4]].any()
    if which == "damaged":
        assert (r["res"]["flags"] != 0).any() and (r["res"]["flags"] == 0).any()
    if which == "i2":
        assert any((u["side"] & 0x1FF == H.REC_ALIGN).any() for u in units) and (r["res"]["flags"] == 0).sum() >= 6
        for s in range(1, 7):                                             # intact: the bins that were coded
            assert r["values"][s].tolist() == (units[s]["side"] >> 15).tolist(), s
    if which == "trm1":
        for s, u in enumerate(units):                                     # the terminate bin did decode to 1, and the walk went on
            assert int(r["values"][s][5 + s]) == 1 and (r["values"][s] != VAL_GUARD).all(), s


# ---------------------------------------------------------------------------------------------- 2. identity E2, every kind
def _corner_plan(rng):
    """The parameter corners, placed on either side of the boundary between the first two 64-element groups (elements 62..65 are
    the long ones: 255 context bins, 63, 32 and 32 bypass bins) -> (plan, values)"""
    fill, fv = E.random_plan(rng, 62, kinds=[E.CTX_BIN, E.EP_BINS, E.ALIGN], guard_frac=0.0)
    rmax = [(rice, cut, ml, E.rem_abs_max(rice, cut, ml)) for rice, cut, ml in ((0, 5, 15), (14, 5, 15), (3, 12, 20), (14, 0, 20), (2, 17, 15))]
    corners = [(el(E.UNARY_MAX, ctx=40, ctx_n=41, max_symbol=255), 255),          # 62: run to the end
               (el(E.EXP_GOLOMB, count=0), (1 << 31) - 1),                        # 63: 31 ones, a 0, 31 suffix bins
               (el(E.EP_BINS, n=32), 0xDEADBEEF), (el(E.UNARY_EP, max_symbol=32), 32),   # 64, 65
               (el(E.EP_BINS, n=0), 0), (el(E.UNARY_EP, max_symbol=32), 31), (el(E.UNARY_EP, max_symbol=0), 0),
               (el(E.EXP_GOLOMB, count=31), 0x7FFFFFFF), (el(E.EXP_GOLOMB, count=31), 0), (el(E.EXP_GOLOMB, count=0), 0),
               (el(E.EXP_GOLOMB, count=0), 0xFFFFFFFE),                           # 31 ones and a suffix of ones: the largest value
               (el(E.UNARY_MAX, ctx=40, ctx_n=41, max_symbol=255), 254), (el(E.UNARY_MAX, ctx=42, max_symbol=0), 0),
               (el(E.TRUNC_BIN, max_symbol=1), 0), (el(E.TRUNC_BIN, max_symbol=(1 << 28) - 1), (1 << 28) - 2),
               (el(E.TRUNC_BIN, max_symbol=(1 << 28) - 1), 0), (el(E.TRUNC_BIN, max_symbol=(1 << 28) - 1), 1),
               (el(E.TRUNC_BIN, max_symbol=5), 4), (el(E.TRUNC_BIN, max_symbol=5), 2)]
    corners += [(el(E.REM_ABS, rice=a, cutoff=b, max_log2=c), v) for a, b, c, top in rmax for v in (top, top - 1, 0, (b << a), max((b << a) - 1, 0))]
    plan = np.concatenate([fill, [[w, 0] for w, _ in corners]]).astype(np.uint32)
    return E.close(plan, fv + [v for _, v in corners])


def test_e2_block_free_plans_of_every_kind_and_the_parameter_corners(hip):
    """Block-free, unguarded plans of 0, 1, 63, 64, 65 and 130 elements of every kind, and the corner plan: values equal
    orc_decode_ops's (the exact reader) and the writer's input, n_bits and flags the oracle's."""
    orc = H.load_oracle()
    rng = np.random.default_rng(0xE20)
    units = []
    for n in (0, 1, 63, 64, 65, 130):
        plan, values = E.random_plan(rng, n, guard_frac=0.0)
        if n:
            plan, values = E.close(plan[:-1], values[:-1])
        units.append(E.make_unit(rng, plan, values, finish=bool(n)))
    units[0]["data"] = np.concatenate([units[0]["data"], np.zeros(1, np.uint8)])   # start() reads two bytes
    units.append(E.make_unit(rng, *_corner_plan(rng)))
    bits = [len(E.records_of([E.op_of(w, v)])) for w, v in zip(units[-1]["plan"][:, 0], units[-1]["values"])]
    assert max(bits) > 32 and (np.array(bits[62:66]) >= 32).all()          # the last unit: the long ones at the group boundary
    r = run_elements(hip, units)
    for s, u in enumerate(units):
        rc, vals = orc.decode_ops(np.array([E.op_of(w) for w in u["plan"][:, 0]], np.uint32).reshape(-1, 4), u["qp"], 2, u["data"])
        assert rc == 0 and r["values"][s].tolist() == vals.tolist() == [v & 0xFFFFFFFF for v in u["values"]], s
        m = E.read_plan(u["plan"], u["data"], u["qp"], finish=u["finish"])
        assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (m["n_bits"], m["flags"]) == (m["n_bits"], 0), s
    assert {int(w) & 15 for u in units for w in u["plan"][:, 0]} == set(range(9))


# ---------------------------------------------------------------------------------------------- 3. round trip through the writer
def _guarded_unit(rng, n_el, n_blocks, backs=(1, 2, 3, 5, 63, 64, 255)):
    """A random guarded plan with n_blocks small blocks at random positions behind random guards, closed by the terminate bin"""
    plan, values = E.close(*E.random_plan(rng, n_el, guard_frac=0.5, small=True, backs=backs))
    at = sorted(int(x) for x in rng.integers(0, n_el + 1, n_blocks))
    metas, blocks = zip(*[small_block(rng) for _ in range(n_blocks)]) if n_blocks else ((), ())
    guards = [E.random_guard(rng, a, values, backs) if rng.random() < 0.7 else 0 for a in at]
    return E.make_unit(rng, plan, values, metas, blocks, at=at, guards=guards)


@pytest.mark.parametrize("int16", [False, True])
def test_round_trip_through_the_library_s_own_writer(hip, int16):
    """values -> cabac_hip_binarize_device -> records with the coded blocks spliced -> cabac_hip_encode_residual_device ->
    cabac_hip_parse_elements_device returns the values and the blocks."""
    from test_gpu_binarize import binarize
    rng = np.random.default_rng(0xE30)
    units = [_guarded_unit(rng, n_el, n_blocks) for n_el, n_blocks in ((130, 6), (64, 3), (7, 3), (20, 0), (300, 5))]
    se, rec_units = [], []
    for u in units:
        _, _, active, _ = E.expand(u["plan"], u["values"], u["metas"], u["blocks"], u["at"], u["guards"])
        se.append(np.array([[w, v] for (w, _), v, on in zip(u["plan"], u["values"], active) if on], np.uint32).reshape(-1, 2))
    recs, _ = binarize(hip, se)
    for u, rec in zip(units, recs):
        _, _, active, _ = E.expand(u["plan"], u["values"], u["metas"], u["blocks"], u["at"], u["guards"])
        n_rec = [len(E.records_of([E.op_of(w, v)])) if on else 0 for (w, _), v, on in zip(u["plan"], u["values"], active)]
        first = np.concatenate([[0], np.cumsum(n_rec)]).astype(int)       # the first record of every element, and the end
        assert first[-1] == len(rec)
        pos = U.positions(u["at"], len(u["plan"]))
        keep = [k for k, on in enumerate(u["coded"]) if on]
        rec_units.append(dict(metas=[u["metas"][k] for k in keep], blocks=[u["blocks"][k] for k in keep], side=rec.astype(np.uint16),
                              at=[int(first[pos[k]]) for k in keep], qp=u["qp"], finish=True, data=u["data"]))
    for u, data in zip(units, device_encode(hip, rec_units, int16)):
        assert np.array_equal(data, u["data"])                            # the writer's bytes are the oracle's
        u["data"] = data
    assert sum(not on for u in units for on in u["coded"]) and sum(u["coded"].count(True) for u in units) >= 4
    assert_valid(run_elements(hip, units, int16), units, int16)


# ---------------------------------------------------------------------------------------------- 4. guards
def _guard_family(rng):
    """cmp x back x three guarding values: element 0 (three bypass bins) guards element `back` (an Exp-Golomb code) against 4,
    a block lies between them, and the same block position carries the same guard"""
    units = []
    for back in (1, 63, 64, 255):
        for cmp in range(4):
            for v0 in (3, 4, 5):
                fill, fv = E.random_plan(rng, back - 1, kinds=[E.CTX_BIN, E.EP_BINS, E.UNARY_EP, E.TRUNC_BIN], guard_frac=0.0, small=True)
                holds = (v0 != 4, v0 == 4, v0 >= 4, v0 < 4)[cmp]
                plan = np.concatenate([[[el(E.EP_BINS, n=3), 0]], fill, [[el(E.EXP_GOLOMB, count=1), gd(back, cmp, 4)]]]).astype(np.uint32)
                plan, values = E.close(plan, [v0] + fv + [9 if holds else 0])
                (m0, c0), (m1, c1) = small_block(rng), small_block(rng)
                mid = (back + 1) // 2                                      # behind element 0, in front of element `back`
                units.append(E.make_unit(rng, plan, values, [m0, m1], [c0, c1], at=[mid, back], guards=[0, gd(back, cmp, 4)]))
                assert units[-1]["coded"] == [True, holds]
    return units


def test_guards_of_every_comparison_and_distance_across_groups_and_blocks(hip):
    rng = np.random.default_rng(0xE40)
    units = _guard_family(rng)
    assert {(u["coded"][1], len(u["plan"])) for u in units} >= {(on, n) for on in (True, False) for n in (3, 65, 66, 257)}
    assert_valid(run_elements(hip, units), units, False)
    # 1 030 substreams, four waves per workgroup: each wave reads its guards from its own ring (the back 1 and back 63 families,
    # repeated)
    wide = [units[k % 24] for k in range(1030)]
    assert_valid(run_elements(hip, wide), wide, False, "wide")
    # two substreams with the same plan and other bytes take different paths
    a, b = units[0], units[1]                                              # back 1, !=, guarding values 3 and 4
    assert np.array_equal(a["plan"], b["plan"]) and a["coded"] != b["coded"] and not np.array_equal(a["data"], b["data"])


def test_chains_a_guarded_terminate_bin_and_blocks_behind_both_cbf_values(hip):
    rng = np.random.default_rng(0xE41)
    units = []
    # a chain of three guards whose first is skipped: 0 -> skipped -> skipped (== 1 on a skipped 0) -> coded (== 0 on a skipped 0)
    plan = np.array([[el(E.EP_BINS, n=1), 0], [el(E.CTX_BIN, ctx=12), gd(1, capi.GUARD_EQ, 1)], [el(E.UNARY_EP, max_symbol=9), gd(1, capi.GUARD_EQ, 1)],
                     [el(E.EP_BINS, n=7), gd(1, capi.GUARD_EQ, 0)]], np.uint32)
    units.append(E.make_unit(rng, *E.close(plan, [0, 0, 0, 0x55])))
    # a guarded terminate bin, coded and skipped (the skipped one is not the stream's last bin: no stop check)
    for v0 in (1, 0):
        plan = np.array([[el(E.CTX_BIN, ctx=3), 0], [el(E.EP_BINS, n=4), 0], [el(E.TRM), gd(2, capi.GUARD_EQ, 1)]], np.uint32)
        units.append(E.make_unit(rng, plan, [v0, 9, v0], finish=bool(v0)))
    string = E.expand(units[-1]["plan"], units[-1]["values"], [], [], None, None)[0]   # a terminate bin is coded behind it and not read
    units[-1]["data"] = H.load_oracle().encode_records(np.concatenate([string, M.TRM_END]), units[-1]["qp"], 2, 3)[0]
    # blocks behind a cbf of 0 and of 1 in one substream, each cbf also guarding a transform_skip_flag element
    (m0, c0), (m1, c1), (m2, c2) = small_block(rng), small_block(rng), small_block(rng)
    plan = np.array([[el(E.CTX_BIN, ctx=20), 0], [el(E.CTX_BIN, ctx=21), 0], [el(E.CTX_BIN, ctx=22), 0],
                     [el(E.CTX_BIN, ctx=310), gd(3, capi.GUARD_EQ, 1)], [el(E.CTX_BIN, ctx=311), gd(3, capi.GUARD_EQ, 1)],
                     [el(E.CTX_BIN, ctx=311), gd(3, capi.GUARD_EQ, 1)]], np.uint32)
    plan, values = E.close(plan, [1, 0, 1, 0, 0, 0])
    units.append(E.make_unit(rng, plan, values, [m0, m1, m2], [c0, c1, c2], at=[4, 5, 6],
                             guards=[gd(4, capi.GUARD_EQ, 1), gd(4, capi.GUARD_EQ, 1), gd(4, capi.GUARD_NE, 0)]))
    assert units[-1]["coded"] == [True, False, True]
    # one context store: thirty skipped elements on the context that thirty coded ones behind them use, skewed so that it moves far
    plan = np.array([[el(E.EP_BINS, n=1), 0]] + [[el(E.CTX_BIN, ctx=50), gd(k + 1, capi.GUARD_EQ, 1)] for k in range(30)] +
                    [[el(E.CTX_BIN, ctx=50), 0]] * 30, np.uint32)
    units.append(E.make_unit(rng, *E.close(plan, [0] + [0] * 30 + [1] * 28 + [0, 1])))
    t_skipped = 1                                                          # the skipped block of the cbf unit, among all blocks

    def mutate(P):                                                         # a skipped block's descriptor is not examined
        P["tus"][t_skipped]["log2_width"], P["tus"][t_skipped]["channel"] = 7, 3
    r = run_elements(hip, units, mutate=mutate)
    assert_valid(r, units, False)
    for s in (0, 1, 2, 4):                                                 # the exact reader agrees where there are no blocks
        m = E.read_plan(units[s]["plan"], units[s]["data"], units[s]["qp"], finish=units[s]["finish"])
        assert m["values"] == units[s]["values"] and (m["n_bits"], m["flags"]) == (int(r["res"]["n_bits"][s]), 0)
    # ... and had the skipped ones adapted the context, the coded ones would read other bins
    orc = H.load_oracle()
    moved = [E.op_of(el(E.EP_BINS, n=1))] + [E.op_of(el(E.CTX_BIN, ctx=50))] * 60
    assert orc.decode_ops(np.array(moved, np.uint32), units[4]["qp"], 2, np.concatenate([units[4]["data"], np.zeros(16, np.uint8)]))[1][31:].tolist() != [1] * 28 + [0, 1]


# ---------------------------------------------------------------------------------------------- 5. damaged input, block-free
# Every kind the writer's helpers have, ALIGN among them (TRM closes the plan).  ALIGN on bytes no writer produced can lead to the
# header's state OUT OF RANGE: the model names the first element met in it, and what lies in front of it is compared exactly.
DAMAGED_KINDS = (E.CTX_BIN, E.EP_BINS, E.REM_ABS, E.UNARY_MAX, E.UNARY_EP, E.EXP_GOLOMB, E.TRUNC_BIN, E.ALIGN)
DAMAGED_SEED = 0xE50   # picked on the CPU with the exact reader: other values, changed guard outcomes, BAD_STOP and BAD_VALUE all occur


@functools.lru_cache(maxsize=None)
def _damaged_plans(seed, n_sub=200):
    rng = np.random.default_rng(seed)
    units = []
    for s in range(n_sub):
        u = E.make_unit(rng, *E.close(*E.random_plan(rng, int(rng.integers(5, 40)), kinds=DAMAGED_KINDS, guard_frac=0.5, small=True)))
        d = u["data"].copy()
        for _ in range(int(rng.integers(1, 4))):
            d[int(rng.integers(0, len(d)))] ^= 1 << int(rng.integers(0, 8))
        if d[0] == 0xFF:
            d[0] = 0x7F                                                    # a refused start is test 6's
        u["data"] = np.concatenate([d, np.zeros(16 * len(u["plan"]) + 16, np.uint8)])   # the input cannot run out
        units.append(u)
    return units


def test_damaged_block_free_streams_against_the_exact_reader(hip):
    """200 substreams, one to three flipped bits, zero-padded: the exact reader judges every one — values up to a stop, nothing
    behind it, n_bits and flags (within {BAD_STOP, BAD_VALUE})."""
    units = _damaged_plans(DAMAGED_SEED)
    r = run_elements(hip, units)
    other = flipped = out_of_range = 0
    seen = set()
    for s, u in enumerate(units):
        first, front = E.first_out_of_range(u["plan"], u["data"], u["qp"])
        if first is not None:                                              # unspecified from element `first` on: the front exactly, the rest bounded
            out_of_range += 1
            assert r["values"][s][:first].tolist() == front == E.read_plan(u["plan"][:first], u["data"], u["qp"])["values"], s
            assert (int(r["res"]["flags"][s]) & ~(H.RES_BAD_STOP | E.RES_BAD_VALUE)) == 0, s
            continue
        m = E.read_plan(u["plan"], u["data"], u["qp"], finish=True)
        fl = int(r["res"]["flags"][s])
        assert fl in (0, H.RES_BAD_STOP, E.RES_BAD_VALUE) and (int(r["res"]["n_bits"][s]), fl) == (m["n_bits"], m["flags"]), s
        n = m["n_written"]
        assert r["values"][s][:n].tolist() == m["values"] and (r["values"][s][n:] == VAL_GUARD).all(), s
        assert (n == len(u["plan"])) == (fl != E.RES_BAD_VALUE), s
        seen.add(fl)
        other += m["values"] != u["values"][:n]
        _, _, was, _ = E.expand(u["plan"], u["values"], [], [], None, None)
        flipped += m["active"] != was[:n]
    print("damaged plans: %d decoded to other values, %d with a changed guard outcome, %d met the state OUT OF RANGE, flags seen %s" %
          (other, flipped, out_of_range, sorted(seen)))
    assert 0 < out_of_range < len(units) // 4
    assert other > 0 and flipped > 0 and seen == {0, H.RES_BAD_STOP, E.RES_BAD_VALUE}


def test_a_terminate_bin_of_one_in_mid_plan_followed_by_each_bypass_kind(hip):
    """The header's state OUT OF RANGE, reached the writer's way: [head, TRM = 1, one bypass-coded element, tail] for every bypass
    kind.  Everything up to the terminate bin is exact and is what the exact reader and the state tracker say; the element behind
    it is the first met in the state, so from there on only this is required: no flag but BAD_STOP / BAD_VALUE, every value of the
    plan written or left alone as a whole tail, nothing outside the substream's values."""
    rng = np.random.default_rng(0xE58)
    kinds = [el(E.EP_BINS, n=1), el(E.EP_BINS, n=2), el(E.EP_BINS, n=32), el(E.UNARY_EP, max_symbol=32), el(E.EXP_GOLOMB, count=0),
             el(E.EXP_GOLOMB, count=31), el(E.REM_ABS, rice=0, cutoff=5, max_log2=15), el(E.REM_ABS, rice=14, cutoff=12, max_log2=20),
             el(E.TRUNC_BIN, max_symbol=5), el(E.TRUNC_BIN, max_symbol=(1 << 28) - 1)]
    units = []
    for w0 in kinds:
        head, hv = E.close(*E.random_plan(rng, 9, guard_frac=0.3, small=True, backs=(1, 2)))
        tail, _ = E.random_plan(rng, 6, guard_frac=0.0, small=True)
        u = E.make_unit(rng, head, hv, finish=False)
        u["plan"] = np.concatenate([head, [[w0, 0]], tail]).astype(np.uint32)
        u["data"] = np.concatenate([u["data"], rng.integers(0, 256, 64).astype(np.uint8)])
        units.append(u)
    r = run_elements(hip, units)
    for s, u in enumerate(units):
        first, front = E.first_out_of_range(u["plan"], u["data"], u["qp"])
        assert first == 10 and front == u["values"] and front[-1] == 1, s
        assert r["values"][s][:10].tolist() == front == E.read_plan(u["plan"][:10], u["data"], u["qp"])["values"], s
        assert (int(r["res"]["flags"][s]) & ~(H.RES_BAD_STOP | E.RES_BAD_VALUE)) == 0, s
        written = r["values"][s] != VAL_GUARD
        assert written[:10].all() and not (np.diff(written.astype(int)) > 0).any(), s       # a prefix of the plan, no holes


# ---------------------------------------------------------------------------------------------- 6. refusals on the device
BAD_ENTRIES = [(9, 0), (15, 0), (el(E.CTX_BIN, ctx=379), 0), (el(E.UNARY_MAX, ctx=1, ctx_n=400, max_symbol=3), 0),
               (el(E.UNARY_MAX, ctx=511, ctx_n=1, max_symbol=3), 0), (el(E.EP_BINS, n=33), 0), (el(E.UNARY_EP, max_symbol=33), 0),
               (el(E.TRUNC_BIN), 0), (el(E.REM_ABS, rice=15, max_log2=15), 0), (el(E.REM_ABS, max_log2=14), 0), (el(E.REM_ABS, max_log2=21), 0),
               (el(E.REM_ABS, cutoff=13, max_log2=20), 0), (el(E.CTX_BIN, ctx=1), 0x400), (el(E.CTX_BIN, ctx=1), 0x8000),
               (el(E.CTX_BIN, ctx=1), gd(8))]


def test_each_kind_of_bad_plan_entry_stops_its_substream_and_no_other(hip):
    """Substream 2k + 1 gets bad entry k as its element 7 (behind block 0 at 3, in front of block 1 at 9) — the guard that reaches
    in front of the plan has back 8 there —, the even substreams stay as they are; then two substreams whose block guard is bad."""
    orc = H.load_oracle()
    rng = np.random.default_rng(0xE60)
    n_bad = len(BAD_ENTRIES)
    units = []
    for s in range(2 * n_bad + 5):
        plan, values = E.close(*E.random_plan(rng, 12, guard_frac=0.4, small=True, backs=(1, 2, 3)))
        units.append(E.make_unit(rng, plan, values, *zip(small_block(rng), small_block(rng)), at=[3, 9], guards=[0, 0]))
    bad_at = {2 * k + 1: 7 for k in range(n_bad)}
    g_res, g_back = 2 * n_bad + 1, 2 * n_bad + 3                            # block 1's guard: reserved bits, back 10 at element 9

    def mutate(P):
        for s, i in bad_at.items():
            P["plan"][int(P["desc"]["rec_offset"][s]) + i] = BAD_ENTRIES[s // 2]
        P["tu_guard"][2 * g_res + 1] = 0x0800 | 1
        P["tu_guard"][2 * g_back + 1] = gd(10)
    r = run_elements(hip, units, mutate=mutate)
    written = []
    for s, u in enumerate(units):
        stop_el = bad_at.get(s, 9 if s in (g_res, g_back) else None)
        if stop_el is None:
            assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == want_walk(u) and r["res"]["flags"][s] == 0, s
            assert r["values"][s].tolist() == u["values"], s
            written.append([True, True])
            continue
        # everything in front of the entry (block 0 and, for a bad block guard, elements 7 and 8), nothing behind it
        string, is_el, _, _ = E.expand(u["plan"][:stop_el], u["values"][:stop_el], u["metas"][:1], u["blocks"][:1], [3], None)
        rc, _, n_bits = orc.decode_records(string, u["qp"], 2, u["data"])
        assert rc == 0 and (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (n_bits, H.RES_BAD_RECORD), s
        assert r["values"][s][:stop_el].tolist() == u["values"][:stop_el] and (r["values"][s][stop_el:] == VAL_GUARD).all(), s
        assert np.array_equal(coded(r["blocks"][s][0]), coded(u["blocks"][0])), s
        t0 = int(r["P"]["tile_first"][s])
        assert int(r["info"][t0]) == want_info(u)[0] and int(r["info"][t0 + 1]) == WORD_GUARD_U, s
        written.append([True, False])
    assert_blocks_untouched(r, units, False, written)


def test_bad_value_no_bytes_and_a_refused_start(hip):
    """An Exp-Golomb prefix out of an all-ones bypass run: CABAC_RES_BAD_VALUE at that element, for count 0, 5 and 31; byte_capacity
    0: CABAC_RES_UNDERRUN with nothing read; a first byte 0xFF: CABAC_RES_BAD_STOP with nothing parsed."""
    orc = H.load_oracle()
    rng = np.random.default_rng(0xE61)
    ones = np.array([H.REC_ALIGN] + [H.REC_EP | 0x8000] * 40 + [0x81FF], np.uint16)
    run = orc.encode_records(ones, 30, 2, 3)[0]
    units = []
    for count in (0, 5, 31):
        plan = np.array([[el(E.ALIGN), 0], [el(E.EXP_GOLOMB, count=count), 0], [el(E.CTX_BIN, ctx=7), 0]], np.uint32)
        units.append(dict(metas=[], blocks=[], plan=plan, values=[0, 0, 0], at=None, guards=None, coded=[], qp=30, finish=True, data=run))
    for _ in range(3):
        plan, values = E.close(*E.random_plan(rng, 6, guard_frac=0.3, small=True, backs=(1, 2)))
        units.append(E.make_unit(rng, plan, values, *zip(small_block(rng)), at=[2], guards=[0]))
    units[4]["data"] = np.concatenate([[0xFF], units[4]["data"][1:]]).astype(np.uint8)

    def mutate(P):                                                         # whatever lies at a substream without bytes is not read
        P["desc"]["byte_capacity"][3] = 0
        P["bytes"][int(P["desc"]["byte_offset"][3]):int(P["desc"]["byte_offset"][3]) + 16] = 0xFF
    r = run_elements(hip, units, mutate=mutate)
    for s, count in enumerate((0, 5, 31)):
        m = E.read_plan(units[s]["plan"], run, 30, finish=True)
        rc, _, n_bits = orc.decode_records(ones[:1 + 32 - count], 30, 2, run)
        assert rc == 0 and m["flags"] == E.RES_BAD_VALUE and m["n_bits"] == n_bits
        assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (n_bits, E.RES_BAD_VALUE), s
        assert r["values"][s].tolist() == [0, VAL_GUARD, VAL_GUARD], s
    # without a byte the flag is reported alone; values and blocks from the read past byte_capacity on are unspecified (the header,
    # as in the unit parse): the walk goes on over zeros, inside the substream's own outputs (the guard words and the neighbours)
    assert int(r["res"]["flags"][3]) == H.RES_UNDERRUN
    assert (int(r["res"]["n_bits"][4]), int(r["res"]["flags"][4])) == (8, H.RES_BAD_STOP) and (r["values"][4] == VAL_GUARD).all()
    assert int(r["info"][1]) == WORD_GUARD_U
    assert (int(r["res"]["n_bits"][5]), int(r["res"]["flags"][5])) == want_walk(units[5]) and r["values"][5].tolist() == units[5]["values"]
    assert np.array_equal(coded(r["blocks"][5][0]), coded(units[5]["blocks"][0]))
    assert_blocks_untouched(r, units, False, [[], [], [], [True], [False], [True]])     # [3]: unspecified, its own region at the most


# ---------------------------------------------------------------------------------------------- 7. the batch form
@functools.lru_cache(maxsize=None)
def _batch_units():
    rng = np.random.default_rng(0xE70)
    return [_guarded_unit(rng, n_el, n_blocks) for n_el, n_blocks in ((130, 6), (7, 3), (1, 1), (20, 0))]


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("int16", [False, True])
def test_batch_form_gives_the_device_form_s_results(hip, pinned, int16):
    units = list(_batch_units())
    r = run_elements(hip, units, int16)
    assert_valid(r, units, int16)
    P = r["P"]
    keep = []

    def buf(a):
        if not pinned:
            return a.copy()
        keep.append(capi.PinnedArray((max(len(a), 1),) + a.shape[1:], a.dtype))
        keep[-1].array[:len(a)] = a
        return keep[-1].array[:len(a)]
    coeff = buf(np.full(P["total"], sentinel(int16), np.int16 if int16 else np.int32))
    values = buf(np.full(len(P["plan"]), VAL_GUARD, np.uint32))
    info = buf(np.full(P["n_tu"], WORD_GUARD_U, np.uint32))
    host = capi.CabacHip(0)
    co, val, res, inf = host.parse_elements_batch(P["desc"], buf(P["bytes"]), P["tile_first"], P["tus"][:P["n_tu"]], P["tu_at"], P["tu_guard"],
                                                  buf(P["plan"]), P["total"], int16=int16, coeff=coeff, values=values, info=info)
    assert np.array_equal(res, r["res"]) and np.array_equal(inf, r["info"]) and np.array_equal(val, r["all_values"])
    if int16:                                                              # output only: zero where nothing is written
        mask = r["co"] != np.int32(np.int16(sentinel(True)))
        assert np.array_equal(co.astype(np.int32)[mask], r["co"][mask]) and not co[~mask].any()
    else:
        assert np.array_equal(co, r["co"])
    host.close()
    for k in keep:
        k.close()


def test_batch_form_refuses_what_the_header_says(hip):
    units = list(_batch_units())
    P = E.pack(units)
    host = capi.CabacHip(0)

    def call(**kw):
        a = dict(desc=P["desc"], tile_first=P["tile_first"], tu_at=P["tu_at"], tu_guard=P["tu_guard"], plan=P["plan"], data=P["bytes"], total=P["total"])
        a.update(kw)
        coeff, values = np.full(P["total"], 0x5A5A5A5A, np.int32), np.full(len(P["plan"]), VAL_GUARD, np.uint32)
        info = np.full(P["n_tu"], WORD_GUARD_U, np.uint32)
        with pytest.raises(capi.CabacHipError) as e:
            host.parse_elements_batch(a["desc"], a["data"], a["tile_first"], P["tus"][:P["n_tu"]], a["tu_at"], a["tu_guard"], a["plan"],
                                      a["total"], coeff=coeff, values=values, info=info)
        assert e.value.status == -2
        assert (coeff == 0x5A5A5A5A).all() and (values == VAL_GUARD).all() and (info == WORD_GUARD_U).all()   # no output touched
        return str(e.value)
    def raw(coeff_bytes=4, **null):                                        # the C entry point itself: a NULL that is needed, a bad coeff_bytes
        coeff, values = np.full(P["total"], 0x5A5A5A5A, np.int32), np.full(len(P["plan"]), VAL_GUARD, np.uint32)
        res = np.zeros(len(units), H.RESULT_DTYPE)
        ptr = dict(desc=P["desc"], bytes=P["bytes"], tile_first=P["tile_first"], tus=P["tus"], plan=P["plan"], coeff=coeff, values=values, results=res)
        a = {k: (None if null.get(k) else v.ctypes.data) for k, v in ptr.items()}
        rc = host.L.cabac_hip_parse_elements_batch(host.h, len(units), a["desc"], a["bytes"], len(P["bytes"]), a["tile_first"], a["tus"],
                                                   P["tu_at"].ctypes.data, P["tu_guard"].ctypes.data, a["plan"], len(P["plan"]), a["coeff"],
                                                   coeff_bytes, P["total"], a["values"], None, a["results"])
        assert rc == -2 and (coeff == 0x5A5A5A5A).all() and (values == VAL_GUARD).all() and not res["flags"].any()
    for name in ("desc", "bytes", "tile_first", "tus", "plan", "coeff", "values", "results"):
        raw(**{name: True})
    for cb in (0, 1, 3, 8):
        raw(coeff_bytes=cb)
    d = P["desc"].copy()
    d["n_records"][3] += 1                                                 # the last plan leaves n_elements_total
    assert "n_elements_total" in call(desc=d)
    d = P["desc"].copy()
    d["rec_offset"][0] = len(P["plan"]) + 1
    assert "n_elements_total" in call(desc=d)
    d = P["desc"].copy()
    d["byte_capacity"][3] = len(P["bytes"])
    assert "bytes out of range" in call(desc=d)
    d = P["desc"].copy()
    d["init_id"][1] |= 3
    assert "init_id" in call(desc=d)
    tf = P["tile_first"].copy()
    tf[2] = tf[1] - 1
    assert "tile_first" in call(tile_first=tf)
    at = P["tu_at"].copy()
    at[2], at[1] = 0, 131
    assert "decreases" in call(tu_at=at)
    at = P["tu_at"].copy()
    at[5] = 132                                                            # the plan has 131 elements
    assert "exceeds" in call(tu_at=at)
    assert "coefficients" in call(total=P["total"] - 1)
    g = P["tu_guard"].copy()
    g[7] = 0x400
    msg = call(tu_guard=g)
    assert "substream 1" in msg and "block 1" in msg
    g = P["tu_guard"].copy()
    g[6] = gd(int(P["tu_at"][6]) + 1)
    assert "substream 1" in call(tu_guard=g) and "block 0" in call(tu_guard=g)
    for k, (w0, gw) in enumerate(BAD_ENTRIES):
        plan = P["plan"].copy()
        s = k % 2                                                          # substreams 0 and 1
        plan[int(P["desc"]["rec_offset"][s]) + 4] = (w0, gw if gw != gd(8) else gd(5))
        msg = call(plan=plan)
        assert "substream %d" % s in msg and "element 4" in msg, (k, msg)
    co, val, res, inf = host.parse_elements_batch(P["desc"], P["bytes"], P["tile_first"], P["tus"][:P["n_tu"]], P["tu_at"], P["tu_guard"],
                                                  P["plan"], P["total"])
    assert not res["flags"].any() and val.tolist() == [v for u in units for v in u["values"]]   # and the ctx still works
    host.close()


# ---------------------------------------------------------------------------------------------- 8. stream order
def test_stream_order_on_the_default_stream(hip):
    """Fill -> call -> read on torch's default stream (stream=0 -> CABAC_HIP_STREAM_DEFAULT), no host synchronisation between."""
    import torch
    assert torch.cuda.current_stream().cuda_stream == 0
    units = list(_batch_units())
    P = E.pack(units)
    own = capi.CabacHip(0, stream=0)
    src = [dev(P["desc"], np.uint8), dev(P["bytes"]), dev(P["tile_first"].view(np.int32)), dev(P["tus"][:P["n_tu"]], np.uint8),
           dev(P["tu_at"].view(np.int32)), dev(P["tu_guard"].view(np.int32)), dev(P["plan"].view(np.int32))]
    torch.cuda.synchronize()
    for _ in range(2):
        big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
        big.fill_(0xA5)                                                    # a long fill in front, then the operands are produced ON the stream
        ops = [torch.zeros_like(s) for s in src]
        for o, s in zip(ops, src):
            o.copy_(s)
        out = Out(P, False)
        p_co, p_val, p_info, p_res = out.ptrs()
        own.parse_elements_device(len(units), *[o.data_ptr() for o in ops], p_co, p_val, p_res, d_tu_info=p_info)
        co, val, info, res = out.read()
        assert not res["flags"].any() and val.tolist() == [v for u in units for v in u["values"]]
        t = 0
        for u in units:
            for c, on in zip(u["blocks"], u["coded"]):
                h, w = c.shape
                got = co[int(P["offsets"][t]):int(P["offsets"][t]) + w * h]
                assert np.array_equal(coded(got.reshape(h, w)), coded(c)) if on else (got == sentinel(False)).all()
                assert (int(info[t]) == E.NOT_CODED) == (not on)
                t += 1
        del big, ops
    own.close()
