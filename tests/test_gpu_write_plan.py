"""GPU: the plan write (include/cabac_hip_write_plan.h; csrc/cabac_plan_write.hip) — a plan, the values of its real elements and
the blocks' coefficients coded into substreams on the device — against tests/write_plan_model.py, that is parse_plan_model's
fill / expand and the oracle's encoder (identity W1), against cabac_hip_binarize_device + cabac_hip_encode_residual_device (W2)
and read back by cabac_hip_parse_plan_device (W3).  Everything is bit-exact: == on integers.  Expected bytes never come from the
code under test.  Every output sits between guard words that are checked, the inputs are checked unchanged, and the slots of
d_values_in that the header says are not used (computed entries, skipped elements) hold garbage."""
import numpy as np
import pytest

import helpers as H
import parse_elements_model as E
import parse_plan_model as PM
import write_plan_model as W
from entropy_coding_amd import capi
from test_gpu_residual_estimate import dev
from test_parse_plan_model import TU_OUTCOMES

pytestmark = pytest.mark.gpu

G = 64                                                             # guard elements on either side of every output
BYTE_GUARD, WORD_GUARD, VAL_GUARD, OFF_GUARD = 0xA5, -0x11223345, 0xEEEEEEEE - (1 << 32), -7
el, gd, cond, bi = capi.element, capi.guard, capi.cond, capi.block_info
NE, EQ, GE, LT = capi.GUARD_NE, capi.GUARD_EQ, capi.GUARD_GE, capi.GUARD_LT
CB = el(E.CTX_BIN, ctx=33)


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


def sub(plan, real, metas=(), blocks=(), at=None, guards=None, qp=30, garbage=True):
    """One substream: the model's answer (want) beside the device's input, in which every slot of values_in that is not used —
    a computed entry, a skipped element — holds garbage"""
    plan = np.asarray(plan, np.uint32).reshape(-1, 2)
    blocks = [np.clip(np.asarray(b, np.int32), -32767, 32767) for b in blocks]
    want = W.write(plan, real, metas, blocks, at, guards, qp)
    vin = np.array([int(v) & 0xFFFFFFFF for v in real], np.uint64).astype(np.uint32)
    if garbage and want["flag"] == 0:
        active = PM.fill(plan, real, metas, blocks, at, guards)[3]
        for i, on in enumerate(active):
            if not on:
                vin[i] = 0xDEAD0000 + (i & 0xFFFF)
    return dict(plan=plan, values_in=vin, metas=list(metas), blocks=blocks, at=None if at is None else list(at),
                guards=None if guards is None else list(guards), qp=int(qp), want=want)


def run(hip, subs, int16=False, in_place=False, null_outputs=False):
    """cabac_hip_write_plan_device over `subs` -> dict(P, payload [per substream], offsets, res, values [per substream], infos
    [per substream]); checks on the way that nothing outside the outputs' ranges was written and no input changed."""
    import torch
    units = [dict(plan=s["plan"], metas=s["metas"], blocks=s["blocks"], at=s["at"], guards=s["guards"], qp=s["qp"], finish=True,
                  data=np.zeros(0, np.uint8)) for s in subs]
    P = PM.pack(units)
    P["desc"]["init_id"] = W.SUB_FLAGS
    P["desc"]["byte_offset"], P["desc"]["byte_capacity"] = 0x7FFFFFF0, 0            # ignored by the contract
    n_sub, n_tu, n_el = len(subs), P["n_tu"], len(P["plan"])
    coeff = np.zeros(max(P["total"], 1), np.int16 if int16 else np.int32)
    t = 0
    for s in subs:
        for b in s["blocks"]:
            coeff[int(P["offsets"][t]): int(P["offsets"][t]) + b.size] = b.reshape(-1)
            t += 1
    vin = np.concatenate([s["values_in"] for s in subs] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    cap = sum(len(s["want"]["data"]) for s in subs) + 40
    t_desc, t_first = dev(P["desc"], np.uint8), dev(P["tile_first"].view(np.int32))
    t_plan, t_vin, t_co = dev(np.concatenate([P["plan"].reshape(-1), np.zeros(2, np.uint32)]).view(np.int32)), dev(np.concatenate([vin, [0]]).astype(np.uint32).view(np.int32)), dev(coeff)
    t_tu = dev(P["tus"], np.uint8)
    t_at = None if P["tu_at"] is None else dev(np.concatenate([P["tu_at"], [0]]).astype(np.uint32).view(np.int32))
    t_gd = None if P["tu_guard"] is None else dev(np.concatenate([P["tu_guard"], [0]]).astype(np.uint32).view(np.int32))
    t_pay = torch.full((cap + 2 * G,), BYTE_GUARD, dtype=torch.uint8, device="cuda")
    t_off = torch.full((n_sub + 1 + 2 * G,), OFF_GUARD, dtype=torch.int64, device="cuda")
    t_res = torch.full((2 * n_sub + 2 * G,), WORD_GUARD, dtype=torch.int32, device="cuda")
    t_val = torch.full((n_el + 2 * G,), VAL_GUARD, dtype=torch.int32, device="cuda")
    t_info = torch.full((n_tu + 2 * G,), WORD_GUARD, dtype=torch.int32, device="cuda")
    if in_place:
        t_val[G:G + n_el] = t_vin[:n_el]
    p_vin = t_val.data_ptr() + 4 * G if in_place else t_vin.data_ptr()
    hip.write_plan_device(n_sub, t_desc.data_ptr(), t_plan.data_ptr() if n_el else 0, p_vin if n_el else 0, t_first.data_ptr(), n_tu,
                          t_tu.data_ptr() if n_tu else 0, t_at.data_ptr() if t_at is not None else 0,
                          t_gd.data_ptr() if t_gd is not None else 0, t_co.data_ptr() if n_tu else 0, t_pay.data_ptr() + G, cap,
                          t_off.data_ptr() + 8 * G, t_res.data_ptr() + 4 * G,
                          0 if (null_outputs or not n_el) else t_val.data_ptr() + 4 * G, 0 if null_outputs else t_info.data_ptr() + 4 * G,
                          int16=int16)
    hip.synchronize()
    pay, off, res = t_pay.cpu().numpy(), t_off.cpu().numpy(), t_res.cpu().numpy()
    val, info = t_val.cpu().numpy().view(np.uint32), t_info.cpu().numpy()
    for a, g, n in ((pay, BYTE_GUARD, cap), (off, OFF_GUARD, n_sub + 1), (res, WORD_GUARD, 2 * n_sub), (t_val.cpu().numpy(), VAL_GUARD, n_el),
                    (info, WORD_GUARD, n_tu)):
        assert (a[:G] == g).all() and (a[G + n:] == g).all(), "written outside an output's range"
    off = off[G:G + n_sub + 1]
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] <= cap
    assert (pay[G + int(off[-1]): G + cap] == BYTE_GUARD).all(), "written behind the reported payload"
    assert np.array_equal(t_co.cpu().numpy(), coeff) and np.array_equal(t_plan.cpu().numpy().view(np.uint32)[:2 * n_el], P["plan"].reshape(-1))
    if not in_place:
        assert np.array_equal(t_vin.cpu().numpy().view(np.uint32)[:n_el], vin)
    if null_outputs:
        assert (val[G:G + n_el] == VAL_GUARD & 0xFFFFFFFF).all() and (info[G:G + n_tu] == WORD_GUARD).all()
    res = res[G:G + 2 * n_sub].view(H.RESULT_DTYPE)
    out = dict(P=P, offsets=off, res=res, payload=[], values=[], infos=[])
    for s in range(n_sub):
        out["payload"].append(pay[G + int(off[s]): G + int(off[s + 1])])
        r0 = int(P["desc"]["rec_offset"][s])
        out["values"].append(val[G + r0: G + r0 + len(subs[s]["plan"])])
        out["infos"].append(info[G + int(P["tile_first"][s]): G + int(P["tile_first"][s + 1])].view(np.uint32))
    return out


def assert_w1(r, subs, what="", outputs=True):
    """Payload, offsets, n_bits, flags, filled values and info words are the model's; a stopped substream codes nothing"""
    for s, x in enumerate(subs):
        w = x["want"]
        assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (w["n_bits"], w["flag"]), (what, s)
        assert np.array_equal(r["payload"][s], w["data"]), (what, s)
        if w["flag"] == 0 and outputs:
            assert r["values"][s].tolist() == w["values"], (what, s)
            assert r["infos"][s].tolist() == w["infos"], (what, s)


# ------------------------------------------------------------------------------------------------ W1: the worked transform unit
def tu_sub(rng, outcomes):
    """Several transform units in a row in one substream, closed by the terminate bin (parse_plan_model.tu_unit's input)"""
    plans, values, metas, blocks, at, guards = [], [], [], [], [], []
    for k, o in enumerate(outcomes):
        p, v, m, b, a, g = PM.tu_case(rng, *o)
        plans.append(p)
        values += v
        metas += m
        blocks += b
        at += [x + PM.TU_LEN * k for x in a]
        guards += g
    plan, values = E.close(np.concatenate(plans), values)
    return sub(plan, values, metas, blocks, at, guards, qp=int(rng.integers(0, 64)))


_TU = {}


def tu_subs(per):
    """Every outcome of TU_OUTCOMES (cbf_cb x cbf_cr x cbf_y x ts x last_zero x violating; a violating block has scanPosLast > 0,
    so those two do not combine) at least once, `per` units per substream — built once, shared by the int32 and int16 runs"""
    if per not in _TU:
        rng = np.random.default_rng(0x7E0 + per)
        order = [TU_OUTCOMES[k] for k in rng.permutation(len(TU_OUTCOMES))]
        order += order[:(-len(order)) % per]
        _TU[per] = [tu_sub(rng, order[k: k + per]) for k in range(0, len(order), per)]
    return _TU[per]


@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
@pytest.mark.parametrize("per", [1, 3])
def test_w1_worked_transform_unit(hip, per, int16):
    """cu_qp_delta behind the OR of three cbfs, tu_cbf_cr on the context tu_cbf_cb selects, mts_idx behind the luma block's
    scanPosLast: decided on the device.  Calls of 1, 4 and 5 substreams in turn; every other call writes the values in place."""
    subs, k, g = tu_subs(per), 0, 0
    coded_some = skipped_some = False
    while k < len(subs):
        n = (1, 4, 5)[g % 3]
        part = subs[k: k + n]
        r = run(hip, part, int16=int16, in_place=bool(g & 1))
        assert_w1(r, part, (per, int16, g))
        coded_some |= any(any(x["want"]["coded"]) for x in part)
        skipped_some |= any(not all(x["want"]["coded"]) for x in part)
        k += n
        g += 1
    assert coded_some and skipped_some


# ------------------------------------------------------------------------------------------------ W1: chunk and ring edges
def chain_plan(n, kind="guards"):
    """A reference chain as deep as the plan is long: entry i lives only if entry i - 1 does -> (plan, real values)"""
    plan, real = [(CB, 0)], [1]
    for i in range(1, n):
        if kind == "guards" or i % 2:
            plan.append((CB, gd(1, NE, 0)))                        # a guard on a guarded element
            real.append(1)
        else:
            plan.append(cond(1, NE, 0, capi.JOIN_AND, 2))          # a COND on it and on the one in front
            real.append(0)
    return np.array(plan, np.uint32), real


def edge_subs():
    rng = np.random.default_rng(0xED6E)
    subs = []
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 600):
        plan, real = PM.random_cond_plan(rng, n)
        subs.append(sub(plan, real, qp=int(rng.integers(0, 64))))
    # a reference 255 back whose ring slot is the next element's: elements 0 .. 299, element i >= 255 guarded by i - 255
    plan = np.array([(el(E.EP_BINS, n=3), gd(255, GE, 4) if i >= 255 else 0) for i in range(300)], np.uint32)
    subs.append(sub(plan, [int(v) for v in rng.integers(0, 8, 300)]))
    # guards on guards across the chunk boundary at 64, alive and dying on the way
    for real_at_60 in (1, 0):
        plan, real = chain_plan(130)
        real[60] = real_at_60
        subs.append(sub(plan, real))
    # as deep as the chunk is wide, through CONDs too; and one that starts inside a chunk
    plan, real = chain_plan(64, "mixed")
    subs.append(sub(plan, real))
    plan, real = chain_plan(100, "mixed")
    real[41] = 0
    lead, lead_real = PM.random_cond_plan(rng, 37)
    subs.append(sub(np.concatenate([lead, plan]), lead_real + real))
    return subs


def test_w1_random_plans_at_the_chunk_and_ring_edges(hip):
    subs = edge_subs()
    assert any(0 in x["want"]["values"][61:] for x in subs[10:12]) and subs[9]["want"]["values"][255:] != [0] * 45
    for in_place in (False, True):
        assert_w1(run(hip, subs, in_place=in_place), subs, in_place)
    assert_w1(run(hip, subs, null_outputs=True), subs, "null", outputs=False)
    for x in subs[:3]:                                             # and each of the shortest alone
        assert_w1(run(hip, [x]), [x], "alone")


# ------------------------------------------------------------------------------------------------ block placement
def small_block(rng, w=4, h=4):
    c = H.random_block(rng, w, h, density=0.6, big=0.1)
    c[0, 0] = c[0, 0] or 3
    return (w, h, int(rng.integers(0, 2)), 0), c


def placement_subs(null_at=False):
    rng = np.random.default_rng(0xB10C + null_at)
    subs = []
    flags = [(CB, 0) for _ in range(12)]
    n = len(flags)
    real = [int(v) for v in rng.integers(0, 2, n)]

    def blocks(k, zero=()):
        m, b = zip(*[small_block(rng, *[(4, 4), (8, 8), (4, 8)][j % 3]) for j in range(k)])
        b = [np.zeros_like(x) if j in zero else x for j, x in enumerate(b)]
        return list(m), b
    if null_at:                                                    # every block behind the plan, guarded by the last elements
        m, b = blocks(3)
        subs.append(sub(flags, real, m, b, None, [gd(1, NE, 0), gd(2, EQ, 0), 0]))
        m, b = blocks(2)
        subs.append(sub(flags[:1], [1], m, b, None, None))
        return subs
    m, b = blocks(7)                                               # at 0 (unguarded: nothing in front), several at 5, at n
    subs.append(sub(flags, real, m, b, [0, 0, 5, 5, 5, n, n], [0, 0, gd(1, NE, 0), gd(2, NE, 0), gd(5, EQ, 0), gd(1, EQ, 0), gd(12, NE, 0)]))
    m, b = blocks(5)                                               # raw positions that need the clip: decreasing, beyond the plan
    subs.append(sub(flags, real, m, b, [7, 3, 9, 2, 1000], [gd(1, NE, 0), gd(7, NE, 0), 0, gd(3, EQ, 1), gd(4, NE, 0)]))
    m, b = blocks(4, zero=(1,))                                    # skipped: one with coefficients, one all zero; coded ones around
    real2 = list(real)
    real2[3], real2[4] = 0, 1
    subs.append(sub(flags, real2, m, b, [4, 4, 5, 5], [gd(1, NE, 0), gd(1, NE, 0), gd(1, NE, 0), gd(2, NE, 0)]))
    assert subs[-1]["want"]["coded"] == [False, False, True, False]
    m, b = blocks(17)                                              # which = 15 with 17 blocks walked: the 2nd of them
    plan = flags + [(bi(15, 0, 16), 0), (bi(0, 0, 16), 0), (bi(15, 18, 1), 0), (CB, gd(3, GE, 1))]
    subs.append(sub(plan, real + [0, 0, 0, 1], m, b, [1] * 2 + [6] * 10 + [12] * 5, [gd(1, NE, 0)] * 2 + [0] * 15))
    subs.append(sub(np.zeros((0, 2), np.uint32), []))              # an empty plan and no block ...
    lead, lead_real = PM.random_cond_plan(rng, 500)                # ... next to a long one
    m, b = blocks(2)
    subs.append(sub(lead, lead_real, m, b, [64, 500], None))
    subs.append(sub(np.zeros((0, 2), np.uint32), [], *blocks(2)))  # no plan, two blocks
    return subs


@pytest.mark.parametrize("null_at", [False, True], ids=["tu_at", "tu_at_null"])
def test_block_placement(hip, null_at):
    subs = placement_subs(null_at)
    for int16 in (False, True):
        assert_w1(run(hip, subs, int16=int16), subs, int16)
    if not null_at:
        x = subs[3]["want"]
        assert x["values"][12] == x["infos"][1] & 0xFFFF and x["values"][13] == x["infos"][16] & 0xFFFF


# ------------------------------------------------------------------------------------------------ W2
def test_w2_guard_free_plans_equal_binarise_and_splice(hip):
    """No guard, no block guard, no computed entry: the payload, offsets, results and info words of binarize_device's records of
    the same elements spliced with the blocks by encode_residual_device (the binariser's info word of a transform-skip block
    mapped to CABAC_TU_INFO_TS, as the header says)"""
    import torch
    rng = np.random.default_rng(0x2222)
    subs = []
    for n, nblk in ((40, 3), (0, 2), (130, 0), (70, 6), (1, 1)):
        plan, real = E.random_plan(rng, n, guard_frac=0.0, small=True)
        metas, blocks = [], []
        for j in range(nblk):
            m, b = small_block(rng, *[(4, 4), (8, 8)][j % 2])
            if j % 3 == 2:
                m = (m[0], m[1], m[2], H.TU_TRANSFORM_SKIP)
            metas.append(m)
            blocks.append(b)
        subs.append(sub(plan, real, metas, blocks, sorted(int(v) for v in rng.integers(0, n + 1, nblk)), None, qp=int(rng.integers(0, 64))))
    r = run(hip, subs)
    assert_w1(r, subs, "w2")
    P = r["P"]
    n_sub, n_tu = len(subs), P["n_tu"]
    # the binariser's records of the same elements, word1 = value
    se = P["plan"].copy()
    se[:, 1] = np.concatenate([x["values_in"] for x in subs])
    se_off = np.concatenate([[0], np.cumsum([len(x["plan"]) for x in subs])]).astype(np.uint64)
    t_se, t_seoff = dev(np.concatenate([se.reshape(-1), np.zeros(2, np.uint32)]).view(np.int32)), dev(se_off.view(np.int64))
    t_n = torch.zeros(n_sub, dtype=torch.int32, device="cuda")
    hip.binarize_device(n_sub, t_seoff.data_ptr(), t_se.data_ptr(), 0, t_n.data_ptr(), 0)
    hip.synchronize()
    n_rec = t_n.cpu().numpy().astype(np.int64)
    rec_off = np.concatenate([[0], np.cumsum(n_rec)]).astype(np.uint64)
    t_recoff = dev(rec_off.view(np.int64))
    t_rec = torch.zeros(int(rec_off[-1]) + 8, dtype=torch.int16, device="cuda")
    hip.binarize_device(n_sub, t_seoff.data_ptr(), t_se.data_ptr(), t_recoff.data_ptr(), t_n.data_ptr(), t_rec.data_ptr())
    # one splice per block at the record index of element at(t): the bins of the elements in front of it
    first_bin = [np.concatenate([[0], np.cumsum([len(E.records_of([E.op_of(w0, v)])) for (w0, _), v in zip(x["plan"], x["values_in"])])])
                 for x in subs]
    splices = np.zeros(max(n_tu, 1), capi.SPLICE_DTYPE)
    t = 0
    for s, x in enumerate(subs):
        for p in PM.positions(len(x["metas"]), x["at"], len(x["plan"])):
            splices[t] = (int(first_bin[s][p]), t)
            t += 1
    desc = P["desc"].copy()
    desc["rec_offset"], desc["n_records"] = rec_off[:-1], n_rec
    cap = int(r["offsets"][-1]) + 64
    t_pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    t_off = torch.zeros(n_sub + 1, dtype=torch.int64, device="cuda")
    t_res = torch.zeros(2 * n_sub, dtype=torch.int32, device="cuda")
    t_info = torch.zeros(max(n_tu, 1), dtype=torch.int32, device="cuda")
    coeff = np.concatenate([b.reshape(-1) for x in subs for b in x["blocks"]]).astype(np.int32)
    t_desc, t_first, t_sp, t_tu, t_co = dev(desc, np.uint8), dev(P["tile_first"].view(np.int32)), dev(splices, np.uint8), dev(P["tus"], np.uint8), dev(coeff)
    hip.encode_residual_device(n_sub, t_desc.data_ptr(), t_rec.data_ptr(), t_first.data_ptr(), t_sp.data_ptr(), n_tu, n_tu, t_tu.data_ptr(),
                               t_co.data_ptr(), t_pay.data_ptr(), cap, t_off.data_ptr(), t_res.data_ptr(), t_info.data_ptr())
    hip.synchronize()
    off, pay = t_off.cpu().numpy(), t_pay.cpu().numpy()
    assert np.array_equal(off, r["offsets"]) and np.array_equal(t_res.cpu().numpy().view(H.RESULT_DTYPE), r["res"])
    assert np.array_equal(pay[:int(off[-1])], np.concatenate(r["payload"]))
    info = t_info.cpu().numpy().view(np.uint32)[:n_tu]
    ts = np.array([bool(m[3] & H.TU_TRANSFORM_SKIP) for x in subs for m in x["metas"]])
    assert np.array_equal(np.where(ts, H.TU_INFO_TS, info), np.concatenate(r["infos"])) and ts.any() and not ts.all()


# ------------------------------------------------------------------------------------------------ W3
def test_w3_written_substreams_are_read_back_by_the_plan_parse(hip):
    """write_plan_device, then parse_plan_device on the same stream with no host synchronisation in between: byte ranges from the
    written offsets (a small kernel of torch's on the stream), the same plan, blocks, positions and guards"""
    import torch
    rng = np.random.default_rng(0x3333)
    subs = tu_subs(3)[:6] + tu_subs(1)[:5]
    for n in (65, 255, 300):                                       # and random plans with blocks, closed by the terminate bin
        plan, real = PM.random_cond_plan(rng, n)
        plan, real = PM.close(plan, real)
        (m0, b0), (m1, b1) = small_block(rng), small_block(rng, 8, 8)
        subs.append(sub(plan, real, [m0, m1], [b0, b1], [n // 3, n], [gd(1, NE, 0), 0], qp=int(rng.integers(0, 64))))
    units = [dict(plan=s["plan"], metas=s["metas"], blocks=s["blocks"], at=s["at"], guards=s["guards"], qp=s["qp"], finish=True,
                  data=np.zeros(0, np.uint8)) for s in subs]
    P = PM.pack(units)
    P["desc"]["init_id"] = W.SUB_FLAGS
    n_sub, n_tu, n_el = len(subs), P["n_tu"], len(P["plan"])
    coeff = np.concatenate([b.reshape(-1) for x in subs for b in x["blocks"]]).astype(np.int32)
    vin = np.concatenate([s["values_in"] for s in subs]).astype(np.uint32)
    cap = sum(len(s["want"]["data"]) for s in subs) + 64
    t_desc = torch.from_numpy(P["desc"].view(np.int64).reshape(n_sub, 4).copy()).cuda()        # rec_offset, byte_offset, (n, cap), (qp, id)
    t_first, t_tu = dev(P["tile_first"].view(np.int32)), dev(P["tus"], np.uint8)
    t_plan, t_vin, t_co = dev(P["plan"].reshape(-1).view(np.int32)), dev(vin.view(np.int32)), dev(coeff)
    t_at, t_gd = dev(P["tu_at"].view(np.int32)), dev(P["tu_guard"].view(np.int32))
    t_pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    t_off = torch.zeros(n_sub + 1, dtype=torch.int64, device="cuda")
    t_res = torch.zeros(2 * n_sub, dtype=torch.int32, device="cuda")
    t_val = torch.zeros(n_el, dtype=torch.int32, device="cuda")
    t_info = torch.zeros(n_tu, dtype=torch.int32, device="cuda")
    t_co2 = torch.full((len(coeff),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    t_val2 = torch.full((n_el,), -1, dtype=torch.int32, device="cuda")
    t_info2 = torch.full((n_tu,), -1, dtype=torch.int32, device="cuda")
    t_res2 = torch.full((2 * n_sub,), -1, dtype=torch.int32, device="cuda")
    args = (t_first.data_ptr(), n_tu, t_tu.data_ptr(), t_at.data_ptr(), t_gd.data_ptr(), t_co.data_ptr())
    hip.write_plan_device(n_sub, t_desc.data_ptr(), t_plan.data_ptr(), t_vin.data_ptr(), *args, t_pay.data_ptr(), cap, t_off.data_ptr(),
                          t_res.data_ptr(), t_val.data_ptr(), t_info.data_ptr())
    # the reader's descriptors on the device: the bytes are unaligned in the payload, so each substream is moved to a 16-aligned slot
    sizes = t_off[1:] - t_off[:-1]
    slot = ((sizes + 15) // 16) * 16 + 16
    begin = torch.cumsum(slot, 0) - slot
    t_desc2 = t_desc.clone()
    t_desc2[:, 1] = begin
    t_desc2[:, 2] = (t_desc[:, 2] & 0xFFFFFFFF) | (sizes << 32)
    t_desc2[:, 3] = (t_desc[:, 3] & 0xFFFFFFFF) | ((2 | H.SUB_FINISH) << 32)
    t_bytes = torch.zeros(cap + 32 * n_sub + 64, dtype=torch.uint8, device="cuda")
    idx = torch.arange(cap, device="cuda")
    owner = torch.clamp(torch.searchsorted(t_off, idx, right=True) - 1, 0, n_sub - 1)
    dest = torch.where(idx < t_off[-1], begin[owner] + idx - t_off[owner], torch.full_like(idx, len(t_bytes) - 1))   # the rest: a spare byte
    t_bytes[dest] = t_pay
    hip.parse_plan_device(n_sub, t_desc2.data_ptr(), t_bytes.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), t_at.data_ptr(),
                          t_gd.data_ptr(), t_plan.data_ptr(), t_co2.data_ptr(), t_val2.data_ptr(), t_res2.data_ptr(),
                          d_tu_info=t_info2.data_ptr())
    hip.synchronize()
    res, res2 = t_res.cpu().numpy().view(H.RESULT_DTYPE), t_res2.cpu().numpy().view(H.RESULT_DTYPE)
    assert not res["flags"].any() and not res2["flags"].any()
    assert np.array_equal(t_val.cpu().numpy(), t_val2.cpu().numpy()) and np.array_equal(t_info.cpu().numpy(), t_info2.cpu().numpy())
    assert np.array_equal(t_val.cpu().numpy().view(np.uint32), np.concatenate([np.array(x["want"]["values"], np.uint32) for x in subs]))
    co2, t = t_co2.cpu().numpy(), 0
    n_coded = 0
    for x in subs:
        for (w, h, *_), b, on in zip(x["metas"], x["blocks"], x["want"]["coded"]):
            got = co2[int(P["offsets"][t]): int(P["offsets"][t]) + w * h].reshape(h, w)
            if on:
                assert np.array_equal(got[:32, :32], b[:32, :32]), t
                n_coded += 1
            else:
                assert (got == 0x5A5A5A5A).all(), t
            t += 1
    assert n_coded > 10


# ------------------------------------------------------------------------------------------------ stops
def good_five():
    rng = np.random.default_rng(0x5707)
    subs = []
    for n in (30, 70, 24, 65, 10):
        plan, real = PM.random_cond_plan(rng, n)
        m, b = small_block(rng)
        subs.append(sub(plan, real, [m], [b], [n // 2], None, qp=int(rng.integers(0, 64))))
    return subs


def outside_cases():
    """(name, plan, real values, metas, blocks, at, guards, the stop): substream 2 of five"""
    flag = (CB, 0)
    cases = []
    kinds = [("ctx_bin", CB), ("trm", el(E.TRM)), ("ep_bins", el(E.EP_BINS, n=5)), ("unary_max", el(E.UNARY_MAX, ctx=1, ctx_n=2, max_symbol=4)),
             ("unary_ep", el(E.UNARY_EP, max_symbol=7)), ("trunc_bin", el(E.TRUNC_BIN, max_symbol=11)), ("exp_golomb", el(E.EXP_GOLOMB, count=3)),
             ("rem_abs", el(E.REM_ABS, rice=2, cutoff=5, max_log2=15)), ("ep_bins_0", el(E.EP_BINS, n=0))]
    for name, w0 in kinds:
        top = W.domain_top(w0)
        plan = [flag] * 70 + [(w0, gd(1, NE, 0))]                  # in the second chunk, active behind a flag of 1
        cases.append((name, plan, [1] * 70 + [top + 1], (), (), None, None, W.BAD_VALUE))
        cases.append((name + "_edge", plan, [1] * 70 + [top], (), (), None, None, 0))
        cases.append((name + "_skipped", plan, [0] * 70 + [top + 1], (), (), None, None, 0))
    meta, zero = (4, 4, 0, 0), np.zeros((4, 4), np.int32)
    cases.append(("coded_zero_block", [flag] * 5, [1] * 5, [meta], [zero], [3], [gd(1, NE, 0)], W.BAD_VALUE))
    cases.append(("skipped_zero_block", [flag] * 5, [1, 1, 0, 1, 1], [meta], [zero], [3], [gd(1, NE, 0)], 0))
    cases.append(("coded_zero_block_unguarded", [flag] * 5, [1] * 5, [meta], [zero], None, None, W.BAD_VALUE))
    for name, entry in (("kind_15", (15, gd(1, NE, 0))), ("ep_bins_33", (el(E.EP_BINS, n=33), gd(1, NE, 0))),
                        ("join_3", (capi.PE_COND | 3 << 12, gd(1, NE, 0))), ("which_beyond", (bi(1, 0, 16), gd(1, NE, 0))),
                        ("reserved_bits", (CB, gd(1, NE, 0) | 0x400)), ("back_beyond", (CB, gd(200, NE, 0)))):
        plan = [flag] * 66 + [entry] + [flag] * 2                   # a bad entry where its guard would skip it
        cases.append((name, plan, [0] * 69, [(4, 4, 0, 0)], [np.ones((4, 4), np.int32)], [2], None, W.BAD_RECORD))
    full = np.ones((4, 4), np.int32)
    cases.append(("bad_block_guard", [flag] * 5, [1] * 5, [meta], [full], [2], [gd(3, NE, 0)], W.BAD_RECORD))
    cases.append(("bad_block_guard_bits", [flag] * 5, [1] * 5, [meta], [full], [2], [0x8000], W.BAD_RECORD))
    cases.append(("bad_entry_behind_bad_value", [(el(E.EP_BINS, n=2), 0), (15, 0)], [9, 0], (), (), None, None, W.BAD_RECORD))
    return cases


def test_a_stop_codes_nothing_and_leaves_the_neighbours_alone(hip):
    """One substream in the middle of five is replaced case by case; its neighbours stay byte-identical to the run without it"""
    base = good_five()
    r0 = run(hip, base)
    assert_w1(r0, base, "base")
    seen = set()
    for name, plan, real, metas, blocks, at, guards, stop in outside_cases():
        x = sub(plan, real, metas, blocks, at, guards, qp=41, garbage=False)
        assert x["want"]["flag"] == stop, name
        subs = base[:2] + [x] + base[3:]
        r = run(hip, subs, in_place=name.endswith("_edge"))
        assert_w1(r, subs, name)
        if stop:
            assert len(r["payload"][2]) == 0 and (int(r["res"]["n_bits"][2]), int(r["res"]["flags"][2])) == (0, stop), name
        for s in (0, 1, 3, 4):
            assert np.array_equal(r["payload"][s], r0["payload"][s]) and tuple(r["res"][s]) == tuple(r0["res"][s]), (name, s)
            assert np.array_equal(r["values"][s], r0["values"][s]) and np.array_equal(r["infos"][s], r0["infos"][s]), (name, s)
        seen.add(stop)
    assert seen == {0, W.BAD_VALUE, W.BAD_RECORD}


# ------------------------------------------------------------------------------------------------ the batch form
def batch_args(subs, int16=False):
    units = [dict(plan=s["plan"], metas=s["metas"], blocks=s["blocks"], at=s["at"], guards=s["guards"], qp=s["qp"], finish=True,
                  data=np.zeros(0, np.uint8)) for s in subs]
    P = PM.pack(units)
    P["desc"]["init_id"] = W.SUB_FLAGS
    coeff = np.concatenate([b.reshape(-1) for x in subs for b in x["blocks"]] + [np.zeros(0, np.int32)]).astype(np.int16 if int16 else np.int32)
    vin = np.concatenate([s["values_in"] for s in subs] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return P, dict(desc=P["desc"], plan=P["plan"], values=vin, tile_first=P["tile_first"], tus=P["tus"][:P["n_tu"]], tu_at=P["tu_at"],
                   tu_guard=P["tu_guard"], coeff=coeff)


def test_batch_form_returns_the_same_and_refuses_what_the_header_lists():
    place = placement_subs()
    subs = tu_subs(3)[:5] + [place[0], place[2], place[3]]         # (not place[1]: its raw positions decrease, which this form refuses)
    hip = capi.CabacHip(0)
    try:
        for int16 in (False, True):
            P, a = batch_args(subs, int16)
            payload = np.full(sum(len(x["want"]["data"]) for x in subs) + 32, BYTE_GUARD, np.uint8)
            pay, off, res, values, info = hip.write_plan_batch(payload=payload, **a)
            assert np.array_equal(pay, np.concatenate([x["want"]["data"] for x in subs])) and (payload[len(pay):] == BYTE_GUARD).all()
            assert off.tolist() == np.concatenate([[0], np.cumsum([len(x["want"]["data"]) for x in subs])]).tolist()
            assert res["n_bits"].tolist() == [x["want"]["n_bits"] for x in subs] and not res["flags"].any()
            assert values.tolist() == [v for x in subs for v in x["want"]["values"]]
            assert info.tolist() == [v for x in subs for v in x["want"]["infos"]]
        P, a = batch_args(subs)

        def refused(**change):
            b = dict(a, **change)
            payload = np.full(1 << 16, BYTE_GUARD, np.uint8)
            values_out = np.full(len(b["plan"]) + 1, 0xEEEEEEEE, np.uint32)
            info = np.full(len(b["tus"]) + 1, 0xEEEEEEEE, np.uint32)
            with pytest.raises(capi.CabacHipError) as e:
                hip.write_plan_batch(payload=payload, values_out=values_out, info=info, **b)
            assert e.value.status == -2, change.keys()
            assert (payload == BYTE_GUARD).all() and (values_out == 0xEEEEEEEE).all() and (info == 0xEEEEEEEE).all()

        def changed(name, idx, value):
            c = a[name].copy()
            c[idx] = value
            return {name: c}
        plan = a["plan"].copy()
        plan[30, 0] = 15
        refused(plan=plan)                                          # a bad plan entry
        plan = a["plan"].copy()
        plan[2, 1] = gd(9, NE, 0)
        refused(plan=plan)                                          # a guard that reaches in front of the plan
        refused(**changed("tu_guard", 0, 0x400))                    # a bad block guard
        refused(**changed("tu_guard", 0, gd(200, NE, 0)))
        refused(**changed("tile_first", 1, int(a["tile_first"][2]) + 1))            # tile_first decreases
        refused(**changed("tu_at", 1, int(a["tu_at"][0]) - 1))      # tu_at decreases inside a substream
        refused(**changed("tu_at", 2, 10_000))                      # ... exceeds its plan length
        tus = a["tus"].copy()
        tus["coeff_offset"][1] = len(a["coeff"])
        refused(tus=tus)                                            # coefficients out of range (of a block, coded or not)
        desc = a["desc"].copy()
        desc["init_id"][0] = 3 | H.SUB_FINISH
        refused(desc=desc)
        desc = a["desc"].copy()
        desc["n_records"][-1] += 1
        refused(desc=desc)                                          # a plan that leaves n_elements_total
        # a flag: CABAC_HIP_ERR_SUBSTREAM, the other substreams as before
        vin = a["values"].copy()
        vin[0] = 2                                                  # tu_cbf_cb, a context bin
        payload = np.full(1 << 16, BYTE_GUARD, np.uint8)
        with pytest.raises(capi.CabacHipError) as e:
            hip.write_plan_batch(payload=payload, **dict(a, values=vin))
        assert e.value.status == -5
        pay, off, res, values, info = hip.write_plan_batch(payload=payload, check=False, **dict(a, values=vin))
        assert (int(res["n_bits"][0]), int(res["flags"][0])) == (0, W.BAD_VALUE) and off[1] == 0 and not res["flags"][1:].any()
        assert np.array_equal(pay, np.concatenate([x["want"]["data"] for x in subs[1:]]))
    finally:
        hip.close()
