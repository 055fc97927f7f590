"""CPU model of include/cabac_hip_search_plan.h, by composition and with no arithmetic of its own: a candidate is a plan, the
values of its real elements and its blocks; its RESOLVED FORM is parse_plan_model.fill / expand's walk cut into side records,
block positions in record units and coded / skipped; the stops are write_plan_model.stop_of; costs, picks and sets are
search_unit_model.estimate_model / select over the resolved form.

A candidate is a dict(plan (n, 2) uint32, values [the real values, one per entry], metas [(w, h, channel, flags[, max_log2])],
blocks [2-D arrays], at [one raw position per block, in plan entries] or None, guards [one guard word per block] or None)."""
import numpy as np

import helpers as H
import parse_elements_model as E
import parse_plan_model as PM
import search_unit_model as U
import write_plan_model as W

BAD_RECORD, BAD_VALUE, OVERFLOW = W.BAD_RECORD, W.BAD_VALUE, 1
NONE, NO_SET, U64_MAX = U.NONE, U.NO_SET, U.U64_MAX
REJECTED = 7                                                       # log2_width = log2_height of a block that is not coded


def cand(plan, values, metas=(), blocks=(), at=None, guards=None):
    plan = np.asarray(plan, np.uint32).reshape(-1, 2)
    return dict(plan=plan, values=[int(v) for v in values], metas=list(metas), blocks=[np.asarray(b, np.int32) for b in blocks],
                at=None if at is None else list(at), guards=None if guards is None else list(guards))


def bin_bound(w0):
    """The header's table: the most bins a value in its domain makes of an entry with this word0 (the entry is not bad)"""
    kind, f = PM.fields(w0)
    if kind in (E.CTX_BIN, E.TRM, E.ALIGN):
        return 1
    if kind == E.EP_BINS:
        return f["n"]
    if kind in (E.UNARY_MAX, E.UNARY_EP):
        return f["max_symbol"]
    if kind == E.TRUNC_BIN:
        return f["max_symbol"].bit_length()                        # floor(log2(maxSymbol)) + 1
    if kind == E.EXP_GOLOMB:
        return 63 - f["count"]
    if kind == E.REM_ABS:
        return max(32, f["cutoff"] + f["rice"] + max(0, 2 * (32 - f["cutoff"] - f["max_log2"]) - 1))
    assert kind in (PM.COND, PM.BLOCK_INFO)
    return 0


def resolve(c):
    """One candidate -> dict(flag, records, at_out [per block, in records], coded [per block], values, infos, active [per entry:
    it has records]); a stopped one has an empty run, every block skipped at 0 and values / infos / active None (unspecified)"""
    n_blk = len(c["metas"])
    flag = W.stop_of(c["plan"], c["values"], c["metas"], c["blocks"], c["at"], c["guards"])
    if flag:
        return dict(flag=flag, records=np.zeros(0, np.uint16), at_out=[0] * n_blk, coded=[False] * n_blk, values=None, infos=None,
                    active=None)
    values, infos, coded, active = PM.fill(c["plan"], c["values"], c["metas"], c["blocks"], c["at"], c["guards"])
    n = len(c["plan"])
    pos = PM.positions(n_blk, c["at"], n)
    parts, in_front = [], [0]                                      # in_front[i]: side records of the entries in front of entry i
    for i in range(n):
        rec = E.records_of([E.op_of(c["plan"][i, 0], values[i])]) if active[i] else np.zeros(0, np.uint16)
        parts.append(rec)
        in_front.append(in_front[-1] + len(rec))
    records = np.concatenate(parts + [np.zeros(0, np.uint16)]).astype(np.uint16)
    return dict(flag=0, records=records, at_out=[in_front[p] for p in pos], coded=list(coded), values=[v & 0xFFFFFFFF for v in values],
                infos=list(infos), active=list(active))


def spliced(c, r):
    """The resolved form with the coded blocks' records spliced in at the resolved positions: search_unit_model's expanded string"""
    recs = [H.load_oracle().residual_records(np.ascontiguousarray(b, np.int32), m[2], m[3],
                                             max_log2_range=m[4] if len(m) > 4 and m[4] else 15)[0] if on else None
            for m, b, on in zip(c["metas"], c["blocks"], r["coded"])]
    return U.expand(r["records"], r["at_out"], recs)[0]


def pack(cands, gap=0):
    """The host arrays of a call -> dict(cand_first, ent_first, plan, values, tus, tu_at, tu_guard, coeff, blocks, n_tu); gap:
    coefficients left unused between two blocks"""
    metas = [m for c in cands for m in c["metas"]]
    blocks = [b for c in cands for b in c["blocks"]]
    tus = np.zeros(len(metas), H.TU_DTYPE)
    off = 0
    for t, m in enumerate(metas):
        w, h, ch, fl = m[:4]
        tus[t]["coeff_offset"], tus[t]["log2_width"], tus[t]["log2_height"] = off, int(np.log2(w)), int(np.log2(h))
        tus[t]["channel"], tus[t]["flags"], tus[t]["max_log2_tr_range"] = ch, fl, m[4] if len(m) > 4 else 0
        off += w * h + gap
    coeff = np.zeros(off, np.int32)
    for t, b in enumerate(blocks):
        coeff[int(tus[t]["coeff_offset"]): int(tus[t]["coeff_offset"]) + b.size] = b.reshape(-1)
    tu_at = tu_guard = None
    if any(c["at"] is not None for c in cands):
        tu_at = np.array([a for c in cands for a in (c["at"] if c["at"] is not None else [len(c["plan"])] * len(c["metas"]))], np.uint32)
    if any(c["guards"] is not None for c in cands):
        tu_guard = np.array([g for c in cands for g in (c["guards"] if c["guards"] is not None else [0] * len(c["metas"]))], np.uint32)
    return dict(cand_first=np.concatenate([[0], np.cumsum([len(c["metas"]) for c in cands])]).astype(np.uint32),
                ent_first=np.concatenate([[0], np.cumsum([len(c["plan"]) for c in cands])]).astype(np.uint64),
                plan=np.concatenate([c["plan"] for c in cands] + [np.zeros((0, 2), np.uint32)]).astype(np.uint32),
                values=np.array([v & 0xFFFFFFFF for c in cands for v in c["values"]], np.uint64).astype(np.uint32),
                tus=tus, tu_at=tu_at, tu_guard=tu_guard, coeff=coeff, blocks=blocks, n_tu=len(metas))


def resolve_all(cands, P=None, capacity=None):
    """cabac_hip_resolve_plan_device -> dict(rec_first, records, tu_at_out, tus_out, values [per candidate or None], infos [per
    candidate or None], flags, total, coded [per block], active [per candidate or None]); capacity None: whatever it needs"""
    P = pack(cands) if P is None else P
    R = [resolve(c) for c in cands]
    total = sum(len(r["records"]) for r in R)
    if capacity is not None and total > capacity:                  # all or nothing
        R = [dict(r, flag=r["flag"] or OVERFLOW, records=np.zeros(0, np.uint16), at_out=[0] * len(r["at_out"]),
                  coded=[False] * len(r["coded"]), values=None, infos=None) for r in R]
    tus_out = P["tus"].copy()
    coded = np.array([on for r in R for on in r["coded"]], bool)
    tus_out["log2_width"][~coded] = REJECTED
    tus_out["log2_height"][~coded] = REJECTED
    return dict(rec_first=np.concatenate([[0], np.cumsum([len(r["records"]) for r in R])]).astype(np.uint64),
                records=np.concatenate([r["records"] for r in R] + [np.zeros(0, np.uint16)]).astype(np.uint16),
                tu_at_out=np.array([a for r in R for a in r["at_out"]], np.uint32), tus_out=tus_out,
                values=[r["values"] for r in R], infos=[r["infos"] for r in R], flags=np.array([r["flag"] for r in R], np.uint32),
                total=total, coded=coded, active=[r["active"] for r in R])


def round_model(cands, group_first, sets, which, group_out_set, dist, lambda_q16, P=None, capacity=None):
    """cabac_hip_search_plan_round_device on a list of sets -> dict(bits, pick, cost, sets [new list; None where the picked
    candidate is flagged: unspecified], tu_bits, flags, resolved [resolve_all's dict], strings)"""
    P = pack(cands) if P is None else P
    R = resolve_all(cands, P, capacity)
    n_cand = len(cands)
    bits, tu_bits, _, est_flags, _, left, strings = U.estimate_model(P["cand_first"], P["blocks"], R["tus_out"], sets, which, R["rec_first"],
                                                                     R["records"], R["tu_at_out"])
    assert not est_flags.any()                                     # the binariser's records are never bad ones
    bits = bits.copy()
    bits[R["flags"] != 0] = U64_MAX
    pick, cost = U.select(group_first, bits, dist, lambda_q16, n_cand_max=n_cand)
    new_sets = list(sets)
    if group_out_set is not None:
        for g in range(len(group_first) - 1):
            if int(group_out_set[g]) != NO_SET and int(pick[g]) != NONE:
                new_sets[int(group_out_set[g])] = None if R["flags"][int(pick[g])] else left[int(pick[g])]
    return dict(bits=bits, pick=pick, cost=cost, sets=new_sets, tu_bits=tu_bits, flags=R["flags"], resolved=R, strings=strings)
