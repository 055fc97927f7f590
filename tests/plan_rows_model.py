"""CPU model of include/cabac_hip_plan_rows.h, composed from what exists: parse_plan_model.fill / expand give a row's filled
values and its record string, ctx_sets_model.encode_from / decode_from / advance_from give bytes, bins and contexts from a start
set, and the level loop follows ctx_sets_model.wpp_starts.  What this module adds is the hand-over point: the record index of
plan entry k is the length of the string of the first k entries with the blocks of position <= k.

A row is a dict(plan, real, metas, blocks, at, guards, qp): the writer's input of one substream (parse_plan_model.tu_case's
tuple, several in a row, closed by the terminate bin).  A context set is ctx_sets_model's triple (s0, s1, rate)."""
import numpy as np

import ctx_sets_model as CS
import helpers as H
import parse_elements_model as E
import parse_plan_model as PM

NO_SET = CS.NO_SET
RES_BAD_SET = CS.RES_BAD_SET
ENC_FLAGS = 3                                                      # finish() and the RBSP alignment, as the plan write codes


def make_row(plan, real, metas=(), blocks=(), at=None, guards=None, qp=30):
    return dict(plan=np.asarray(plan, np.uint32).reshape(-1, 2), real=list(real), metas=list(metas),
                blocks=[np.clip(np.asarray(b, np.int32), -32767, 32767) for b in blocks], at=None if at is None else list(at),
                guards=None if guards is None else list(guards), qp=int(qp))


def tu_row(rng, outcomes, qp=None, marker=False):
    """Transform units in a row in one substream (parse_plan_model.tu_unit's input), closed by the terminate bin.  marker: a
    zero-bin EP_BINS entry in front of every unit but the first, as a CTU that begins with a block is separated from its
    predecessor — the units here begin with entries, so the marker only shifts them; tests put blocks behind it themselves."""
    plans, real, metas, blocks, at, guards, base = [], [], [], [], [], [], 0
    for k, o in enumerate(outcomes):
        p, v, m, b, a, g = PM.tu_case(rng, *o)
        if marker and k:
            plans.append(np.array([[PM.el(E.EP_BINS, n=0), 0]], np.uint32))
            real.append(0)
            base += 1
        plans.append(p)
        real += v
        metas += m
        blocks += b
        at += [x + base for x in a]
        guards += g
        base += len(p)
    plan, real = E.close(np.concatenate(plans), real)
    return make_row(plan, real, metas, blocks, at, guards, int(rng.integers(0, 64)) if qp is None else qp)


def filled(row):
    """-> (values, infos, coded, string): the walk on the writer's side and the row's expanded record string"""
    values, infos, coded, _ = PM.fill(row["plan"], row["real"], row["metas"], row["blocks"], row["at"], row["guards"])
    string = PM.expand(row["plan"], values, row["metas"], row["blocks"], row["at"], row["guards"])[0]
    return values, infos, coded, string


def handover_index(row, values, k):
    """The index into the row's record string that corresponds to plan entry k, clipped to the plan: the records of entries
    0 .. k - 1 and of every coded block with clipped position <= k."""
    n = len(row["plan"])
    k = min(int(k), n)
    pos = PM.positions(len(row["metas"]), row["at"], n)
    m = sum(1 for p in pos if p <= k)
    head = PM.expand(row["plan"][:k], values, row["metas"][:m], row["blocks"][:m], None if row["at"] is None else row["at"][:m],
                     None if row["guards"] is None else row["guards"][:m])[0]
    return len(head)


def start_of(row, sets, start):
    if start is None or int(start) == NO_SET:
        return CS.init_set(row["qp"], 2)
    return sets[int(start)]


def write_row(row, ctx, k=None):
    """One row coded from the contexts `ctx` -> dict(values, infos, coded, string, data, n_bits, at_rec, handed): at_rec the
    hand-over record index of entry k (None: the end), handed the hand-over contexts, left the contexts behind the last record"""
    values, infos, coded, string = filled(row)
    n, data, n_bits, left = CS.encode_from(string, ctx, ENC_FLAGS)
    assert n >= 0
    at_rec = handover_index(row, values, len(row["plan"]) if k is None else k)
    return dict(values=[v & 0xFFFFFFFF for v in values], infos=infos, coded=coded, string=string, data=data, n_bits=n_bits,
                at_rec=at_rec, handed=CS.advance_from(string[:at_rec], ctx), left=left, start=ctx)


def read_row(row, w, data=None):
    """What the parser must report for the row written as `w` when it reads `data` (default: w's own bytes) from w's start
    contexts: (n_bits, flags).  The bins must be the string's own."""
    rc, bins, nread, left = CS.decode_from(w["string"], w["start"], w["data"] if data is None else data, 1)
    assert rc in (0, -5) and np.array_equal(bins, w["string"] >> 15)
    return nread, {0: 0, -5: H.RES_BAD_STOP}[rc], left


def rows(rows_, level_first, sync_from, sync_at):
    """The level loop of ctx_sets_model.wpp_starts over plan rows -> [write_row's dict, or None for a refused row or one linked
    to a refused row], ok: row s codes from the hand-over contexts of row sync_from[s] at plan entry sync_at[sync_from[s]]"""
    n = len(rows_)
    out, ok = [None] * n, [False] * n
    for l in range(len(level_first) - 1):
        first = int(level_first[l])
        for s in range(first, int(level_first[l + 1])):
            f = int(sync_from[s])
            if f == NO_SET:
                ctx = CS.init_set(rows_[s]["qp"], 2)
            elif f < first and out[f] is not None:
                ctx = out[f]["handed"]
            else:
                ok[s] = f < first                                  # linked to a refused row: unspecified, not refused itself
                continue
            ok[s] = True
            out[s] = write_row(rows_[s], ctx, int(sync_at[s]))
    return out, ok


def batch(seed, n_pic=3, n_row=4, sync_ats=(0, PM.TU_LEN, None, 10 ** 6), unlinked_row=(1, 2), outcomes=None):
    """n_pic pictures x n_row ragged rows of one to three transform units in LEVEL ORDER, linked as ctx_sets_model.wpp_batch links
    them -> (rows, level_first, sync_from, sync_at); sync_at in plan entries, None: exactly the plan's length."""
    from test_parse_plan_model import TU_OUTCOMES
    rng = np.random.default_rng(seed)
    outcomes = TU_OUTCOMES if outcomes is None else outcomes
    n_sub = n_pic * n_row
    rows_ = []
    for s in range(n_sub):
        units = 3 if s == 0 else int(rng.integers(1, 4))
        rows_.append(tu_row(rng, [outcomes[int(rng.integers(0, len(outcomes)))] for _ in range(units)]))
    level_first = np.arange(0, n_sub + 1, n_pic, dtype=np.uint32)
    sync_from = np.full(n_sub, NO_SET, np.uint32)
    sync_at = np.zeros(n_sub, np.uint32)
    for r in range(n_row):
        for p in range(n_pic):
            s = r * n_pic + p
            if r > 0 and (p, r) != tuple(unlinked_row):
                sync_from[s] = (r - 1) * n_pic + p
            at = sync_ats[s % len(sync_ats)]
            sync_at[s] = len(rows_[s]["plan"]) if at is None else at
    return rows_, level_first, sync_from, sync_at


def pack(rows_, written=None):
    """parse_plan_model.pack of the rows (bytes: the written rows' where given) plus coeff: the blocks' coefficients int32"""
    units = [dict(plan=r["plan"], metas=r["metas"], blocks=r["blocks"], at=r["at"], guards=r["guards"], qp=r["qp"], finish=True,
                  data=np.zeros(0, np.uint8) if written is None or written[s] is None else written[s]["data"])
             for s, r in enumerate(rows_)]
    P = PM.pack(units)
    coeff = np.zeros(max(P["total"], 1), np.int32)
    t = 0
    for r in rows_:
        for b in r["blocks"]:
            coeff[int(P["offsets"][t]): int(P["offsets"][t]) + b.size] = b.reshape(-1)
            t += 1
    P["coeff"] = coeff
    P["values_in"] = np.array([int(v) & 0xFFFFFFFF for r in rows_ for v in r["real"]], np.uint64).astype(np.uint32)
    return P
