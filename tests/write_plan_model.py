"""CPU model of include/cabac_hip_write_plan.h: the plan write is parse_plan_model's writer's side (fill / expand / build, which
stay what they are) plus what the header adds — the domain of every element kind, the two stops and their precedence, and the
outputs of a stopped substream.  Everything that touches bins is the oracle's.

write(rng-free) -> dict(flag, values, infos, coded, data, n_bits): what one substream of cabac_hip_write_plan_device must give."""
import numpy as np

import helpers as H
import parse_elements_model as E
import parse_plan_model as PM

BAD_RECORD, BAD_VALUE = H.RES_BAD_RECORD, E.RES_BAD_VALUE
SUB_FLAGS = 2 | H.SUB_FINISH | H.SUB_ALIGN_RBSP                   # init_id of a written substream: I slice tables, finish(), RBSP


def domain_top(w0):
    """The largest value an element of this word0 carries (the element is not a bad entry); -1: none at all; None: any (ALIGN)"""
    kind, f = E.fields(w0)
    if kind in (E.CTX_BIN, E.TRM):
        return 1
    if kind == E.EP_BINS:
        return (1 << f["n"]) - 1
    if kind in (E.UNARY_MAX, E.UNARY_EP):
        return f["max_symbol"]
    if kind == E.TRUNC_BIN:
        return f["max_symbol"] - 1
    if kind == E.REM_ABS:                                          # the longest prefix and a suffix of ones
        return (((1 << (32 - f["max_log2"] - f["cutoff"])) + f["cutoff"] - 1) << f["rice"]) + (1 << f["max_log2"]) - 1
    if kind == E.EXP_GOLOMB:                                       # count + prefix ones < 32
        return (1 << 32) - (1 << f["count"]) - 1
    assert kind == E.ALIGN
    return None


def in_domain(w0, value):
    top = domain_top(w0)
    return top is None or 0 <= int(value) <= min(top, 0xFFFFFFFF)


def block_unwritable(meta, coeff):
    """A block the binariser gives no records for: CABAC_TU_INFO_EMPTY (its coded region holds no level) or _BAD_DESC"""
    w, h, ch, fl = meta[:4]
    ml = meta[4] if len(meta) > 4 and meta[4] else 15
    if w > 64 or h > 64 or ch > 1 or ml > 20 or ((fl & H.TU_TRANSFORM_SKIP) and (w > 32 or h > 32)):
        return True
    return not np.asarray(coeff)[:32, :32].any()


def stop_of(plan, real_values, metas=(), blocks=(), at=None, guards=None):
    """0, BAD_RECORD or BAD_VALUE: a bad entry or block guard anywhere wins, whatever the values say; else the first active
    element outside its domain or coded block without records"""
    plan = np.asarray(plan, np.uint32).reshape(-1, 2)
    n = len(plan)
    pos = PM.positions(len(metas), at, n)
    nb = PM.nb_of(pos, n)
    if any(PM.is_bad_entry(w0, w1, i, nb[i]) for i, (w0, w1) in enumerate(plan)):
        return BAD_RECORD
    if guards is not None and any(E.is_bad_guard(g, pos[t]) for t, g in enumerate(guards)):
        return BAD_RECORD
    values, infos, t = [], [], 0
    for i in range(n + 1):
        while t < len(metas) and pos[t] == i:
            on = guards is None or E.guard_holds(guards[t], values, i)
            if on and block_unwritable(metas[t], blocks[t]):
                return BAD_VALUE
            infos.append(PM.info_of(metas[t], blocks[t]) if on else PM.NOT_CODED)
            t += 1
        if i < n:
            w0, w1 = plan[i]
            if PM.is_computed(w0):
                values.append(PM.computed_value(w0, w1, values, i, infos))
            elif E.guard_holds(w1, values, i):
                if not in_domain(w0, real_values[i]):
                    return BAD_VALUE
                values.append(int(real_values[i]))
            else:
                values.append(0)
    return 0


def write(plan, real_values, metas=(), blocks=(), at=None, guards=None, qp=30):
    """One substream of the plan write -> dict(flag, values, infos, coded, data, n_bits).  A stop codes nothing."""
    plan = np.asarray(plan, np.uint32).reshape(-1, 2)
    flag = stop_of(plan, real_values, metas, blocks, at, guards)
    if flag:
        return dict(flag=flag, values=None, infos=None, coded=None, data=np.zeros(0, np.uint8), n_bits=0)
    values, infos, coded, _ = PM.fill(plan, real_values, metas, blocks, at, guards)
    string = PM.expand(plan, values, list(metas), list(blocks), at, guards)[0]
    data, n_bits = H.load_oracle().encode_records(string, int(qp), 2, 3)
    return dict(flag=0, values=[v & 0xFFFFFFFF for v in values], infos=infos, coded=coded, data=data, n_bits=n_bits)


def edge_values(w0):
    """Values at and around the edges of an element's domain, each with whether it is inside"""
    top = domain_top(w0)
    if top is None:
        return [(0, True), (7, True), (0xFFFFFFFF, True)]
    cand = {0, 1, top - 1, top, top + 1, top + 2, 0xFFFFFFFF, top // 2}
    return [(v, v <= top) for v in sorted(c for c in cand if 0 <= c <= 0xFFFFFFFF)]
