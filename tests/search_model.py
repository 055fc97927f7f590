"""Plain-Python model of include/cabac_hip_search.h: the set a candidate leaves, the cost, the pick and one round.

Composed of parts that are pinned elsewhere: orc.residual_records (tests/test_residual_oracle.py) and orc.estimate_records_from
(tests/test_estimator_oracle.py, tests/test_residual_estimate_oracle.py), with advance() / block_records() of
tests/test_gpu_residual_estimate.py; tests/test_search_model.py pins the contexts this model carries from round to round to
the compiled reference.  Costs are Python integers, so the 128-bit product and the saturation are exact by construction."""
import numpy as np

import helpers as H
from test_gpu_residual_estimate import advance, block_records

NONE = NO_SET = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1
COST_MAX = (1 << 64) - 2


def cost_of(frac_bits, dist, lambda_q16):
    """dist + floor(lambda_q16 * frac_bits / 2^31), saturating at 2^64 - 2."""
    return min(int(dist) + ((int(lambda_q16) * int(frac_bits)) >> 31), COST_MAX)


def select(group_first, frac_bits, dist, lambda_q16, n_cand_max=None):
    """(pick uint32[n_group], cost uint64[n_group]); dist None = all zeros; dist == 2^64 - 1 excludes a candidate; runs are
    clipped to group_first[-1] (and to n_cand_max) and a run that goes backwards is empty, as the device clips them."""
    n_group = len(group_first) - 1
    n = int(group_first[n_group])
    if n_cand_max is not None:
        n = min(n, int(n_cand_max))
    pick = np.full(n_group, NONE, np.uint32)
    cost = np.full(n_group, U64_MAX, np.uint64)
    for g in range(n_group):
        first = min(int(group_first[g]), n)
        end = max(min(int(group_first[g + 1]), n), first)
        best, best_c = None, NONE
        for c in range(first, end):
            d = 0 if dist is None else int(dist[c])
            if d == U64_MAX:
                continue
            v = cost_of(frac_bits[c], d, lambda_q16)
            if best is None or v < best:
                best, best_c = v, c
        if best is not None:
            pick[g], cost[g] = best_c, best
    return pick, cost


def walk_candidate(blocks, tus, first, end, start):
    """One candidate = blocks [first, end) from the set `start` = (s0, s1, rate).
    -> (bits, {t: share}, {t: info}, the set it leaves (s0 uint16, s1 uint16, rate), its records back to back)"""
    orc = H.load_oracle()
    s0, s1, rate = start[0].astype(np.int64), start[1].astype(np.int64), start[2]
    total, shares, infos, recs = 0, {}, {}, []
    for t in range(first, end):
        rec, info = block_records(blocks, tus, t)
        infos[t] = info
        shares[t] = 0
        if rec is None:            # empty block / bad descriptor: costs 0, leaves the contexts alone
            continue
        rc, bits = orc.estimate_records_from(rec, s0.astype(np.uint16), s1.astype(np.uint16), rate)
        assert rc == 0
        shares[t] = bits
        total += bits
        advance(s0, s1, rate, rec)
        recs.append(rec)
    left = (s0.astype(np.uint16), s1.astype(np.uint16), rate.copy())
    return total, shares, infos, left, (np.concatenate(recs) if recs else np.zeros(0, np.uint16))


def export_model(cand_first, blocks, tus, sets, which, out_set):
    """cabac_hip_estimate_residual_ctx_device: (cand_bits, tu_bits, tu_info, {out set: (s0, s1, rate)})"""
    n_cand = len(cand_first) - 1
    cand_bits = np.zeros(n_cand, np.uint64)
    tu_bits = np.zeros(len(tus), np.uint64)
    tu_info = np.zeros(len(tus), np.uint32)
    written = {}
    for c in range(n_cand):
        bits, shares, infos, left, _ = walk_candidate(blocks, tus, int(cand_first[c]), int(cand_first[c + 1]), sets[int(which[c])])
        cand_bits[c] = bits
        for t, v in shares.items():
            tu_bits[t] = v
        for t, v in infos.items():
            tu_info[t] = v
        if int(out_set[c]) != NO_SET:
            written[int(out_set[c])] = left
    return cand_bits, tu_bits, tu_info, written


def round_model(group_first, cand_first, blocks, tus, sets, which, group_out_set, dist, lambda_q16):
    """cabac_hip_search_round_device on a list of sets [(s0, s1, rate)]: estimate every candidate from its start set, select per
    group, commit the picked candidates' sets.  -> (cand_bits, pick, cost, new list of sets, tu_bits, tu_info, records of
    every candidate)"""
    n_cand = len(cand_first) - 1
    cand_bits = np.zeros(n_cand, np.uint64)
    tu_bits = np.zeros(len(tus), np.uint64)
    tu_info = np.zeros(len(tus), np.uint32)
    left, recs = [], []
    for c in range(n_cand):
        bits, shares, infos, l, r = walk_candidate(blocks, tus, int(cand_first[c]), int(cand_first[c + 1]), sets[int(which[c])])
        cand_bits[c] = bits
        for t, v in shares.items():
            tu_bits[t] = v
        for t, v in infos.items():
            tu_info[t] = v
        left.append(l)
        recs.append(r)
    pick, cost = select(group_first, cand_bits, dist, lambda_q16, n_cand_max=n_cand)
    new_sets = list(sets)
    if group_out_set is not None:
        for g in range(len(group_first) - 1):
            if int(group_out_set[g]) != NO_SET and int(pick[g]) != NONE:
                new_sets[int(group_out_set[g])] = left[int(pick[g])]
    return cand_bits, pick, cost, new_sets, tu_bits, tu_info, recs
