"""Plain-Python model of include/cabac_hip_search_unit.h: a candidate is a run of side records with blocks spliced in.

expand() builds the expanded string of the header's definition; the cost is orc.estimate_records_from of the whole string, the
set left is advance() over it, and a block's share is the cost of its own records from the contexts the string has reached in
front of them (a bin's cost depends on nothing but its context, so that is the sum of the block's bin costs within the
string).  Composed of parts pinned elsewhere (tests/search_model.py, tests/test_gpu_residual_estimate.py);
tests/test_search_unit_model.py pins the whole to the compiled reference."""
import numpy as np

import helpers as H
from search_model import NONE, NO_SET, U64_MAX, cost_of, select            # noqa: F401  (re-exported)
from test_gpu_residual_estimate import advance, block_records

REC_ALIGN, REC_EP, REC_TRM = 0x1FD, 0x1FE, 0x1FF
BAD_RECORD = 2                                                            # CABAC_RES_BAD_RECORD


def clip_run(rec_first, c):
    """(first, n) of candidate c's side run: clipped to rec_first[-1]; a run that goes backwards is empty."""
    n_all = int(rec_first[len(rec_first) - 1])
    first = min(int(rec_first[c]), n_all)
    end = max(min(int(rec_first[c + 1]), n_all), first)
    return first, min(end - first, 0xFFFFFFFF)


def positions(at, n_rec):
    """Effective positions: at(t) = min(max(at[t], at(t - 1)), n_rec), 0 in front of the first block; at None: all behind."""
    out, prev = [], 0
    for a in at:
        prev = n_rec if a is None else min(max(int(a), prev), n_rec)
        out.append(prev)
    return out


def expand(side, at, block_recs):
    """side: uint16 records; at: one raw position per block (None: behind the run); block_recs: the blocks' records (None for an
    empty block / a bad descriptor).  -> (the expanded string, [(start, end) of every block's records in it])"""
    side = np.asarray(side, np.uint16)
    pos = positions(at, len(side))
    parts, spans, done, length = [], [], 0, 0
    for p, rec in zip(pos, block_recs):
        parts.append(side[done:p]); length += p - done; done = p
        n = 0 if rec is None else len(rec)
        if n:
            parts.append(np.asarray(rec, np.uint16))
        spans.append((length, length + n)); length += n
    parts.append(side[done:])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint16)).astype(np.uint16), spans


def is_bad(rec):
    ids = np.asarray(rec, np.uint16) & 0x1FF
    return bool(((ids >= 379) & (ids < REC_ALIGN)).any())


def walk_candidate(blocks, tus, first, end, side, at, start):
    """One candidate = blocks [first, end) spliced into `side` at `at` (a sequence indexed by block number t, or None), from the
    set `start` = (s0, s1, rate).  -> (bits, {t: share}, {t: info}, the set it leaves, its expanded string, flags)"""
    orc = H.load_oracle()
    recs, infos = [], {}
    for t in range(first, end):
        rec, info = block_records(blocks, tus, t)
        infos[t] = info
        recs.append(rec)
    string, spans = expand(side, [None if at is None else at[t] for t in range(first, end)], recs)
    if is_bad(side):
        return U64_MAX, None, infos, None, string, BAD_RECORD
    rc, total = orc.estimate_records_from(string, start[0], start[1], start[2])
    assert rc == 0
    s0, s1, rate = start[0].astype(np.int64), start[1].astype(np.int64), start[2].copy()
    shares, done = {}, 0
    for t, (a, b) in zip(range(first, end), spans):
        advance(s0, s1, rate, string[done:a]); done = a
        shares[t] = 0
        if b > a:
            rc, shares[t] = orc.estimate_records_from(string[a:b], s0.astype(np.uint16), s1.astype(np.uint16), rate)
            assert rc == 0
    advance(s0, s1, rate, string[done:])
    return total, shares, infos, (s0.astype(np.uint16), s1.astype(np.uint16), rate), string, 0


def estimate_model(cand_first, blocks, tus, sets, which, rec_first, records, tu_at, out_set=None):
    """cabac_hip_estimate_unit_device: (cand_bits, tu_bits, tu_info, flags, {out set: (s0, s1, rate)}, [left], [strings]); a
    candidate with a bad record has tu_bits of its blocks left 0 (the header leaves them unspecified) and left None."""
    n_cand = len(cand_first) - 1
    n_tu = int(cand_first[n_cand])
    cand_bits, flags = np.zeros(n_cand, np.uint64), np.zeros(n_cand, np.uint32)
    tu_bits, tu_info = np.zeros(len(tus), np.uint64), np.zeros(len(tus), np.uint32)
    written, left, strings = {}, [], []
    for c in range(n_cand):
        f, n = clip_run(rec_first, c)
        first, end = min(int(cand_first[c]), n_tu), min(int(cand_first[c + 1]), n_tu)
        bits, shares, infos, l, string, fl = walk_candidate(blocks, tus, first, max(end, first), records[f:f + n], tu_at, sets[int(which[c])])
        cand_bits[c], flags[c] = bits, fl
        for t, v in (shares or {}).items():
            tu_bits[t] = v
        for t, v in infos.items():
            tu_info[t] = v
        left.append(l)
        strings.append(string)
        if out_set is not None and int(out_set[c]) != NO_SET and l is not None:
            written[int(out_set[c])] = l
    return cand_bits, tu_bits, tu_info, flags, written, left, strings


def round_model(group_first, cand_first, blocks, tus, sets, which, rec_first, records, tu_at, group_out_set, dist, lambda_q16):
    """cabac_hip_search_unit_round_device on a list of sets: -> (cand_bits, pick, cost, new list of sets, tu_bits, tu_info, the
    expanded string of every candidate, flags)"""
    n_cand = len(cand_first) - 1
    cand_bits, tu_bits, tu_info, flags, _, left, strings = estimate_model(cand_first, blocks, tus, sets, which, rec_first, records, tu_at)
    pick, cost = select(group_first, cand_bits, dist, lambda_q16, n_cand_max=n_cand)
    new_sets = list(sets)
    if group_out_set is not None:
        for g in range(len(group_first) - 1):
            if int(group_out_set[g]) != NO_SET and int(pick[g]) != NONE:
                new_sets[int(group_out_set[g])] = left[int(pick[g])]
    return cand_bits, pick, cost, new_sets, tu_bits, tu_info, strings, flags


# ---------------------------------------------------------------------------------------------- generators for the tests
SIDE_POOL = np.concatenate([np.arange(0, 86), np.arange(292, 357)])        # contexts residual coding never touches


def side_run(rng, n, ts_flag=None, trm=False, align=False):
    """n side records: context-coded ones drawn from SIDE_POOL and, one in eight, from the contexts blocks use too (86..291,
    357..378); a fifth bypass bins; with ts_flag = 0 / 1 a transform_skip_flag record (context 310 / 311) of a random value
    among them; with trm a terminate bin of each value; with align an align record."""
    rec = np.zeros(n, np.uint16)
    for i in range(n):
        r = rng.random()
        if r < 0.2:
            rec[i] = REC_EP | (int(rng.integers(0, 2)) << 15)
        else:
            pool = SIDE_POOL if rng.random() < 0.875 else np.concatenate([np.arange(86, 292), np.arange(357, 379)])
            rec[i] = int(rng.choice(pool)) | (int(rng.integers(0, 2)) << 15)
    spots = list(rng.permutation(n)) if n else []
    if ts_flag is not None and spots:
        rec[spots.pop()] = (310 + ts_flag) | (int(rng.integers(0, 2)) << 15)
    if trm and len(spots) >= 2:
        rec[spots.pop()] = REC_TRM
        rec[spots.pop()] = REC_TRM | 0x8000
    if align and spots:
        rec[spots.pop()] = REC_ALIGN
    return rec
