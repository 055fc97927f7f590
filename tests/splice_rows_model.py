"""CPU model of include/cabac_hip_splice_rows.h, composed from what exists: search_unit_model.expand / positions and
test_gpu_residual_estimate.block_records give a substream's expanded record string, ctx_sets_model.encode_from / advance_from give
bytes and contexts from a start set, the level loop is ctx_sets_model.wpp_starts, and the log is search_emit_model.LogModel with
marks beside it.  What this module adds is the hand-over point: the clipping of the pair (clip_pair) and the index into the
expanded string it stands for (Sub.index).

A context set is ctx_sets_model's triple (s0, s1, rate)."""
import numpy as np

import ctx_sets_model as CS
import helpers as H
import search_emit_model as E
import search_unit_model as U
from entropy_coding_amd import capi
from test_gpu_residual_estimate import block_records

NO_SET = END = 0xFFFFFFFF
RES_BAD_SET = CS.RES_BAD_SET
ENC_FLAGS = 3                                                      # finish() and the RBSP alignment


def clip_pair(ats, n, k, m=None):
    """The hand-over pair of a substream of n host records with splices at the sorted positions `ats`: k host records in front,
    clipped to n; m splices in front, clipped to [#{at < k}, #{at <= k}] (None: the upper end)."""
    k = min(int(k), n)
    lo, hi = sum(1 for a in ats if a < k), sum(1 for a in ats if a <= k)
    return k, hi if m is None else min(max(int(m), lo), hi)


class Sub:
    """One substream: host records, effective splice positions (sorted), the blocks' records (None: an empty, badly described or
    rejected block) and info words."""

    def __init__(self, side, ats, recs, infos=()):
        self.side, self.recs, self.infos = np.asarray(side, np.uint16), list(recs), list(infos)
        self.ats = U.positions(list(ats), len(self.side))
        self.string, self.spans = U.expand(self.side, self.ats, self.recs)

    def index(self, k, m=None):
        """the hand-over pair as an index into the expanded string: the k host records and the records of the m blocks in front"""
        k, m = clip_pair(self.ats, len(self.side), k, m)
        return k + sum(len(r) for r in self.recs[:m] if r is not None)


def subs_of(case):
    """The substreams of a test_gpu_search_unit.Case: candidate s = substream s, its run the host records, its blocks the splices."""
    out = []
    for s in range(case.n_cand):
        first, end = int(case.cand_first[s]), int(case.cand_first[s + 1])
        got = [block_records(case.blocks, case.tus, t) for t in range(first, end)]
        out.append(Sub(case.runs[s], [int(case.tu_at[t]) for t in range(first, end)], [g[0] for g in got], [g[1] for g in got]))
    return out


def device_form(case, subs, qp, init, flags=H.SUB_FINISH | H.SUB_ALIGN_RBSP):
    """What the C ABI takes for the substreams of `case`: (desc, records, splice_first, splices, tus, coeff)."""
    desc, _ = H.make_desc([len(s.side) for s in subs], qp, init, flags)
    desc["byte_offset"] = 0
    desc["byte_capacity"] = 0                                       # ignored by the calls
    flat = [(at, int(case.cand_first[s]) + j) for s, sub in enumerate(subs) for j, at in enumerate(sub.ats)]
    splices = np.array(flat, capi.SPLICE_DTYPE) if flat else np.zeros(0, capi.SPLICE_DTYPE)
    return desc, case.records, np.asarray(case.cand_first, np.uint32), splices, case.tus, case.coeff


def tu_info(subs):
    return np.array([i for s in subs for i in s.infos], np.uint32)


def payload_of(chunks):
    """(payload, offsets) of the substreams' bytes back to back (None: nothing)"""
    chunks = [np.zeros(0, np.uint8) if c is None else c for c in chunks]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64)
    return (np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)).astype(np.uint8), offsets


def encode_plain(subs, qp, init, flags=ENC_FLAGS):
    """cabac_hip_encode_residual_device by the oracle's own entry point -> ([bytes], n_bits)"""
    orc = H.load_oracle()
    got = [orc.encode_records(s.string, int(qp[k]), int(init[k]) & 3, flags) for k, s in enumerate(subs)]
    return [g[0] for g in got], np.array([g[1] for g in got], np.uint32)


def encode_sets(subs, qp, init, sets, start=None, out=None, flags=ENC_FLAGS):
    """cabac_hip_encode_residual_sets_device -> ([bytes], results, {out index: the contexts written there}).  Every substream reads
    its start set from `sets` as it was before the call (the IN-PLACE RULE lets nobody see another's out set)."""
    res, chunks, written = np.zeros(len(subs), H.RESULT_DTYPE), [], {}
    for s, sub in enumerate(subs):
        st = NO_SET if start is None else int(start[s])
        o = NO_SET if out is None else int(out[s])
        if (st != NO_SET and st >= len(sets)) or (o != NO_SET and o >= len(sets)):
            res[s] = (0, RES_BAD_SET)
            chunks.append(np.zeros(0, np.uint8))
            continue
        ctx = CS.init_set(int(qp[s]), int(init[s])) if st == NO_SET else sets[st]
        n, data, n_bits, left = CS.encode_from(sub.string, ctx, flags)
        assert n >= 0
        res[s] = (n_bits, 0)
        chunks.append(data)
        if o != NO_SET:
            written[o] = left
    return chunks, res, written


def indices(subs, sync_at, sync_splice=None):
    return np.array([sub.index(int(sync_at[s]), None if sync_splice is None else int(sync_splice[s])) for s, sub in enumerate(subs)],
                    np.uint32)


def encode_rows(subs, qp, init, level_first, sync_from, sync_at, sync_splice=None, flags=ENC_FLAGS):
    """cabac_hip_encode_residual_rows_* -> ([bytes; empty for a refused row; None where the contexts are unspecified: a row linked
    to a refused one], results, the hand-over indices, the start contexts).  The level loop is ctx_sets_model.wpp_starts over the
    expanded strings cut at the indices."""
    desc, _ = H.make_desc([len(s.string) for s in subs], qp, init, 0)
    records = np.concatenate([s.string for s in subs] + [np.zeros(0, np.uint16)]).astype(np.uint16)
    idx = indices(subs, sync_at, sync_splice)
    start, ok = CS.wpp_starts(desc, records, level_first, sync_from, idx)
    res, chunks = np.zeros(len(subs), H.RESULT_DTYPE), []
    for s, sub in enumerate(subs):
        if start[s] is None:
            res[s] = (0, 0 if ok[s] else RES_BAD_SET)
            chunks.append(None if ok[s] else np.zeros(0, np.uint8))
            continue
        n, data, n_bits, _ = CS.encode_from(sub.string, start[s], flags)
        assert n >= 0
        res[s] = (n_bits, 0)
        chunks.append(data)
    return chunks, res, idx, start


class MarkedLog:
    """search_emit_model.LogModel and, beside it, the chains' marks (cabac_hip_search_log_mark_device)."""

    def __init__(self, n_chain, *caps, **kw):
        self.log = E.LogModel(n_chain, *caps, **kw)
        self.n_chain = n_chain
        self.marks = [(END, END)] * n_chain

    def append(self, *a):
        return self.log.append(*a)

    def mark(self, chains):
        for ch in chains:
            if int(ch) < self.n_chain:                              # 0xFFFFFFFF among the skipped
                self.marks[int(ch)] = (self.log.chain_rec[int(ch)], self.log.chain_tu[int(ch)])

    def reset(self):
        self.log.reset()
        self.marks = [(END, END)] * self.n_chain

    def pairs(self):
        return np.array([m[0] for m in self.marks], np.uint32), np.array([m[1] for m in self.marks], np.uint32)

    def subs(self):
        """every chain as a Sub: its side records behind one another, its logged blocks at their positions"""
        log = self.log
        lens, records, first, splices = log.host_form()
        tus = np.array(log.tu, H.TU_DTYPE) if log.tu else np.zeros(0, H.TU_DTYPE)
        blocks = [log.block(t) for t in range(len(log.tu))]
        base = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
        out = []
        for k in range(self.n_chain):
            sp = splices[int(first[k]):int(first[k + 1])]
            got = [block_records(blocks, tus, int(t)) for t in sp["tu"]]
            out.append(Sub(records[int(base[k]):int(base[k + 1])], [int(a) for a in sp["at"]], [g[0] for g in got], [g[1] for g in got]))
        return out

    def info(self):
        """tu_info per LOGGED block, in log order"""
        return self.log.strings()[1]

    def encode_rows(self, qp, init, level_first, sync_from, flags=ENC_FLAGS):
        at, sp = self.pairs()
        return encode_rows(self.subs(), qp, init, level_first, sync_from, at, sp, flags)

    def encode_sets(self, qp, init, sets, start=None, out=None, flags=ENC_FLAGS):
        return encode_sets(self.subs(), qp, init, sets, start, out, flags)


# ---------------------------------------------------------------------------------------------- the batches of the tests
def ctu(rng, n_side=None, n_blocks=None, first_at_zero=False):
    """One "CTU": a side run of 10 .. 40 records with 1 .. 3 blocks of 4 x 4 to 16 x 16 inside -> (run, [(block, chroma, flags, at)])"""
    from test_gpu_search_unit import _block
    n = int(rng.integers(10, 41)) if n_side is None else n_side
    k = int(rng.integers(1, 4)) if n_blocks is None else n_blocks
    ats = sorted(int(rng.integers(1, n + 1)) for _ in range(k))
    if first_at_zero:
        ats[0] = 0
    items = []
    for at in ats:
        w, h = [(4, 4), (8, 8), (16, 16), (8, 4), (4, 16)][int(rng.integers(0, 5))]
        items.append((_block(rng, w, h), int(rng.integers(0, 2)), int(rng.integers(0, 4)), at))
    return U.side_run(rng, n), items


def row(ctus):
    """CTUs behind one another in one substream, closed by the terminate bin -> (run, items, [host records in front of every CTU], [blocks in front of it])"""
    run, items, rec_at, blk_at = [], [], [], []
    for r, it in ctus:
        rec_at.append(len(run))
        blk_at.append(len(items))
        items += [(b, ch, fl, at + len(run)) for b, ch, fl, at in it]
        run += [int(x) for x in r]
    run.append(U.REC_TRM | 0x8000)                                  # end_of_slice: the row's last record
    return np.array(run, np.uint16), items, rec_at, blk_at


def rows_batch(seed, n_pic=3, n_row=4):
    """n_pic pictures x n_row rows of 3 CTUs each, in LEVEL ORDER (substream r * n_pic + p is row r of picture p; level r = row r
    of every picture), row r linked to row r - 1 of its picture.  Hand-over points cycle through 0, "after CTU 1" and 10**6; the
    natural sync_splice of "after CTU 1" is the number of blocks of CTU 0, so that blocks the next CTU begins with stay behind.
    What the tests are about, by substream:
      1 (picture 1, row 0)   a rejected block (channel 2) and an empty one in front of its point
      2 (picture 2, row 0)   70 blocks in its first CTU: more than 64 splices in front of its point
      n_pic (picture 0, row 1)   its CTU 1 BEGINS WITH TWO BLOCKS: the pair decides whether row 2 of picture 0 sees them
      2 * n_pic + 1          unlinked, in the middle
    -> dict(case, subs, level_first, sync_from, sync_at, splice: {"lower", "middle", "upper"}, probe: the substream with the
    blocks at its point, child: the one linked to it)"""
    from test_gpu_search_unit import Case, _block
    rng = np.random.default_rng(seed)
    n_sub = n_pic * n_row
    case, meta, empty, bad = Case(), [], [], []
    for s in range(n_sub):
        ctus = [ctu(rng) for _ in range(3)]
        if s == 2:
            ctus[0] = ctu(rng, n_side=40, n_blocks=70)
        if s == n_pic:
            run, items = ctu(rng, n_blocks=3)
            items = [(b, ch, fl, 0 if j < 2 else max(at, 1)) for j, (b, ch, fl, at) in enumerate(items)]
            ctus[1] = (run, items)
        run, items, rec_at, blk_at = row(ctus)
        if s == 1:
            assert blk_at[1] >= 1
            items.insert(0, (_block(rng, 8, 8), 0, 0, 1))
            items.insert(1, (_block(rng, 4, 4), 0, 0, 1))
            blk_at = [blk_at[0]] + [b + 2 for b in blk_at[1:]]
            bad.append(len(case.blocks))
            empty.append(len(case.blocks) + 1)
        meta.append((rec_at, blk_at))
        case.add(run, items)
    case.finish(empty=empty, bad=bad)
    subs = subs_of(case)
    level_first = np.arange(0, n_sub + 1, n_pic, dtype=np.uint32)
    sync_from = np.full(n_sub, NO_SET, np.uint32)
    sync_at, natural = np.zeros(n_sub, np.uint32), np.zeros(n_sub, np.uint32)
    for r in range(n_row):
        for p in range(n_pic):
            s = r * n_pic + p
            if r > 0 and s != 2 * n_pic + 1:
                sync_from[s] = s - n_pic
            kind = 1 if s in (1, 2, n_pic) else s % 3
            sync_at[s], natural[s] = [(0, 0), (meta[s][0][1], meta[s][1][1]), (10 ** 6, END)][kind]
    probe = n_pic
    lower = natural.copy()
    middle, upper = lower.copy(), lower.copy()
    middle[probe] += 1
    upper[probe] += 2
    return dict(case=case, subs=subs, level_first=level_first, sync_from=sync_from, sync_at=sync_at,
                splice=dict(lower=lower, middle=middle, upper=upper), probe=probe, child=probe + n_pic, meta=meta)
