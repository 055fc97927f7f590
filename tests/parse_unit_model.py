"""CPU model of include/cabac_hip_parse_unit.h: a substream is a run of side records with transform blocks spliced in, read back in
one walk.  There is no CPU reader for such streams, so the model rests on two things the oracle already pins to the compiled
reference (tests/test_residual_oracle.py, tests/test_oracle_vs_reference.py):

  * for valid streams the expected result is the encoder's input (encode_unit: the oracle's bytes of the expanded string);
  * for ANY bytes a result (C, B) — blocks and side bins — is right if and only if it is CONSISTENT: re-binarise the decoded
    blocks C with orc.residual_records, splice them into the side ids at at(t), and orc.decode_records of that expanded id string
    on the same bytes returns exactly the bins of that string — the blocks' own and B — and the same n_bits.  The reader's next
    context is a function of the bins so far, so a string that reproduces itself IS the reader's walk.

A unit is a dict: metas [(w, h, channel, flags[, max_log2_tr_range])], blocks [(h, w) int32], side (uint16 records, bin bits set),
at (one raw position per block, or None: every block behind the run), qp, finish, data (bytes)."""
import numpy as np

import helpers as H
import parse_corpus as PC
import search_unit_model as U

TRM_END = PC.TRM_END


class Skip(Exception):
    """consistent() cannot judge: a decoded block is all zero (the binariser refuses it) or a level leaves 16 bits."""


def block_records(meta, coeff, info=None):
    """The records of one block as the binariser writes them.  With CABAC_TU_TS_FLAG the coded flag decides how the block was
    read: `info` (the parser's word for the block) says which, and the block is binarised that way."""
    orc = H.load_oracle()
    fl = meta[3]
    if info is not None and (fl & H.TU_TS_FLAG):
        fl = (fl | H.TU_TRANSFORM_SKIP) if (int(info) & H.TU_INFO_TS) else (fl & ~H.TU_TRANSFORM_SKIP)
    return orc.residual_records(np.ascontiguousarray(coeff, np.int32), meta[2], fl, max_log2_range=meta[4] if len(meta) > 4 and meta[4] else 15)[0]


def expand(side, blocks, tu_at):
    """side: uint16 records; blocks: [(meta, coefficients[, info])]; tu_at: one raw position per block or None.  -> (the expanded
    string, [(start, end) of every block's records in it], [(start, end) of the pieces of the side run in it])"""
    side = np.asarray(side, np.uint16)
    recs = [block_records(*b) for b in blocks]
    at = [None] * len(blocks) if tu_at is None else list(tu_at)
    string, spans = U.expand(side, at, recs)
    is_side = np.ones(len(string), bool)
    for a, b in spans:
        is_side[a:b] = False
    assert int(is_side.sum()) == len(side)
    return string, spans, is_side


def encode_unit(unit, closed=True):
    """The oracle's bytes of the unit's expanded string, closed by finish() and the RBSP alignment.  closed=False: the string does
    not end with the terminate bin; one is coded behind it (and not read back) so that the bins in front of it can be decoded."""
    orc = H.load_oracle()
    string, _, _ = expand(unit["side"], list(zip(unit["metas"], unit["blocks"])), unit["at"])
    return orc.encode_records(string if closed else np.concatenate([string, TRM_END]), int(unit["qp"]), 2, 3)[0]


def consistent(data, qp, side, metas, tu_at, C, B, n_bits, finish=False, infos=None):
    """-> (True / False, rc of the oracle's decode of the expanded string: 0, or -5 for a failed stop check).  Raises Skip where
    a decoded block cannot be binarised again."""
    orc = H.load_oracle()
    for c in C:
        c = np.asarray(c)
        he, we = min(c.shape[0], 32), min(c.shape[1], 32)
        if not c[:he, :we].any() or np.abs(c.astype(np.int64)).max() > 32767:
            raise Skip()
    blocks = [(m, c) + ((infos[k],) if infos is not None else ()) for k, (m, c) in enumerate(zip(metas, C))]
    try:
        string, spans, is_side = expand(side, blocks, tu_at)
    except ValueError:
        raise Skip()
    rc, bins, nread = orc.decode_records(string, int(qp), 2, np.ascontiguousarray(data, np.uint8), flags=1 if finish else 0)
    if rc not in (0, -5):
        return False, rc
    own = (string >> 15).astype(np.uint8)
    ok = np.array_equal(bins[~is_side], own[~is_side]) and np.array_equal(bins[is_side], np.asarray(B, np.uint8)) and nread == int(n_bits)
    return bool(ok), rc


# ------------------------------------------------------------------------------------------------ corpus builders
def make_unit(rng, styles, n_side, qp=None, at="random", trm=True, finish=True, ts_side=False, shapes=None):
    """One unit of len(styles) blocks (styles of parse_corpus.random_tu; shapes: regular blocks of these (w, h) instead) in a run
    of n_side random side records (search_unit_model.side_run) closed by the terminate bin (with at None the blocks lie behind the run: the terminate bin is coded
    behind them and is not part of the unit, and there is no stop check).  at: "random" (sorted positions),
    None, or a list of raw positions.  ts_side (True, or the blocks it applies to): a block's transform_skip_flag is coded as a side record in front of it."""
    orc = H.load_oracle()
    qp = int(rng.integers(0, 64)) if qp is None else int(qp)
    metas, blocks = [], []
    for k, st in enumerate(styles):
        if shapes is not None:
            w, h = shapes[k]
            m, c = (w, h, int(rng.integers(0, 2)), int(rng.integers(0, 2))), H.random_block(rng, w, h, density=float(rng.choice([0.3, 0.7])), big=0.1)
        else:
            m, c = PC.random_tu(rng, st)
        metas.append(m)
        blocks.append(c)
    side = U.side_run(rng, n_side)
    if at == "random":
        at = sorted(int(x) for x in rng.integers(0, n_side + 1, len(styles)))
    if ts_side:                                                    # the flag in front of its block, CABAC_TU_TS_FLAG clear
        assert at is not None
        pos = U.positions(at, len(side))
        for k in reversed(range(len(metas))):
            w, h, ch, fl = metas[k][:4]
            if not (fl & H.TU_TS_FLAG) or (ts_side is not True and k not in ts_side):
                continue
            flag = np.array([(310 + ch) | (0x8000 if fl & H.TU_TRANSFORM_SKIP else 0)], np.uint16)
            side = np.concatenate([side[:pos[k]], flag, side[pos[k]:]])
            for j in range(k, len(metas)):
                pos[j] += 1
            metas[k] = (w, h, ch, fl & ~H.TU_TS_FLAG)
        at = pos
    if at is None:
        trm = finish = False                                        # the blocks lie behind the run: no terminate bin in front of them
    if trm:
        side = np.concatenate([side, TRM_END])
    unit = dict(metas=metas, blocks=blocks, side=side.astype(np.uint16), at=at, qp=qp, finish=finish)
    unit["data"] = encode_unit(unit, closed=trm)
    return unit


def damaged_units(seed, n_sub=200, block_only=False):
    """n_sub units of one to four regular blocks of 4 x 4 .. 8 x 8 with side records between them (none with block_only), one to
    three bits flipped, and zero padding by (7 * CABAC_TU_MAX_RECORDS(n) + 7) / 8 bytes per block plus one byte per side record:
    the input cannot run out."""
    rng = np.random.default_rng(seed)
    units = []
    for s in range(n_sub):
        n_blocks = int(rng.integers(1, 5))
        shapes = [(int(rng.choice([4, 8])), int(rng.choice([4, 8]))) for _ in range(n_blocks)]
        n_side = 0 if block_only else int(rng.integers(1, 13))
        u = make_unit(rng, ["regular"] * n_blocks, n_side, shapes=shapes)
        data = u["data"].copy()
        for _ in range(int(rng.integers(1, 4))):
            data[int(rng.integers(0, len(data)))] ^= 1 << int(rng.integers(0, 8))
        if data[0] == 0xFF:
            data[0] = 0x7F                                          # a refused start is test 8's, not this corpus's
        pad = sum((7 * H.TU_MAX_RECORDS(w * h) + 7) // 8 for w, h in shapes) + len(u["side"])
        u["data"] = np.concatenate([data, np.zeros(pad, np.uint8)])
        units.append(u)
    return units


def pack(units, capacities=None):
    """The host arrays of a unit parse -> dict(desc, bytes, tile_first, tus, tu_at (None when no unit has positions), records,
    offsets (coeff_offset per block), total): blocks back to back, runs back to back, byte slots 16-aligned with 16 spare."""
    n = len(units)
    metas = [m for u in units for m in u["metas"]]
    sizes = np.array([m[0] * m[1] for m in metas], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if len(sizes) else np.zeros(0, np.int64)
    tus = np.zeros(max(len(metas), 1), H.TU_DTYPE)
    for i, m in enumerate(metas):
        w, h, ch, fl = m[:4]
        tus[i]["coeff_offset"], tus[i]["log2_width"], tus[i]["log2_height"] = int(offsets[i]), int(np.log2(w)), int(np.log2(h))
        tus[i]["channel"], tus[i]["flags"], tus[i]["max_log2_tr_range"] = ch, fl, m[4] if len(m) > 4 else 0
    tile_first = np.concatenate([[0], np.cumsum([len(u["metas"]) for u in units])]).astype(np.uint32)
    lens = np.array([len(u["side"]) for u in units], np.uint64)
    desc = np.zeros(n, H.DESC_DTYPE)
    desc["n_records"] = lens
    desc["rec_offset"] = np.concatenate([[0], np.cumsum(lens)[:-1]])
    nbytes = np.array([len(u["data"]) for u in units], np.uint64)
    slots = (nbytes + 15) // 16 * 16 + 16
    desc["byte_offset"] = np.concatenate([[0], np.cumsum(slots)[:-1]])
    desc["byte_capacity"] = nbytes if capacities is None else np.asarray(capacities, np.uint64)
    desc["qp"] = [u["qp"] for u in units]
    desc["init_id"] = [2 | (H.SUB_FINISH if u["finish"] else 0) for u in units]
    buf = np.zeros(int(slots.sum()), np.uint8)
    for s, u in enumerate(units):
        buf[int(desc["byte_offset"][s]): int(desc["byte_offset"][s]) + len(u["data"])] = u["data"]
    records = np.concatenate([u["side"] for u in units] + [np.zeros(0, np.uint16)]).astype(np.uint16)
    tu_at = None
    if any(u["at"] is not None for u in units):
        tu_at = np.concatenate([np.asarray(u["at"] if u["at"] is not None else [len(u["side"])] * len(u["metas"]), np.uint64)
                                for u in units] + [np.zeros(0, np.uint64)]).astype(np.uint32)
    return dict(desc=desc, bytes=buf, tile_first=tile_first, tus=tus, tu_at=tu_at, records=records, offsets=offsets,
                total=int(sizes.sum()), n_tu=len(metas))
