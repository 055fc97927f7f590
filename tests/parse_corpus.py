"""Inputs for the residual parser's large tests (tests/test_gpu_residual_parse_large.py) and what the oracle's parser
(orc_residual_decode, oracle/cabac_oracle.c) makes of them.  CPU only: the GPU tests compare the device with expectation(),
tests/test_sanitizers.py runs the damaged corpus through the oracle under AddressSanitizer / UBSan:

    python3 tests/parse_corpus.py --oracle <sanitized libcabac_oracle.so>

A corpus is a dict: subs[s] = (metas, blocks, bytes) as tests/test_gpu_residual_parse.py::parse takes them (metas =
[(w, h, channel, flags[, max_log2_tr_range])]), qps, caps (byte_capacity per substream), finish (CABAC_SUB_FINISH per
substream), and for the damaged corpus kind (a letter per substream)."""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helpers as H  # noqa: E402
import test_gpu_residual_parse as P  # noqa: E402

SBT_SHAPES = [(32, 32), (32, 8), (8, 32), (32, 16), (16, 32), (32, 4), (4, 32), (16, 16), (8, 8), (4, 4), (64, 32)]
TS_SIZES = [1, 2, 4, 8, 16, 32]
TRM_END = np.array([0x81FF], np.uint16)   # encodeBinTrm(1) closes a substream

# What the oracle's parser returns -> cabac_substream_result.flags of the device (include/cabac_hip_parse.h).  -4: the input ran
# out — in a block, or in the terminate bin — and that is reported ALONE, instead of the stop check and of the refusal of a
# block behind it (the reference's readByte throws first); -5: terminate bin 0 or a wrong stop pattern; -2: a block the parser does not cover, the parse
# stops there.  The int16 store adds CABAC_RES_RANGE where a stored level lies outside int16.
RC_FLAGS = {0: 0, -2: H.RES_BAD_RECORD, -4: H.RES_UNDERRUN, -5: H.RES_BAD_STOP}


def ts_block(rng, w, h, kind):
    c = ((rng.random((h, w)) < [0.3, 1.0, 0.8, 0.05][kind]) *
         rng.integers(-[4, 40, 3, 3000][kind], [4, 40, 3, 3000][kind] + 1, (h, w))).astype(np.int32)
    if not c.any():
        c[rng.integers(0, h), rng.integers(0, w)] = 1
    return c


def random_tu(rng, style):
    """One block of the given style -> (meta, coefficients).  regular: any shape up to 64 x 64; ts_flag_0: a regular block whose
    transform_skip_flag is coded (0); sbt: SBT / MTS zero-out; ts_flag_1 / ts / bdpcm: transform-skip residual coding with the
    flag coded, not coded, and BDPCM."""
    dq, ch = int(rng.integers(0, 2)), int(rng.integers(0, 2))
    if style in ("regular", "ts_flag_0"):
        w, h, c = P.random_regular(rng)
        if style == "ts_flag_0":
            w, h = min(w, 32), min(h, 32)
            c = np.ascontiguousarray(c[:h, :w])     # random_block leaves nothing outside the top-left 32 x 32
        fl = dq | (H.TU_TS_FLAG if style == "ts_flag_0" else 0)
    elif style == "sbt":
        w, h = SBT_SHAPES[int(rng.integers(0, len(SBT_SHAPES)))]
        ch = int(rng.random() < 0.15)
        c = H.random_block(rng, w, h, density=float(rng.choice([0.05, 0.4, 1.0])), big=float(rng.choice([0.0, 0.3])))
        if not ch and max(w, h) <= 32:   # what the zero-out leaves: the left / upper 16 of a 32-wide / tall luma block
            if w == 32:
                c[:, 16:] = 0
            if h == 32:
                c[16:, :] = 0
            if not c.any():
                c[0, 0] = 1
        fl = dq | H.TU_SBT_ZERO_OUT
    else:
        w, h = TS_SIZES[int(rng.integers(0, 6))], TS_SIZES[int(rng.integers(0, 6))]
        if w * h == 1:
            h = 4
        c = ts_block(rng, w, h, int(rng.integers(0, 4)))
        fl = dq | H.TU_TRANSFORM_SKIP | {"ts_flag_1": H.TU_TS_FLAG, "ts": 0, "bdpcm": H.TU_BDPCM}[style]
    return (w, h, ch, fl), c


def encode(orc, metas, blocks, qp):
    """The blocks coded as one substream, closed by the terminate bin and the stop pattern."""
    rec = [orc.residual_records(c, m[2], m[3], max_log2_range=m[4] if len(m) > 4 else 15)[0] for m, c in zip(metas, blocks)]
    return orc.encode_records(np.concatenate(rec + [TRM_END]), int(qp), 2, 3)[0]


MIXED_STYLES = ["regular", "regular", "ts_flag_0", "ts_flag_1", "ts", "bdpcm", "sbt"]


def random_substream(rng, orc, s, n_blocks, qp):
    """Every third substream: test_gpu_residual_parse.build's — regular blocks of every shape — with sign hiding (what the
    oracle parses is the expectation); the others: every style mixed, no sign hiding (the coded blocks must come back)."""
    if s % 3 == 0:
        fl = H.TU_SIGN_HIDING | int(rng.integers(0, 2))
        return P.build(rng, 1, lambda _: fl, [qp], n_blocks=n_blocks)[0]
    metas, blocks = [], []
    for _ in range(n_blocks):
        m, c = random_tu(rng, MIXED_STYLES[int(rng.integers(0, len(MIXED_STYLES)))])
        metas.append(m)
        blocks.append(c)
    return metas, blocks, encode(orc, metas, blocks, qp)


def ragged(seed, n_sub, empties=True):
    """n_sub substreams: of every eight neighbours one holds 1 block and the next 30..34, the others 1..8; with `empties`
    substreams 3, 10, n/2, n-2 and n-1 hold no block at all — the first, third and last with byte_capacity 0, the others
    with the two bytes of a closed empty substream; CABAC_SUB_FINISH on about two thirds."""
    orc = H.load_oracle()
    rng = np.random.default_rng(seed)
    qps = rng.integers(0, 64, n_sub)
    finish = rng.random(n_sub) < 0.67
    empty = [3, 10, n_sub // 2, n_sub - 2, n_sub - 1] if empties else []
    subs = []
    for s in range(n_sub):
        if s in empty:
            data = orc.encode_records(TRM_END, int(qps[s]), 2, 3)[0] if empty.index(s) & 1 else np.zeros(0, np.uint8)
            subs.append(([], [], data))
            continue
        n_blocks = 1 if s % 8 == 1 else int(rng.integers(30, 35)) if s % 8 == 2 else int(rng.integers(1, 9))
        subs.append(random_substream(rng, orc, s, n_blocks, qps[s]))
    return dict(subs=subs, qps=qps, caps=np.array([len(x[2]) for x in subs]), finish=finish)


REFUSED = ["ts_64_wide", "ts_flag_64_wide", "log2_width_7", "channel_2"]


def with_errors(seed, n_sub):
    """ragged() without empty substreams, and every ninth substream (s % 9 == 4: each wave of a four-wave workgroup in turn,
    three intact neighbours on either side) damaged: truncated to half its bytes, its stop byte destroyed, or one of its blocks
    given a descriptor the parser refuses (REFUSED).  -> corpus with damage[s] = None or what was done."""
    orc = H.load_oracle()
    c = ragged(seed, n_sub, empties=False)
    rng = np.random.default_rng(seed + 1)
    c["finish"][:] = True
    c["damage"] = [None] * n_sub
    kinds = ["truncated", "stop"] + REFUSED
    for i, s in enumerate(range(4, n_sub, 9)):
        kind = kinds[i % len(kinds)]
        metas, blocks, data = c["subs"][s]
        if kind == "truncated":
            c["caps"][s] = max(1, len(data) // 2)
        elif kind == "stop":
            data = data.copy()
            data[-1] = 0x00 if data[-1] != 0 else 0x55
        else:
            # a fresh substream of >= 3 blocks whose block k gets the bad descriptor; for ts_flag_64_wide block k is a
            # transform-skip block with its flag coded 1 and the descriptor claims it to be 64 wide
            n_blocks = max(3, len(metas))
            k = int(rng.integers(1, n_blocks - 1))
            metas, blocks = [], []
            for b in range(n_blocks):
                m, co = random_tu(rng, "ts_flag_1" if (b == k and kind == "ts_flag_64_wide") else MIXED_STYLES[int(rng.integers(0, len(MIXED_STYLES)))])
                metas.append(m)
                blocks.append(co)
            data = encode(orc, metas, blocks, c["qps"][s])
            w, h, ch, fl = metas[k]
            metas[k] = {"ts_64_wide": (64, 16, ch, H.TU_TRANSFORM_SKIP), "ts_flag_64_wide": (64, h, ch, fl),
                        "log2_width_7": (128, h, ch, fl), "channel_2": (w, h, 2, fl)}[kind]
            blocks[k] = None
            c["caps"][s] = len(data)
            kind = (kind, k)
        c["subs"][s] = (metas, blocks, data)
        c["damage"][s] = kind
    return c


def underrun_meets_refusal(seed):
    """The corners where two reasons to stop meet, and descriptors only the range check refuses.  Per substream:
    0: truncated to half, and a block behind the truncation has log2_width 7; 1: the same with a 64-wide block whose coded
    transform_skip_flag says transform skip; 2: byte_capacity 1 and the first block is that 64-wide one (the flag's own read
    is past the end); 3, 4: max_log2_tr_range 14 and 21 on the second of three blocks; 5: intact."""
    orc = H.load_oracle()
    rng = np.random.default_rng(seed)
    subs, qps, caps = [], rng.integers(0, 64, 6), []
    for s in range(6):
        metas, blocks = [], []
        for b in range(8 if s < 2 else 3):
            m, c = random_tu(rng, "ts_flag_1" if (s in (1, 2) and b == (6 if s == 1 else 0)) else MIXED_STYLES[int(rng.integers(0, len(MIXED_STYLES)))])
            metas.append(m)
            blocks.append(c)
        data = encode(orc, metas, blocks, qps[s])
        cap = len(data)
        if s == 0:
            metas[6], cap = (128,) + metas[6][1:], len(data) // 2
        elif s == 1:
            metas[6], cap = (64,) + metas[6][1:], len(data) // 2
        elif s == 2:
            metas[0], cap = (64,) + metas[0][1:], 1
        elif s in (3, 4):
            metas[1] = metas[1] + (14 if s == 3 else 21,)
        subs.append((metas, None, data))
        caps.append(cap)
    return dict(subs=subs, qps=qps, caps=np.array(caps), finish=np.ones(6, bool))


def escape_block(rng, w, h, max_log2, limit):
    """Most coefficients of the coded region escape-coded: |level| from 1 000 up to `limit`."""
    c = np.zeros((h, w), np.int32)
    he, we = min(h, 32), min(w, 32)
    mag = rng.integers(1000, limit + 1, (he, we))
    mag = np.where(rng.random((he, we)) < 0.15, limit - rng.integers(0, 3, (he, we)), mag)   # crowd the upper end
    c[:he, :we] = (rng.random((he, we)) < 0.85) * mag * np.where(rng.random((he, we)) < 0.5, -1, 1)
    if not c.any():
        c[0, 0] = limit
    return c


ESCAPE_SHAPES = {"regular": [(32, 32), (16, 16), (8, 8), (4, 4), (64, 64), (64, 8), (2, 8), (1, 16), (32, 4), (16, 1)],
                 "ts": [(32, 32), (16, 16), (8, 8), (4, 4), (2, 8), (1, 16), (32, 4), (16, 1)]}


def escapes(seed, per_combination=12):
    """For max_log2_tr_range 15..20 and regular / transform-skip / BDPCM blocks: substreams of three escape blocks with
    ordinary context-coded blocks in front of each.  In every second substream of a range above 15 the levels stay inside
    int16; in the others they go up to the range's limit, and the first escape block of a substream holds both limits,
    -(1 << max_log2) and (1 << max_log2) - 1."""
    orc = H.load_oracle()
    rng = np.random.default_rng(seed)
    subs, qps = [], []
    for max_log2 in (15, 16, 17, 18, 19, 20):
        for kind in ("regular", "ts", "bdpcm"):
            for n in range(per_combination):
                limit = 32767 if n & 1 else (1 << max_log2) - 1
                metas, blocks = [], []
                for b in range(3):
                    for _ in range(int(rng.integers(1, 3))):
                        m, c = random_tu(rng, MIXED_STYLES[int(rng.integers(0, len(MIXED_STYLES)))])
                        metas.append(m + (max_log2,))
                        blocks.append(c)
                    w, h = ESCAPE_SHAPES["regular" if kind == "regular" else "ts"][int(rng.integers(0, 10 if kind == "regular" else 8))]
                    c = escape_block(rng, w, h, max_log2, limit)
                    if b == 0 and w * h >= 4:
                        c[0, 0], c[min(h, 32) - 1, min(w, 32) - 1] = -limit - 1, limit
                    fl = int(rng.integers(0, 2)) | {"regular": 0, "ts": H.TU_TRANSFORM_SKIP, "bdpcm": H.TU_TRANSFORM_SKIP | H.TU_BDPCM}[kind]
                    metas.append((w, h, int(rng.integers(0, 2)), fl, max_log2))
                    blocks.append(c)
                qps.append(int(rng.integers(0, 64)))
                subs.append((metas, blocks, encode(orc, metas, blocks, qps[-1])))
    n_sub = len(subs)
    return dict(subs=subs, qps=np.array(qps), caps=np.array([len(x[2]) for x in subs]), finish=np.ones(n_sub, bool))


DAMAGE_KINDS = "abcdef"


def damaged(seed, per_kind=600, max_blocks=6):
    """per_kind substreams of each kind, every one made from an intact substream of 1..max_blocks mixed blocks:
    (a) one flipped bit; (b) one flipped bit in every 16 bytes; (c) the right bytes with a wrong qp; (d) uniformly random bytes
    of the same length; (e) the right bytes with the block list reversed; (f) truncated to 3/4 of the length.  In the eighth
    substream of (a), (b) and (d) the damage is made to leave 0xFF as the first byte."""
    orc = H.load_oracle()
    rng = np.random.default_rng(seed)
    subs, qps, caps, kinds = [], [], [], []
    for kind in DAMAGE_KINDS:
        for n in range(per_kind):
            qp = int(rng.integers(0, 64))
            metas, blocks = [], []
            for _ in range(int(rng.integers(1, max_blocks + 1))):
                m, c = random_tu(rng, MIXED_STYLES[int(rng.integers(0, len(MIXED_STYLES)))])
                metas.append(m)
                blocks.append(c)
            data = encode(orc, metas, blocks, qp).copy()
            cap = len(data)
            if kind == "a":
                data[int(rng.integers(0, len(data)))] ^= 1 << int(rng.integers(0, 8))
            elif kind == "b":
                for o in range(0, len(data), 16):
                    data[o + int(rng.integers(0, min(16, len(data) - o)))] ^= 1 << int(rng.integers(0, 8))
            elif kind == "c":
                qp = (qp + int(rng.integers(1, 64))) % 64
            elif kind == "d":
                data = rng.integers(0, 256, len(data)).astype(np.uint8)
            elif kind == "e":
                metas = metas[::-1]
            else:
                cap = 3 * len(data) // 4
            if n == 7 and kind in "abd":
                data[0] = 0xFF    # the damage that no decoder can start from (a refused start): present whatever the seed gives
            subs.append((metas, None, data))
            qps.append(qp)
            caps.append(cap)
            kinds.append(kind)
    n_sub = len(subs)
    return dict(subs=subs, qps=np.array(qps), caps=np.array(caps), finish=np.ones(n_sub, bool), kind=np.array(kinds))


def take(corpus, index):
    """The substreams `index` (a slice or an index array) of a corpus as a corpus of their own."""
    pick = np.arange(len(corpus["subs"]))[index]
    return {k: ([v[i] for i in pick] if isinstance(v, list) else v[pick]) for k, v in corpus.items()}


def expectation(corpus):
    """The oracle's parse of every substream (its first byte_capacity bytes) -> [(rc, blocks, n_bits, info, n_whole)] with
    n_whole the number of blocks the oracle parsed to their end without running out of input: all of them for rc 0 / -5,
    those before the refused one for -2, those before the block in which the input ran out for -4."""
    orc = H.load_oracle()
    out = []
    for s, (metas, _, data) in enumerate(corpus["subs"]):
        rc, want, nbits, info = orc.residual_decode(data[:int(corpus["caps"][s])], int(corpus["qps"][s]), metas,
                                                    finish=bool(corpus["finish"][s]), with_info=True)
        assert rc in RC_FLAGS, rc
        # a block the oracle did not reach still holds residual_decode's fill (parse_block clears a block before it parses it)
        reached = [k for k, b in enumerate(want) if not (b == 0x5A5A5A5A).all()]
        assert reached == list(range(len(reached)))
        n_whole = len(reached)
        if rc == -4 and n_whole:
            n_whole -= 1    # the block in which the input ran out (or, when it ran out in the terminate bin, the last block)
        if rc == -4 and len(reached) == len(metas):
            # ... which one cannot tell from the outside: parse it again without the terminate bin
            rc2 = orc.residual_decode(data[:int(corpus["caps"][s])], int(corpus["qps"][s]), metas, finish=False)[0]
            n_whole = len(metas) if rc2 == 0 else n_whole
        out.append((rc, want, nbits, info, n_whole))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--oracle", required=True, help="the oracle's shared library to run the damaged corpus through")
    ap.add_argument("--seed", type=int, default=0xDA)
    ap.add_argument("--per-kind", type=int, default=600)
    a = ap.parse_args()
    H._oracle = H.CodecLib(ctypes.CDLL(a.oracle), "orc_")
    c = damaged(a.seed, a.per_kind)
    exp = expectation(c)
    share = {k: float(np.mean([exp[s][0] != -4 for s in np.flatnonzero(c["kind"] == k)])) for k in DAMAGE_KINDS}
    print("damaged corpus parsed: %d substreams, not underrun per kind %s" % (len(exp), share))


if __name__ == "__main__":
    main()
