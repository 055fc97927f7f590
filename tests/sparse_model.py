"""The sparse coefficient transport in numpy: the two walks of include/cabac_hip_sparse.h (DEFINITION OF THE RESULT) as the tests
state them.  pack: dense blocks -> (ent_first, entries, status); unpack: the lists written into a dense array.  A status is a dict
(n_entries, flags, first_bad); the helpers at the end build the cases the CPU and the GPU tests share."""
import numpy as np

from entropy_coding_amd import capi

OVERFLOW, RANGE, BAD_POS, BAD_FIRST, BAD_BLOCK = 1, 2, 4, 8, 16
NO_BAD = 0xFFFFFFFF


def status_dict(rec):
    return dict(n_entries=int(rec["n_entries"]), flags=int(rec["flags"]), first_bad=int(rec["first_bad"]))


def _good(tu, n_total):
    lw, lh, off = int(tu["log2_width"]), int(tu["log2_height"]), int(tu["coeff_offset"])
    return lw <= 6 and lh <= 6 and off + (1 << (lw + lh)) <= n_total


def pack(tus, coeff, capacity=None):
    """COMPACT: the coded region (x < min(w, 32), y < min(h, 32)) of every good block scanned in ascending pos."""
    n_total = len(coeff)
    first, ent, flags, bad = [], [], 0, NO_BAD
    for t, tu in enumerate(tus):
        first.append(len(ent))
        if not _good(tu, n_total):
            flags |= BAD_BLOCK
            bad = min(bad, t)
            continue
        w, h, off = 1 << int(tu["log2_width"]), 1 << int(tu["log2_height"]), int(tu["coeff_offset"])
        blk = coeff[off:off + w * h].reshape(h, w)[:min(h, 32), :min(w, 32)].astype(np.int64)
        ys, xs = np.nonzero(blk)
        lev = blk[ys, xs]
        if np.any((lev < -32768) | (lev > 32767)):
            flags |= RANGE
            bad = min(bad, t)
        ent += list((ys * w + xs).astype(np.uint32) | ((lev & 0xFFFF).astype(np.uint32) << 16))
    first.append(len(ent))
    n = len(ent)
    if capacity is None:
        capacity = n
    if n > capacity:
        flags |= OVERFLOW
    return (np.array(first, np.uint32), np.array(ent[:capacity], np.uint32),
            dict(n_entries=n, flags=flags, first_bad=bad))


def unpack(tus, ent_first, entries, coeff, n_entries=None):
    """EXPAND into `coeff` (in place): every element of every good block written, nothing else.  Of two entries with the same pos
    the later one is taken here (the contract allows either)."""
    n_total = len(coeff)
    n_entries = len(entries) if n_entries is None else n_entries
    flags, bad = 0, NO_BAD
    for t, tu in enumerate(tus):
        if not _good(tu, n_total):
            flags |= BAD_BLOCK
            bad = min(bad, t)
            continue
        n, off = 1 << (int(tu["log2_width"]) + int(tu["log2_height"])), int(tu["coeff_offset"])
        coeff[off:off + n] = 0
        lo, hi = int(ent_first[t]), int(ent_first[t + 1])
        if lo > hi:
            flags |= BAD_FIRST
            bad = min(bad, t)
            hi = lo
        if hi > n_entries:
            flags |= BAD_FIRST
            bad = min(bad, t)
            hi = n_entries
            lo = min(lo, hi)
        for e in entries[lo:hi]:
            pos = int(e) & 0xFFFF
            if pos >= n:
                flags |= BAD_POS
                bad = min(bad, t)
            else:
                coeff[off + pos] = ((int(e) >> 16) ^ 0x8000) - 0x8000        # the level, an int16
    return dict(n_entries=min(int(ent_first[len(tus)]), n_entries), flags=flags, first_bad=bad)


# ---------------------------------------------------------------------------------------------------------------- cases
def layout(shapes, rng=None, gaps=False, odd=False):
    """Block descriptors for (log2 w, log2 h) shapes laid one behind the other; gaps: 0 .. 5 spare elements in front of each
    block (odd: at least an odd offset for the first); returns (tus, n_coeff_total)."""
    tus = np.zeros(len(shapes), capi.TU_DTYPE)
    at = 1 if odd else 0
    for t, (lw, lh) in enumerate(shapes):
        if gaps:
            at += int(rng.integers(0, 6))
        tus[t]["coeff_offset"], tus[t]["log2_width"], tus[t]["log2_height"] = at, lw, lh
        at += 1 << (lw + lh)
    return tus, at + (int(rng.integers(0, 4)) if gaps else 0)


def fill(rng, tus, n_total, dtype, density=0.3, junk=True, sentinel=True):
    """A dense array for the blocks: the coded region of each random at `density` (levels over the whole int16 range now and
    then), junk outside the coded region of 64-wide / tall blocks, the sentinel 0x5A.. in the gaps."""
    info = np.iinfo(dtype)
    coeff = np.full(n_total, 0x5A5A if dtype == np.int16 else 0x5A5A5A5A, dtype) if sentinel else np.zeros(n_total, dtype)
    for tu in tus:
        w, h, off = 1 << int(tu["log2_width"]), 1 << int(tu["log2_height"]), int(tu["coeff_offset"])
        blk = np.zeros((h, w), np.int64)
        if junk:
            blk[:] = rng.integers(1, 100, (h, w))
        cw, ch = min(w, 32), min(h, 32)
        lev = rng.integers(-6, 7, (ch, cw))
        wide = rng.random((ch, cw)) < 0.05
        lev = np.where(wide, rng.integers(max(info.min, -32768), min(info.max, 32767) + 1, (ch, cw)), lev)
        blk[:ch, :cw] = np.where(rng.random((ch, cw)) < density, lev, 0)
        coeff[off:off + w * h] = blk.ravel().astype(dtype)
    return coeff


ALL_SHAPES = [(lw, lh) for lw in range(7) for lh in range(7)]


def mixed_shapes(rng, n, max_log2=4):
    """n shapes, mostly small (as transform blocks are), every size up to 2^max_log2 a side"""
    return [(int(rng.integers(0, max_log2 + 1)), int(rng.integers(0, max_log2 + 1))) for _ in range(n)]
