"""GPU: the residual binariser (csrc/cabac_residual.hip) on the far side of its capped grids.

launch_residual_passes orders the blocks by size class — 7 (rejected), 6, 5, then 4, then the rest —, pads every class to
kRowsPerBlock = 16 rows and gives each group of 16 rows to one workgroup.  The classes 7, 6 and 5 (big_wgs groups) go to the
launch staged with 1 024 dwords per row, whose grid is capped at 1 024 workgroups; class 4 (mid_wgs groups) to the launch
staged with 256 dwords per row, capped at 8 192.  Both walk `for (wg = blockIdx.x; wg < ...; wg += gridDim.x)`: a workgroup
takes a second trip — and stages a second block over each row's LDS region — only with more than 16 * 1 024 = 16 384 blocks of
class >= 5, or more than 16 * 8 192 = 131 072 blocks of class 4.

The far batch has 16 + 4 800 + 11 608 = 16 424 blocks of the classes 7, 6, 5 (1 + 300 + 726 = 1 027 groups: the workgroups 0,
1 and 2 of 1 024 take a second trip) and 131 112 of class 4 (8 195 groups: again three second trips), the near batch
16 + 4 800 + 11 560 = 16 376 (exactly 1 024 groups) and 131 064 (exactly 8 192): every workgroup takes one trip, none two.
Both have 4 000 blocks of the classes 0..3 more, and enough blocks for the uncapped grid to exceed both caps.

The blocks are drawn, by index arrays, from a pool of about a thousand distinct blocks which the oracle has binarised once
(orc.residual_records, pinned to the reference's writer by tests/test_residual_oracle.py); everything is compared exactly
and whole arrays at a time."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
from entropy_coding_amd import capi
from test_gpu_residual import _ts_block

pytestmark = pytest.mark.gpu

ROWS, CAP_BIG, CAP_MID = 16, 1024, 8192          # kRowsPerBlock and the two grid caps of launch_residual_passes
FILL, SLACK = 0x5555, 2
FIN = H.SUB_FINISH | H.SUB_ALIGN_RBSP
# blocks per size class (index = class); the classes 7 and 6 are whole groups, so that the groups of 7 + 6 + 5 are those of the sum
FAR = {7: 16, 6: 4800, 5: ROWS * CAP_BIG + 40 - 4816, 4: ROWS * CAP_MID + 40, 3: 1000, 2: 1000, 1: 1000, 0: 1000}
NEAR = {7: 16, 6: 4800, 5: ROWS * CAP_BIG - 8 - 4816, 4: ROWS * CAP_MID - 8, 3: 1000, 2: 1000, 1: 1000, 0: 1000}
FAR_NO_REJECTS = {**FAR, 7: 0, 5: FAR[5] + 16}


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    yield c
    c.close()


def size_class(lw, lh):
    """size_class() of csrc/cabac_residual.hip: log2 of the number of coefficient groups of the coded region, 7 if rejected."""
    if lw > 6 or lh > 6:
        return 7
    if lw == 0:
        gw, gh = 0, min(lh, 4)
    elif lh == 0:
        gw, gh = min(lw, 4), 0
    elif lw == 1:
        gw, gh = 1, (1 if lh <= 2 else 3)
    elif lh == 1:
        gw, gh = (1 if lw <= 2 else 3), 1
    else:
        gw, gh = 2, 2
    return (min(lw, 5) - gw) + (min(lh, 5) - gh)


def groups(counts, classes):
    return sum((counts[c] + ROWS - 1) // ROWS for c in classes)


# ---------------------------------------------------------------------------------------------- the pool
class Pool:
    """Distinct blocks and what the oracle makes of them: per entry the coefficients (flat, as the descriptor's width and
    height lay them out), log2 width / height, channel, flags, size class, records and info."""

    def __init__(self):
        self.coeff, self.lw, self.lh, self.ch, self.fl, self.rec, self.info, self.real = [], [], [], [], [], [], [], []

    def add(self, c, ch, fl, lw=None, lh=None):
        orc = H.load_oracle()
        h, w = c.shape
        lw, lh = int(np.log2(w)) if lw is None else lw, int(np.log2(h)) if lh is None else lh
        rejected = lw > 6 or lh > 6 or ch > 1
        if rejected:
            rec, info = np.zeros(0, np.uint16), H.TU_INFO_BAD_DESC
        else:
            try:
                rec, last, mts = orc.residual_records(c, ch, fl)
                info = last | (H.TU_INFO_MTS_VIOLATION if mts else 0)
            except ValueError:                       # an all-zero block: no records and a flag
                rec, info = np.zeros(0, np.uint16), H.TU_INFO_EMPTY
        self.coeff.append(np.ascontiguousarray(c, np.int32).ravel())
        self.lw.append(lw); self.lh.append(lh); self.ch.append(ch); self.fl.append(fl)
        self.rec.append(rec); self.info.append(info); self.real.append(not rejected and len(rec) > 0)

    def freeze(self):
        self.lw, self.lh, self.ch, self.fl = (np.array(a, np.uint8) for a in (self.lw, self.lh, self.ch, self.fl))
        self.info = np.array(self.info, np.uint32)
        self.real = np.array(self.real)
        self.cls = np.array([size_class(int(a), int(b)) for a, b in zip(self.lw, self.lh)])
        self.n_rec = np.array([len(r) for r in self.rec], np.int64)
        self.n_coeff = np.array([len(c) for c in self.coeff], np.int64)
        self.rec_slack = [np.concatenate([r, np.full(SLACK, FILL, np.uint16)]) for r in self.rec]
        return self


@functools.lru_cache(None)
def pool():
    rng = np.random.default_rng(0x6B1D)
    p = Pool()
    regular = [((32, 16), 100), ((16, 32), 100),                                   # class 5
               ((32, 32), 110), ((64, 32), 12), ((64, 64), 8),                     # class 6
               ((16, 16), 200), ((32, 8), 100), ((8, 32), 100),                    # class 4
               ((16, 8), 50), ((8, 8), 60), ((8, 4), 50), ((4, 4), 40), ((2, 8), 40)]      # classes 3, 2, 1, 0, 0
    for (w, h), n in regular:
        for k in range(n):
            c = H.random_block(rng, w, h, density=0.3 if k % 4 == 3 else 0.05, big=[0.0, 0.05, 0.3][k % 3],
                               last_frac=[1.0, 0.5][k % 2])
            fl = int(rng.integers(0, 8))
            p.add(c, int(rng.integers(0, 2)), fl & ~H.TU_TS_FLAG if max(w, h) > 32 else fl)
    for w, h in [(32, 32), (32, 32), (32, 16), (16, 32), (16, 16), (16, 16), (32, 8), (8, 8), (8, 4), (4, 4), (16, 8), (2, 8)]:
        for k in range(2):                                                          # transform-skip blocks, up to 32 x 32
            p.add(_ts_block(rng, w, h, (k + w) % 3 if w * h > 256 else k), int(rng.integers(0, 2)),
                  H.TU_TRANSFORM_SKIP | [H.TU_TS_FLAG, H.TU_BDPCM][k] | int(rng.integers(0, 4)))
    for k in range(4):                                                              # rejected by their size: class 7
        p.add(np.ones((4, 4), np.int32), 0, 0, lw=7 if k % 2 else 2, lh=2 if k % 2 else 7)
    for w, h in [(32, 32), (32, 16), (16, 16), (8, 8)]:                             # rejected for their channel; all-zero blocks
        p.add(H.random_block(rng, w, h, density=0.05), 2, 0)
        p.add(np.zeros((h, w), np.int32), 0, 3)
    p.freeze()
    assert 900 <= len(p.rec) <= 1100 and all((p.cls == c).sum() >= 4 for c in range(8))
    assert max(int(np.abs(c).max()) for c in p.coeff) < 32768                       # the int16 form holds every block
    return p


def draw(counts, seed, real_only=False):
    """Index array into the pool with counts[c] blocks of class c, shuffled."""
    p = pool()
    rng = np.random.default_rng(seed)
    idx = []
    for c, n in counts.items():
        if n == 0:
            continue
        have = np.flatnonzero((p.cls == c) & (p.real | (not real_only)))
        idx.append(rng.choice(have, size=n))
    idx = np.concatenate(idx)
    rng.shuffle(idx)
    return idx


def descriptors(idx):
    p = pool()
    tus = np.zeros(len(idx), H.TU_DTYPE)
    tus["coeff_offset"] = np.concatenate([[0], np.cumsum(p.n_coeff[idx])[:-1]])
    tus["log2_width"], tus["log2_height"], tus["channel"], tus["flags"] = p.lw[idx], p.lh[idx], p.ch[idx], p.fl[idx]
    coeff = np.concatenate([p.coeff[i] for i in idx])
    return tus, coeff


def first_block(pos, roff, idx):
    p = pool()
    b = int(np.searchsorted(roff, pos, side="right")) - 1
    return "record %d: block %d (pool entry %d, class %d, %d records from %d)" % (pos, b, idx[b], p.cls[idx[b]], p.n_rec[idx[b]],
                                                                                  roff[b])


def check_both_passes(hip, counts, seed):
    """cabac_hip_residual_device as tests/test_gpu_residual.py::residual() runs it — the sizes pass, then the records pass at
    offsets that leave SLACK words behind every block — with every output compared as one array."""
    p = pool()
    idx = draw(counts, seed)
    n = len(idx)
    assert n // ROWS >= CAP_MID                      # the uncapped grid is larger than both caps: they are what is launched
    tus, coeff = descriptors(idx)
    want_cnt, want_info = p.n_rec[idx].astype(np.uint32), p.info[idx]
    t_tu = torch.from_numpy(tus.view(np.uint8).reshape(-1).copy()).cuda()
    t_co = torch.from_numpy(coeff).cuda()
    del coeff
    t_cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    t_info = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hip.residual_device(n, t_tu.data_ptr(), t_co.data_ptr(), 0, t_cnt.data_ptr(), t_info.data_ptr(), 0)
    hip.synchronize()
    cnt, info = t_cnt.cpu().numpy().view(np.uint32), t_info.cpu().numpy().view(np.uint32)
    # (0xFFFFFFFF is no value of either array: no block has that many records, and bit 29 is no info flag)
    left = np.flatnonzero((cnt == 0xFFFFFFFF) | (info == 0xFFFFFFFF))
    assert not len(left), "sizes pass: %d blocks not written, first block %d of class %d" % (len(left), left[0], p.cls[idx[left[0]]])
    assert np.array_equal(cnt, want_cnt), np.flatnonzero(cnt != want_cnt)[:8]
    assert np.array_equal(info, want_info), np.flatnonzero(info != want_info)[:8]
    roff = np.concatenate([[0], np.cumsum(want_cnt.astype(np.int64) + SLACK)[:-1]])
    total = int(want_cnt.sum()) + SLACK * n
    t_roff = torch.from_numpy(roff).cuda()
    t_rec = torch.full((total,), FILL, dtype=torch.int16, device="cuda")
    t_cnt2 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    t_info.fill_(-1)
    torch.cuda.synchronize()
    hip.residual_device(n, t_tu.data_ptr(), t_co.data_ptr(), t_roff.data_ptr(), t_cnt2.data_ptr(), t_info.data_ptr(), t_rec.data_ptr())
    hip.synchronize()
    cnt2, info2 = t_cnt2.cpu().numpy().view(np.uint32), t_info.cpu().numpy().view(np.uint32)
    left = np.flatnonzero((cnt2 == 0xFFFFFFFF) | (info2 == 0xFFFFFFFF))
    assert not len(left), "records pass: %d blocks not written, first block %d of class %d" % (len(left), left[0], p.cls[idx[left[0]]])
    assert np.array_equal(cnt2, want_cnt) and np.array_equal(info2, want_info)
    got = t_rec.cpu().numpy().view(np.uint16)
    del t_tu, t_co, t_rec, t_roff
    torch.cuda.empty_cache()
    want = np.concatenate([p.rec_slack[i] for i in idx])      # every block's records and the fill behind them
    assert len(want) == total
    in_slack = np.ones(total, bool)                            # the SLACK words behind every block: block b's are SLACK * b on
    in_slack[np.arange(total - SLACK * n) + SLACK * np.repeat(np.arange(n), want_cnt)] = False
    assert in_slack.sum() == SLACK * n and (want[in_slack] == FILL).all()
    wrong = np.flatnonzero(got[in_slack] != FILL)
    assert not len(wrong), "written behind a block's records: " + first_block(int(np.flatnonzero(in_slack)[wrong[0]]), roff, idx)
    wrong = np.flatnonzero(got != want)
    assert not len(wrong), "%d records differ, first " % len(wrong) + first_block(int(wrong[0]), roff, idx)


# ---------------------------------------------------------------------------------------------- a. / c. both passes
def test_second_trips_of_both_staged_loops(hip):
    """16 424 blocks of class >= 5 and 131 112 of class 4: three workgroups of each staged launch take a second trip."""
    assert groups(FAR, (7, 6, 5)) == CAP_BIG + 3 and groups(FAR, (4,)) == CAP_MID + 3
    assert sum(FAR[c] for c in (7, 6, 5)) == ROWS * CAP_BIG + 40
    check_both_passes(hip, FAR, seed=0x6B20)


def test_full_caps_and_no_second_trip(hip):
    """The guard on the near side: 16 376 blocks of class >= 5 and 131 064 of class 4 fill the two capped grids exactly, one
    trip each.  (A loop that entered a second trip here would write a block twice; with this case passing, a failure of the
    far case is the second trip's.)"""
    assert groups(NEAR, (7, 6, 5)) == CAP_BIG and groups(NEAR, (4,)) == CAP_MID
    assert sum(NEAR[c] for c in (7, 6, 5)) == ROWS * CAP_BIG - 8
    check_both_passes(hip, NEAR, seed=0x6B21)


# ---------------------------------------------------------------------------------------------- b. the spliced path
@pytest.mark.parametrize("int16", [False, True], ids=["int32", "int16"])
def test_second_trips_through_the_spliced_path(hip, int16):
    """The far batch without rejected descriptors and empty blocks (16 424 real blocks of the classes 6 and 5), as 1 024
    substreams of consecutive blocks and one terminate record each, through cabac_hip_encode_residual_device: the sizes pass,
    then the records pass on the order the first one left, with int32 and with int16 coefficients.  Bytes, n_bits, flags and
    the blocks' info against the oracle's encoder on the oracle's records."""
    orc = H.load_oracle()
    p = pool()
    assert groups(FAR_NO_REJECTS, (7, 6, 5)) == CAP_BIG + 3 and groups(FAR_NO_REJECTS, (4,)) == CAP_MID + 3
    idx = draw(FAR_NO_REJECTS, seed=0x6B22, real_only=True)
    n, n_sub = len(idx), 1024
    rng = np.random.default_rng(0x6B23)
    first = np.concatenate([[0], np.sort(rng.choice(np.arange(1, n), size=n_sub - 1, replace=False)), [n]]).astype(np.uint32)
    tus, coeff = descriptors(idx)
    splices = np.zeros(n, capi.SPLICE_DTYPE)
    splices["tu"] = np.arange(n)                     # every block in front of its substream's only host record
    host_rec = np.full(n_sub, H.REC_TRM | H.REC_BIN, np.uint16)
    qp, init = rng.integers(0, 64, size=n_sub), rng.integers(0, 3, size=n_sub)
    desc, _ = H.make_desc([1] * n_sub, qp, init, FIN)
    desc["byte_offset"] = 0
    desc["byte_capacity"] = 0                        # ignored by the call
    # expected: the blocks' records, a terminate record behind every run, coded by the oracle
    block_end = np.cumsum(p.n_rec[idx])
    expanded = np.insert(np.concatenate([p.rec[i] for i in idx]), block_end[first[1:] - 1], H.REC_TRM | H.REC_BIN)
    sub_len = np.diff(np.concatenate([[0], block_end[first[1:] - 1]])) + 1
    want_desc, want_total = H.make_desc(sub_len, qp, init, FIN)
    want_bytes, want_res = orc.encode_batch(want_desc, expanded, want_total)
    assert not want_res["flags"].any()
    nb = (want_res["n_bits"].astype(np.int64) + 7) // 8
    want_pay = np.concatenate([want_bytes[int(o): int(o) + int(k)] for o, k in zip(want_desc["byte_offset"], nb)])
    total = len(want_pay)

    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()
    t_desc, t_rec, t_first = dev(desc, np.uint8), dev(host_rec, np.int16), dev(first, np.int32)
    t_sp, t_tu = dev(splices, np.uint8), dev(tus, np.uint8)
    t_co = dev(coeff.astype(np.int16), np.int16) if int16 else dev(coeff, np.int32)
    del coeff
    t_pay = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    t_off = torch.full((n_sub + 1,), -1, dtype=torch.int64, device="cuda")
    t_res = torch.full((2 * n_sub,), -1, dtype=torch.int32, device="cuda")
    t_info = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hip.encode_residual_device(n_sub, t_desc.data_ptr(), t_rec.data_ptr(), t_first.data_ptr(), t_sp.data_ptr(), n, n, t_tu.data_ptr(),
                               t_co.data_ptr(), t_pay.data_ptr(), total + 64, t_off.data_ptr(), t_res.data_ptr(), t_info.data_ptr(), 0,
                               int16=int16)
    hip.synchronize()
    res, offs = t_res.cpu().numpy().view(H.RESULT_DTYPE), t_off.cpu().numpy()
    info, pay = t_info.cpu().numpy().view(np.uint32), t_pay.cpu().numpy()
    del t_co, t_pay, t_tu, t_sp
    torch.cuda.empty_cache()
    regular = (p.fl[idx] & H.TU_TRANSFORM_SKIP) == 0          # (as tests/test_gpu_splice.py: the info of regular blocks)
    wrong = np.flatnonzero((info != p.info[idx]) & regular)
    assert not len(wrong), "info of %d blocks, first block %d of class %d" % (len(wrong), wrong[0], p.cls[idx[wrong[0]]])
    assert np.array_equal(res["flags"], want_res["flags"])
    wrong = np.flatnonzero(res["n_bits"] != want_res["n_bits"])
    assert not len(wrong), "n_bits of %d substreams, first %d (blocks %d..%d)" % (len(wrong), wrong[0], first[wrong[0]], first[wrong[0] + 1])
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(nb)]))
    assert np.array_equal(pay[:total], want_pay), int(np.searchsorted(offs, np.flatnonzero(pay[:total] != want_pay)[0], side="right")) - 1
    assert (pay[total:] == 0xEE).all()
