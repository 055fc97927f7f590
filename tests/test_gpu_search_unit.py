"""GPU: search rounds over candidates with side records (include/cabac_hip_search_unit.h; the kSide variant of the kernel in
csrc/cabac_residual_estimate.hip) against tests/search_unit_model.py, which tests/test_search_unit_model.py pins to the compiled
reference, and against the two entry points the header names as identities.  Everything is bit-exact: == on integers, no
tolerance, no case left out of a comparison.  Every test has its own bounded input, and nothing is run again after a failure."""
import numpy as np
import pytest

import helpers as H
import search_unit_model as M
from entropy_coding_amd import capi
from test_gpu_residual import make_tus
from test_gpu_residual_estimate import SENTINEL32, SENTINEL64, _ts_block, dev, make_sets, pack_sets
from test_gpu_search import assert_sets_equal, mixed_candidates, run_export, t_u32, t_u64

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U = (1 << 64) - 1
TS, TS_FLAG, DQ, SH = H.TU_TRANSFORM_SKIP, H.TU_TS_FLAG, H.TU_DEP_QUANT, H.TU_SIGN_HIDING
EP, TRM, ALIGN, BIN = M.REC_EP, M.REC_TRM, M.REC_ALIGN, 0x8000


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


def t_rec(records):
    import torch
    records = np.asarray(records, np.uint16)
    return dev(records, np.int16) if len(records) else torch.zeros(1, dtype=torch.int16, device="cuda")


def run_unit(hip, cand_first, tus, coeff, state, rate, which, rec_first, records, tu_at, out_set=None, n_out=0, int16=False,
             in_place=False, pad=2):
    """cabac_hip_estimate_unit_device on torch tensors, every output between guard words; out_set None: no set is written (the set
    outputs then keep their sentinels); in_place: the output arrays are the input arrays.
    -> (bits, tu_bits, tu_info, flags, out_state, out_rate)"""
    import torch
    n_cand, n_tu = len(cand_first) - 1, len(tus)
    t_first = t_u32(cand_first)
    t_tu = dev(tus, np.uint8) if n_tu else torch.zeros(16, dtype=torch.uint8, device="cuda")
    t_co = dev(np.asarray(coeff, np.int16 if int16 else np.int32)) if len(coeff) else torch.zeros(4, dtype=torch.int32, device="cuda")
    t_state, t_rate, t_set = dev(np.asarray(state, np.uint32), np.int32), dev(np.asarray(rate, np.uint8)), t_u32(which)
    t_rf, t_records = t_u64(rec_first), t_rec(records)
    t_at = t_u32(tu_at) if tu_at is not None else None
    t_out = t_u32(out_set) if out_set is not None else None
    before_state, before_rate = t_state.clone(), t_rate.clone()
    t_bits = torch.full((n_cand + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
    t_tub = torch.full((n_tu + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
    t_info = torch.full((n_tu + 2,), SENTINEL32, dtype=torch.int32, device="cuda")
    t_flags = torch.full((n_cand + 2,), SENTINEL32, dtype=torch.int32, device="cuda")
    if in_place:
        t_os, t_or, off = t_state, t_rate, 0
    else:
        t_os = torch.full(((n_out + 2 * pad) * 379,), SENTINEL32, dtype=torch.int32, device="cuda")
        t_or = torch.full(((n_out + 2 * pad) * 379,), 0x5A, dtype=torch.uint8, device="cuda")
        off = pad * 379
    hip.estimate_unit_device(n_cand, t_first.data_ptr(), t_tu.data_ptr(), t_co.data_ptr(), t_state.data_ptr(), t_rate.data_ptr(),
                             t_set.data_ptr(), t_rf.data_ptr(), t_records.data_ptr() if len(records) else 0, t_at.data_ptr() if t_at is not None else 0,
                             t_bits.data_ptr() + 8, t_tub.data_ptr() + 8, t_info.data_ptr() + 4, t_flags.data_ptr() + 4,
                             t_out.data_ptr() if t_out is not None else 0, t_os.data_ptr() + 4 * off, t_or.data_ptr() + off, int16=int16)
    hip.synchronize()
    bits, tub = t_bits.cpu().numpy().view(np.uint64), t_tub.cpu().numpy().view(np.uint64)
    info, flags = t_info.cpu().numpy().view(np.uint32), t_flags.cpu().numpy().view(np.uint32)
    assert bits[0] == SENTINEL64 and bits[-1] == SENTINEL64 and tub[0] == SENTINEL64 and tub[-1] == SENTINEL64
    assert info[0] == SENTINEL32 and info[-1] == SENTINEL32 and flags[0] == SENTINEL32 and flags[-1] == SENTINEL32
    os_, or_ = t_os.cpu().numpy().view(np.uint32), t_or.cpu().numpy()
    if not in_place:
        assert torch.equal(t_state, before_state) and torch.equal(t_rate, before_rate)       # the start sets are not modified
        assert (os_[:off] == SENTINEL32).all() and (os_[off + n_out * 379:] == SENTINEL32).all()
        assert (or_[:off] == 0x5A).all() and (or_[off + n_out * 379:] == 0x5A).all()
        os_, or_ = os_[off:off + n_out * 379], or_[off:off + n_out * 379]
    return bits[1:-1].copy(), tub[1:-1].copy(), info[1:-1].copy(), flags[1:-1].copy(), os_.copy(), or_.copy()


# ---------------------------------------------------------------------------------------------- identity 1: no side records
@pytest.mark.parametrize("int16", [False, True])
def test_without_side_records_it_is_the_exporting_estimator(hip, int16):
    """Empty side runs (and a NULL d_records), any d_tu_at: every output array — costs, per-block costs, infos, every entry of
    every written set — equals cabac_hip_estimate_residual_ctx_device's on the same inputs; the flags are 0."""
    rng = np.random.default_rng(0x1DE1 + int16)
    blocks, tus, coeff, first = mixed_candidates(rng, 260, 5)
    n_cand = len(first) - 1
    sets = make_sets(rng, 5)
    state, rate = pack_sets(sets)
    which = rng.integers(0, 5, n_cand).astype(np.uint32)
    n_out = n_cand + 3
    slots = rng.permutation(n_out)[:n_cand].astype(np.uint32)
    out_set = np.where(rng.random(n_cand) < 0.25, NONE, slots).astype(np.uint32)
    co = coeff.astype(np.int16) if int16 else coeff
    want = run_export(hip, first, tus, co, state, rate, which, out_set, n_out, int16)
    rec_first = np.zeros(n_cand + 1, np.uint64)
    for tu_at in (None, rng.integers(0, 1 << 32, len(tus), dtype=np.uint64).astype(np.uint32)):
        bits, tub, info, flags, o_state, o_rate = run_unit(hip, first, tus, co, state, rate, which, rec_first, [], tu_at, out_set, n_out, int16)
        for got, w in zip((bits, tub, info, o_state, o_rate), want):
            assert np.array_equal(got, w)
        assert not flags.any()


# ---------------------------------------------------------------------------------------------- identity 2: no blocks
def test_without_blocks_it_is_the_record_estimator(hip):
    """Side runs of 0, 1, 15, 16, 17, 33 and 100 records (context-coded on all 379 contexts, bypass, terminate of both values,
    align; one candidate with a record that is none) and no block: cost and flags equal cabac_hip_estimate_from_device's."""
    import torch
    rng = np.random.default_rng(0x1DE2)
    sets = make_sets(rng, 3)
    state, rate = pack_sets(sets)
    runs = []
    for n in (0, 1, 15, 16, 17, 33, 100) * 4:
        r = H.random_records(rng, n, ctx_frac=0.75, end_trm=False, trm0_frac=0.05)
        for k in range(n):
            if rng.random() < 0.04:
                r[k] = [ALIGN, TRM | BIN][int(rng.integers(0, 2))]
        runs.append(r)
    runs[12][30] = 0x1F0                                                   # a 33-record run with a record that is none
    n_cand = len(runs)
    records = np.concatenate(runs)
    rec_first = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.uint64)
    which = rng.integers(0, 3, n_cand).astype(np.uint32)
    assert (records & 0x1FF == ALIGN).any() and (records == TRM).any() and (records == (TRM | BIN)).any()
    bits, _, _, flags, _, _ = run_unit(hip, np.zeros(n_cand + 1, np.uint32), np.zeros(0, H.TU_DTYPE), [], state, rate, which, rec_first,
                                       records, None)
    desc = np.zeros(n_cand, H.DESC_DTYPE)
    desc["rec_offset"], desc["n_records"] = rec_first[:-1], np.diff(rec_first).astype(np.uint32)
    t_desc, t_records = dev(desc, np.uint8), t_rec(records)
    t_state, t_rate, t_set = dev(state, np.int32), dev(rate), t_u32(which)
    t_bits = torch.zeros(n_cand, dtype=torch.int64, device="cuda")
    t_flags = torch.zeros(n_cand, dtype=torch.int32, device="cuda")
    hip.estimate_from_device(n_cand, t_desc.data_ptr(), t_records.data_ptr(), t_state.data_ptr(), t_rate.data_ptr(), t_set.data_ptr(),
                             t_bits.data_ptr(), t_flags.data_ptr())
    hip.synchronize()
    want_bits, want_flags = t_bits.cpu().numpy().view(np.uint64), t_flags.cpu().numpy().view(np.uint32)
    assert np.array_equal(flags, want_flags) and flags[12] == capi.RES_BAD_RECORD and int(flags.sum()) == capi.RES_BAD_RECORD
    ok = flags == 0
    assert np.array_equal(bits[ok], want_bits[ok]) and bits[12] == U
    for c in np.nonzero(ok)[0]:                                            # and the model says the same
        assert int(bits[c]) == M.walk_candidate([], [], 0, 0, runs[c], None, sets[int(which[c])])[0], c


# ---------------------------------------------------------------------------------------------- model parity, exported sets
def _block(rng, w, h, kind="regular"):
    if kind == "ts":
        return _ts_block(rng, w, h, int(rng.integers(0, 4)))
    return H.random_block(rng, w, h, density=float(rng.choice([0.3, 0.8])), big=0.1)


class Case:
    """Candidates built one at a time: add(run, [(block, chroma, flags, raw position), ...])."""

    def __init__(self):
        self.blocks, self.chromas, self.flags, self.first, self.runs, self.at = [], [], [], [0], [], []

    def add(self, run, items):
        for b, ch, fl, at in items:
            self.blocks.append(b); self.chromas.append(ch); self.flags.append(fl); self.at.append(at)
        self.first.append(len(self.blocks))
        self.runs.append(np.asarray(run, np.uint16))

    def finish(self, empty=(), bad=()):
        for t in empty:
            self.blocks[t] = np.zeros_like(self.blocks[t])
        self.tus, self.coeff = make_tus(self.blocks, self.chromas, self.flags)
        for t in bad:
            self.tus[t]["channel"] = 2
        self.cand_first = np.asarray(self.first, np.uint32)
        self.tu_at = np.asarray(self.at, np.uint64).astype(np.uint32)
        self.records = np.concatenate(self.runs) if self.runs else np.zeros(0, np.uint16)
        self.rec_first = np.concatenate([[0], np.cumsum([len(r) for r in self.runs])]).astype(np.uint64)
        self.n_cand = len(self.runs)
        return self


def _parity_case():
    rng = np.random.default_rng(0x9A21)
    c = Case()
    reg = lambda w=8, h=8, ch=0, fl=SH: (_block(rng, w, h), ch, fl)
    ts = lambda w=8, h=8, ch=0, fl=TS: (_block(rng, w, h, "ts"), ch, fl)
    run = lambda n, **kw: M.side_run(rng, n, **kw)
    # one block at position 0, in the middle, at the end
    c.add(run(20), [reg(4, 4) + (0,)])
    c.add(run(20), [reg(16, 16, 1) + (7,)])
    c.add(run(20), [reg(8, 4, 0, DQ) + (20,)])
    # two blocks at one position; three blocks: position 0, a 16-record step boundary and the end of the run
    c.add(run(12), [reg() + (5,), reg(4, 4, 1) + (5,)])
    c.add(run(40), [reg(4, 8) + (0,), reg(16, 8) + (16,), reg(4, 4, 1, DQ) + (40,)])
    c.add(run(40), [reg(8, 8) + (17,), reg(4, 4) + (32,), reg(8, 8, 1) + (33,)])       # off the boundary, on it, one behind it
    # 16 records on ONE context, then a block; the same context on both sides of a step boundary
    c.add([3 | (BIN if k % 3 else 0) for k in range(16)], [reg() + (16,)])
    c.add([300 | (BIN if k % 2 else 0) for k in range(23)], [reg(4, 4) + (10,)])
    # transform_skip_flag records (310 luma, 311 chroma) in front of CABAC_TU_TRANSFORM_SKIP blocks; one block codes the flag itself
    r = run(10); r[4] = 310 | BIN
    c.add(r, [ts() + (5,)])
    r = run(10); r[9] = 311 | BIN; r[2] = 311
    c.add(r, [ts(4, 4, 1) + (10,), ts(16, 16, 0, TS | TS_FLAG) + (10,)])
    r = run(6); r[0] = 310
    c.add(r, [reg(8, 8, 0, TS_FLAG | SH) + (1,), ts(8, 8, 0, TS | H.TU_BDPCM) + (3,)])
    # terminate bins of both values and an align between two blocks
    r = run(14); r[1] = TRM; r[6] = ALIGN; r[12] = TRM | BIN
    c.add(r, [reg() + (3,), reg(4, 4, 1) + (9,)])
    r = run(33); r[16] = ALIGN; r[32] = ALIGN                                             # an align first in a step and last in the run
    c.add(r, [reg(4, 4) + (16,), reg(8, 8) + (32,)])
    # an empty block and a bad descriptor among side records (block numbers noted below)
    first_special = len(c.blocks)
    c.add(run(9), [reg() + (2,), reg() + (4,), reg(4, 4) + (8,)])                         # its middle block is emptied
    c.add(run(9), [reg() + (2,), reg(4, 4) + (2,)])                                       # its first block gets a bad descriptor
    # garbage in d_tu_at: past the end, going backwards
    c.add(run(11), [reg(4, 4) + (9,), reg(4, 4, 1) + (2,), reg(8, 8) + (0xFFFFFFFF,)])
    c.add(run(5), [reg(4, 4) + (0x80000000,), reg(4, 4) + (0,)])
    # no block at all; no side record at all; one 32 x 32 block
    c.add(run(17, ts_flag=1, trm=True), [])
    c.add([], [])
    c.add([], [reg(16, 16) + (0,)])
    c.add(run(3), [reg(32, 32) + (2,)])
    # a run of 100 next to runs of 0
    c.add(run(100, align=True), [reg(4, 4) + (50,)])
    c.add([], [reg(4, 4) + (0,)])
    # and a random tail: 1 .. 3 blocks, runs of 0 .. 40, any raw position
    for _ in range(24):
        n = int(rng.integers(0, 41))
        items = []
        for _ in range(int(rng.integers(1, 4))):
            w, h = [(4, 4), (8, 8), (16, 16), (8, 4), (4, 16)][int(rng.integers(0, 5))]
            if rng.random() < 0.3:
                items.append(ts(w, h, int(rng.integers(0, 2)), TS | [TS_FLAG, H.TU_BDPCM, 0][int(rng.integers(0, 3))]) + (int(rng.integers(0, n + 3)),))
            else:
                items.append(reg(w, h, int(rng.integers(0, 2)), int(rng.integers(0, 8))) + (int(rng.integers(0, n + 3)),))
        c.add(run(n, ts_flag=int(rng.integers(0, 2)), trm=rng.random() < 0.3, align=rng.random() < 0.3), items)
    c.finish(empty=[first_special + 1], bad=[first_special + 3])
    c.sets = make_sets(rng, 3)
    c.which = rng.integers(0, 3, c.n_cand).astype(np.uint32)               # candidates share start sets
    c.n_out = c.n_cand + 2
    c.out_set = np.where(rng.random(c.n_cand) < 0.2, NONE, rng.permutation(c.n_out)[:c.n_cand]).astype(np.uint32)
    c.want = M.estimate_model(c.cand_first, c.blocks, c.tus, c.sets, c.which, c.rec_first, c.records, c.tu_at, c.out_set)
    return c


@pytest.fixture(scope="module")
def parity():
    return _parity_case()


def check_unit(got, want, n_out=0, what=""):
    bits, tub, info, flags, o_state, o_rate = got
    w_bits, w_tub, w_info, w_flags, written = want[:5]
    assert np.array_equal(bits, w_bits), (what, np.nonzero(bits != w_bits)[0][:8])
    assert np.array_equal(tub, w_tub), (what, np.nonzero(tub != w_tub)[0][:8])
    assert np.array_equal(info, w_info) and np.array_equal(flags, w_flags), what
    if n_out:
        o_state, o_rate = o_state.reshape(n_out, 379), o_rate.reshape(n_out, 379)
        for k in range(n_out):
            if k in written:
                assert_sets_equal(o_state[k], o_rate[k], [written[k]], "%s set %d" % (what, k))
            else:
                assert (o_state[k] == SENTINEL32).all() and (o_rate[k] == 0x5A).all(), (what, k)


@pytest.mark.parametrize("int16", [False, True])
def test_model_parity_and_exported_sets(hip, parity, int16):
    """The cases of _parity_case: costs, per-block costs, infos and flags equal the model's; all 379 entries of every written set
    equal the model's, NO_SET candidates write nothing, the guard words around every output are intact; d_out_set == NULL writes
    no set at all."""
    c = parity
    assert np.abs(c.coeff).max() <= 32767 and (np.diff(c.cand_first.astype(np.int64)) == 0).sum() >= 2
    assert int(c.want[2][c.tus["channel"] == 2][0]) == H.TU_INFO_BAD_DESC and (c.want[2] == H.TU_INFO_EMPTY).sum() == 1
    state, rate = pack_sets(c.sets)
    co = c.coeff.astype(np.int16) if int16 else c.coeff
    got = run_unit(hip, c.cand_first, c.tus, co, state, rate, c.which, c.rec_first, c.records, c.tu_at, c.out_set, c.n_out, int16)
    check_unit(got, c.want, c.n_out, "out of place")
    got = run_unit(hip, c.cand_first, c.tus, co, state, rate, c.which, c.rec_first, c.records, c.tu_at, None, 3, int16)
    check_unit(got[:4] + (None, None), c.want, 0, "no sets")
    assert (got[4] == SENTINEL32).all() and (got[5] == 0x5A).all()


def test_sets_in_place(hip, parity):
    """Every candidate owns its start set and some write the set they leave back into it (the in-place rule of cabac_hip_search.h)."""
    c = parity
    rng = np.random.default_rng(0x1A9)
    own = [c.sets[int(w)] for w in c.which]
    state, rate = pack_sets(own)
    out = np.where(rng.random(c.n_cand) < 0.3, NONE, np.arange(c.n_cand)).astype(np.uint32)
    bits, tub, info, flags, s2, r2 = run_unit(hip, c.cand_first, c.tus, c.coeff, state, rate, np.arange(c.n_cand, dtype=np.uint32), c.rec_first,
                                              c.records, c.tu_at, out, c.n_cand, in_place=True)
    check_unit((bits, tub, info, flags, None, None), c.want)
    left = c.want[5]
    assert_sets_equal(s2, r2, [left[k] if out[k] != NONE else own[k] for k in range(c.n_cand)], "in place")


def test_null_positions_put_every_block_behind_the_run(hip, parity):
    c = parity
    state, rate = pack_sets(c.sets)
    want = M.estimate_model(c.cand_first, c.blocks, c.tus, c.sets, c.which, c.rec_first, c.records, None, c.out_set)
    assert not np.array_equal(want[0], c.want[0])
    got = run_unit(hip, c.cand_first, c.tus, c.coeff, state, rate, c.which, c.rec_first, c.records, None, c.out_set, c.n_out)
    check_unit(got, want, c.n_out, "NULL d_tu_at")


def test_rows_of_one_wave_with_very_different_runs_and_clipped_runs(hip):
    """Four candidates — the rows of one wave — with runs of 0, 100, 0 and 100 records; then a d_rec_first that goes backwards
    and past its last entry, which is clipped as the header says."""
    rng = np.random.default_rng(0x0A64)
    c = Case()
    for n in (0, 100, 0, 100):
        c.add(M.side_run(rng, n, ts_flag=0, trm=n > 0, align=n > 0), [(_block(rng, 4, 4), 0, SH, n // 2), (_block(rng, 8, 8), 1, 0, n)])
    c.finish()
    sets = make_sets(rng, 2)
    state, rate = pack_sets(sets)
    which, out_set = np.array([0, 0, 1, 1], np.uint32), np.array([3, 2, 1, 0], np.uint32)
    for rec_first in (c.rec_first, np.array([0, 150, 100, 120, 200], np.uint64), np.array([30, 10, 60, 260, 200], np.uint64)):
        want = M.estimate_model(c.cand_first, c.blocks, c.tus, sets, which, rec_first, c.records, c.tu_at, out_set)
        got = run_unit(hip, c.cand_first, c.tus, c.coeff, state, rate, which, rec_first, c.records, c.tu_at, out_set, 4)
        check_unit(got, want, 4, str(rec_first.tolist()))


# ---------------------------------------------------------------------------------------------- a bad record
def test_a_bad_record_flags_its_candidate_and_nothing_else(hip, parity):
    c = parity
    state, rate = pack_sets(c.sets)
    victim = 4                                                            # three blocks, 40 records
    records = c.records.copy()
    records[int(c.rec_first[victim]) + 20] = M.REC_ALIGN - 1              # CABAC_REC_EST_RESETBITS
    out_set = c.out_set.copy()
    out_set[victim] = NONE
    bits, tub, info, flags, o_state, o_rate = run_unit(hip, c.cand_first, c.tus, c.coeff, state, rate, c.which, c.rec_first, records, c.tu_at,
                                                       out_set, c.n_out)
    want = M.estimate_model(c.cand_first, c.blocks, c.tus, c.sets, c.which, c.rec_first, records, c.tu_at, out_set)
    assert flags[victim] == capi.RES_BAD_RECORD and bits[victim] == U and int(flags.sum()) == capi.RES_BAD_RECORD
    assert want[3][victim] == M.BAD_RECORD and int(want[0][victim]) == U
    mine = np.zeros(len(c.tus), bool)
    mine[int(c.cand_first[victim]):int(c.cand_first[victim + 1])] = True
    tub[mine] = 0                                                          # unspecified for the flagged candidate's own blocks
    check_unit((bits, tub, info, flags, o_state, o_rate), want, c.n_out, "bad record")
    others = np.arange(c.n_cand) != victim
    assert np.array_equal(bits[others], c.want[0][others]) and np.array_equal(tub[~mine], c.want[1][~mine])


# ---------------------------------------------------------------------------------------------- rounds
class UnitRound:
    """The device buffers of one cabac_hip_search_unit_round_device call (outputs filled with sentinels)."""

    def __init__(self, group_first, case, which, out_set, dist):
        import torch
        c = case
        self.n_group, self.n_cand, self.n_tu = len(group_first) - 1, c.n_cand, len(c.tus)
        self.t_gf, self.t_cf, self.t_tu, self.t_co = t_u32(group_first), t_u32(c.cand_first), dev(c.tus, np.uint8), dev(c.coeff)
        self.t_set, self.t_out = t_u32(which), t_u32(out_set) if out_set is not None else None
        self.t_dist = t_u64(dist) if dist is not None else None
        self.t_rf, self.t_rec, self.t_at = t_u64(c.rec_first), t_rec(c.records), t_u32(c.tu_at)
        self.t_bits = torch.full((self.n_cand + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
        self.t_pick = torch.full((self.n_group + 2,), SENTINEL32, dtype=torch.int32, device="cuda")
        self.t_cost = torch.full((self.n_group + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
        self.t_tub = torch.full((self.n_tu + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
        self.t_info = torch.full((self.n_tu + 2,), SENTINEL32, dtype=torch.int32, device="cuda")
        self.t_flags = torch.full((self.n_cand + 2,), SENTINEL32, dtype=torch.int32, device="cuda")

    def enqueue(self, hip, t_state, t_rate, lam):
        hip.search_unit_round_device(self.n_group, self.t_gf.data_ptr(), self.n_cand, self.t_cf.data_ptr(), self.t_tu.data_ptr(),
                                     self.t_co.data_ptr(), t_state.data_ptr(), t_rate.data_ptr(), self.t_set.data_ptr(),
                                     self.t_rf.data_ptr(), self.t_rec.data_ptr(), self.t_at.data_ptr(),
                                     self.t_out.data_ptr() if self.t_out is not None else 0,
                                     self.t_dist.data_ptr() if self.t_dist is not None else 0, lam, self.t_bits.data_ptr() + 8,
                                     self.t_pick.data_ptr() + 4, self.t_cost.data_ptr() + 8, self.t_tub.data_ptr() + 8,
                                     self.t_info.data_ptr() + 4, self.t_flags.data_ptr() + 4)

    def results(self):
        out = []
        for t, dt, s in ((self.t_bits, np.uint64, SENTINEL64), (self.t_pick, np.uint32, SENTINEL32), (self.t_cost, np.uint64, SENTINEL64),
                         (self.t_tub, np.uint64, SENTINEL64), (self.t_info, np.uint32, SENTINEL32), (self.t_flags, np.uint32, SENTINEL32)):
            a = t.cpu().numpy().view(dt)
            assert a[0] == s and a[-1] == s
            out.append(a[1:-1].copy())
        return out


def check_round(got, want, what):
    bits, pick, cost, tub, info, flags = got
    w_bits, w_pick, w_cost, _, w_tub, w_info, _, w_flags = want
    assert np.array_equal(bits, w_bits), what
    assert np.array_equal(pick, w_pick), (what, pick[:8], w_pick[:8])
    assert np.array_equal(cost, w_cost), what
    assert np.array_equal(tub, w_tub) and np.array_equal(info, w_info) and np.array_equal(flags, w_flags), what


def chain_round(rng, n_chain, n_alt):
    """One position of n_chain chains: group k = n_alt alternatives from set k — a side-only one ("all cbf zero"), and 1 .. 2
    blocks inside 0 .. 24 side records, a transform_skip_flag record in front of a transform-skip block."""
    c = Case()
    for k in range(n_chain):
        lone = int(rng.integers(0, n_alt))
        for a in range(n_alt):
            n = int(rng.integers(0, 25))
            if a == lone:
                c.add(M.side_run(rng, n + 1, ts_flag=0), [])
                continue
            run, items = M.side_run(rng, n, trm=rng.random() < 0.2, align=rng.random() < 0.2), []
            for _ in range(int(rng.integers(1, 3))):
                w, h = [(4, 4), (8, 8), (16, 16), (8, 4)][int(rng.integers(0, 4))]
                at = int(rng.integers(0, n + 1))
                if rng.random() < 0.4:
                    if at:
                        run[at - 1] = 310 | BIN
                    items.append((_block(rng, w, h, "ts"), 0, TS, at))
                else:
                    items.append((_block(rng, w, h), int(rng.integers(0, 2)), int(rng.integers(0, 4)), at))
            items.sort(key=lambda it: it[3])
            c.add(run, items)
    c.finish()
    group_first = np.arange(0, n_chain * n_alt + 1, n_alt, dtype=np.uint32)
    which = np.repeat(np.arange(n_chain, dtype=np.uint32), n_alt)
    return c, group_first, which


def test_chains_advance_in_place(hip):
    """K = 8 chains x 4 alternatives x 5 rounds: chain k owns set k; ALL rounds are enqueued on one stream before a single
    synchronise; costs, picks and the final sets (all 379 entries, the side contexts among them) equal the model's."""
    rng = np.random.default_rng(0xC4A2)
    K, R, G = 8, 5, 4
    sets = make_sets(rng, K)
    start = sets
    state, rate = pack_sets(sets)
    t_state, t_rate = dev(state, np.int32), dev(rate)
    lam = int(2.7 * (1 << 16))
    rounds, wants, lone_wins = [], [], 0
    for r in range(R):
        c, gf, which = chain_round(rng, K, G)
        dist = rng.integers(0, 3000, K * G).astype(np.uint64)                # about the spread of lambda * rate
        if r == 2:
            dist[3 * G:4 * G] = U                                          # chain 3 has nothing to pick in round 2: its set stays
        out_set = np.arange(K, dtype=np.uint32)
        rounds.append(UnitRound(gf, c, which, out_set, dist))
        want = M.round_model(gf, c.cand_first, c.blocks, c.tus, sets, which, c.rec_first, c.records, c.tu_at, out_set, dist, lam)
        lone_wins += sum(1 for p in want[1] if int(p) != NONE and c.cand_first[int(p)] == c.cand_first[int(p) + 1])
        sets = want[3]
        wants.append(want)
    for rd in rounds:
        rd.enqueue(hip, t_state, t_rate, lam)
    hip.synchronize()
    for r, (rd, want) in enumerate(zip(rounds, wants)):
        check_round(rd.results(), want, "round %d" % r)
    assert int(wants[2][1][3]) == NONE and 1 <= lone_wins < K * R - 8      # side-only alternatives win, and others do
    assert_sets_equal(t_state.cpu().numpy().view(np.uint32), t_rate.cpu().numpy(), sets, "final sets")
    # the side contexts moved: entries below 86 or in 292..356 of some chain differ from where it started
    side = np.r_[0:86, 292:357]
    assert any(not np.array_equal(a[0][side], b[0][side]) for a, b in zip(sets, start))


# ---------------------------------------------------------------------------------------------- host form
def raw_batch(hip, gf, c, state, rate, which, out_set, dist, lam, rec_first=None, tu_at=None, records=None, n_records=None, n_coeff=None,
              cand_first=None):
    """cabac_hip_search_unit_round_batch with sentinel-filled outputs -> (rc, outputs, state, rate)"""
    gf = np.ascontiguousarray(gf, np.uint32)
    cf = np.ascontiguousarray(c.cand_first if cand_first is None else cand_first, np.uint32)
    tus, coeff = np.ascontiguousarray(c.tus, H.TU_DTYPE), np.ascontiguousarray(c.coeff, np.int32)
    state, rate = np.array(state, np.uint32), np.array(rate, np.uint8)
    which, out_set = np.ascontiguousarray(which, np.uint32), np.ascontiguousarray(out_set, np.uint32)
    records = np.ascontiguousarray(c.records if records is None else records, np.uint16)
    rf = np.ascontiguousarray(c.rec_first if rec_first is None else rec_first, np.uint64)
    at = np.ascontiguousarray(c.tu_at if tu_at is None else tu_at, np.uint32)
    n_group, n_cand = len(gf) - 1, len(which)
    outs = [np.full(n_cand + 1, SENTINEL64, np.uint64), np.full(n_group + 1, SENTINEL32, np.uint32), np.full(n_group + 1, SENTINEL64, np.uint64),
            np.full(len(tus) + 1, SENTINEL64, np.uint64), np.full(len(tus) + 1, SENTINEL32, np.uint32)]
    d = np.ascontiguousarray(dist, np.uint64)
    rc = hip.L.cabac_hip_search_unit_round_batch(hip.h, n_group, gf.ctypes.data, n_cand, cf.ctypes.data, tus.ctypes.data, coeff.ctypes.data, 4,
                                                 len(coeff) if n_coeff is None else n_coeff, state.ctypes.data, rate.ctypes.data,
                                                 len(state) // 379, which.ctypes.data, records.ctypes.data,
                                                 len(records) if n_records is None else n_records, rf.ctypes.data, at.ctypes.data,
                                                 out_set.ctypes.data, d.ctypes.data, lam, *[o.ctypes.data for o in outs])
    return rc, outs, state, rate


def test_host_form(hip):
    """cabac_hip_search_unit_round_batch == the device form (results and the written sets), int32 and int16, with and without
    d_tu_at; every CABAC_HIP_ERR_INVALID case of the header — the existing host form's and the new ones — is refused with every
    output and the sets untouched, and a bad side record is named by candidate and record."""
    rng = np.random.default_rng(0x4058)
    K, G = 6, 4
    c, gf, which = chain_round(rng, K, G)
    sets = make_sets(rng, K + 1)
    state, rate = pack_sets(sets)
    out_set = np.arange(K, dtype=np.uint32)
    dist = rng.integers(0, 500, K * G).astype(np.uint64)
    lam = 7 << 28
    want = M.round_model(gf, c.cand_first, c.blocks, c.tus, sets, which, c.rec_first, c.records, c.tu_at, out_set, dist, lam)
    t_state, t_rate = dev(state, np.int32), dev(rate)
    rd = UnitRound(gf, c, which, out_set, dist)
    rd.enqueue(hip, t_state, t_rate, lam)
    hip.synchronize()
    d_res = rd.results()
    check_round(d_res, want, "device")
    assert_sets_equal(t_state.cpu().numpy().view(np.uint32), t_rate.cpu().numpy(), want[3], "device")
    h_state, h_rate = state.copy(), rate.copy()
    got = hip.search_unit_round_batch(gf, c.cand_first, c.tus, c.coeff, h_state, h_rate, which, c.records, c.rec_first, c.tu_at, out_set, dist,
                                      lam, with_blocks=True)
    for a, b in zip(got, d_res[:5]):
        assert np.array_equal(a, b)
    assert_sets_equal(h_state, h_rate, want[3], "host")
    h_state, h_rate = state.copy(), rate.copy()
    b16, p16, c16 = hip.search_unit_round_batch(gf, c.cand_first, c.tus, c.coeff.astype(np.int16), h_state, h_rate, which, c.records,
                                                c.rec_first, c.tu_at, out_set, dist, lam, int16=True)
    assert np.array_equal(b16, got[0]) and np.array_equal(p16, got[1]) and np.array_equal(c16, got[2])
    assert_sets_equal(h_state, h_rate, want[3], "host int16")
    # tu_at None, no out sets, no distortions: the sets stay
    h_state, h_rate = state.copy(), rate.copy()
    b0, p0, c0 = hip.search_unit_round_batch(gf, c.cand_first, c.tus, c.coeff, h_state, h_rate, which, c.records, c.rec_first, None, None,
                                             None, 1 << 31)
    w0 = M.round_model(gf, c.cand_first, c.blocks, c.tus, sets, which, c.rec_first, c.records, None, None, None, 1 << 31)
    assert np.array_equal(b0, w0[0]) and np.array_equal(p0, w0[1]) and np.array_equal(c0, w0[2])
    assert np.array_equal(h_state, state) and np.array_equal(h_rate, rate)
    # ---- the refusals ----
    cf = c.cand_first
    two = next(k for k in range(K * G) if cf[k + 1] - cf[k] == 2 and c.rec_first[k + 1] - c.rec_first[k] >= 2)   # two blocks, a run
    t0 = int(cf[two])
    n_rec = int(c.rec_first[two + 1] - c.rec_first[two])
    gf_back = gf.copy(); gf_back[2], gf_back[3] = gf[3], gf[2]
    cf_back = cf.copy(); cf_back[4], cf_back[5] = cf[5] + 1, cf[4]
    gf_short = gf.copy(); gf_short[-1] -= 1
    set_big = which.copy(); set_big[5] = K + 1
    out_big = out_set.copy(); out_big[1] = K + 1
    out_dup = out_set.copy(); out_dup[4] = out_set[2]
    out_foreign = out_set.copy(); out_foreign[0] = 3; out_foreign[3] = NONE
    set_foreign = which.copy(); set_foreign[G] = 0
    rf_back = c.rec_first.copy(); rf_back[3], rf_back[4] = rf_back[4] + 1, rf_back[3]
    at_down = c.tu_at.copy(); at_down[t0], at_down[t0 + 1] = n_rec, n_rec - 1
    at_far = c.tu_at.copy(); at_far[t0 + 1] = n_rec + 1
    rec_bad = c.records.copy(); rec_bad[int(c.rec_first[two]) + 1] = 0x1FB | BIN
    rec_379 = c.records.copy(); rec_379[int(c.rec_first[two])] = 379
    refusals = [
        ("group_first", dict(gf=gf_back)), ("cand_first", dict(cand_first=cf_back)), ("n_cand", dict(gf=gf_short)),
        ("set out of range", dict(which=set_big)), ("out set out of range", dict(out_set=out_big)),
        ("coefficients", dict(n_coeff=len(c.coeff) - 1)), ("same out set", dict(out_set=out_dup)),
        ("in-place", dict(out_set=out_foreign)), ("in-place", dict(which=set_foreign)),
        ("rec_first is not non-decreasing", dict(rec_first=rf_back)), ("past n_records_total", dict(n_records=len(c.records) - 1)),
        ("tu_at decreases", dict(tu_at=at_down)), ("tu_at exceeds", dict(tu_at=at_far)),
        ("candidate %d, record 1 " % two, dict(records=rec_bad)), ("candidate %d, record 0 " % two, dict(records=rec_379)),
    ]
    for word, kw in refusals:
        args = dict(gf=gf, which=which, out_set=out_set)
        args.update(kw)
        rc, outs, s, r = raw_batch(hip, args.pop("gf"), c, state, rate, args.pop("which"), args.pop("out_set"), dist, lam, **args)
        msg = hip.L.cabac_hip_last_error(hip.h).decode()
        assert rc == -2 and word in msg, (word, rc, msg)
        assert np.array_equal(s, state) and np.array_equal(r, rate), word
        for o, sentinel in zip(outs, (SENTINEL64, SENTINEL32, SENTINEL64, SENTINEL64, SENTINEL32)):
            assert (o == sentinel).all(), word
    # the same call with nothing wrong runs, and leaves the sentinel behind the outputs alone
    rc, outs, s, r = raw_batch(hip, gf, c, state, rate, which, out_set, dist, lam)
    assert rc == 0 and all(np.array_equal(o[:-1], b) for o, b in zip(outs, d_res[:5]))
    assert [int(o[-1]) for o in outs] == [SENTINEL64, SENTINEL32, SENTINEL64, SENTINEL64, SENTINEL32]
    assert_sets_equal(s, r, want[3], "raw")


# ---------------------------------------------------------------------------------------------- stream contract
def test_stream_contract_on_the_default_stream(parity):
    """With torch's default stream adopted the call needs no torch.cuda.synchronize() before or after: a long fill in front, the
    operands produced on the stream, the results read on the stream."""
    import torch
    assert torch.cuda.current_stream().cuda_stream == 0
    c = parity
    state, rate = pack_sets(c.sets)
    hip = H.gpu_ctx()
    src = [t_u32(c.cand_first), dev(c.tus, np.uint8), dev(c.coeff), dev(state, np.int32), dev(rate), t_u32(c.which), t_u64(c.rec_first),
           t_rec(c.records), t_u32(c.tu_at)]
    for _ in range(3):
        big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
        big.fill_(0xA5)                          # a long fill in front, then the operands are produced ON the stream
        ops = [torch.zeros_like(s) for s in src]
        for o, s in zip(ops, src):
            o.copy_(s)
        t_bits = torch.full((c.n_cand,), SENTINEL64, dtype=torch.int64, device="cuda")
        t_tub = torch.full((len(c.tus),), SENTINEL64, dtype=torch.int64, device="cuda")
        t_flags = torch.full((c.n_cand,), SENTINEL32, dtype=torch.int32, device="cuda")
        hip.estimate_unit_device(c.n_cand, *[o.data_ptr() for o in ops], t_bits.data_ptr(), t_tub.data_ptr(), 0, t_flags.data_ptr())
        assert np.array_equal(t_bits.cpu().numpy().view(np.uint64), c.want[0])
        assert np.array_equal(t_tub.cpu().numpy().view(np.uint64), c.want[1])
        assert not t_flags.cpu().numpy().any()
        del big, ops
    hip.close()
