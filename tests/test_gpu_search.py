"""GPU: the search rounds (include/cabac_hip_search.h; csrc/cabac_search.hip and the exporting variant of the kernel in
csrc/cabac_residual_estimate.hip) against tests/search_model.py, which tests/test_search_model.py pins to the compiled
reference.  Everything is bit-exact: == on integers, no tolerance, no case left out of a comparison.  Every test has its own
bounded input, and nothing is run again after a failure."""

import numpy as np
import pytest

import helpers as H
import search_model as M
from entropy_coding_amd import capi
from test_gpu_residual import SIZES, make_tus
from test_gpu_residual_estimate import SENTINEL32, SENTINEL64, _mixed_kinds, dev, make_sets, pack_sets, run_device

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U = (1 << 64) - 1
LAMBDA_ONE = 1 << 31


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


def unpack_sets(state, rate):
    state, rate = np.asarray(state, np.uint32).reshape(-1, 379), np.asarray(rate, np.uint8).reshape(-1, 379)
    return [((s & 0xFFFF).astype(np.uint16), (s >> 16).astype(np.uint16), r.copy()) for s, r in zip(state, rate)]


def assert_sets_equal(got_state, got_rate, want_sets, what=""):
    want_state, want_rate = pack_sets(want_sets)
    got_state, got_rate = np.asarray(got_state).reshape(-1), np.asarray(got_rate).reshape(-1)
    bad = np.nonzero((got_state != want_state) | (got_rate != want_rate))[0]
    assert len(bad) == 0, (what, len(bad), [(int(k) // 379, int(k) % 379, hex(int(got_state[k])), hex(int(want_state[k])),
                                             int(got_rate[k]), int(want_rate[k])) for k in bad[:8]])


def u64(a):
    return np.asarray(a, np.uint64)


def t_u64(a):
    return dev(u64(a), np.int64)


def t_u32(a):
    import torch
    a = np.asarray(a, np.uint32)
    return dev(a, np.int32) if len(a) else torch.zeros(1, dtype=torch.int32, device="cuda")


def mixed_candidates(rng, n_blocks, max_run):
    """Blocks of every kind (regular, transform skip, BDPCM, TS_FLAG, dependent quantisation, sign hiding, SBT zero-out,
    64-wide), some empty and some with a bad descriptor, cut into candidates of 0 .. max_run blocks."""
    blocks, chromas, flags = _mixed_kinds(rng, n_blocks)
    for k in range(7, n_blocks, 23):
        blocks[k] = np.zeros_like(blocks[k])                  # empty
    tus, coeff = make_tus(blocks, chromas, flags)
    for k in range(11, n_blocks, 29):
        tus[k]["channel"] = 2                                  # bad descriptor
    for k in range(40, n_blocks, 97):
        tus[k]["log2_width"] = 7
    first = [0]
    while first[-1] < n_blocks:
        first.append(min(n_blocks, first[-1] + int(rng.integers(0, max_run + 1))))
    return blocks, tus, coeff, np.asarray(first, np.uint32)


# ---------------------------------------------------------------------------------------------- 1. exported sets
def run_export(hip, cand_first, tus, coeff, state, rate, which, out_set, n_out, int16, pad=2, in_place=False):
    """cabac_hip_estimate_residual_ctx_device; separate output arrays of n_out sets with `pad` sentinel sets on both sides, or
    (in_place) the input arrays.  -> (bits, tu_bits, tu_info, out_state, out_rate)"""
    import torch
    n_cand, n_tu = len(cand_first) - 1, len(tus)
    t_first, t_tu = t_u32(cand_first), dev(tus, np.uint8)
    t_co = dev(np.asarray(coeff, np.int16 if int16 else np.int32))
    t_state, t_rate, t_set, t_out = dev(np.asarray(state, np.uint32), np.int32), dev(np.asarray(rate, np.uint8)), t_u32(which), t_u32(out_set)
    before_state, before_rate = t_state.clone(), t_rate.clone()
    t_bits = torch.full((n_cand + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
    t_tub = torch.full((n_tu + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
    t_info = torch.full((n_tu + 2,), SENTINEL32, dtype=torch.int32, device="cuda")
    if in_place:
        t_os, t_or, off = t_state, t_rate, 0
    else:
        t_os = torch.full(((n_out + 2 * pad) * 379,), SENTINEL32, dtype=torch.int32, device="cuda")
        t_or = torch.full(((n_out + 2 * pad) * 379,), 0x5A, dtype=torch.uint8, device="cuda")
        off = pad * 379
    hip.estimate_residual_ctx_device(n_cand, t_first.data_ptr(), t_tu.data_ptr(), t_co.data_ptr(), t_state.data_ptr(), t_rate.data_ptr(),
                                     t_set.data_ptr(), t_bits.data_ptr() + 8, t_out.data_ptr(), t_os.data_ptr() + 4 * off,
                                     t_or.data_ptr() + off, t_tub.data_ptr() + 8, t_info.data_ptr() + 4, int16=int16)
    hip.synchronize()
    bits, tub, info = t_bits.cpu().numpy().view(np.uint64), t_tub.cpu().numpy().view(np.uint64), t_info.cpu().numpy().view(np.uint32)
    assert bits[0] == SENTINEL64 and bits[-1] == SENTINEL64 and tub[0] == SENTINEL64 and tub[-1] == SENTINEL64
    assert info[0] == SENTINEL32 and info[-1] == SENTINEL32
    os_, or_ = t_os.cpu().numpy().view(np.uint32), t_or.cpu().numpy()
    if not in_place:
        assert torch.equal(t_state, before_state) and torch.equal(t_rate, before_rate)       # the start sets are not modified
        assert (os_[:off] == SENTINEL32).all() and (os_[off + n_out * 379:] == SENTINEL32).all()
        assert (or_[:off] == 0x5A).all() and (or_[off + n_out * 379:] == 0x5A).all()
    return bits[1:-1].copy(), tub[1:-1].copy(), info[1:-1].copy(), os_[off:off + n_out * 379].copy() if not in_place else os_.copy(), \
        or_[off:off + n_out * 379].copy() if not in_place else or_.copy()


@pytest.mark.parametrize("int16", [False, True])
def test_exported_sets(hip, int16):
    """Mixed candidates (0 .. 5 blocks, every kind of block, empty and bad ones): all 379 entries of every written set equal
    the model; NO_SET candidates write nothing (their slots and the padding keep the sentinel); the three cost outputs equal
    cabac_hip_estimate_residual_device's for the same inputs; then the same with the output arrays being the input arrays."""
    rng = np.random.default_rng(0x5E7 + int16)
    blocks, tus, coeff, first = mixed_candidates(rng, 260, 5)
    assert np.abs(coeff).max() <= 32767
    n_cand = len(first) - 1
    assert (np.diff(first.astype(np.int64)) == 0).any()                  # zero-block candidates are in
    sets = make_sets(rng, 5)
    state, rate = pack_sets(sets)
    which = rng.integers(0, 5, n_cand).astype(np.uint32)
    n_out = n_cand + 3
    slots = rng.permutation(n_out)[:n_cand].astype(np.uint32)
    out_set = np.where(rng.random(n_cand) < 0.25, NONE, slots).astype(np.uint32)
    co = coeff.astype(np.int16) if int16 else coeff
    bits, tub, info, o_state, o_rate = run_export(hip, first, tus, co, state, rate, which, out_set, n_out, int16)
    want_bits, want_tub, want_info, written = M.export_model(first, blocks, tus, sets, which, out_set)
    assert np.array_equal(bits, want_bits) and np.array_equal(tub, want_tub) and np.array_equal(info, want_info)
    e_bits, e_tub, e_info = run_device(hip, first, tus, co, state, rate, which, int16=int16)
    assert np.array_equal(bits, e_bits) and np.array_equal(tub, e_tub) and np.array_equal(info, e_info)
    assert len(written) == int((out_set != NONE).sum()) and len(written) >= 20
    o_state, o_rate = o_state.reshape(n_out, 379), o_rate.reshape(n_out, 379)
    for k in range(n_out):
        if k in written:
            assert_sets_equal(o_state[k], o_rate[k], [written[k]], "set %d" % k)
        else:
            assert (o_state[k] == SENTINEL32).all() and (o_rate[k] == 0x5A).all(), k
    # a candidate that leaves its start set behind unchanged (no blocks, or only empty / bad ones) wrote a copy of it
    quiet = [c for c in range(n_cand) if out_set[c] != NONE and
             all(int(info[t]) & (H.TU_INFO_EMPTY | H.TU_INFO_BAD_DESC) for t in range(int(first[c]), int(first[c + 1])))]
    assert quiet
    for c in quiet:
        assert_sets_equal(o_state[out_set[c]], o_rate[out_set[c]], [sets[int(which[c])]], "candidate %d" % c)
    # in place: every candidate owns its start set; some write it back, the others leave it
    own = [sets[int(w)] for w in which]
    state2, rate2 = pack_sets(own)
    out2 = np.where(rng.random(n_cand) < 0.3, NONE, np.arange(n_cand)).astype(np.uint32)
    bits2, tub2, info2, s2, r2 = run_export(hip, first, tus, co, state2, rate2, np.arange(n_cand, dtype=np.uint32), out2, n_cand, int16,
                                            in_place=True)
    assert np.array_equal(bits2, want_bits) and np.array_equal(tub2, want_tub) and np.array_equal(info2, want_info)
    _, _, _, written2 = M.export_model(first, blocks, tus, own, np.arange(n_cand), out2)
    assert_sets_equal(s2, r2, [written2.get(c, own[c]) for c in range(n_cand)], "in place")


# ---------------------------------------------------------------------------------------------- 2. select
def run_select(hip, group_first, frac, dist, lam):
    import torch
    n_group = len(group_first) - 1
    t_first, t_frac = t_u32(group_first), t_u64(frac)
    t_dist = t_u64(dist) if dist is not None else None
    t_pick = torch.full((n_group + 2,), SENTINEL32, dtype=torch.int32, device="cuda")
    t_cost = torch.full((n_group + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
    hip.search_select_device(n_group, t_first.data_ptr(), t_frac.data_ptr(), t_dist.data_ptr() if t_dist is not None else 0, lam,
                             t_pick.data_ptr() + 4, t_cost.data_ptr() + 8)
    hip.synchronize()
    pick, cost = t_pick.cpu().numpy().view(np.uint32), t_cost.cpu().numpy().view(np.uint64)
    assert pick[0] == SENTINEL32 and pick[-1] == SENTINEL32 and cost[0] == SENTINEL64 and cost[-1] == SENTINEL64
    return pick[1:-1].copy(), cost[1:-1].copy()


def test_select(hip):
    """Random groups of 0, 1, 2, 15, 16, 17, 33 and several thousand candidates; ties (few distinct costs), excluded
    candidates, all-excluded groups, NULL d_dist, costs that saturate, lambda from 0 to 2^64 - 1."""
    rng = np.random.default_rng(0x5E1EC7)
    sizes = [0, 1, 17, 4097, 0, 2, 16, 15, 33, 6000, 1, 0] + [int(s) for s in rng.integers(0, 40, 200)]
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(first[-1])
    small = rng.integers(0, 4, n).astype(np.uint64)                                   # ties everywhere
    wide = rng.integers(0, 1 << 62, n, dtype=np.uint64) >> rng.integers(0, 62, n).astype(np.uint64)
    huge = (np.uint64(U) - rng.integers(0, 3, n).astype(np.uint64))                   # frac bits near 2^64: saturation
    dist_small = rng.integers(0, 3, n).astype(np.uint64)
    dist_wide = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2)
    dist_excl = np.where(rng.random(n) < 0.3, np.uint64(U), dist_small)
    for g in (3, 8, 20, 21):                                                          # whole groups excluded (one of them large)
        dist_excl[int(first[g]):int(first[g + 1])] = U
    dist_near = np.uint64(U) - np.uint64(1) - rng.integers(0, 3, n).astype(np.uint64)  # sums that pass 2^64 - 2
    cases = [(small, None, LAMBDA_ONE), (small, dist_small, LAMBDA_ONE), (wide, None, LAMBDA_ONE), (wide, dist_wide, 12345678901),
             (small, dist_excl, LAMBDA_ONE), (wide, dist_excl, (1 << 31) - 1), (huge, None, LAMBDA_ONE), (huge, dist_small, U),
             (wide, dist_near, 3 << 30), (small, dist_near, LAMBDA_ONE), (wide, dist_wide, 0), (wide, None, 1), (wide, dist_excl, 1 << 47)]
    for k, (frac, dist, lam) in enumerate(cases):
        pick, cost = run_select(hip, first, frac, dist, lam)
        want_pick, want_cost = M.select(first, frac, dist, lam)
        assert np.array_equal(pick, want_pick), (k, np.nonzero(pick != want_pick)[0][:8])
        assert np.array_equal(cost, want_cost), (k, np.nonzero(cost != want_cost)[0][:8])
    assert (want_pick == NONE).sum() >= 7
    # a group_first that goes backwards or past its last entry is clipped; no groups is fine
    bent = np.array([0, 9, 2, 3], np.uint32)
    pick, cost = run_select(hip, bent, small[:4], None, LAMBDA_ONE)
    want_pick, want_cost = M.select(bent, small[:4], None, LAMBDA_ONE)
    assert np.array_equal(pick, want_pick) and np.array_equal(cost, want_cost)
    hip.search_select_device(0, 0, 0, 0, LAMBDA_ONE, 0, 0)


# ---------------------------------------------------------------------------------------------- 3. rounds
class Round:
    """The device buffers of one cabac_hip_search_round_device call (outputs filled with sentinels)."""

    def __init__(self, group_first, cand_first, tus, coeff, which, out_set, dist, int16=False):
        import torch
        self.n_group, self.n_cand, self.n_tu = len(group_first) - 1, len(cand_first) - 1, len(tus)
        self.int16 = int16
        self.t_gf, self.t_cf = t_u32(group_first), t_u32(cand_first)
        self.t_tu = dev(tus, np.uint8) if self.n_tu else torch.zeros(16, dtype=torch.uint8, device="cuda")
        self.t_co = dev(np.asarray(coeff, np.int16 if int16 else np.int32))
        self.t_set = t_u32(which)
        self.t_out = t_u32(out_set) if out_set is not None else None
        self.t_dist = t_u64(dist) if dist is not None and len(dist) else None
        self.t_bits = torch.full((self.n_cand + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
        self.t_pick = torch.full((self.n_group + 2,), SENTINEL32, dtype=torch.int32, device="cuda")
        self.t_cost = torch.full((self.n_group + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
        self.t_tub = torch.full((self.n_tu + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
        self.t_info = torch.full((self.n_tu + 2,), SENTINEL32, dtype=torch.int32, device="cuda")

    def enqueue(self, hip, t_state, t_rate, lam):
        hip.search_round_device(self.n_group, self.t_gf.data_ptr(), self.n_cand, self.t_cf.data_ptr(), self.t_tu.data_ptr(),
                                self.t_co.data_ptr(), t_state.data_ptr(), t_rate.data_ptr(), self.t_set.data_ptr(),
                                self.t_out.data_ptr() if self.t_out is not None else 0,
                                self.t_dist.data_ptr() if self.t_dist is not None else 0, lam, self.t_bits.data_ptr() + 8,
                                self.t_pick.data_ptr() + 4, self.t_cost.data_ptr() + 8, self.t_tub.data_ptr() + 8,
                                self.t_info.data_ptr() + 4, int16=self.int16)

    def results(self):
        out = []
        for t, dt, s in ((self.t_bits, np.uint64, SENTINEL64), (self.t_pick, np.uint32, SENTINEL32), (self.t_cost, np.uint64, SENTINEL64),
                         (self.t_tub, np.uint64, SENTINEL64), (self.t_info, np.uint32, SENTINEL32)):
            a = t.cpu().numpy().view(dt)
            assert a[0] == s and a[-1] == s
            out.append(a[1:-1].copy())
        return out


def check_round(got, want, what):
    bits, pick, cost, tub, info = got
    w_bits, w_pick, w_cost, _, w_tub, w_info, _ = want
    assert np.array_equal(bits, w_bits), what
    assert np.array_equal(pick, w_pick), (what, pick[:8], w_pick[:8])
    assert np.array_equal(cost, w_cost), what
    assert np.array_equal(tub, w_tub) and np.array_equal(info, w_info), what


def some_kinds(rng, n):
    """n blocks drawn from one _mixed_kinds cycle (transform skip, SBT zero-out, regular)."""
    b, c, f = _mixed_kinds(rng, 5)
    idx = rng.permutation(5)[:n]
    return [b[i] for i in idx], [c[i] for i in idx], [f[i] for i in idx]


def chain_round(rng, n_chain, n_alt, kinds):
    """One position of n_chain chains: group k = n_alt alternatives of 1 .. 2 blocks, all started from set k, out set k."""
    blocks, chromas, flags, first = [], [], [], [0]
    for k in range(n_chain):
        for a in range(n_alt):
            b, c, f = kinds(rng, int(rng.integers(1, 3)))
            blocks += b; chromas += c; flags += f
            first.append(len(blocks))
    tus, coeff = make_tus(blocks, chromas, flags)
    group_first = np.arange(0, n_chain * n_alt + 1, n_alt, dtype=np.uint32)
    which = np.repeat(np.arange(n_chain, dtype=np.uint32), n_alt)
    return blocks, tus, coeff, group_first, np.asarray(first, np.uint32), which


def test_chains_advance_in_place(hip):
    """K chains x R rounds: chain k owns set k, its group's candidates start from it and the winner's contexts are written back
    into it.  ALL rounds are enqueued before a single synchronise; picks, costs and the final sets equal the model's."""
    rng = np.random.default_rng(0xC4A1)
    K, R, G = 7, 6, 3
    sets = make_sets(rng, K)
    state, rate = pack_sets(sets)
    t_state, t_rate = dev(state, np.int32), dev(rate)
    lam = int(2.7 * (1 << 16))                                         # 2.7 distortion units per bit
    rounds, wants = [], []
    for r in range(R):
        blocks, tus, coeff, gf, cf, which = chain_round(rng, K, G, some_kinds)
        dist = rng.integers(0, 200, K * G).astype(np.uint64)
        if r == 2:
            dist[3 * G:4 * G] = U                                      # chain 3 has nothing to pick in round 2: its set stays
        out_set = np.arange(K, dtype=np.uint32)
        rounds.append(Round(gf, cf, tus, coeff, which, out_set, dist))
        want = M.round_model(gf, cf, blocks, tus, sets, which, out_set, dist, lam)
        sets = want[3]
        wants.append(want)
    for rd in rounds:
        rd.enqueue(hip, t_state, t_rate, lam)
    hip.synchronize()
    for r, (rd, want) in enumerate(zip(rounds, wants)):
        check_round(rd.results(), want, "round %d" % r)
    assert int(wants[2][1][3]) == NONE
    assert len({int(p) % G for w in wants for p in w[1] if int(p) != NONE}) == G       # every alternative wins somewhere
    assert_sets_equal(t_state.cpu().numpy().view(np.uint32), t_rate.cpu().numpy(), sets, "final sets")


def test_groups_share_a_start_set_and_write_distinct_sets(hip):
    """Several groups read ONE shared set (which no group writes) and write distinct out sets; a group without an out set and
    a NULL d_dist; int16 coefficients."""
    rng = np.random.default_rng(0x54A2ED)
    n_group, G = 9, 4
    blocks, tus, coeff, gf, cf, _ = chain_round(rng, n_group, G, some_kinds)
    assert np.abs(coeff).max() <= 32767
    sets = make_sets(rng, 2) + [(np.zeros(379, np.uint16), np.zeros(379, np.uint16), np.zeros(379, np.uint8))] * n_group
    which = np.zeros(n_group * G, np.uint32)
    which[G:2 * G] = 1                                               # group 1 starts from the other shared set
    out_set = (2 + np.arange(n_group)).astype(np.uint32)
    out_set[4] = NONE
    for dist, int16 in ((None, False), (rng.integers(0, 1 << 40, n_group * G).astype(np.uint64), True)):
        state, rate = pack_sets(sets)
        t_state, t_rate = dev(state, np.int32), dev(rate)
        rd = Round(gf, cf, tus, coeff.astype(np.int16) if int16 else coeff, which, out_set, dist, int16=int16)
        rd.enqueue(hip, t_state, t_rate, 5 << 29)
        hip.synchronize()
        want = M.round_model(gf, cf, blocks, tus, sets, which, out_set, dist, 5 << 29)
        check_round(rd.results(), want, "shared")
        assert_sets_equal(t_state.cpu().numpy().view(np.uint32), t_rate.cpu().numpy(), want[3], "shared")
        assert want[3][2 + 4] is sets[2 + 4] and want[3][0] is sets[0]
    # no out sets at all: the round is estimate + select, the sets are not modified
    state, rate = pack_sets(sets)
    t_state, t_rate = dev(state, np.int32), dev(rate)
    rd = Round(gf, cf, tus, coeff, which, None, None)
    rd.enqueue(hip, t_state, t_rate, LAMBDA_ONE)
    hip.synchronize()
    check_round(rd.results(), M.round_model(gf, cf, blocks, tus, sets, which, None, None, LAMBDA_ONE), "no out sets")
    assert np.array_equal(t_state.cpu().numpy().view(np.uint32), state) and np.array_equal(t_rate.cpu().numpy(), rate)


# ---------------------------------------------------------------------------------------------- 4. host form
def raw_batch(hip, group_first, cand_first, tus, coeff, state, rate, which, out_set, dist, lam, n_coeff=None):
    """cabac_hip_search_round_batch with sentinel-filled outputs -> (rc, outputs, state, rate)"""
    gf, cf = np.ascontiguousarray(group_first, np.uint32), np.ascontiguousarray(cand_first, np.uint32)
    tus, coeff = np.ascontiguousarray(tus, H.TU_DTYPE), np.ascontiguousarray(coeff, np.int32)
    state, rate = np.array(state, np.uint32), np.array(rate, np.uint8)
    which, out_set = np.ascontiguousarray(which, np.uint32), np.ascontiguousarray(out_set, np.uint32)
    n_group, n_cand = len(gf) - 1, len(which)
    outs = [np.full(n_cand + 1, SENTINEL64, np.uint64), np.full(n_group + 1, SENTINEL32, np.uint32), np.full(n_group + 1, SENTINEL64, np.uint64),
            np.full(len(tus) + 1, SENTINEL64, np.uint64), np.full(len(tus) + 1, SENTINEL32, np.uint32)]
    d = None if dist is None else np.ascontiguousarray(dist, np.uint64)
    rc = hip.L.cabac_hip_search_round_batch(hip.h, n_group, gf.ctypes.data, n_cand, cf.ctypes.data, tus.ctypes.data, coeff.ctypes.data, 4,
                                            len(coeff) if n_coeff is None else n_coeff, state.ctypes.data, rate.ctypes.data,
                                            len(state) // 379, which.ctypes.data, out_set.ctypes.data,
                                            d.ctypes.data if d is not None else None, lam, *[o.ctypes.data for o in outs])
    return rc, outs, state, rate


def test_host_form(hip):
    """cabac_hip_search_round_batch == the device form (results and the written sets); every CABAC_HIP_ERR_INVALID case of the
    header is refused with every output and the sets untouched; an in-place violation is named in cabac_hip_last_error; an
    empty block gives CABAC_HIP_ERR_SUBSTREAM with the numbers still arriving."""
    rng = np.random.default_rng(0x4057)
    K, G = 6, 3
    blocks, tus, coeff, gf, cf, which = chain_round(rng, K, G, some_kinds)
    sets = make_sets(rng, K + 1)
    state, rate = pack_sets(sets)
    out_set = np.arange(K, dtype=np.uint32)
    dist = rng.integers(0, 500, K * G).astype(np.uint64)
    lam = 7 << 28
    want = M.round_model(gf, cf, blocks, tus, sets, which, out_set, dist, lam)
    # device form
    t_state, t_rate = dev(state, np.int32), dev(rate)
    rd = Round(gf, cf, tus, coeff, which, out_set, dist)
    rd.enqueue(hip, t_state, t_rate, lam)
    hip.synchronize()
    d_res = rd.results()
    check_round(d_res, want, "device")
    # host form through the binding: state / rate updated in place
    h_state, h_rate = state.copy(), rate.copy()
    bits, pick, cost, tub, info = hip.search_round_batch(gf, cf, tus, coeff, h_state, h_rate, which, out_set, dist, lam, with_blocks=True)
    for a, b in zip((bits, pick, cost, tub, info), d_res):
        assert np.array_equal(a, b)
    assert np.array_equal(h_state, t_state.cpu().numpy().view(np.uint32)) and np.array_equal(h_rate, t_rate.cpu().numpy())
    assert_sets_equal(h_state, h_rate, want[3], "host")
    h_state, h_rate = state.copy(), rate.copy()
    b16, p16, c16 = hip.search_round_batch(gf, cf, tus, coeff.astype(np.int16), h_state, h_rate, which, out_set, dist, lam, int16=True)
    assert np.array_equal(b16, bits) and np.array_equal(p16, pick) and np.array_equal(c16, cost)
    assert_sets_equal(h_state, h_rate, want[3], "host int16")
    # NULL out sets / distortions; nothing to do
    h_state, h_rate = state.copy(), rate.copy()
    b0, p0, c0 = hip.search_round_batch(gf, cf, tus, coeff, h_state, h_rate, which, None, None, LAMBDA_ONE)
    w0 = M.round_model(gf, cf, blocks, tus, sets, which, None, None, LAMBDA_ONE)
    assert np.array_equal(b0, w0[0]) and np.array_equal(p0, w0[1]) and np.array_equal(c0, w0[2])
    assert np.array_equal(h_state, state) and np.array_equal(h_rate, rate)
    assert [len(a) for a in hip.search_round_batch([0], [0], tus[:0], coeff, h_state, h_rate, [], [], [], lam)] == [0, 0, 0]
    # ---- the refusals ----
    gf_back = gf.copy(); gf_back[2], gf_back[3] = gf[3], gf[2]
    cf_back = cf.copy(); cf_back[4], cf_back[5] = cf[5] + 1, cf[4]
    gf_short = gf.copy(); gf_short[-1] -= 1
    set_big = which.copy(); set_big[5] = K + 1
    out_big = out_set.copy(); out_big[1] = K + 1
    out_dup = out_set.copy(); out_dup[4] = out_set[2]
    out_foreign = out_set.copy(); out_foreign[0] = 3; out_foreign[3] = NONE        # group 0 writes the set group 3 starts from
    set_foreign = which.copy(); set_foreign[G] = 0                                  # a candidate of group 1 starts from group 0's out set
    refusals = [
        ("group_first", (gf_back, cf, tus, coeff, state, rate, which, out_set, dist, lam), {}),
        ("cand_first", (gf, cf_back, tus, coeff, state, rate, which, out_set, dist, lam), {}),
        ("n_cand", (gf_short, cf, tus, coeff, state, rate, which, out_set, dist, lam), {}),
        ("set out of range", (gf, cf, tus, coeff, state, rate, set_big, out_set, dist, lam), {}),
        ("out set out of range", (gf, cf, tus, coeff, state, rate, which, out_big, dist, lam), {}),
        ("coefficients", (gf, cf, tus, coeff, state, rate, which, out_set, dist, lam), {"n_coeff": len(coeff) - 1}),
        ("same out set", (gf, cf, tus, coeff, state, rate, which, out_dup, dist, lam), {}),
        ("in-place", (gf, cf, tus, coeff, state, rate, which, out_foreign, dist, lam), {}),
        ("in-place", (gf, cf, tus, coeff, state, rate, set_foreign, out_set, dist, lam), {}),
    ]
    for word, args, kw in refusals:
        rc, outs, s, r = raw_batch(hip, *args, **kw)
        msg = hip.L.cabac_hip_last_error(hip.h).decode()
        assert rc == -2 and word in msg, (word, rc, msg)
        assert np.array_equal(s, state) and np.array_equal(r, rate), word
        for o, sentinel in zip(outs, (SENTINEL64, SENTINEL32, SENTINEL64, SENTINEL64, SENTINEL32)):
            assert (o == sentinel).all(), word
    # the same call with nothing wrong runs, and leaves the sentinel behind the outputs alone
    rc, outs, s, r = raw_batch(hip, gf, cf, tus, coeff, state, rate, which, out_set, dist, lam)
    assert rc == 0 and all(np.array_equal(o[:-1], b) for o, b in zip(outs, d_res))
    assert [int(o[-1]) for o in outs] == [SENTINEL64, SENTINEL32, SENTINEL64, SENTINEL64, SENTINEL32]
    assert_sets_equal(s, r, want[3], "raw")
    # an empty block: CABAC_HIP_ERR_SUBSTREAM, and with check=False the numbers still arrive
    blocks2 = list(blocks); blocks2[1] = np.zeros_like(blocks[1])
    tus2, coeff2 = make_tus(blocks2, [int(t["channel"]) for t in tus], [int(t["flags"]) for t in tus])
    with pytest.raises(capi.CabacHipError) as e:
        hip.search_round_batch(gf, cf, tus2, coeff2, state.copy(), rate.copy(), which, out_set, dist, lam)
    assert e.value.status == -5
    h_state, h_rate = state.copy(), rate.copy()
    got = hip.search_round_batch(gf, cf, tus2, coeff2, h_state, h_rate, which, out_set, dist, lam, with_blocks=True, check=False)
    want2 = M.round_model(gf, cf, blocks2, tus2, sets, which, out_set, dist, lam)
    check_round(got, want2, "with an empty block")
    assert_sets_equal(h_state, h_rate, want2[3], "with an empty block")
    assert int(got[4][1]) == H.TU_INFO_EMPTY


# ---------------------------------------------------------------------------------------------- 5. random sweep
def _sweep_kinds(rng, n):
    """n blocks of random geometry (test_gpu_residual.SIZES) and flags; three in ten are transform-skip blocks of the sizes
    test_gpu_residual_estimate._mixed_kinds uses for them."""
    blocks, chromas, flags = [], [], []
    for _ in range(n):
        w, h = SIZES[int(rng.integers(0, len(SIZES)))]
        fl = int(rng.integers(0, 8))
        if rng.random() < 0.3:
            w, h = [(1, 4), (4, 4), (8, 8), (16, 16), (32, 32), (2, 16), (32, 4), (8, 2)][int(rng.integers(0, 8))]
            c = rng.integers(-4, 5, (h, w)).astype(np.int32) * (rng.random((h, w)) < rng.choice([0.2, 0.8]))
            if not c.any():
                c[h - 1, w - 1] = -1
            fl = (fl & 3) | H.TU_TRANSFORM_SKIP | [H.TU_TS_FLAG, H.TU_BDPCM, 0][int(rng.integers(0, 3))]
            blocks.append(c.astype(np.int32))
        else:
            if max(w, h) > 32:
                fl &= ~H.TU_TS_FLAG
            blocks.append(H.random_block(rng, w, h, density=float(rng.choice([0.1, 0.5, 1.0])), big=0.1))
        chromas.append(int(rng.integers(0, 2)))
        flags.append(fl)
    return blocks, chromas, flags


def test_random_sweep_of_small_rounds(hip):
    """240 small rounds from a fixed seed: random geometry and flags, 1 .. 4 groups of 0 .. 4 candidates of 0 .. 2 blocks,
    group g owning set g (its candidates start from it or from one of two shared sets; its out set is g or none), random
    distortions with exclusions and a random lambda.  Each round continues from the sets the round before left."""
    rng = np.random.default_rng(0x5EED5EA2)
    n_own, n_shared = 4, 2
    sets = make_sets(rng, n_own + n_shared)
    state, rate = pack_sets(sets)
    t_state, t_rate = dev(state, np.int32), dev(rate)
    n_pick = 0
    for k in range(240):
        n_group = int(rng.integers(1, n_own + 1))
        sizes = rng.integers(0, 5, n_group)
        gf = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        n_cand = int(gf[-1])
        runs = rng.integers(0, 3, n_cand)
        cf = np.concatenate([[0], np.cumsum(runs)]).astype(np.uint32)
        blocks, chromas, flags = _sweep_kinds(rng, int(cf[-1]))
        tus, coeff = make_tus(blocks, chromas, flags)
        owner = np.repeat(np.arange(n_group), sizes)
        which = np.where(rng.random(n_cand) < 0.7, owner, n_own + rng.integers(0, n_shared, n_cand)).astype(np.uint32)
        out_set = np.where(rng.random(n_group) < 0.8, np.arange(n_group), NONE).astype(np.uint32)
        dist = np.where(rng.random(n_cand) < 0.15, np.uint64(U), rng.integers(0, 3000, n_cand).astype(np.uint64))
        lam = int(rng.integers(0, 1 << 20)) << int(rng.integers(0, 16))
        rd = Round(gf, cf, tus, coeff, which, out_set, dist if k % 5 else None)
        rd.enqueue(hip, t_state, t_rate, lam)
        hip.synchronize()
        want = M.round_model(gf, cf, blocks, tus, sets, which, out_set, dist if k % 5 else None, lam)
        check_round(rd.results(), want, "round %d" % k)
        sets = want[3]
        assert_sets_equal(t_state.cpu().numpy().view(np.uint32), t_rate.cpu().numpy(), sets, "round %d" % k)
        n_pick += int((want[1] != NONE).sum())
    assert n_pick >= 300
