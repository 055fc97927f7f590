"""GPU: probe points across spliced blocks (include/cabac_hip_probe.h, part 3) — cabac_hip_encode_residual_probes_device / _batch.
The expanded string of every substream is built here from the oracle's residual_records of each block spliced at its `at`; the
value of a probe (k, m) is the oracle's written bits (flags=4) of the part of that string in front of the point.  Payload,
offsets, results, tu_info and bin_counts are compared byte for byte with cabac_hip_encode_residual_device on the same input."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
from entropy_coding_amd import capi
from test_gpu_residual_estimate import block_records

pytestmark = pytest.mark.gpu

W = capi.BIN_COUNT_WORDS
N_HOST = [12, 30, 25, 40, 18, 50]
# per substream the `at` of its blocks: none; one in the middle; two at ONE position; at 0, inside and at n_records; ...
ATS = [[], [7], [10, 10], [0, 7, 40], [0, 0, 9, 18], [3, 3, 9, 50, 50]]
SHAPES = [(4, 4), (8, 8), (16, 4)]
UPPER = 0xFFFFFFFF


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@functools.lru_cache(None)
def case():
    rng = np.random.default_rng(4800)
    sides = [H.random_records(rng, n, ctx_frac=0.7, end_trm=False) for n in N_HOST]
    blocks, tus, splices, first = [], [], [], [0]
    off = 0
    for s, ats in enumerate(ATS):
        for at in ats:
            t = len(blocks)
            w, h = SHAPES[t % 3]
            c = H.random_block(rng, w, h, density=0.5, big=0.1)
            flags = int(rng.integers(0, 4))
            if t == 4:
                flags = H.TU_TRANSFORM_SKIP                      # one transform-skip block
            if t == 8:
                c = np.zeros((h, w), np.int32)                   # one empty block: it contributes no records
            d = np.zeros(1, H.TU_DTYPE)[0]
            d["coeff_offset"], d["log2_width"], d["log2_height"], d["flags"] = off, int(np.log2(w)), int(np.log2(h)), flags
            off += w * h
            blocks.append(c)
            tus.append(d)
            splices.append((at, t))
        first.append(len(blocks))
    tus = np.array(tus, H.TU_DTYPE)
    got = [block_records(blocks, tus, t) for t in range(len(blocks))]
    recs, info = [g[0] for g in got], np.array([g[1] for g in got], np.uint32)
    assert info[8] == H.TU_INFO_EMPTY and recs[8] is None and all(r is not None for t, r in enumerate(recs) if t != 8)
    strings = []
    for s, ats in enumerate(ATS):
        parts = []
        for i in range(N_HOST[s] + 1):
            parts += [recs[first[s] + j] for j, at in enumerate(ats) if at == i and recs[first[s] + j] is not None]
            if i < N_HOST[s]:
                parts.append(sides[s][i:i + 1])
        strings.append(np.concatenate(parts + [np.zeros(0, np.uint16)]).astype(np.uint16))
    qp, init = rng.integers(20, 45, len(ATS)), rng.integers(0, 3, len(ATS))
    desc, _ = H.make_desc(N_HOST, qp, init, H.SUB_FINISH | H.SUB_ALIGN_RBSP)
    desc["byte_offset"] = 0
    desc["byte_capacity"] = 0                                    # ignored by the calls
    coeff = np.concatenate([b.reshape(-1) for b in blocks]).astype(np.int32)
    return dict(desc=desc, records=np.concatenate(sides).astype(np.uint16), first=np.array(first, np.uint32),
                splices=np.array(splices, capi.SPLICE_DTYPE), tus=tus, coeff=coeff, recs=recs, info=info, strings=strings, qp=qp, init=init)


def probe_pairs(with_splice):
    """Per substream, in ascending order: k = 0, every position that has blocks, the end and beyond it — at the lower and at the
    upper end of the position when the splice counts are given (lower: #{at < k}; upper: 0xFFFFFFFF, clipped to #{at <= k}), each
    k twice otherwise (NULL: the upper end everywhere)."""
    first, at, sp = [0], [], []
    for s, ats in enumerate(ATS):
        n = N_HOST[s]
        for k in sorted(set([0, n, n + 5] + ats)):
            at += [k, k]
            # (beyond the end both are the upper end: clipped to k = n, a lower end there would step back behind the pair in front)
            sp += [sum(1 for a in ats if a < k) if k <= n else UPPER, UPPER]
        first.append(len(at))
    return np.array(first, np.uint32), np.array(at, np.uint32), (np.array(sp, np.uint32) if with_splice else None)


def expected_bits(C, first, at, sp):
    orc = H.load_oracle()
    out = []
    for s, ats in enumerate(ATS):
        n = N_HOST[s]
        for p in range(int(first[s]), int(first[s + 1])):
            k = min(int(at[p]), n)
            lo, hi = sum(1 for a in ats if a < k), sum(1 for a in ats if a <= k)
            m = hi if sp is None else min(max(int(sp[p]), lo), hi)
            idx = k + sum(len(r) for r in C["recs"][int(C["first"][s]):int(C["first"][s]) + m] if r is not None)
            out.append(orc.encode_records(C["strings"][s][:idx], int(C["qp"][s]), int(C["init"][s]) & 3, flags=4)[1])
    return np.array(out, np.uint32)


class Call:
    """The device arguments of one spliced call and its outputs between guard words."""

    def __init__(self, C, total=8192):
        self.n_sub, self.n_tu, self.total = len(C["desc"]), len(C["tus"]), total
        self.t = [dev(C["desc"]), dev(np.concatenate([C["records"], np.zeros(8, np.uint16)])), dev(C["first"]), dev(C["splices"]),
                  dev(C["tus"]), dev(C["coeff"])]
        self.t_pay = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        self.t_off = torch.full((self.n_sub + 2,), -1, dtype=torch.int64, device="cuda")
        self.t_res = torch.full((2 * self.n_sub + 2,), -1, dtype=torch.int32, device="cuda")
        self.t_info = torch.full((self.n_tu + 2,), -1, dtype=torch.int32, device="cuda")
        self.t_cnt = torch.full((self.n_sub * W + 1,), -1, dtype=torch.int32, device="cuda")

    def head(self):
        p = [x.data_ptr() for x in self.t]
        return (self.n_sub, p[0], p[1], p[2], p[3], self.n_tu, self.n_tu, p[4], p[5], self.t_pay.data_ptr(), self.total + 64,
                self.t_off.data_ptr(), self.t_res.data_ptr())

    def read(self):
        return [x.cpu().numpy().copy() for x in (self.t_pay, self.t_off, self.t_res, self.t_info, self.t_cnt)]


def run_plain(hip, C):
    c = Call(C)
    hip.encode_residual_device(*c.head(), c.t_info.data_ptr(), c.t_cnt.data_ptr())
    hip.synchronize()
    return c.read()


def run_probes(hip, C, first, at, sp):
    c = Call(C)
    t_first, t_at, t_sp = dev(first), dev(at), (dev(sp) if sp is not None else None)
    t_bits = torch.full((len(at) + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    hip.encode_residual_probes_device(*c.head(), t_first.data_ptr(), t_at.data_ptr(), len(at), t_bits.data_ptr() + 32,
                                      d_probe_splice=t_sp.data_ptr() if t_sp is not None else 0, d_tu_info=c.t_info.data_ptr(),
                                      d_bin_counts=c.t_cnt.data_ptr())
    hip.synchronize()
    bits = t_bits.cpu().numpy().view(np.uint32)
    assert (bits[:8] == 0x5A5A5A5A).all() and (bits[8 + len(at):] == 0x5A5A5A5A).all(), "guard words"
    return c.read(), bits[8:8 + len(at)]


@pytest.mark.parametrize("with_splice", [False, True], ids=["upper-end", "given"])
def test_probes_of_a_spliced_call_against_the_oracle_and_the_plain_call(hip, with_splice):
    C = case()
    first, at, sp = probe_pairs(with_splice)
    want = expected_bits(C, first, at, sp)
    plain = run_plain(hip, C)
    outs, bits = run_probes(hip, C, first, at, sp)
    assert np.array_equal(bits, want), (bits, want)
    for a, b in zip(plain, outs):                                # payload, offsets, results, tu_info, bin_counts and their guards
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # what the plain call itself gives is the oracle's: n_bits of the finished expanded strings, the info words
    orc = H.load_oracle()
    res = plain[2][:2 * len(ATS)].view(H.RESULT_DTYPE)
    assert not res["flags"].any()
    assert [int(v) for v in res["n_bits"]] == [orc.encode_records(s, int(C["qp"][i]), int(C["init"][i]) & 3, 3)[1]
                                               for i, s in enumerate(C["strings"])]
    assert np.array_equal(plain[3][:len(C["tus"])].view(np.uint32), C["info"])
    if with_splice:                                               # the lower and the upper end differ where a position has blocks
        assert (want[0::2] != want[1::2]).any()
    # a call with no probe at all is the plain call too
    outs0, bits0 = run_probes(hip, C, np.zeros(len(ATS) + 1, np.uint32), np.zeros(0, np.uint32), None)
    assert len(bits0) == 0
    for a, b in zip(plain, outs0):
        assert np.array_equal(a, b)


def test_the_host_pointer_form(hip):
    C = case()
    first, at, sp = probe_pairs(True)
    payload = np.zeros(8192, np.uint8)
    off, res, bits, info, cnt = hip.encode_residual_probes_batch(C["desc"], C["records"], C["first"], C["splices"], C["tus"], C["coeff"], payload,
                                                                 first, at, sp, check=False, with_info=True, with_counts=True)
    assert np.array_equal(bits, expected_bits(C, first, at, sp))
    pay2 = np.zeros(8192, np.uint8)
    off2, res2, info2, cnt2 = hip.encode_batch_residual(C["desc"], C["records"], C["first"], C["splices"], C["tus"], C["coeff"], pay2, check=False,
                                                        with_info=True, with_counts=True)
    assert np.array_equal(off, off2) and np.array_equal(res, res2) and np.array_equal(info, info2) and np.array_equal(cnt, cnt2)
    assert np.array_equal(payload, pay2)
    bad = at.copy()
    bad[int(first[3]) + 1], bad[int(first[3]) + 2] = 30, 2        # positions go backwards inside a substream
    with pytest.raises(capi.CabacHipError) as e:
        hip.encode_residual_probes_batch(C["desc"], C["records"], C["first"], C["splices"], C["tus"], C["coeff"], payload, first, bad, sp)
    assert e.value.status == -2


def test_a_fixed_workspace_has_no_probe_form(hip):
    C = case()
    first, at, sp = probe_pairs(False)
    hip.workspace_fix(8, 16, 1 << 16, 1 << 17)
    try:
        with pytest.raises(capi.CabacHipError) as e:
            run_probes(hip, C, first, at, sp)
        assert e.value.status == -2
    finally:
        hip.workspace_release()
    outs, bits = run_probes(hip, C, first, at, sp)                # and the ctx works as before
    assert np.array_equal(bits, expected_bits(C, first, at, sp))
