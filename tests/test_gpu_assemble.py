"""GPU: substream assembly / split / start-code-emulation count on the device against
numpy concatenation and the oracle's restatement of OutputBitstream::countStartCodeEmulations
(bit_stream.cpp:157-181, pinned to the reference in tests/test_oracle_vs_reference.py)."""
import ctypes

import numpy as np
import pytest

import assemble_model as M
import helpers as H
from entropy_coding_amd import capi

pytestmark = pytest.mark.gpu


def test_assemble_split_count_roundtrip():
    import torch
    hip = H.gpu_ctx()
    orc = H.load_oracle()
    orc.lib.orc_count_emulations.argtypes = [H.u8p, ctypes.c_long]
    rng = np.random.default_rng(12)
    lens = [1, 2, 17, 500] + [int(x) for x in rng.integers(1, 6000, size=300)]
    # low-entropy streams (P(1) tiny on one context) give long zero runs -> start-code emulations
    recs = [H.random_records(rng, n - 1, ctx_frac=1.0, p_one=np.full(379, 0.002), ctx_pool=np.array([7])) if k % 3 == 0
            else H.random_records(rng, n - 1) for k, n in enumerate(lens)]
    records = np.concatenate(recs)
    desc, total = H.make_desc([len(r) for r in recs], rng.integers(0, 64, size=len(recs)), [2] * len(recs),
                              H.SUB_FINISH | H.SUB_ALIGN_RBSP)
    n = len(desc)
    t_desc = torch.from_numpy(desc.view(np.uint8)).cuda()
    t_rec = torch.from_numpy(records.view(np.int16)).cuda()
    t_bytes = torch.zeros(total, dtype=torch.uint8, device="cuda")
    t_res = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    hip.encode_device(n, t_desc.data_ptr(), t_rec.data_ptr(), t_bytes.data_ptr(), t_res.data_ptr())
    t_pay = torch.zeros(total, dtype=torch.uint8, device="cuda")
    t_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    hip.assemble_device(n, t_desc.data_ptr(), t_res.data_ptr(), t_bytes.data_ptr(), t_pay.data_ptr(), total, t_off.data_ptr())
    t_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    hip.count_emulations_device(n, t_desc.data_ptr(), t_res.data_ptr(), t_bytes.data_ptr(), t_cnt.data_ptr())
    t_back = torch.zeros(total, dtype=torch.uint8, device="cuda")
    hip.split_device(n, t_desc.data_ptr(), t_off.data_ptr(), t_pay.data_ptr(), t_back.data_ptr())
    hip.synchronize()
    res = t_res.cpu().numpy().view(capi.RESULT_DTYPE)
    out = t_bytes.cpu().numpy()
    sizes = (res["n_bits"].astype(np.int64) + 7) // 8
    streams = [out[int(desc["byte_offset"][s]):int(desc["byte_offset"][s]) + int(sizes[s])] for s in range(n)]
    want = np.concatenate(streams)
    off = t_off.cpu().numpy()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)]))
    assert np.array_equal(t_pay.cpu().numpy()[: len(want)], want)            # addSubstream order and bytes
    back = t_back.cpu().numpy()
    for s in range(n):
        o = int(desc["byte_offset"][s])
        assert np.array_equal(back[o:o + int(sizes[s])], streams[s])          # extractSubstream inverse
    cnt = t_cnt.cpu().numpy()
    want_cnt = [orc.lib.orc_count_emulations(H._ptr(np.ascontiguousarray(b), H.u8p), len(b)) for b in streams]
    assert np.array_equal(cnt, np.array(want_cnt, np.int32)) and max(want_cnt) > 0
    hip.close()


def test_count_emulations_on_crafted_zero_runs():
    """Zero runs of every length and alignment (the kernel takes 64 bytes per step and carries the run length across
    steps), bytes 0..4 mixed in: against the oracle's countStartCodeEmulations (pinned to the reference)."""
    import torch
    hip = H.gpu_ctx()
    orc = H.load_oracle()
    orc.lib.orc_count_emulations.argtypes = [H.u8p, ctypes.c_long]
    rng = np.random.default_rng(5)
    streams = [np.zeros(n, np.uint8) for n in (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 200, 1000)]
    for k in range(600):
        n = int(rng.integers(1, 400))
        p0 = float(rng.choice([0.3, 0.6, 0.9, 0.98]))
        b = rng.choice(np.array([0, 1, 2, 3, 4, 255], np.uint8), size=n, p=[p0] + [(1 - p0) / 5] * 5)
        streams.append(b.astype(np.uint8))
    for lead in range(0, 70, 3):           # a long run placed at every offset around the 64-byte step
        for run in (2, 3, 4, 63, 64, 65, 130):
            streams.append(np.concatenate([np.full(lead, 9, np.uint8), np.zeros(run, np.uint8), np.array([1, 0, 0, 2, 0, 0, 0, 3, 7], np.uint8)]))
    n = len(streams)
    desc = np.zeros(n, H.DESC_DTYPE)
    cap = np.array([(len(b) + 15) // 16 * 16 + 16 for b in streams], np.uint64)
    desc["byte_offset"] = np.concatenate([[0], np.cumsum(cap)[:-1]])
    desc["byte_capacity"] = cap
    res = np.zeros(n, H.RESULT_DTYPE)
    res["n_bits"] = [8 * len(b) for b in streams]
    buf = np.full(int(cap.sum()), 0, np.uint8)
    for k, b in enumerate(streams):
        buf[int(desc["byte_offset"][k]): int(desc["byte_offset"][k]) + len(b)] = b
    t_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    t_res = torch.from_numpy(res.view(np.uint8).copy()).cuda()
    t_buf = torch.from_numpy(buf).cuda()
    t_cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hip.count_emulations_device(n, t_desc.data_ptr(), t_res.data_ptr(), t_buf.data_ptr(), t_cnt.data_ptr())
    hip.synchronize()
    got = t_cnt.cpu().numpy()
    want = np.array([orc.lib.orc_count_emulations(H._ptr(np.ascontiguousarray(b), H.u8p), len(b)) for b in streams], np.int32)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert want.max() > 30
    hip.close()


def test_pack_shard_gathers_on_the_device():
    """sharding.pack_shard on a device-resident batch: one gather launch (cabac_hip_gather_records_device) gives the shard the
    host-side slicing gives — odd and even offsets and lengths, empty substreams, a permuted selection."""
    import torch
    from entropy_coding_amd import sharding
    rng = np.random.default_rng(12)
    lens = [0, 1, 2, 3, 7, 8, 9, 1000, 1001] + [int(x) for x in rng.integers(0, 5000, size=300)]
    recs = [rng.integers(0, 1 << 16, size=n, dtype=np.uint16) for n in lens]
    desc, total = H.make_desc(lens, [30] * len(lens), [2] * len(lens))
    records = np.concatenate(recs)
    for trial in range(3):
        idxs = np.sort(rng.choice(len(lens), size=len(lens) // 2, replace=False)) if trial else np.arange(len(lens))
        want_d, want_r, want_t = sharding.pack_shard(desc, records, idxs)
        got_d, got_r, got_t = sharding.pack_shard(desc, torch.from_numpy(records.view(np.int16)).cuda(), idxs)
        torch.cuda.synchronize()
        assert np.array_equal(got_d, want_d) and got_t == want_t
        assert np.array_equal(got_r.cpu().numpy().view(np.uint16), want_r)


# ---------------------------------------------------------------------------------------------------------------------------
# Below: every kernel of csrc/cabac_assemble.hip against tests/assemble_model.py, bit for bit, on batches made by writing results and
# slot bytes directly (tests/test_assemble_model.py checks on the CPU that they reach the branches they are made for).  Every
# device buffer a kernel writes, and every one it reads, is a view into a larger tensor of sentinel bytes that is compared whole
# afterwards: nothing outside the view, and nothing inside it that the model leaves alone, may change.
GUARD = 4096


class Guarded:
    """`content` (a numpy array) on the device between two guards of `sentinel` bytes: GUARD bytes in front (plus `shift`, to
    misalign the view) and `after` bytes behind"""

    def __init__(self, content, sentinel, after=GUARD, shift=0):
        import torch
        self.content = np.ascontiguousarray(content).view(np.uint8).reshape(-1).copy()
        self.front, self.after, self.sentinel = GUARD + shift, after, sentinel
        self.t = torch.from_numpy(self.expect(self.content)).cuda()
        self.ptr = self.t.data_ptr() + self.front
        assert self.t.data_ptr() % 256 == 0

    def expect(self, content):
        content = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
        assert len(content) == len(self.content)
        return np.concatenate([np.full(self.front, self.sentinel, np.uint8), content, np.full(self.after, self.sentinel, np.uint8)])

    def check(self, want=None, what=""):
        """The whole tensor is the guards around `want` (default: what went in)"""
        got, full = self.t.cpu().numpy(), self.expect(self.content if want is None else want)
        bad = np.nonzero(got != full)[0]
        assert len(bad) == 0, "%s: %d bytes differ, the first at %d of the view (%d bytes long): %d for %d" % (
            what, len(bad), int(bad[0]) - self.front, len(self.content), int(got[bad[0]]), int(full[bad[0]]))


def _inputs(batch):
    return Guarded(batch["desc"], 0x3C), Guarded(batch["results"], 0x3C), Guarded(batch["slots"], 0x3C)


@pytest.mark.parametrize("n_sub", M.N_SUBS)
def test_assemble_clips_at_the_capacity_and_keeps_its_bounds(n_sub):
    """cabac_hip_assemble_device on the shared batch with the payload as large as the total, with every clipping capacity of
    assemble_model.clip_capacities and with the payload 1, 2 and 3 bytes off its alignment: the offsets are the unclipped sums
    whatever the capacity, the payload is the model's up to the capacity and untouched behind it (the guard there is larger
    than the whole unclipped payload), the slots, descriptors and results are as they were."""
    hip = H.gpu_ctx()
    b = M.shared_batch(n_sub)
    offs = M.offsets(b["desc"], b["results"])
    total = int(offs[-1])
    caps = M.clip_capacities(offs)
    g_desc, g_res, g_slots = _inputs(b)
    runs = [(name, cap, 0) for name, cap in caps.items()]
    runs += [(name, caps[name], shift) for name in ("total", "total-1", "into+2") if name in caps for shift in (1, 2, 3)]
    for name, cap, shift in runs:
        init = np.full(cap, M.PAY_SENTINEL, np.uint8)
        g_pay = Guarded(init, M.PAY_SENTINEL, after=max(GUARD, total) + 8, shift=shift)
        g_off = Guarded(np.full(n_sub + 1, 0xA7A7A7A7A7A7A7A7, np.uint64), 0xA7)
        hip.assemble_device(n_sub, g_desc.ptr, g_res.ptr, g_slots.ptr, g_pay.ptr, cap, g_off.ptr)
        hip.synchronize()
        what = "n_sub %d, capacity %s = %d of %d, payload + %d" % (n_sub, name, cap, total, shift)
        g_off.check(offs, what + ": offsets")
        g_pay.check(M.assemble(b["desc"], b["results"], b["slots"], cap, init), what + ": payload")
        g_slots.check(what=what + ": slots")
    g_desc.check(what="descriptors")
    g_res.check(what="results")
    hip.close()


@pytest.mark.parametrize("n_sub", M.N_SUBS)
def test_split_is_the_inverse_and_stays_inside_the_slots(n_sub):
    """cabac_hip_split_device of the assembled payload (the model's) back into slots full of sentinels: every slot holds its
    substream again and its sentinel behind it, from the first byte behind the size on; then with hand-made entry points whose
    spans exceed the slots they go to: no more than byte_capacity arrives, the neighbouring slot stays as it was.  Both with
    the payload at every alignment."""
    hip = H.gpu_ctx()
    b = M.shared_batch(n_sub)
    desc, res, slots = b["desc"], b["results"], b["slots"]
    offs = M.offsets(desc, res)
    payload = M.assemble(desc, res, slots, int(offs[-1]), np.zeros(int(offs[-1]), np.uint8))
    g_desc = Guarded(desc, 0x3C)
    empty = np.full(len(slots), M.SLOT_SENTINEL, np.uint8)
    for what, o, p in (("inverse", offs, payload), ("wide spans",) + M.wide_offsets(b)):
        g_off = Guarded(o, 0x3C)
        want = M.split(desc, o, p, empty)
        if what == "inverse":                                      # the batch's own slots again, slack and padding included
            assert np.array_equal(want, slots)
        for shift in range(4):
            g_pay, g_slots = Guarded(p, M.PAY_SENTINEL, shift=shift), Guarded(empty, 0x3C)
            hip.split_device(n_sub, g_desc.ptr, g_off.ptr, g_pay.ptr, g_slots.ptr)
            hip.synchronize()
            g_slots.check(want, "n_sub %d, %s, payload + %d: slots" % (n_sub, what, shift))
            g_pay.check(what="payload")
        g_off.check(what="offsets")
    g_desc.check(what="descriptors")
    hip.close()


@pytest.mark.parametrize("n_sub", M.COUNT_N_SUBS + ("long runs",))
def test_count_takes_the_whole_bytes_inside_the_slot(n_sub):
    """cabac_hip_count_emulations_device over substreams that end in a partial byte (not part of the reference's FIFO: not
    counted, though it would complete a match), that overflowed (counted up to byte_capacity, though matches follow) and whole
    ones, four to a workgroup; "long runs": zero runs of 65 535 .. 100 000 bytes, ending 0 .. 3 bytes before a partial byte."""
    hip = H.gpu_ctx()
    b = M.long_run_batch() if n_sub == "long runs" else M.count_batch(n_sub)
    n = len(b["desc"])
    g_desc, g_res, g_slots = _inputs(b)
    g_cnt = Guarded(np.full(n, 0x91919191, np.uint32), 0x91)
    hip.count_emulations_device(n, g_desc.ptr, g_res.ptr, g_slots.ptr, g_cnt.ptr)
    hip.synchronize()
    got = g_cnt.t.cpu().numpy()[g_cnt.front: g_cnt.front + 4 * n].view(np.uint32)
    want = M.counts_of(b)
    assert np.array_equal(got, want), [(int(s), int(got[s]), int(want[s]), int(b["kind"][s])) for s in np.nonzero(got != want)[0][:10]]
    g_cnt.check(want, "counts")
    for g in (g_desc, g_res, g_slots):
        g.check(what="inputs")
    hip.close()


@pytest.mark.parametrize("n_seg", [0, 1, 300])
def test_gather_at_every_parity_and_leaves_the_gaps(n_seg):
    """cabac_hip_gather_records_device itself: runs of 0 .. 513 records with source and destination offsets of either parity,
    the destination runs apart from each other; n_seg 1: each of the 32 combinations alone."""
    import torch
    hip = H.gpu_ctx()
    for first in range(32 if n_seg == 1 else 1):
        c = M.gather_case(n_seg, first)
        if n_seg:
            assert c["length"][0] == M.GATHER_LENGTHS[first % 8]
            assert (int(c["src_off"][0]) & 1, int(c["dst_off"][0]) & 1) == (first >> 3 & 1, first >> 4 & 1)
        if n_seg == 300:
            assert len({(int(n), int(s) & 1, int(d) & 1) for n, s, d in zip(c["length"], c["src_off"], c["dst_off"])}) == 32
            ends = c["dst_off"][:-1].astype(np.int64) + c["length"][:-1]
            assert (c["dst_off"][1:].astype(np.int64) - ends >= 1).all()
        init = np.full(c["n_dst"], 0xBEEF, np.uint16)
        g_src, g_dst = Guarded(c["src"], 0x3C), Guarded(init, 0xE1)
        t_so, t_do, t_len = (torch.from_numpy(np.concatenate([c[k], np.zeros(1, c[k].dtype)]).view(np.uint8)).cuda()
                             for k in ("src_off", "dst_off", "length"))
        hip.gather_records_device(n_seg, t_so.data_ptr(), t_do.data_ptr(), t_len.data_ptr(), g_src.ptr, g_dst.ptr)
        hip.synchronize()
        g_dst.check(M.gather(c["src_off"], c["dst_off"], c["length"], c["src"], init), "n_seg %d from %d: destination" % (n_seg, first))
        g_src.check(what="source")
    hip.close()


def test_packed_bins_byte_for_byte():
    """cabac_hip_decode_batch_packed on batches whose substreams cover every record: all (n + 7) // 8 bytes are the model's, the
    bits behind the last bin zero, the caller's bytes behind them untouched."""
    hip = capi.CabacHip(0)
    orc = H.load_oracle()
    rng = np.random.default_rng(8)
    for n in (1, 7, 8, 9, 2047, 2048, 2049):
        parts = [n] if n < 7 else [n // 3, n // 3, n - 2 * (n // 3)]
        recs = [H.random_records(rng, k - 1) for k in parts]
        records = np.concatenate(recs)
        desc, total = H.make_desc(parts, rng.integers(0, 64, size=len(parts)), [2] * len(parts), H.SUB_FINISH | H.SUB_ALIGN_RBSP)
        out, res = orc.encode_batch(desc, records, total)
        assert len(records) == n and int(desc["n_records"].sum()) == n and not res["flags"].any()
        dd = desc.copy()
        dd["byte_capacity"] = (res["n_bits"] + 7) // 8
        mine = np.full((n + 7) // 8 + 64, 0xEE, np.uint8)
        packed, rp = hip.decode_batch_packed(dd, records, out, packed=mine)
        bins_o, ro = orc.decode_batch(dd, records, out)
        assert not rp["flags"].any() and np.array_equal(rp["n_bits"], ro["n_bits"]) and np.array_equal(bins_o, records >> 15)
        want = M.pack_bins(records >> 15)
        assert len(want) == (n + 7) // 8 and np.array_equal(packed, want), n
        assert np.array_equal(mine[: len(want)], want) and (mine[len(want):] == 0xEE).all(), n
    hip.close()
