"""GPU: emulation prevention on the device (include/cabac_hip_nal.h) — cabac_hip_nal_escape_device / _unescape_device, their
host-pointer forms and cabac_hip_encode_batch_nal, bit-exact against tests/nal_model.py (bytes, every offset, the status word).
The model is pinned to the oracle's countStartCodeEmulations in tests/test_nal_model.py."""
import ctypes

import numpy as np
import pytest

import helpers as H
import nal_model as M
from entropy_coding_amd import capi

pytestmark = pytest.mark.gpu

GUARD = 64


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _status(t):
    s = t.cpu().numpy().view(capi.NAL_STATUS_DTYPE)[0]
    return dict(out_bytes=int(s["out_bytes"]), n_changed=int(s["n_changed"]), flags=int(s["flags"]))


def _padded(data, room, shift=0):
    """`data` on the device at byte `shift` of a buffer with `room` spare bytes behind it."""
    import torch
    t = torch.full((shift + len(data) + room + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    if len(data):
        t[shift:shift + len(data)] = torch.from_numpy(np.ascontiguousarray(data, np.uint8)).cuda()
    return t


def check_escape(hip, offsets, payload, bytes_max=None, capacity=None, shift=0, want=None):
    """Run cabac_hip_nal_escape_device and compare everything with the model; returns (model nal, model offsets, status)."""
    import torch
    payload = np.ascontiguousarray(payload, np.uint8)
    offsets = np.asarray(offsets, np.uint64)
    n = len(payload)
    if bytes_max is None:
        bytes_max = 4 * n + 4096               # as a real caller's slot total: well above the real length
    if capacity is None:
        capacity = M.escape_bound(n)
    w_nal, w_off, w_st = want if want is not None else M.escape(offsets, payload, capacity=capacity, bytes_max=bytes_max)
    if want is not None:
        w_st = dict(w_st, flags=(w_st["flags"] & ~M.NAL_OVERFLOW) | (M.NAL_OVERFLOW if w_st["out_bytes"] > capacity else 0))
    t_pay = _padded(payload, 0, shift)
    t_off = _dev(offsets)
    t_nal = torch.full((shift + capacity + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    t_noff = torch.full((len(offsets),), -1, dtype=torch.int64, device="cuda")
    t_st = torch.full((16,), 0x77, dtype=torch.uint8, device="cuda")
    hip.nal_escape_device(len(offsets) - 1, t_off.data_ptr(), t_pay.data_ptr() + shift, bytes_max, t_nal.data_ptr() + shift, capacity,
                          t_noff.data_ptr(), t_st.data_ptr())
    hip.synchronize()
    st = _status(t_st)
    assert st == w_st, (st, w_st)
    got = t_nal.cpu().numpy()
    k = min(capacity, len(w_nal))
    assert np.array_equal(got[shift:shift + k], w_nal[:k]), np.nonzero(got[shift:shift + k] != w_nal[:k])[0][:8]
    assert np.all(got[shift + k:] == 0xEE) and np.all(got[:shift] == 0xEE)       # nothing behind the result / the capacity
    assert np.array_equal(t_noff.cpu().numpy().view(np.uint64), w_off)
    return w_nal, w_off, st


def check_unescape(hip, nal_offsets, nal, bytes_max=None, capacity=None, loc_capacity=None, loc_base=0, with_loc=True, shift=0,
                   want=None):
    import torch
    nal = np.ascontiguousarray(nal, np.uint8)
    nal_offsets = np.asarray(nal_offsets, np.uint64)
    n = len(nal)
    if bytes_max is None:
        bytes_max = 4 * n + 4096
    if capacity is None:
        capacity = n
    if loc_capacity is None:
        loc_capacity = n // 3 + 1
    if want is not None:
        w_pay, w_off, w_loc, w_st = want
        fl = w_st["flags"] & ~(M.NAL_OVERFLOW | M.NAL_LOC_OVERFLOW)
        fl |= M.NAL_OVERFLOW if w_st["out_bytes"] > capacity else 0
        fl |= M.NAL_LOC_OVERFLOW if with_loc and len(w_loc) > loc_capacity else 0
        w_st = dict(w_st, flags=fl)
    else:
        w_pay, w_off, w_loc, w_st = M.unescape(nal_offsets, nal, capacity=capacity, loc_capacity=loc_capacity if with_loc else None,
                                               loc_base=loc_base, bytes_max=bytes_max)
    t_nal = _padded(nal, 0, shift)
    t_noff = _dev(nal_offsets)
    t_pay = torch.full((shift + capacity + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    t_off = torch.full((len(nal_offsets),), -1, dtype=torch.int64, device="cuda")
    t_loc = torch.full((loc_capacity + 16,), -1, dtype=torch.int32, device="cuda")
    t_st = torch.full((16,), 0x77, dtype=torch.uint8, device="cuda")
    hip.nal_unescape_device(len(nal_offsets) - 1, t_noff.data_ptr(), t_nal.data_ptr() + shift, bytes_max, t_pay.data_ptr() + shift,
                            capacity, t_off.data_ptr(), t_st.data_ptr(), d_locations=t_loc.data_ptr() if with_loc else 0,
                            loc_capacity=loc_capacity if with_loc else 0, loc_base=loc_base)
    hip.synchronize()
    st = _status(t_st)
    assert st == w_st, (st, w_st)
    got = t_pay.cpu().numpy()
    k = min(capacity, len(w_pay))
    assert np.array_equal(got[shift:shift + k], w_pay[:k]), np.nonzero(got[shift:shift + k] != w_pay[:k])[0][:8]
    assert np.all(got[shift + k:] == 0xEE) and np.all(got[:shift] == 0xEE)
    assert np.array_equal(t_off.cpu().numpy().view(np.uint64), w_off)
    loc = t_loc.cpu().numpy().view(np.uint32)
    kl = min(loc_capacity, len(w_loc)) if with_loc else 0
    assert np.array_equal(loc[:kl], w_loc[:kl]) and np.all(loc[kl:] == 0xFFFFFFFF)
    return w_pay, w_off, w_loc, st


def roundtrip(hip, offsets, payload, **kw):
    nal, nal_off, st = check_escape(hip, offsets, payload, **kw)
    pay, off, loc, st2 = check_unescape(hip, nal_off, nal, shift=kw.get("shift", 0))
    assert np.array_equal(pay, np.ascontiguousarray(payload, np.uint8)) and np.array_equal(off, np.asarray(offsets, np.uint64))
    assert st2["n_changed"] == st["n_changed"] and st2["flags"] == 0
    return nal, nal_off, st


def _coded_batch(hip, recs, qps):
    """encode_device + assemble_device of a batch of record strings: a dict of what the cases below need."""
    import torch
    records = np.concatenate(recs)
    desc, total = H.make_desc([len(r) for r in recs], qps, [2] * len(recs), H.SUB_FINISH | H.SUB_ALIGN_RBSP)
    n = len(desc)
    t = dict(n=n, desc=desc, records=records, total=total)
    t["t_desc"] = torch.from_numpy(desc.view(np.uint8)).cuda()
    t["t_rec"] = torch.from_numpy(records.view(np.int16)).cuda()
    t["t_bytes"] = torch.zeros(total, dtype=torch.uint8, device="cuda")
    t["t_res"] = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    hip.encode_device(n, t["t_desc"].data_ptr(), t["t_rec"].data_ptr(), t["t_bytes"].data_ptr(), t["t_res"].data_ptr())
    t["t_pay"] = torch.zeros(total, dtype=torch.uint8, device="cuda")
    t["t_off"] = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    hip.assemble_device(n, t["t_desc"].data_ptr(), t["t_res"].data_ptr(), t["t_bytes"].data_ptr(), t["t_pay"].data_ptr(), total,
                        t["t_off"].data_ptr())
    t["t_cnt"] = torch.zeros(n, dtype=torch.int32, device="cuda")
    hip.count_emulations_device(n, t["t_desc"].data_ptr(), t["t_res"].data_ptr(), t["t_bytes"].data_ptr(), t["t_cnt"].data_ptr())
    hip.synchronize()
    t["res"] = t["t_res"].cpu().numpy().view(capi.RESULT_DTYPE)
    assert not t["res"]["flags"].any() and not (t["res"]["n_bits"] & 7).any()      # no partial byte (ALIGN_RBSP)
    t["off"] = t["t_off"].cpu().numpy().view(np.uint64)
    t["pay"] = t["t_pay"].cpu().numpy()[: int(t["off"][n])]
    t["cnt"] = t["t_cnt"].cpu().numpy()
    return t


def _batch_304(rng):
    """The recipe of test_assemble_split_count_roundtrip (seed 12): every third substream low-entropy."""
    lens = [1, 2, 17, 500] + [int(x) for x in rng.integers(1, 6000, size=300)]
    recs = [H.random_records(rng, n - 1, ctx_frac=1.0, p_one=np.full(379, 0.002), ctx_pool=np.array([7])) if k % 3 == 0
            else H.random_records(rng, n - 1) for k, n in enumerate(lens)]
    return recs, rng.integers(0, 64, size=len(recs))


def _segments(off, data):
    return [data[int(off[s]):int(off[s + 1])] for s in range(len(off) - 1)]


def test_coded_substreams_end_to_end():
    """encode_device -> assemble_device -> nal_escape_device -> nal_unescape_device -> split_device -> decode_device."""
    import torch
    hip = H.gpu_ctx()
    orc = H.load_oracle()
    orc.lib.orc_count_emulations.argtypes = [H.u8p, ctypes.c_long]
    recs, qps = _batch_304(np.random.default_rng(12))
    b = _coded_batch(hip, recs, qps)
    n, total = b["n"], b["total"]
    # device to device, with the capacities a caller knows without a synchronisation
    cap = M.escape_bound(total)
    t_nal = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    t_noff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    t_st = torch.zeros(16, dtype=torch.uint8, device="cuda")
    hip.nal_escape_device(n, b["t_off"].data_ptr(), b["t_pay"].data_ptr(), total, t_nal.data_ptr(), cap, t_noff.data_ptr(), t_st.data_ptr())
    t_back = torch.full((total + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    t_boff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    t_loc = torch.full((4096,), -1, dtype=torch.int32, device="cuda")
    t_st2 = torch.zeros(16, dtype=torch.uint8, device="cuda")
    hip.nal_unescape_device(n, t_noff.data_ptr(), t_nal.data_ptr(), cap, t_back.data_ptr(), total, t_boff.data_ptr(), t_st2.data_ptr(),
                            d_locations=t_loc.data_ptr(), loc_capacity=4096, loc_base=1000)
    t_slots = torch.zeros(total, dtype=torch.uint8, device="cuda")
    hip.split_device(n, b["t_desc"].data_ptr(), t_boff.data_ptr(), t_back.data_ptr(), t_slots.data_ptr())
    ddesc = b["desc"].copy()
    ddesc["byte_capacity"] = (b["res"]["n_bits"] + 7) // 8
    t_ddesc = torch.from_numpy(ddesc.view(np.uint8)).cuda()
    t_bins = torch.zeros(len(b["records"]), dtype=torch.uint8, device="cuda")
    t_res2 = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    hip.decode_device(n, t_ddesc.data_ptr(), b["t_rec"].data_ptr(), t_slots.data_ptr(), t_bins.data_ptr(), t_res2.data_ptr())
    hip.synchronize()

    pay, off = b["pay"], b["off"]
    w_nal, w_noff, w_st = M.escape(off, pay, capacity=cap, bytes_max=total)
    st, noff = _status(t_st), t_noff.cpu().numpy().view(np.uint64)
    print("payload %d bytes, %d insertions" % (len(pay), st["n_changed"]))
    assert st == w_st and np.array_equal(noff, w_noff)
    nal = t_nal.cpu().numpy()
    assert np.array_equal(nal[: len(w_nal)], w_nal) and np.all(nal[len(w_nal):] == 0xEE)
    assert not M.has_forbidden(w_nal)
    # per-segment growth == the count kernel == the oracle's countStartCodeEmulations of each substream
    growth = (np.diff(noff.astype(np.int64)) - np.diff(off.astype(np.int64)))
    want_cnt = np.array([orc.lib.orc_count_emulations(H._ptr(np.ascontiguousarray(s), H.u8p), len(s)) for s in _segments(off, pay)])
    assert np.array_equal(growth, b["cnt"]) and np.array_equal(growth, want_cnt)
    # the batch really exercises the feature (a condition on the generator, not a measurement)
    assert growth.sum() >= 700 and (growth > 0).sum() >= 90 and all(len(s) and s[-1] != 0 for s in _segments(off, pay))
    # ... and back
    w_pay, w_off, w_loc, w_st2 = M.unescape(w_noff, w_nal, capacity=total, loc_capacity=4096, loc_base=1000, bytes_max=cap)
    assert _status(t_st2) == w_st2 and w_st2["flags"] == 0
    assert np.array_equal(t_back.cpu().numpy()[: len(pay)], pay) and np.all(t_back.cpu().numpy()[len(pay):] == 0xEE)
    assert np.array_equal(t_boff.cpu().numpy().view(np.uint64), off)
    loc = t_loc.cpu().numpy().view(np.uint32)
    assert np.array_equal(loc[: len(w_loc)], w_loc) and np.all(loc[len(w_loc):] == 0xFFFFFFFF) and len(w_loc) == st["n_changed"]
    assert np.all(w_nal[(w_loc - 1000).astype(np.int64)] == 3)
    assert np.array_equal(t_bins.cpu().numpy(), (b["records"] >> 15).astype(np.uint8))
    assert not t_res2.cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any()
    hip.close()


def _crafted_strings():
    """The strings of test_count_emulations_on_crafted_zero_runs (tests/test_gpu_assemble.py)."""
    rng = np.random.default_rng(5)
    streams = [np.zeros(n, np.uint8) for n in (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 200, 1000)]
    for k in range(600):
        n = int(rng.integers(1, 400))
        p0 = float(rng.choice([0.3, 0.6, 0.9, 0.98]))
        streams.append(rng.choice(np.array([0, 1, 2, 3, 4, 255], np.uint8), size=n, p=[p0] + [(1 - p0) / 5] * 5).astype(np.uint8))
    for lead in range(0, 70, 3):
        for run in (2, 3, 4, 63, 64, 65, 130):
            streams.append(np.concatenate([np.full(lead, 9, np.uint8), np.zeros(run, np.uint8), np.array([1, 0, 0, 2, 0, 0, 0, 3, 7], np.uint8)]))
    return streams


def test_crafted_strings_as_segments_of_one_payload():
    """Runs that cross segment boundaries: the result is the escape of the concatenation, an inserted byte belongs to the
    segment of the byte it precedes."""
    hip = H.gpu_ctx()
    streams = _crafted_strings()
    assert len(streams) > 750
    payload = np.concatenate(streams)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
    nal, nal_off, st = roundtrip(hip, offsets, payload)
    assert st["n_changed"] > 10000
    # somewhere a segment starts with a byte that gets its 03 from zeros of the segment in front of it
    assert any(int(nal_off[s]) < len(nal) and nal[int(nal_off[s])] == 3 and int(offsets[s]) < len(payload) and payload[int(offsets[s])] != 3
               for s in range(1, len(streams)))
    roundtrip(hip, offsets, payload, shift=5)         # buffers that are not 16-byte aligned
    hip.close()


def test_crafted_strings_one_at_a_time():
    hip = H.gpu_ctx()
    orc = H.load_oracle()
    orc.lib.orc_count_emulations.argtypes = [H.u8p, ctypes.c_long]
    for s in _crafted_strings():
        nal, nal_off, st = roundtrip(hip, [0, len(s)], s)
        assert st["n_changed"] == orc.lib.orc_count_emulations(H._ptr(np.ascontiguousarray(s), H.u8p), len(s))
    hip.close()


def _seam_payloads():
    """3 MiB of filler 0xAB; around multiples of every plausible tile size B, zero runs of length {2,3,4,5,64,65} that end at
    every distance -3..+3 from the seam, followed by one of {00,01,03,04} (one payload per follower, so that every pattern has a
    seam of its own)."""
    size = 3 << 20
    for follow in (0, 1, 3, 4):
        p = np.full(size, 0xAB, np.uint8)
        used = np.zeros(size, bool)
        for B in (65536, 16384, 4096, 1024, 256, 64):       # the sizes with the fewest seams choose first
            m = (128 + B - 1) // B
            for run in (2, 3, 4, 5, 64, 65):
                for dist in range(-3, 4):
                    while used[B * m - 80: B * m + 16].any():
                        m += 1
                    seam = B * m
                    assert seam + 16 < size
                    p[seam + dist - run: seam + dist] = 0      # the run ends `dist` bytes behind the seam
                    p[seam + dist] = follow
                    used[seam - 80: seam + 16] = True
                    m += 1
        yield follow, p


def test_tile_seams():
    hip = H.gpu_ctx()
    for follow, p in _seam_payloads():
        cuts = [0, 4095, 4096, 65536 + 1, 1 << 20, len(p)]
        nal, nal_off, st = roundtrip(hip, cuts, p)
        assert st["n_changed"] >= 6 * 7 * 4, (follow, st)
    z = np.zeros(300001, np.uint8)
    nal, nal_off, st = roundtrip(hip, [0, 1, 2, 3, 4096, 150000, 300001], z)
    assert st == dict(out_bytes=450001, n_changed=150000, flags=M.NAL_TRAILING_ZERO)
    z1 = np.concatenate([np.zeros(300000, np.uint8), np.array([1], np.uint8)])
    nal, nal_off, st = roundtrip(hip, [0, 300000, 300001], z1)
    assert st["n_changed"] == 150000 and st["flags"] == 0 and int(nal_off[1]) == 300000 + 149999
    hip.close()


def test_capacity_and_clipping():
    hip = H.gpu_ctx()
    recs, qps = _batch_304(np.random.default_rng(12))
    b = _coded_batch(hip, recs, qps)
    pay, off = b["pay"], b["off"]
    n = len(pay)
    # a length above the bound the host gave: clipped, flagged, and the result is that of the clipped input
    nal, nal_off, st = check_escape(hip, off, pay, bytes_max=n - 1)
    assert st["flags"] & M.NAL_INPUT_CLIPPED
    nal, nal_off, st = check_escape(hip, off, pay, bytes_max=n // 2 + 3)
    assert st["flags"] & M.NAL_INPUT_CLIPPED and int(nal_off[-1]) == st["out_bytes"]
    full = M.escape(off, pay)
    for cap in (full[2]["out_bytes"] - 1, full[2]["out_bytes"] // 2, 0):
        nal, nal_off, st = check_escape(hip, off, pay, capacity=cap, want=full)
        assert st["flags"] == M.NAL_OVERFLOW and st["out_bytes"] == full[2]["out_bytes"] and st["n_changed"] == full[2]["n_changed"]
    nal, nal_off = full[0], full[1]
    pay2, off2, loc, st = check_unescape(hip, nal_off, nal, bytes_max=len(nal) - 1)
    assert st["flags"] & M.NAL_INPUT_CLIPPED
    back = M.unescape(nal_off, nal, loc_capacity=len(nal))
    assert len(back[2]) > 700
    for cap in (n - 1, n // 2, 0):
        pay2, off2, loc, st = check_unescape(hip, nal_off, nal, capacity=cap, want=back)
        assert st["flags"] == M.NAL_OVERFLOW and st["out_bytes"] == n
    for lcap in (len(back[2]) - 1, 100, 0):
        pay2, off2, loc, st = check_unescape(hip, nal_off, nal, loc_capacity=lcap, want=back)
        assert st["flags"] == M.NAL_LOC_OVERFLOW and st["n_changed"] == len(back[2])
    pay2, off2, loc, st = check_unescape(hip, nal_off, nal, with_loc=False, want=back)       # no list asked for: no flag
    assert st["flags"] == 0
    pay2, off2, loc, st = check_unescape(hip, nal_off, nal, capacity=n // 2, loc_capacity=7, want=back)
    assert st["flags"] == M.NAL_OVERFLOW | M.NAL_LOC_OVERFLOW
    hip.close()


def test_invalid_nal_input_to_unescape():
    hip = H.gpu_ctx()
    F, B = M.NAL_FORBIDDEN, M.NAL_BAD_ESCAPE
    cases = [([0, 0, 0], F), ([0, 0, 1], F), ([0, 0, 2], F), ([0, 0, 3, 4], B), ([0, 0, 0, 3], F), ([7, 0, 0, 3], 0),
             ([0, 0, 3, 0, 0, 3, 255, 0, 0, 0], F | B), ([0, 0, 3, 3], 0), ([0, 0, 3, 0, 0, 2], F)]
    filler = np.full(5000, 0x11, np.uint8)
    for nal, flags in cases:
        nal = np.array(nal, np.uint8)
        for data in (nal, np.concatenate([filler[:1021], nal, filler]), np.concatenate([filler[:4094], nal]),
                     np.concatenate([filler[:1008 + 15], nal, filler[:3]])):
            pay, off, loc, st = check_unescape(hip, [0, len(data) // 2, len(data)], data)      # flags and bytes as the model says
            if data is nal:
                assert st["flags"] == flags, (nal, st)
            else:       # (a removed 03 at the end of the string now has a filler byte behind it)
                assert st["flags"] & F == flags & F, (nal, len(data), st)
    hip.close()


def test_trailing_zero_and_degenerate_shapes():
    import torch
    hip = H.gpu_ctx()
    nal, nal_off, st = check_escape(hip, [0, 2, 5], np.array([1, 2, 3, 4, 0], np.uint8))
    assert st["flags"] == M.NAL_TRAILING_ZERO and st["n_changed"] == 0
    nal, nal_off, st = roundtrip(hip, [0, 1], np.array([0], np.uint8))
    assert st == dict(out_bytes=1, n_changed=0, flags=M.NAL_TRAILING_ZERO)
    nal, nal_off, st = roundtrip(hip, [0, 1], np.array([3], np.uint8))
    assert st == dict(out_bytes=1, n_changed=0, flags=0)
    nal, nal_off, st = roundtrip(hip, [0, 0, 0, 0], np.zeros(0, np.uint8))        # all segments empty
    assert st == dict(out_bytes=0, n_changed=0, flags=0) and not nal_off.any()
    nal, nal_off, st = roundtrip(hip, [0], np.zeros(0, np.uint8))                 # n_seg = 0 with an offsets array
    nal, nal_off, st = roundtrip(hip, [0, 0, 3, 3, 3, 6, 6], np.array([0, 0, 1, 0, 0, 0], np.uint8))   # empty ones between
    assert st["n_changed"] == 2
    # n_seg = 0 with no offsets at all: only the status is written
    for call in ("esc", "unesc"):
        t_st = torch.full((16,), 0x77, dtype=torch.uint8, device="cuda")
        if call == "esc":
            hip.nal_escape_device(0, 0, 0, 0, 0, 0, 0, t_st.data_ptr())
        else:
            hip.nal_unescape_device(0, 0, 0, 0, 0, 0, 0, t_st.data_ptr())
        hip.synchronize()
        assert _status(t_st) == dict(out_bytes=0, n_changed=0, flags=0)
    hip.close()


def test_host_forms():
    hip = capi.CabacHip(0)
    recs, qps = _batch_304(np.random.default_rng(12))
    records = np.concatenate(recs)
    desc, total = H.make_desc([len(r) for r in recs], qps, [2] * len(recs), H.SUB_FINISH | H.SUB_ALIGN_RBSP)
    payload = np.zeros(total, np.uint8)
    off, res = hip.encode_batch_payload(desc, records, payload)
    pay = payload[: int(off[-1])]
    w_nal, w_noff, w_st = M.escape(off, pay)
    w_pay, w_off, w_loc, w_st2 = M.unescape(w_noff, w_nal, loc_capacity=len(w_nal), loc_base=77)
    pins = [capi.PinnedArray((M.escape_bound(len(pay)),), np.uint8), capi.PinnedArray((len(pay),), np.uint8),
            capi.PinnedArray((len(w_loc),), np.uint32), capi.PinnedArray((M.escape_bound(total),), np.uint8)]
    for pinned in (False, True):
        nal = pins[0].array if pinned else np.zeros(M.escape_bound(len(pay)), np.uint8)
        assert capi.host_is_pinned(nal) == pinned
        noff, st = hip.nal_escape_batch(off, pay, nal)
        assert dict(out_bytes=int(st["out_bytes"]), n_changed=int(st["n_changed"]), flags=int(st["flags"])) == w_st
        assert np.array_equal(nal[: len(w_nal)], w_nal) and np.array_equal(noff, w_noff)
        back = pins[1].array if pinned else np.zeros(len(pay), np.uint8)
        loc = pins[2].array if pinned else np.zeros(len(w_loc), np.uint32)
        boff, st2 = hip.nal_unescape_batch(noff, nal[: len(w_nal)], back, locations=loc, loc_base=77)
        assert dict(out_bytes=int(st2["out_bytes"]), n_changed=int(st2["n_changed"]), flags=int(st2["flags"])) == w_st2
        assert np.array_equal(back, pay) and np.array_equal(boff, off) and np.array_equal(loc, w_loc)
        # records in, NAL payload out
        out = pins[3].array if pinned else np.zeros(M.escape_bound(total), np.uint8)
        eoff, eres, est = hip.encode_batch_nal(desc, records, out)
        assert np.array_equal(eoff, w_noff) and np.array_equal(out[: len(w_nal)], w_nal) and np.array_equal(eres, res)
        assert int(est["out_bytes"]) == len(w_nal) and int(est["n_changed"]) == w_st["n_changed"] and int(est["flags"]) == 0
    # a capacity that is too small: an overflow flag from the plain forms, an error that tells the size from encode_batch_nal
    small = np.full(len(w_nal) - 1 + GUARD, 0xEE, np.uint8)
    noff, st = hip.nal_escape_batch(off, pay, small[: len(w_nal) - 1])
    assert int(st["flags"]) == M.NAL_OVERFLOW and int(st["out_bytes"]) == len(w_nal) and np.array_equal(noff, w_noff)
    assert np.array_equal(small[: len(w_nal) - 1], w_nal[:-1]) and np.all(small[len(w_nal) - 1:] == 0xEE)
    with pytest.raises(capi.CabacHipError) as e:
        hip.encode_batch_nal(desc, records, small[: len(w_nal) - 1])
    assert e.value.status == -2 and int(e.value.nal_status["out_bytes"]) == len(w_nal)
    with pytest.raises(capi.CabacHipError) as e:
        hip.nal_escape_batch([0, 5, 3], pay, small)
    assert e.value.status == -2
    # the C2 workload: ten long substreams (parallelism from tiles of the string, not from segments)
    from entropy_coding_amd.workload import CONFIGS, build_batch
    desc, records, total = build_batch(CONFIGS["C2"])
    payload = np.zeros(total, np.uint8)
    off, res = hip.encode_batch_payload(desc, records, payload)
    w_nal, w_noff, w_st = M.escape(off, payload[: int(off[-1])])
    out = np.zeros(M.escape_bound(total), np.uint8)
    eoff, eres, est = hip.encode_batch_nal(desc, records, out)
    assert np.array_equal(eoff, w_noff) and np.array_equal(out[: len(w_nal)], w_nal) and np.array_equal(eres, res)
    assert int(est["out_bytes"]) == len(w_nal) and int(est["n_changed"]) == w_st["n_changed"]
    for p in pins:
        p.close()
    hip.close()


def test_larger_realistic_payload():
    """4 096 low-entropy substreams of 8 192 bins (the insertions) among 1 024 ordinary ones of 16 384 (the megabytes)."""
    hip = H.gpu_ctx()
    rng = np.random.default_rng(2024)
    recs = []
    for k in range(5120):
        if k % 5 == 4:
            recs.append(H.random_records(rng, 16383))
        else:
            recs.append(H.random_records(rng, 8191, ctx_frac=1.0, p_one=np.full(379, 0.002), ctx_pool=np.array([7])))
    b = _coded_batch(hip, recs, rng.integers(0, 64, size=len(recs)))
    pay, off = b["pay"], b["off"]
    print("payload %d bytes in %d segments" % (len(pay), b["n"]))
    assert len(pay) > (1 << 20)
    nal, nal_off, st = check_escape(hip, off, pay, bytes_max=b["total"])
    growth = np.diff(nal_off.astype(np.int64)) - np.diff(off.astype(np.int64))
    assert np.array_equal(growth, b["cnt"]) and growth.sum() == st["n_changed"] > 1000
    pay2, off2, loc, st2 = check_unescape(hip, nal_off, nal, bytes_max=M.escape_bound(b["total"]))
    assert np.array_equal(pay2, pay) and np.array_equal(off2, off) and st2["flags"] == 0
    hip.close()
