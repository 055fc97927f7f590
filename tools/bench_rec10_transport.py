#!/usr/bin/env python3
"""Packed bin records (include/cabac_hip_rec10.h) beside the 16-bit records they stand in for, on the host-pointer path.

Workload: the C4 batch (4 096 substreams x 16 384 synthetic records, workload.build_batch as bench.py builds it).  In one process:
  wall    cabac_hip_encode_batch against cabac_hip_rec10_encode_batch, and cabac_hip_decode_batch_packed against
          cabac_hip_rec10_decode_batch with packed bins — from pinned and from pageable memory, with the default chunking and with
          CABAC_HIP_CHUNKS 1 / 2 / 3 (a ctx of its own each: the variable is read when a ctx sets up its streams).  3 warm-up calls
          each, then the two forms alternate, R repetitions each; median and spread.  Packing is done beforehand and is not timed.
  h2d     the rate of one hipMemcpyAsync of the 16-bit records from pinned memory, HIP events: the expected saving of a call is
          0.75 B x records / that rate.
  device  cabac_hip_rec10_unpack_device (kind 43) and cabac_hip_rec10_pack_device (kind 44) on resident buffers alternating with a
          device-to-device hipMemcpyAsync of the 2 n-byte record buffer, HIP events, medians.  The unpack moves 3.25 n bytes where
          the copy moves 4 n; bar: 1.25 x the copy's time, for both.
  host    cabac_hip_rec10_pack_host and _unpack_host on one thread, in GB/s of 16-bit records, beside the DMA time packing saves.
Writes one JSON object (--out, default profiles/rec10_transport.json) with the acceptance checks.

  python tools/bench_rec10_transport.py [--reps 12] [--substreams 4096] [--out FILE]
  python tools/bench_rec10_transport.py --host-only             # CPU only: the host pack / unpack rates
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from entropy_coding_amd import capi  # noqa: E402
from entropy_coding_amd import workload as W  # noqa: E402

CHUNKS = [("default", None), ("1", 1), ("2", 2), ("3", 3)]


def med(xs):
    return {"median_ms": round(statistics.median(xs) * 1e3, 4), "min_ms": round(min(xs) * 1e3, 4), "max_ms": round(max(xs) * 1e3, 4),
            "spread_ms": round((max(xs) - min(xs)) * 1e3, 4)}


def host_rates(records, packed, reps=3):
    """single-thread pack and unpack of the whole batch; rates in GB/s of 16-bit records"""
    t_pack, t_unpack = [], []
    back = np.zeros(len(records), np.uint16)
    for _ in range(reps):
        t0 = time.perf_counter()
        capi.rec10_pack_host(records, packed=packed)
        t_pack.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        capi.rec10_unpack_host(packed, 0, len(records), records=back)
        t_unpack.append(time.perf_counter() - t0)
    assert np.array_equal(back, records)
    return {"pack_host": med(t_pack), "unpack_host": med(t_unpack),
            "pack_host_gbs_of_u16": round(2 * len(records) / statistics.median(t_pack) / 1e9, 2),
            "unpack_host_gbs_of_u16": round(2 * len(records) / statistics.median(t_unpack) / 1e9, 2)}


def alternate(first, second, reps):
    for _ in range(3):
        first(), second()
    a, b = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        first()
        a.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        second()
        b.append(time.perf_counter() - t0)
    return med(a), med(b)


def wall_times(desc, total, rec, packed, n, reps, chunks, pinned):
    """one ctx with its own chunk setting: (encode u16, encode rec10, decode u16, decode rec10) wall times"""
    if chunks is None:
        os.environ.pop("CABAC_HIP_CHUNKS", None)
    else:
        os.environ["CABAC_HIP_CHUNKS"] = str(chunks)
    hip = capi.CabacHip(0)
    keep = []

    def buf(shape, dtype):
        if not pinned:
            return np.zeros(shape, dtype)
        keep.append(capi.PinnedArray(shape, dtype))
        keep[-1].array[...] = 0
        return keep[-1].array

    out_u, out_r = buf((total,), np.uint8), buf((total,), np.uint8)
    _, res_u = hip.encode_batch(desc, rec, total, out=out_u)
    _, res_r = hip.rec10_encode_batch(desc, packed, n, total, out=out_r)
    assert np.array_equal(res_u, res_r) and np.array_equal(out_u, out_r) and not res_u["flags"].any()
    enc = alternate(lambda: hip.encode_batch(desc, rec, total, out=out_u), lambda: hip.rec10_encode_batch(desc, packed, n, total, out=out_r),
                    reps)
    dd = desc.copy()
    dd["byte_capacity"] = (res_u["n_bits"] + 7) // 8
    bins_u, bins_r = buf(((n + 7) // 8 + 1,), np.uint8), buf(((n + 7) // 8 + 1,), np.uint8)
    _, rd_u = hip.decode_batch_packed(dd, rec, out_u, packed=bins_u)
    _, rd_r = hip.rec10_decode_batch(dd, packed, n, out_u, bins_packed=True, bins=bins_r)
    assert np.array_equal(rd_u, rd_r) and not rd_u["flags"].any()
    dec = alternate(lambda: hip.decode_batch_packed(dd, rec, out_u, packed=bins_u),
                    lambda: hip.rec10_decode_batch(dd, packed, n, out_u, bins_packed=True, bins=bins_r), reps)
    hip.close()
    for k in keep:
        k.close()
    os.environ.pop("CABAC_HIP_CHUNKS", None)
    return {"encode": {"u16": enc[0], "rec10": enc[1]}, "decode_packed_bins": {"u16": dec[0], "rec10": dec[1]}}


def device_forms(rec, packed, reps):
    """kind 43 and kind 44 on resident buffers beside a device-to-device copy of the records, and the H2D rate from pinned memory"""
    import torch
    n = len(rec)
    dev = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_rec = torch.from_numpy(rec.view(np.int16)).cuda()
    t_rec2 = torch.empty_like(t_rec)
    t_packed = torch.from_numpy(packed).cuda()
    t_packed2 = torch.empty_like(t_packed)
    t_st = torch.zeros(16, dtype=torch.uint8, device="cuda")
    hiprt = ctypes.CDLL("libamdhip64.so")
    hiprt.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream

    def timed(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    def copy():
        assert hiprt.hipMemcpyAsync(t_rec2.data_ptr(), t_rec.data_ptr(), 2 * n, 3, stream) == 0        # hipMemcpyDeviceToDevice

    def h2d():
        assert hiprt.hipMemcpyAsync(t_rec2.data_ptr(), rec.ctypes.data, 2 * n, 1, stream) == 0          # hipMemcpyHostToDevice

    def unpack():
        dev.rec10_unpack_device(t_packed.data_ptr(), 0, n, t_rec2.data_ptr())

    def pack():
        dev.rec10_pack_device(t_rec.data_ptr(), n, t_packed2.data_ptr(), len(packed), t_st.data_ptr())

    for _ in range(3):
        copy(), pack(), unpack(), h2d()
    torch.cuda.synchronize()
    unpack(), pack()
    torch.cuda.synchronize()
    assert torch.equal(t_rec, t_rec2) and torch.equal(t_packed, t_packed2) and int(t_st.cpu().numpy()[8:12].view(np.uint32)[0]) == 0
    t_copy, t_unpack, t_pack, t_h2d = [], [], [], []
    for _ in range(reps):
        t_copy.append(timed(copy))
        t_unpack.append(timed(unpack))
        t_pack.append(timed(pack))
        t_h2d.append(timed(h2d))
    dev.close()
    return {"d2d_copy_of_u16": med(t_copy), "unpack_kind_43": med(t_unpack), "pack_kind_44": med(t_pack), "h2d_of_u16_pinned": med(t_h2d),
            "copy_gbs_read_plus_write": round(4 * n / statistics.median(t_copy) / 1e9, 1),
            "unpack_gbs_read_plus_write": round(3.25 * n / statistics.median(t_unpack) / 1e9, 1),
            "pack_gbs_read_plus_write": round(3.25 * n / statistics.median(t_pack) / 1e9, 1),
            "h2d_gbs": round(2 * n / statistics.median(t_h2d) / 1e9, 2)}


def verdicts(r):
    n, rate = r["records"], r["device_forms"]["h2d_gbs"] * 1e9
    expected_ms = round(0.75 * n / rate * 1e3, 4)
    out = {"expected_saving_ms_0p75_bytes_per_record_over_the_h2d_rate": expected_ms}
    for leg in ("encode", "decode_packed_bins"):
        w = r["wall"]["pinned"]["default"][leg]
        gain = round(w["u16"]["median_ms"] - w["rec10"]["median_ms"], 4)
        out["pinned_default_chunks_rec10_%s_faster" % leg] = {
            "passed": bool(gain > 0), "saving_ms": gain, "share_of_expected": round(gain / expected_ms, 3),
            "at_least_half_of_expected": bool(gain >= 0.5 * expected_ms), "u16_spread_ms": w["u16"]["spread_ms"]}
    d = r["device_forms"]
    copy = d["d2d_copy_of_u16"]["median_ms"]
    for name in ("unpack_kind_43", "pack_kind_44"):
        out["%s_within_1p25_of_the_d2d_copy" % name] = {"passed": bool(d[name]["median_ms"] <= 1.25 * copy), "ms": d[name]["median_ms"],
                                                        "copy_ms": copy, "ratio": round(d[name]["median_ms"] / copy, 3)}
    saved_dma_ms = expected_ms
    out["host_pack_one_thread_vs_the_dma_it_saves"] = {"pack_ms": r["host_single_thread"]["pack_host"]["median_ms"], "dma_saved_ms": saved_dma_ms,
                                                       "pays_at_flush": bool(r["host_single_thread"]["pack_host"]["median_ms"] < saved_dma_ms)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--substreams", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rec10_transport.json"))
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 10 or a.host_only
    desc, records, total = W.build_batch(W.CONFIGS["C4"], count=a.substreams)
    n = len(records)
    if a.host_only:
        print(json.dumps(host_rates(records, np.zeros(capi.rec10_bytes(n), np.uint8)), indent=1))
        return
    import torch
    p_rec, p_packed = capi.PinnedArray((n,), np.uint16), capi.PinnedArray((capi.rec10_bytes(n),), np.uint8)
    p_rec.array[:] = records
    result = {"tool": "tools/bench_rec10_transport.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "substreams": len(desc),
              "records": n, "bins": int(desc["n_records"].sum()), "bytes_up": {"u16": 2 * n, "rec10": capi.rec10_bytes(n)}}
    result["host_single_thread"] = host_rates(p_rec.array, p_packed.array)
    result["device_forms"] = device_forms(p_rec.array, p_packed.array, a.reps)
    print("device", json.dumps(result["device_forms"]), flush=True)
    result["wall"] = {}
    pageable = (records, p_packed.array.copy())
    for label, (rec, packed) in (("pinned", (p_rec.array, p_packed.array)), ("pageable", pageable)):
        result["wall"][label] = {}
        for name, chunks in CHUNKS:
            result["wall"][label][name] = wall_times(desc, total, rec, packed, n, a.reps, chunks, label == "pinned")
            print(label, name, json.dumps(result["wall"][label][name]), flush=True)
    w = result["wall"]["pinned"]["default"]
    result["gbins_per_s_pinned_default_chunks"] = {
        leg: {form: round(result["bins"] / w[leg][form]["median_ms"] / 1e6, 2) for form in ("u16", "rec10")} for leg in w}
    result["accept"] = verdicts(result)
    p_rec.close()
    p_packed.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["accept"], indent=1))
    print(json.dumps(result["gbins_per_s_pinned_default_chunks"]))


if __name__ == "__main__":
    main()
