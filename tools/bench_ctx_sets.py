#!/usr/bin/env python3
"""The codec calls from and into context sets, and WPP, next to the plain calls (include/cabac_hip_ctx_sets.h).

Workload: the C4 batch of BASELINE.json (4 096 substreams x 16 384 bins), device buffers resident.  Legs, each timed with a pair of
HIP events around the call on the ctx's stream, W warm-up + R timed repetitions, medians and minima:
  plain        cabac_hip_encode_device / cabac_hip_decode_device
  sets_noset   the sets calls with every start set CABAC_CTX_NO_SET and no out sets (the plain result)
  sets_shared  the sets calls from 64 shared start sets (substream s from set s % 64) with every out set written
  wpp          the same 4 096 substreams as 256 pictures x 16 rows (level r = row r of every picture, row r linked to row r - 1
               of its picture, hand-over after sync_at records) under the WPP calls — against `plain`, which is the same batch
               without links.  What the schedule predicts: 15 prefix launches of 256 substreams each (encode: the context
               advance; decode: the sets decoder) plus one full launch; the profile ring gives the prefix launches' share.
`--legs plain` runs on a library without the sets calls too (CABAC_HIP_LIBRARY=<a build of the parent commit> --label parent):
the plain legs run unchanged kernel instantiations, so they must lie within the parent's run-to-run spread.
Writes one JSON object (--out, default profiles/ctx_sets.json; merged with what the file holds under other labels).

  python tools/bench_ctx_sets.py [--reps 20] [--warmup 3] [--legs plain,sets_noset,sets_shared,wpp] [--sync-at 2048] [--label NAME]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from entropy_coding_amd import capi  # noqa: E402
from entropy_coding_amd.workload import CONFIGS, build_batch  # noqa: E402

N_SHARED = 64
PICTURES, ROWS = 256, 16


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="plain,sets_noset,sets_shared,wpp")
    ap.add_argument("--sync-at", type=int, default=2048, help="records of a row after which its contexts are handed over")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctx_sets.json"))
    a = ap.parse_args()
    legs = a.legs.split(",")
    desc, records, total = build_batch(CONFIGS["C4"])
    n = len(desc)
    assert n == PICTURES * ROWS
    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_desc, t_rec = dev(desc), dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    t_bytes = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    t_res = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    t_bins = torch.zeros(len(records) + 16, dtype=torch.uint8, device="cuda")
    P = [t.data_ptr() for t in (t_desc, t_rec, t_bytes, t_res, t_bins)]
    want_bins = torch.from_numpy((records >> 15).astype(np.uint8)).cuda()
    mask = np.zeros(len(records), np.uint8)           # the gaps between the substreams' record slots are never written
    for d in desc:
        mask[int(d["rec_offset"]):int(d["rec_offset"]) + int(d["n_records"])] = 1
    live = torch.from_numpy(mask).cuda()
    want_bins *= live
    out = {"device": torch.cuda.get_device_name(0), "substreams": n, "bins": int(desc["n_records"].sum()), "reps": a.reps}

    def flags_clear():
        hip.synchronize()
        assert not t_res.cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any()

    def bins_right():
        flags_clear()
        assert torch.equal(t_bins[:len(records)] * live, want_bins)

    if "plain" in legs:
        out["plain_encode"] = timed(lambda: hip.encode_device(n, P[0], P[1], P[2], P[3]), a.warmup, a.reps)
        flags_clear()
        plain_bytes = t_bytes.clone()
        out["plain_decode"] = timed(lambda: hip.decode_device(n, P[0], P[1], P[2], P[4], P[3]), a.warmup, a.reps)
        bins_right()
    if "sets_noset" in legs:
        t_none = dev(np.full(n, capi.CTX_NO_SET, np.uint32))
        t_bytes.zero_()
        out["sets_noset_encode"] = timed(lambda: hip.encode_sets_device(n, P[0], P[1], P[2], P[3], 0, 0, 0, t_none.data_ptr()),
                                         a.warmup, a.reps)
        flags_clear()
        if "plain" in legs:
            out["sets_noset_bytes_equal_plain"] = bool(torch.equal(t_bytes, plain_bytes))
            assert out["sets_noset_bytes_equal_plain"]
        out["sets_noset_decode"] = timed(lambda: hip.decode_sets_device(n, P[0], P[1], P[2], P[4], P[3], 0, 0, 0, t_none.data_ptr()),
                                         a.warmup, a.reps)
        bins_right()
    if "sets_shared" in legs:
        # n sets (one n_sets bounds the start and the out arrays); the first 64 are the shared start sets
        t_qp = dev(((np.arange(n) * 7) % 52).astype(np.int32))
        t_iid = dev((np.arange(n) % 3).astype(np.uint32))
        t_state = torch.zeros(n * capi.NUM_CTX, dtype=torch.int32, device="cuda")
        t_rate = torch.zeros(n * capi.NUM_CTX, dtype=torch.uint8, device="cuda")
        hip.ctx_init_device(n, t_qp.data_ptr(), t_iid.data_ptr(), t_state.data_ptr(), t_rate.data_ptr())
        t_start = dev((np.arange(n) % N_SHARED).astype(np.uint32))
        t_outset = dev(np.arange(n, dtype=np.uint32))
        t_ostate, t_orate = torch.zeros_like(t_state), torch.zeros_like(t_rate)
        S = [t.data_ptr() for t in (t_state, t_rate, t_start, t_outset, t_ostate, t_orate)]
        out["sets_shared_encode"] = timed(lambda: hip.encode_sets_device(n, P[0], P[1], P[2], P[3], n, *S), a.warmup, a.reps)
        flags_clear()
        enc_state = t_ostate.clone()
        out["sets_shared_decode"] = timed(lambda: hip.decode_sets_device(n, P[0], P[1], P[2], P[4], P[3], n, *S), a.warmup, a.reps)
        bins_right()
        assert torch.equal(enc_state, t_ostate) and torch.equal(t_orate[:capi.NUM_CTX], t_rate[:capi.NUM_CTX])
    if "wpp" in legs:
        level_first = np.arange(0, n + 1, PICTURES, dtype=np.uint32)
        sync_from = np.where(np.arange(n) < PICTURES, capi.CTX_NO_SET, np.arange(n) - PICTURES).astype(np.uint32)
        t_from, t_at = dev(sync_from), dev(np.full(n, a.sync_at, np.uint32))

        def one_call_profiled(fn, full_kind):
            fn()                                       # (scratch allocation and code loading stay outside)
            hip.profile_enable(64)
            fn()
            prof = hip.profile_read()
            hip.profile_enable(0)
            return {"prefix": sum(1 for k, _ in prof if k == 33), "prefix_ms": sum(t for k, t in prof if k == 33),
                    "full_ms": sum(t for k, t in prof if k == full_kind)}

        out["wpp_encode_launches"] = one_call_profiled(lambda: hip.encode_wpp_device(n, P[0], P[1], P[2], P[3], level_first,
                                                                                     t_from.data_ptr(), t_at.data_ptr()), 30)
        out["wpp_encode"] = timed(lambda: hip.encode_wpp_device(n, P[0], P[1], P[2], P[3], level_first, t_from.data_ptr(),
                                                                t_at.data_ptr()), a.warmup, a.reps)
        flags_clear()
        if "plain" in legs:
            out["wpp_bytes_differ_from_plain"] = not bool(torch.equal(t_bytes, plain_bytes))
        out["wpp_decode_launches"] = one_call_profiled(lambda: hip.decode_wpp_device(n, P[0], P[1], P[2], P[4], P[3], level_first,
                                                                                     t_from.data_ptr(), t_at.data_ptr()), 31)
        out["wpp_decode"] = timed(lambda: hip.decode_wpp_device(n, P[0], P[1], P[2], P[4], P[3], level_first, t_from.data_ptr(),
                                                                t_at.data_ptr()), a.warmup, a.reps)
        bins_right()
        out["wpp_schedule"] = {"pictures": PICTURES, "rows": ROWS, "sync_at": a.sync_at,
                               "predicted": "%d prefix launches of %d substreams each, plus one full launch" % (ROWS - 1, PICTURES)}
    hip.close()

    merged = {}
    if os.path.exists(a.out):
        try:
            merged = json.load(open(a.out))
        except ValueError:
            merged = {}
    merged[a.label] = out
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({a.label: out}))


if __name__ == "__main__":
    main()
