#!/usr/bin/env python3
"""Probe points next to the calls they are measured against (include/cabac_hip_probe.h).

Workload: the C4 batch of BASELINE.json (4 096 substreams x 16 384 records from cabac_synth_records), device buffers resident.
Legs, each timed with a pair of HIP events around the call on the ctx's stream, W warm-up + R timed repetitions, medians and
minima, all from the same run:
  written_bits, written_bits_no_probe      cabac_hip_written_bits_device with one probe per 1 024 records / with n_probe == 0
  encode_v4                                cabac_hip_encode_device with set_variant forcing the baseline encode_kernel_v4
  encode_dispatch                          cabac_hip_encode_device as dispatched
  estimate                                 cabac_hip_estimate_device
  estimate_probes, estimate_probes_no_probe  cabac_hip_estimate_probes_device, the same two probe lists
What to expect: the written-bits walk is phase (a) plus a chain without low, flush checks and stores, so it should not be slower
than encode_v4; the estimate with one probe per 64 steps sends 1/64 of its steps down the ordered path: within 10 % of the plain
estimate.  The JSON says whether each expectation held.  The last probe of every substream is checked against the encoder's
CABAC_SUB_PROBE answer and the estimator's total.
Writes one JSON object (--out, default profiles/probes.json).

  python tools/bench_probes.py [--reps 20] [--warmup 3] [--every 1024]
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
    ap.add_argument("--every", type=int, default=1024, help="records between two probes of a substream")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probes.json"))
    a = ap.parse_args()
    desc, records, total = build_batch(CONFIGS["C4"])
    n = len(desc)
    lens = desc["n_records"].astype(np.int64)
    per = [np.arange(a.every, int(m) + 1, a.every, dtype=np.uint32) for m in lens]      # the last one sits at the end
    first = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.uint32)
    at = np.concatenate(per).astype(np.uint32)
    n_probe = len(at)
    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_desc, t_rec = dev(desc), dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    probe_desc = desc.copy()
    probe_desc["init_id"] = (probe_desc["init_id"] & 3) | capi.SUB_PROBE
    t_pdesc = dev(probe_desc)
    t_first, t_at, t_none = dev(first), dev(at), dev(np.zeros(n + 1, np.uint32))
    t_bytes = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    t_res = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    t_bits = torch.zeros(n_probe + 1, dtype=torch.int32, device="cuda")
    t_frac = torch.zeros(n_probe + 1, dtype=torch.int64, device="cuda")
    t_tot = torch.zeros(n, dtype=torch.int64, device="cuda")
    t_flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    D, R, PD = t_desc.data_ptr(), t_rec.data_ptr(), t_pdesc.data_ptr()
    out = {"device": torch.cuda.get_device_name(0), "substreams": n, "records": int(lens.sum()), "probes": n_probe,
           "records_per_probe": a.every, "reps": a.reps}

    out["written_bits"] = timed(lambda: hip.written_bits_device(n, D, R, t_first.data_ptr(), t_at.data_ptr(), n_probe, t_bits.data_ptr(),
                                                                t_flags.data_ptr()), a.warmup, a.reps)
    hip.synchronize()
    assert not t_flags.cpu().numpy().any()
    bits = t_bits.cpu().numpy()[:n_probe].view(np.uint32)
    out["written_bits_no_probe"] = timed(lambda: hip.written_bits_device(n, D, R, t_none.data_ptr(), 0, 0, 0, t_flags.data_ptr()),
                                         a.warmup, a.reps)
    for name, variant in (("encode_v4", 4), ("encode_dispatch", 0)):
        hip.set_variant(variant, 0)
        out[name] = timed(lambda: hip.encode_device(n, D, R, t_bytes.data_ptr(), t_res.data_ptr()), a.warmup, a.reps)
        hip.synchronize()
        assert not t_res.cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any()
    hip.encode_device(n, PD, R, t_bytes.data_ptr(), t_res.data_ptr())                   # the encoder's own probe: the last values
    hip.synchronize()
    ends = first[1:] - 1
    whole = lens % a.every == 0                                                         # substreams whose last probe sits at the end
    own = t_res.cpu().numpy().view(capi.RESULT_DTYPE)["n_bits"]
    out["last_probe_equals_sub_probe"] = bool(np.array_equal(bits[ends[whole]], own[whole]))
    assert out["last_probe_equals_sub_probe"]

    out["estimate"] = timed(lambda: hip.estimate_device(n, D, R, t_tot.data_ptr(), t_flags.data_ptr()), a.warmup, a.reps)
    out["estimate_probes"] = timed(lambda: hip.estimate_probes_device(n, D, R, t_first.data_ptr(), t_at.data_ptr(), n_probe,
                                                                      t_frac.data_ptr(), t_flags.data_ptr()), a.warmup, a.reps)
    hip.synchronize()
    assert not t_flags.cpu().numpy().any()
    frac = t_frac.cpu().numpy()[:n_probe]
    out["last_probe_equals_estimate"] = bool(np.array_equal(frac[ends[whole]], t_tot.cpu().numpy()[whole]))
    assert out["last_probe_equals_estimate"]
    out["estimate_probes_no_probe"] = timed(lambda: hip.estimate_probes_device(n, D, R, t_none.data_ptr(), 0, 0, 0, t_flags.data_ptr()),
                                            a.warmup, a.reps)
    w, e4 = out["written_bits"]["ms_median"], out["encode_v4"]["ms_median"]
    ep, e = out["estimate_probes"]["ms_median"], out["estimate"]["ms_median"]
    out["written_bits_over_encode_v4"] = w / e4
    out["written_bits_not_slower_than_encode_v4"] = bool(w <= e4)
    out["estimate_probes_over_estimate"] = ep / e
    out["estimate_probes_within_10_percent"] = bool(ep <= 1.10 * e)
    hip.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
