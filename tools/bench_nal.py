#!/usr/bin/env python3
"""Emulation prevention on the device next to the kernels around it.

Workloads: the C4 batch of BASELINE.json (4 096 substreams x 16 384 bins), and a low-entropy variant of the same shape (one
context, P(1) = 0.002, as in tests/test_gpu_assemble.py) in which start-code emulations really occur.  Device buffers resident.
One repetition runs, in this order and in one process,
  encode_device, assemble_device, nal_escape_device, nal_unescape_device, split_device, decode_device
so the six alternate; times are the HIP events of cabac_hip_profile_enable (the library's launches only), 3 warm-up + R timed
repetitions, medians.  GB/s are algorithmic bytes: escape / unescape read the string twice (summary pass, write pass) and write
it once; assemble / split read once and write once.
Writes one JSON object (--out, default profiles/nal_escape.json; merged with what the file holds under other labels).
Under rocprofv3 collect kernel statistics in a run of their own (--kernel-trace --stats, nothing else).

  python tools/bench_nal.py [--reps 20] [--batch both|c4|low] [--label NAME] [--out FILE]
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

KINDS = {0: "encode", 6: "assemble", 13: "nal_escape", 14: "nal_unescape", 7: "split", 1: "decode"}


def low_entropy_like(desc, records):
    """The same descriptors with every substream's records replaced: context 7, P(1) = 0.002, a terminating bin."""
    rng = np.random.default_rng(0xC4)
    rec = records.copy()
    for d in desc:
        o, n = int(d["rec_offset"]), int(d["n_records"])
        bins = (rng.random(n) < 0.002).astype(np.uint16)
        rec[o:o + n] = 7 | (bins << 15)
        rec[o + n - 1] = capi.REC_TRM | capi.REC_BIN
    return rec


def run_batch(hip, desc, records, total, reps):
    n = len(desc)
    t_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    t_rec = torch.from_numpy(records.view(np.int16)).cuda()
    t_bytes = torch.zeros(total, dtype=torch.uint8, device="cuda")
    t_res = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    t_pay = torch.zeros(total, dtype=torch.uint8, device="cuda")
    t_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    nal_cap = capi.nal_escape_bound(total)
    t_nal = torch.zeros(nal_cap, dtype=torch.uint8, device="cuda")
    t_noff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    t_st = torch.zeros(32, dtype=torch.uint8, device="cuda")
    t_back = torch.zeros(total, dtype=torch.uint8, device="cuda")
    t_boff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    t_loc = torch.zeros(total // 3 + 1, dtype=torch.int32, device="cuda")
    t_slots = torch.zeros(total, dtype=torch.uint8, device="cuda")
    t_bins = torch.zeros(len(records), dtype=torch.uint8, device="cuda")
    t_res2 = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    hip.encode_device(n, t_desc.data_ptr(), t_rec.data_ptr(), t_bytes.data_ptr(), t_res.data_ptr())
    hip.synchronize()
    res = t_res.cpu().numpy().view(capi.RESULT_DTYPE)
    assert not res["flags"].any()
    ddesc = desc.copy()
    ddesc["byte_capacity"] = (res["n_bits"] + 7) // 8
    t_ddesc = torch.from_numpy(ddesc.view(np.uint8).copy()).cuda()

    def once():
        hip.encode_device(n, t_desc.data_ptr(), t_rec.data_ptr(), t_bytes.data_ptr(), t_res.data_ptr())
        # the bounds are what a caller knows without a synchronisation: the slot total and its escape bound
        hip.assemble_device(n, t_desc.data_ptr(), t_res.data_ptr(), t_bytes.data_ptr(), t_pay.data_ptr(), total, t_off.data_ptr())
        hip.nal_escape_device(n, t_off.data_ptr(), t_pay.data_ptr(), total, t_nal.data_ptr(), nal_cap, t_noff.data_ptr(), t_st.data_ptr())
        hip.nal_unescape_device(n, t_noff.data_ptr(), t_nal.data_ptr(), nal_cap, t_back.data_ptr(), total, t_boff.data_ptr(),
                                t_st.data_ptr() + 16, d_locations=t_loc.data_ptr(), loc_capacity=len(t_loc))
        hip.split_device(n, t_ddesc.data_ptr(), t_boff.data_ptr(), t_back.data_ptr(), t_slots.data_ptr())
        hip.decode_device(n, t_ddesc.data_ptr(), t_rec.data_ptr(), t_slots.data_ptr(), t_bins.data_ptr(), t_res2.data_ptr())

    for _ in range(3):
        once()
    hip.synchronize()
    st = t_st.cpu().numpy().view(capi.NAL_STATUS_DTYPE)
    payload_bytes = int(t_off[n].item())
    assert int(st[0]["flags"]) == 0 and int(st[1]["flags"]) == 0 and int(st[1]["out_bytes"]) == payload_bytes
    assert torch.equal(t_back[:payload_bytes], t_pay[:payload_bytes]) and torch.equal(t_boff, t_off)
    assert np.array_equal(t_bins.cpu().numpy(), (records >> 15).astype(np.uint8))
    hip.profile_enable(8)
    ms = {name: [] for name in KINDS.values()}
    for _ in range(reps):
        once()
        got = hip.profile_read()
        assert [k for k, _ in got] == [0, 6, 13, 14, 7, 1], got
        for k, t in got:
            ms[KINDS[k]].append(t)
    hip.profile_enable(0)
    med = {k: statistics.median(v) for k, v in ms.items()}
    nal_bytes = int(st[0]["out_bytes"])
    out = {"substreams": n, "bins": int(desc["n_records"].sum()), "payload_bytes": payload_bytes, "nal_bytes": nal_bytes,
           "insertions": int(st[0]["n_changed"]), "payload_bytes_max": total, "reps": reps,
           "ms_median": med, "ms_min": {k: min(v) for k, v in ms.items()},
           "gb_per_s": {"nal_escape": (2 * payload_bytes + nal_bytes) / med["nal_escape"] / 1e6,
                        "nal_unescape": (2 * nal_bytes + payload_bytes) / med["nal_unescape"] / 1e6,
                        "assemble": 2 * payload_bytes / med["assemble"] / 1e6, "split": 2 * payload_bytes / med["split"] / 1e6},
           "escape_over_assemble": med["nal_escape"] / med["assemble"], "unescape_over_split": med["nal_unescape"] / med["split"],
           "escape_below_encode": med["nal_escape"] < med["encode"], "unescape_below_decode": med["nal_unescape"] < med["decode"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", default="both", choices=["both", "c4", "low"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nal_escape.json"))
    a = ap.parse_args()
    assert a.reps >= 1
    desc, records, total = build_batch(CONFIGS["C4"])
    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    out = {"device": torch.cuda.get_device_name(0)}
    if a.batch in ("both", "c4"):
        out["C4"] = run_batch(hip, desc, records, total, a.reps)
    if a.batch in ("both", "low"):
        out["C4_low_entropy"] = run_batch(hip, desc, low_entropy_like(desc, records), total, a.reps)
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
