#!/usr/bin/env python3
"""The bin codec in pieces next to the one-call forms (include/cabac_hip_pieces.h).

Workload: the C4 batch of BASELINE.json (4 096 substreams x 16 384 bins), device buffers resident, every substream from a context
set of its own and writing its contexts back.  Legs, all in ONE run and alternating (every repetition runs every leg once, so
that what else the machine is doing falls on all of them alike); each leg is timed with a pair of HIP events around its launches
on the ctx's stream, W warm-up + R timed repetitions, medians and minima:
  pieces_K     cabac_hip_encode_pieces_device / cabac_hip_decode_pieces_device with K = 1, 4 and 16 equal pieces per substream:
               K launches, the contexts handed over through the substream's set, the coder states in place
  v4           cabac_hip_encode_sets_device / cabac_hip_decode_sets_device under forced variant 4 (the geometries the pieces calls
               instantiate), one call
  dispatch     the same calls as the dispatch chooses them, for orientation
The bytes, results, bins and out sets of every pieces leg are compared with the v4 leg's before anything is timed.

Expectation (stated before the run; reported as met or MISSED): four pieces cost at most 1.10 x the v4 one-call time, for encode
and for decode.  Per piece the extra work is one launch, one load and one export of 379 context words per substream, the
decoder's table and ring set-up and one partial trip.
Writes one JSON object (--out, default profiles/pieces.json).

  python tools/bench_pieces.py [--reps 15] [--warmup 2] [--out FILE]
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

PIECES = (1, 4, 16)
BOUND = 1.10


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="C4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pieces.json"))
    a = ap.parse_args()
    desc, records, total = build_batch(CONFIGS[a.config])
    n = len(desc)
    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_rec = dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    t_res = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    t_bins = torch.zeros(len(records) + 16, dtype=torch.uint8, device="cuda")
    t_enc = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")      # what the encode legs write
    # the start sets (never written) and the sets the substreams write and, between pieces, start from
    t_qp, t_iid = dev(desc["qp"].astype(np.int32)), dev((desc["init_id"] & 3).astype(np.uint32))
    t_state = torch.zeros(n * capi.NUM_CTX, dtype=torch.int32, device="cuda")
    t_rate = torch.zeros(n * capi.NUM_CTX, dtype=torch.uint8, device="cuda")
    hip.ctx_init_device(n, t_qp.data_ptr(), t_iid.data_ptr(), t_state.data_ptr(), t_rate.data_ptr())
    t_ostate, t_orate = torch.zeros_like(t_state), torch.zeros_like(t_rate)
    t_idx = dev(np.arange(n, dtype=np.uint32))
    t_coder = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
    first_sets = (n, t_state.data_ptr(), t_rate.data_ptr(), t_idx.data_ptr(), t_idx.data_ptr(), t_ostate.data_ptr(), t_orate.data_ptr())
    next_sets = (n, t_ostate.data_ptr(), t_orate.data_ptr(), t_idx.data_ptr(), t_idx.data_ptr(), t_ostate.data_ptr(), t_orate.data_ptr())
    t_desc = dev(desc)

    def piece_descs(k):
        out = []
        for i in range(k):
            d = desc.copy()
            lo = desc["n_records"].astype(np.uint64) * i // k
            hi = desc["n_records"].astype(np.uint64) * (i + 1) // k
            d["rec_offset"] = desc["rec_offset"] + lo
            d["n_records"] = hi - lo
            if i < k - 1:
                d["init_id"] = desc["init_id"] & 3
            out.append(dev(d))
        return out

    descs = {k: piece_descs(k) for k in PIECES}

    def pieces(k, decode, t_bytes):
        for i, d in enumerate(descs[k]):
            sets = first_sets if i == 0 else next_sets
            cin = 0 if i == 0 else t_coder.data_ptr()
            if decode:
                hip.decode_pieces_device(n, d.data_ptr(), t_rec.data_ptr(), t_bytes.data_ptr(), t_bins.data_ptr(), t_res.data_ptr(), *sets,
                                         cin, t_coder.data_ptr())
            else:
                hip.encode_pieces_device(n, d.data_ptr(), t_rec.data_ptr(), t_bytes.data_ptr(), t_res.data_ptr(), *sets, cin, t_coder.data_ptr())

    def one_call(variant, decode, t_bytes):
        hip.set_variant(variant, variant)
        if decode:
            hip.decode_sets_device(n, t_desc.data_ptr(), t_rec.data_ptr(), t_bytes.data_ptr(), t_bins.data_ptr(), t_res.data_ptr(), *first_sets)
        else:
            hip.encode_sets_device(n, t_desc.data_ptr(), t_rec.data_ptr(), t_bytes.data_ptr(), t_res.data_ptr(), *first_sets)

    # ---- the reference of this run: the v4 one-call forms
    one_call(4, False, t_enc)
    hip.synchronize()
    ref_res = t_res.clone()
    assert not ref_res.cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any()
    ref_bytes, ref_state = t_enc.clone(), t_ostate.clone()
    one_call(4, True, ref_bytes)
    hip.synchronize()
    ref_dres, ref_bins = t_res.clone(), t_bins.clone()
    assert not ref_dres.cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any() and torch.equal(ref_state, t_ostate)
    out = {"device": torch.cuda.get_device_name(0), "config": a.config, "substreams": n, "bins": int(desc["n_records"].sum()),
           "reps": a.reps, "warmup": a.warmup, "equal_to_v4_one_call": {}}
    for k in PIECES:
        t_enc.zero_()
        t_ostate.zero_()
        pieces(k, False, t_enc)
        hip.synchronize()
        ok = bool(torch.equal(t_enc, ref_bytes) and torch.equal(t_res, ref_res) and torch.equal(t_ostate, ref_state))
        t_bins.zero_()
        t_ostate.zero_()
        pieces(k, True, ref_bytes)
        hip.synchronize()
        ok = ok and bool(torch.equal(t_bins, ref_bins) and torch.equal(t_res, ref_dres) and torch.equal(t_ostate, ref_state))
        out["equal_to_v4_one_call"]["pieces_%d" % k] = ok
        assert ok, k

    # ---- the timed legs, alternating
    legs = {}
    for k in PIECES:
        legs["pieces_%d_encode" % k] = lambda k=k: pieces(k, False, t_enc)
        legs["pieces_%d_decode" % k] = lambda k=k: pieces(k, True, ref_bytes)
    legs["v4_encode"] = lambda: one_call(4, False, t_enc)
    legs["v4_decode"] = lambda: one_call(4, True, ref_bytes)
    legs["dispatch_encode"] = lambda: one_call(0, False, t_enc)
    legs["dispatch_decode"] = lambda: one_call(0, True, ref_bytes)
    ms = {name: [] for name in legs}
    for rep in range(a.warmup + a.reps):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    hip.set_variant(0, 0)
    hip.close()
    for name, v in ms.items():
        out[name] = {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}
    exp = {}
    for coder in ("encode", "decode"):
        ratio = out["pieces_4_%s" % coder]["ms_median"] / out["v4_%s" % coder]["ms_median"]
        exp[coder] = {"pieces_4_over_v4_one_call": round(ratio, 4), "bound": BOUND, "outcome": "met" if ratio <= BOUND else "MISSED"}
    out["expectation"] = exp
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
