#!/usr/bin/env python3
"""The pieces under both encoders (include/cabac_hip_piece_encoder.h) next to the one-call forms.

Workload: the C4 batch of BASELINE.json (4 096 substreams x 16 384 bins), device buffers resident, every substream from a context
set of its own and writing its contexts back — the batch of tools/bench_pieces.py.  Legs, all in ONE run and alternating (every
repetition runs every leg once, so that what else the machine is doing falls on all of them alike); each leg is timed with a pair
of HIP events around its launches on the ctx's stream, W warm-up + R timed repetitions, medians, minima and maxima:
  enc4_pieces_K, enc7_pieces_K   cabac_hip_encode_pieces_device with K = 1, 4 and 16 equal pieces per substream under
                                 cabac_hip_piece_encoder_set(ctx, 4) and (ctx, 7): K launches, the contexts handed over through
                                 the substream's set, the coder states in place
  v4_one_call                    cabac_hip_encode_sets_device under forced variant 4
  dispatch_one_call              the same call as the dispatch chooses it (v7)
  sizes: enc4_n_N, enc7_n_N      the 4-piece form on the first N = 256, 1 024, 2 048 substreams of the batch under both settings
                                 (N = 4 096 is enc*_pieces_4): the smallest N from which 7 is the faster one is the threshold of
                                 setting 0 (0 if 7 never loses)
The bytes, results, out sets and states of every pieces leg are compared with the v4 one call's (and between the settings) before
anything is timed.

Expectation (stated before the run; reported as met or MISSED): four pieces under setting 7 cost at most 1.10 x the one-call
form of the same kernel, which is the dispatched one.  No gate.
Writes one JSON object (--out, default profiles/piece_encoder.json).

  python tools/bench_piece_encoder.py [--reps 15] [--warmup 2] [--out FILE]
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
SIZES = (256, 1024, 2048)
SETTINGS = (4, 7)
BOUND = 1.10


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="C4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "piece_encoder.json"))
    a = ap.parse_args()
    print("expectation: enc7_pieces_4 <= %.2f x dispatch_one_call (medians of %d repetitions, same run)" % (BOUND, a.reps), flush=True)
    desc, records, total = build_batch(CONFIGS[a.config])
    n = len(desc)
    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_rec = dev(np.concatenate([records, np.zeros(8, np.uint16)]))
    t_res = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    t_enc = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
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

    def pieces(setting, k, n_sub=n):
        hip.piece_encoder_set(setting)
        for i, d in enumerate(descs[k]):
            sets = first_sets if i == 0 else next_sets
            cin = 0 if i == 0 else t_coder.data_ptr()
            hip.encode_pieces_device(n_sub, d.data_ptr(), t_rec.data_ptr(), t_enc.data_ptr(), t_res.data_ptr(), *sets, cin, t_coder.data_ptr())

    def one_call(variant):
        hip.set_variant(variant, 0)
        hip.encode_sets_device(n, t_desc.data_ptr(), t_rec.data_ptr(), t_enc.data_ptr(), t_res.data_ptr(), *first_sets)

    # ---- the reference of this run: the v4 one-call form
    one_call(4)
    hip.synchronize()
    ref_res = t_res.clone()
    assert not ref_res.cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any()
    ref_bytes, ref_state, ref_rate = t_enc.clone(), t_ostate.clone(), t_orate.clone()
    out = {"device": torch.cuda.get_device_name(0), "config": a.config, "substreams": n, "bins": int(desc["n_records"].sum()),
           "reps": a.reps, "warmup": a.warmup, "equal_to_v4_one_call": {}}
    for k in PIECES:
        states = {}
        for setting in SETTINGS:
            for t in (t_enc, t_ostate, t_orate, t_coder, t_res):
                t.zero_()
            pieces(setting, k)
            hip.synchronize()
            ok = bool(torch.equal(t_enc, ref_bytes) and torch.equal(t_res, ref_res) and torch.equal(t_ostate, ref_state) and
                      torch.equal(t_orate, ref_rate))
            states[setting] = t_coder.clone()
            out["equal_to_v4_one_call"]["enc%d_pieces_%d" % (setting, k)] = ok
            assert ok, (setting, k)
        assert torch.equal(states[4], states[7]), k

    # ---- the timed legs, alternating
    legs = {}
    for setting in SETTINGS:
        for k in PIECES:
            legs["enc%d_pieces_%d" % (setting, k)] = lambda s=setting, k=k: pieces(s, k)
        for m in SIZES:
            if m < n:
                legs["enc%d_n_%d" % (setting, m)] = lambda s=setting, m=m: pieces(s, 4, m)
    legs["v4_one_call"] = lambda: one_call(4)
    legs["dispatch_one_call"] = lambda: one_call(0)
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
    hip.piece_encoder_set(4)
    hip.close()
    for name, v in ms.items():
        out[name] = {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}
    ratio = out["enc7_pieces_4"]["ms_median"] / out["dispatch_one_call"]["ms_median"]
    out["expectation"] = {"text": "enc7_pieces_4 <= %.2f x dispatch_one_call" % BOUND, "enc7_pieces_4_over_dispatch_one_call": round(ratio, 4),
                          "bound": BOUND, "outcome": "met" if ratio <= BOUND else "MISSED",
                          "enc4_pieces_4_over_v4_one_call": round(out["enc4_pieces_4"]["ms_median"] / out["v4_one_call"]["ms_median"], 4),
                          "enc4_pieces_4_over_enc7_pieces_4": round(out["enc4_pieces_4"]["ms_median"] / out["enc7_pieces_4"]["ms_median"], 4)}
    sizes = {}
    for m in [m for m in SIZES if m < n] + [n]:
        t4 = out["enc4_n_%d" % m if m < n else "enc4_pieces_4"]["ms_median"]
        t7 = out["enc7_n_%d" % m if m < n else "enc7_pieces_4"]["ms_median"]
        sizes[str(m)] = {"enc4_ms": t4, "enc7_ms": t7, "enc7_faster": t7 < t4}
    order = sorted(int(m) for m in sizes)
    threshold = None
    for m in reversed(order):                  # the smallest measured size from which 7 is faster at every larger one too
        if not sizes[str(m)]["enc7_faster"]:
            break
        threshold = m
    if threshold == order[0]:
        threshold = 0                          # 7 never loses
    out["setting_0"] = {"four_pieces_by_substreams": sizes, "threshold": threshold}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
