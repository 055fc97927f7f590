#!/usr/bin/env python3
"""The plan parse in pieces (include/cabac_hip_plan_resume.h) beside the one-call plan parse with sets.

Workload: that of tools/bench_plan_rows.py — build_residual_tiles(N) (N = 4096: the bench's residual leg), one substream per tile
of 400 blocks; the plan of a tile is one cbf bin (1) per block with the block behind it, guarded by that cbf, and the terminate
bin.  Device buffers resident; the payload is made by the device's own writer.  Legs, ALTERNATING in one run (rep by rep):
  one_call     cabac_hip_plan_parse_sets_device, every substream from Ctx::init, writing an out set
  pieces_1     cabac_hip_plan_resume_parse_device, one final piece from a fresh state: the cost of the instantiation itself
  pieces_4     the same substreams in 4 equal pieces (100 cbfs and their blocks each; the terminate bin in the last): 4 launches,
               state and contexts handed over in place
  pieces_16    in 16 equal pieces (25 blocks: the "CTU" of tools/bench_plan_rows.py)
Before anything is timed every leg runs once and its values, coefficients, results and out sets are compared with the one call's.
Times are HIP events from cabac_hip_profile_enable around the launches of a leg, 2 warm-up + R timed rounds; median, minimum,
maximum of the per-round sum, and the median of every launch of a leg on its own.

EXPECTATION, stated before the run: four pieces cost at most 1.10 x the one-call form timed in the same run — the bound
profiles/pieces.json held the bin codec's pieces to.  Every piece initialises 379 contexts and the LDS tables again, so the
per-launch floor may dominate; the ratio is reported either way (met / MISSED), with the 1-piece and 16-piece ratios.  The bound is
no gate.

Writes one JSON object (--out, default profiles/plan_resume.json).

  python tools/bench_plan_resume.py [--tiles 4096] [--reps 7] [--out FILE]
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
from entropy_coding_amd.workload import build_residual_tiles  # noqa: E402

QP = 32
NO = capi.CTX_NO_SET
BOUND = 1.10
PIECES = (1, 4, 16)


def dev(a, dt=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_resume.json"))
    a = ap.parse_args()
    assert a.reps >= 3
    print("expectation: pieces_4 <= %.2f x one_call (sum of the launches, median of %d rounds, same run)" % (BOUND, a.reps), flush=True)

    tus, coeff, _ = build_residual_tiles(a.tiles)
    n, n_sub = len(tus), a.tiles
    per_tile = n // n_sub
    assert per_tile * n_sub == n and all(per_tile % p == 0 for p in PIECES)
    n_el = per_tile + 1
    plan = np.zeros((n_sub, n_el, 2), np.uint32)
    plan[:, :-1, 0] = capi.element(capi.SE_CTX_BIN, ctx=0)
    plan[:, -1, 0] = capi.SE_TRM
    values = np.ones((n_sub, n_el), np.uint32)
    tu_at = np.tile(np.arange(per_tile, dtype=np.uint32) + 1, n_sub)      # block k behind its cbf, entry k
    tu_guard = np.full(n, capi.guard(1, capi.GUARD_EQ, 1), np.uint32)
    desc = np.zeros(n_sub, capi.DESC_DTYPE)
    desc["rec_offset"], desc["n_records"], desc["qp"] = np.arange(n_sub, dtype=np.uint64) * n_el, n_el, QP
    desc["init_id"] = 2 | capi.SUB_FINISH | capi.SUB_ALIGN_RBSP

    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_desc, t_plan, t_vin = dev(desc), dev(plan, np.int32), dev(values, np.int32)
    t_first = (torch.arange(n_sub + 1, device="cuda", dtype=torch.int32) * per_tile).contiguous()
    t_tu, t_at, t_gd, t_co = dev(tus), dev(tu_at, np.int32), dev(tu_guard, np.int32), dev(coeff, np.int32)
    cap = int(len(coeff)) + 64 * n_sub
    t_off = torch.zeros(n_sub + 1, dtype=torch.int64, device="cuda")
    t_res = torch.zeros(2 * n_sub, dtype=torch.int32, device="cuda")
    t_val = torch.zeros(n_sub * n_el, dtype=torch.int32, device="cuda")
    t_info = torch.zeros(n, dtype=torch.int32, device="cuda")
    t_dec = torch.zeros_like(t_co)
    t_state = torch.zeros(n_sub * capi.NUM_CTX, dtype=torch.int32, device="cuda")
    t_rate = torch.zeros(n_sub * capi.NUM_CTX, dtype=torch.uint8, device="cuda")
    t_noset = dev(np.full(n_sub, NO, np.uint32), np.int32)
    t_own = dev(np.arange(n_sub, dtype=np.uint32), np.int32)
    t_coder = torch.zeros(32 * n_sub, dtype=torch.uint8, device="cuda")
    pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")

    # the payload, by the device's own writer, in 16-aligned byte slots
    hip.write_plan_device(n_sub, t_desc.data_ptr(), t_plan.data_ptr(), t_vin.data_ptr(), t_first.data_ptr(), n, t_tu.data_ptr(),
                          t_at.data_ptr(), t_gd.data_ptr(), t_co.data_ptr(), pay.data_ptr(), cap, t_off.data_ptr(), t_res.data_ptr(),
                          t_val.data_ptr(), t_info.data_ptr())
    hip.synchronize()
    assert not t_res.cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any()
    off = t_off.cpu().numpy()
    lens = np.diff(off).astype(np.uint64)
    slots = (lens + 15) // 16 * 16 + 16
    d = desc.copy()
    d["byte_offset"], d["byte_capacity"], d["init_id"] = np.concatenate([[0], np.cumsum(slots)[:-1]]), lens, 2 | capi.SUB_FINISH
    host, buf = pay[:int(off[-1])].cpu().numpy(), np.zeros(int(slots.sum()), np.uint8)
    for s in range(n_sub):
        buf[int(d["byte_offset"][s]):int(d["byte_offset"][s]) + int(lens[s])] = host[int(off[s]):int(off[s + 1])]
    t_d, t_b = dev(d), dev(buf)

    # the pieces: piece p of substream s is the cbfs [p L, (p + 1) L) with their blocks (block k stands at entry k + 1, so it goes
    # with its cbf; positions relative to the piece), the last one with the terminate bin.  The blocks of a launch lie in substream
    # order, so every piece count has its own copy of the block descriptors, ordered (piece, substream, block).
    launches = {}
    tus_v = np.ascontiguousarray(tus).view(np.uint8).reshape(n_sub, per_tile, -1)
    for P in PIECES:
        L = per_tile // P
        ls = []
        for p in range(P):
            dp = d.copy()
            dp["rec_offset"] = d["rec_offset"] + p * L
            dp["n_records"] = L + (1 if p == P - 1 else 0)
            dp["init_id"] = 2 | (capi.SUB_FINISH if p == P - 1 else 0)
            t_tu_p = dev(tus_v[:, p * L:(p + 1) * L])
            t_at_p = dev(np.tile(np.arange(L, dtype=np.uint32) + 1, n_sub), np.int32)
            t_first_p = (torch.arange(n_sub + 1, device="cuda", dtype=torch.int32) * L).contiguous()
            ls.append((dev(dp), t_first_p, t_tu_p, t_at_p, p))
        launches[P] = ls
    sets_kw = dict(n_sets=n_sub, d_state=t_state.data_ptr(), d_rate=t_rate.data_ptr(), d_out_set=t_own.data_ptr(),
                   d_out_state=t_state.data_ptr(), d_out_rate=t_rate.data_ptr())

    def one_call():
        hip.plan_parse_sets_device(n_sub, t_d.data_ptr(), t_b.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), t_at.data_ptr(),
                                   t_gd.data_ptr(), t_plan.data_ptr(), t_dec.data_ptr(), t_val.data_ptr(), t_res.data_ptr(),
                                   d_start_set=t_noset.data_ptr(), **sets_kw)

    def pieces(P):
        for t_dp, t_first_p, t_tu_p, t_at_p, p in launches[P]:
            hip.plan_resume_parse_device(n_sub, t_dp.data_ptr(), t_b.data_ptr(), t_first_p.data_ptr(), t_tu_p.data_ptr(), t_at_p.data_ptr(),
                                         t_gd.data_ptr(), t_plan.data_ptr(), t_dec.data_ptr(), t_val.data_ptr(), t_res.data_ptr(),
                                         d_start_set=(t_noset if p == 0 else t_own).data_ptr(), **sets_kw,
                                         d_coder_in=t_coder.data_ptr(), d_coder_out=t_coder.data_ptr())

    legs = [("one_call", one_call)] + [("pieces_%d" % P, (lambda P=P: pieces(P))) for P in PIECES]

    def clear():
        for t in (t_dec, t_val, t_res, t_state, t_rate, t_coder):
            t.zero_()

    # the outputs first: every leg gives what the one call gives
    want = None
    for name, run in legs:
        clear()
        run()
        hip.synchronize()
        got = [t.clone() for t in (t_dec, t_val, t_res, t_state, t_rate)]
        assert not t_res.cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any(), name
        assert bool(torch.equal(t_dec, t_co)) and bool(torch.equal(t_val, t_vin)), name + ": values or coefficients did not come back"
        if want is None:
            want = got
        assert all(bool(torch.equal(x, y)) for x, y in zip(got, want)), name + ": not the one call's outputs"
        if name != "one_call":
            kinds = t_coder.cpu().numpy().view(capi.CODER_STATE_DTYPE)["kind"]
            assert (kinds == capi.CODER_CLOSED).all(), name

    samples = {name: [] for name, _ in legs}
    n_launch, per_launch = {}, {}
    for rep in range(-2, a.reps):
        for name, run in legs:                                      # alternating: every round runs every leg
            clear()
            hip.synchronize()
            hip.profile_enable(64)
            run()
            hip.synchronize()
            got = hip.profile_read()
            hip.profile_enable(0)
            n_launch[name] = len(got)
            if rep >= 0:
                samples[name].append(sum(ms for _, ms in got))
                per_launch.setdefault(name, []).append([ms for _, ms in got])

    out = {"tiles": n_sub, "blocks": n, "plan_entries": int(n_sub * n_el), "coded_bytes": int(lens.sum()), "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "outputs_equal_one_call": True}
    for name, _ in legs:
        out[name] = dict(stats(samples[name]), launches=n_launch[name],
                         ms_per_launch_median=[statistics.median(col) for col in zip(*per_launch[name])])
    base = out["one_call"]["ms_median"]
    for P in PIECES:
        out["pieces_%d_over_one_call" % P] = out["pieces_%d" % P]["ms_median"] / base
    ratio = out["pieces_4_over_one_call"]
    out["expectation"] = {"text": "pieces_4 <= %.2f x one_call, same run" % BOUND, "bound": BOUND, "ratio": ratio,
                          "verdict": "met" if ratio <= BOUND else "MISSED"}
    hip.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("expectation %s: pieces_4 / one_call = %.3f (pieces_1 %.3f, pieces_16 %.3f)" %
          (out["expectation"]["verdict"], ratio, out["pieces_1_over_one_call"], out["pieces_16_over_one_call"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
