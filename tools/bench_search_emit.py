#!/usr/bin/env python3
"""The winner log against the round that feeds it, against a plain copy of the same bytes, and against the encode it ends in.

Workload: that of tools/bench_search_unit.py — the blocks of build_residual_tiles(N) (N = 4096), every block a GROUP of G = 4
candidates of one block each, 64 start sets, an out set and a CHAIN per group, empty side runs, device buffers resident.  Legs,
alternating in one process, 3 warm-up + R timed repetitions each, all times from HIP events on the ctx's stream:
  round        cabac_hip_search_unit_round_device (kinds 20 / 21 / 22 of cabac_hip_profile_read) — code this change does not touch;
               run this file in a checkout of the parent with --leg round --label parent to show that it did not move
  append       cabac_hip_search_log_append_device of that round's picks into an emptied log (kind 23)
  memcpy       one device-to-device hipMemcpyAsync of exactly the bytes the append moved (coefficients, descriptors, positions,
               records), between two events
  log_encode   cabac_hip_search_log_encode_device of the filled log, between two events (its two waits for the stream included)
  encode       cabac_hip_encode_residual_device on the same strings and splices prepared by the host, between two events;
               log_encode - encode is the place step and the first wait
Writes one JSON object (--out, default profiles/search_emit.json; merged with what the file holds under other labels) with two
ratios: append / round — and append / the round's commit part, kind 22, which re-walks the same winners — and append / memcpy,
whose margin is memcpy's own (median - min) / median: nothing tighter can be claimed.

  python tools/bench_search_emit.py [--tiles 4096] [--reps 10] [--leg all|round] [--label NAME] [--out FILE]
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

N_SETS, G = 64, 4
LAMBDA_Q16 = int(1.5 * (1 << 16))


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms_spread": max(ms) - min(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--leg", default="all", choices=["all", "round"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_emit.json"))
    a = ap.parse_args()
    assert a.reps >= 10

    tus, coeff, _ = build_residual_tiles(a.tiles)
    n, n_coeff = len(tus), len(coeff)
    n_cand = n * G
    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    sizes = (1 << (tus["log2_width"].astype(np.int64) + tus["log2_height"].astype(np.int64)))
    t_base = dev(coeff, np.int32)
    t_block = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.from_numpy(sizes).cuda())
    t_mag = t_base.abs()
    t_top = torch.zeros(n, dtype=torch.int32, device="cuda").scatter_reduce_(0, t_block, t_mag, "amax")[t_block]
    t_co = torch.empty(G * n_coeff, dtype=torch.int32, device="cuda")
    for j in range(G):
        keep = t_mag >= torch.clamp(t_top, max=j + 1)
        t_co[j * n_coeff:(j + 1) * n_coeff] = torch.where(keep, t_base, torch.zeros_like(t_base))
        del keep
    del t_block, t_mag, t_top
    ctus = np.repeat(tus, G)
    ctus["coeff_offset"] += np.tile(np.arange(G, dtype=np.uint64) * np.uint64(n_coeff), n)
    t_tu = dev(ctus, np.uint8)
    t_first = torch.arange(n_cand + 1, dtype=torch.int32, device="cuda")
    t_gfirst = (torch.arange(n + 1, dtype=torch.int32, device="cuda") * G).contiguous()
    t_set = (torch.arange(n, dtype=torch.int32, device="cuda") * 37 % N_SETS).repeat_interleave(G).contiguous()
    t_qp = torch.arange(N_SETS, dtype=torch.int32, device="cuda") % 52 + 10
    t_init = (torch.arange(N_SETS, dtype=torch.int32, device="cuda") % 3).contiguous()
    t_state = torch.zeros((N_SETS + n) * capi.NUM_CTX, dtype=torch.int32, device="cuda")
    t_rate = torch.zeros((N_SETS + n) * capi.NUM_CTX, dtype=torch.uint8, device="cuda")
    hip.ctx_init_device(N_SETS, t_qp.data_ptr(), t_init.data_ptr(), t_state.data_ptr(), t_rate.data_ptr())
    hip.synchronize()
    gen = torch.Generator(device="cuda").manual_seed(1234)
    t_dist = torch.randint(0, 4096, (n_cand,), dtype=torch.int64, device="cuda", generator=gen)
    t_out = (torch.arange(n, dtype=torch.int32, device="cuda") + N_SETS).contiguous()
    t_bits = torch.zeros(n_cand, dtype=torch.int64, device="cuda")
    t_pick = torch.zeros(n, dtype=torch.int32, device="cuda")
    t_cost = torch.zeros(n, dtype=torch.int64, device="cuda")
    t_rf = torch.zeros(n_cand + 1, dtype=torch.int64, device="cuda")
    t_chain = torch.arange(n, dtype=torch.int32, device="cuda")
    out = {"tiles": a.tiles, "groups": n, "G": G, "candidates": n_cand, "coefficients": int(G * n_coeff), "start_sets": N_SETS,
           "reps": a.reps, "lambda_q16": LAMBDA_Q16, "device": torch.cuda.get_device_name(0)}

    def one_round():
        hip.search_unit_round_device(n, t_gfirst.data_ptr(), n_cand, t_first.data_ptr(), t_tu.data_ptr(), t_co.data_ptr(),
                                     t_state.data_ptr(), t_rate.data_ptr(), t_set.data_ptr(), t_rf.data_ptr(), 0, 0, t_out.data_ptr(),
                                     t_dist.data_ptr(), LAMBDA_Q16, t_bits.data_ptr(), t_pick.data_ptr(), t_cost.data_ptr())

    def between_events(run):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    samples = {k: [] for k in ("round", "estimate", "select", "commit", "append", "memcpy", "log_encode", "encode")}
    full = a.leg == "all"
    if full:
        log = hip.search_log(n, n, 0, n, n_coeff)

        def one_append():
            log.reset()
            log.append_device(n, t_pick.data_ptr(), t_chain.data_ptr(), n_cand, t_first.data_ptr(), t_tu.data_ptr(), t_co.data_ptr(),
                              t_rf.data_ptr(), 0, 0)

        one_round()
        one_append()
        got = log.read()
        cnt = got["counters"]
        assert int(cnt["flags"]) == 0 and int(cnt["n_entry"]) == n and int(cnt["n_tu"]) == n and int(cnt["n_coeff"]) == n_coeff
        moved = int(cnt["n_coeff"]) * 4 + int(cnt["n_tu"]) * (16 + 4) + int(cnt["n_record"]) * 2
        out["append_bytes"] = moved
        t_src = torch.zeros(moved, dtype=torch.uint8, device="cuda")
        t_dst = torch.empty_like(t_src)
        # the encode's buffers, and the host's form of the same strings: chain k is block k of the log spliced at 0 into no record
        cap = 8 * n_coeff + 64 * n
        desc = np.zeros(n, capi.DESC_DTYPE)
        desc["qp"], desc["init_id"] = 30, capi.SUB_FINISH | capi.SUB_ALIGN_RBSP
        t_desc = dev(desc, np.uint8)
        t_pay = torch.empty(cap, dtype=torch.uint8, device="cuda")
        t_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        t_res = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
        t_pay2, t_off2, t_res2 = torch.empty_like(t_pay), torch.zeros_like(t_off), torch.zeros_like(t_res)
        sp = np.zeros(n, capi.SPLICE_DTYPE)
        sp["tu"] = np.arange(n)
        t_sp, t_spf = dev(sp, np.uint8), torch.arange(n + 1, dtype=torch.int32, device="cuda")
        t_norec = torch.zeros(8, dtype=torch.int16, device="cuda")
        t_ltu, t_lco = dev(got["tu"], np.uint8), dev(got["coeff"], np.int32)

        def log_encode():
            log.encode_device(t_desc.data_ptr(), t_pay.data_ptr(), cap, t_off.data_ptr(), t_res.data_ptr())

        def host_encode():
            hip.encode_residual_device(n, t_desc.data_ptr(), t_norec.data_ptr(), t_spf.data_ptr(), t_sp.data_ptr(), n, n, t_ltu.data_ptr(),
                                       t_lco.data_ptr(), t_pay2.data_ptr(), cap, t_off2.data_ptr(), t_res2.data_ptr())

    for rep in range(3 + a.reps):
        hip.profile_enable(8)
        one_round()
        if full:
            one_append()
        s = hip.profile_read()
        hip.profile_enable(0)
        assert [k for k, _ in s] == ([20, 21, 22, 23] if full else [20, 21, 22]), s
        row = {"round": sum(ms for _, ms in s[:3]), "estimate": s[0][1], "select": s[1][1], "commit": s[2][1]}
        if full:
            row["append"] = s[3][1]
            row["memcpy"] = between_events(lambda: t_dst.copy_(t_src))
            row["log_encode"] = between_events(log_encode)
            row["encode"] = between_events(host_encode)
        if rep >= 3:
            for k, v in row.items():
                samples[k].append(v)
    for k, v in samples.items():
        if v:
            out[k] = stats(v)
    if full:
        hip.synchronize()
        assert torch.equal(t_off, t_off2) and torch.equal(t_res, t_res2) and torch.equal(t_pay[:int(t_off[-1])], t_pay2[:int(t_off2[-1])])
        out["payload_bytes"] = int(t_off[-1])
        m = out["memcpy"]
        out["append_over_round"] = out["append"]["ms_median"] / out["round"]["ms_median"]
        out["append_over_commit"] = out["append"]["ms_median"] / out["commit"]["ms_median"]
        out["append_over_memcpy"] = out["append"]["ms_median"] / m["ms_median"]
        out["memcpy_min_to_median_spread"] = (m["ms_median"] - m["ms_min"]) / m["ms_median"]
        out["place_ms"] = out["log_encode"]["ms_median"] - out["encode"]["ms_median"]
        log.close()
    hip.close()

    merged = {}
    if os.path.exists(a.out):
        try:
            merged = json.load(open(a.out))
        except ValueError:
            merged = {}
    merged.pop("status", None)   # the placeholder the file holds until a first run
    merged.pop("note", None)
    merged[a.label] = out
    par =merged.get("parent", {}).get("round")
    if a.label != "parent" and par:
        out["round"]["over_parent_round"] = out["round"]["ms_median"] / par["ms_median"]
        out["parent_round_min_to_median_spread"] = (par["ms_median"] - par["ms_min"]) / par["ms_median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({a.label: out}))


if __name__ == "__main__":
    main()
