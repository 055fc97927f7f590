#!/usr/bin/env python3
"""One search round on the device against costing the same candidates only.

Workload: the blocks of build_residual_tiles(N) (N = 4096: the bench's residual leg).  Every block is a GROUP of G candidates
(G = 2, 4, 8), one block per candidate: the block itself, then copies with the coefficients below a rising threshold zeroed
(copy j keeps |c| >= j + 1, or the block's largest levels where that would leave it empty).  64 start sets (ctx_init of 64
(qp, init) pairs) shared by the groups, device buffers resident.
  estimate_only  cabac_hip_estimate_residual_device on exactly these candidates — an entry point every commit since the
                 estimator has; run this leg on the parent commit as well (--leg estimate_only --label parent)
  round          cabac_hip_search_round_device with an out set per group (sets 64 .. 64 + groups - 1 of the same arrays)
Times are HIP events from cabac_hip_profile_enable (the library's launches only), 3 warm-up + R timed repetitions; median,
minimum and spread (max - min) per leg, and per part of a round (kinds 17 estimate, 16 select, 18 commit).
Writes one JSON object (--out, default profiles/search_round.json; merged with what the file holds under other labels).  When
the file holds a `parent` label, the ratios round / estimate_only(parent) are written against the expectation
round <= estimate_only(parent) * (1 + 1 / G) + spread of the parent's repetitions.

  python tools/bench_search_round.py [--tiles 4096] [--reps 10] [--groups 2,4,8] [--leg both|estimate_only|round] [--label NAME]
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

N_SETS = 64
LAMBDA_Q16 = int(1.5 * (1 << 16))


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms_spread": max(ms) - min(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--groups", default="2,4,8")
    ap.add_argument("--leg", default="both", choices=["both", "estimate_only", "round"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_round.json"))
    a = ap.parse_args()
    assert a.reps >= 10

    tus, coeff, _ = build_residual_tiles(a.tiles)
    n, n_coeff = len(tus), len(coeff)
    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    sizes = (1 << (tus["log2_width"].astype(np.int64) + tus["log2_height"].astype(np.int64)))
    t_base = dev(coeff, np.int32)
    t_block = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.from_numpy(sizes).cuda())
    t_mag = t_base.abs()
    t_top = torch.zeros(n, dtype=torch.int32, device="cuda").scatter_reduce_(0, t_block, t_mag, "amax")[t_block]
    t_qp = torch.arange(N_SETS, dtype=torch.int32, device="cuda") % 52 + 10
    t_init = (torch.arange(N_SETS, dtype=torch.int32, device="cuda") % 3).contiguous()
    out = {"tiles": a.tiles, "groups": n, "coefficients_per_copy": int(n_coeff), "start_sets": N_SETS, "reps": a.reps,
           "lambda_q16": LAMBDA_Q16, "device": torch.cuda.get_device_name(0)}

    def timed(run, kinds):
        for _ in range(3):
            run()
        hip.synchronize()
        hip.profile_enable(8)
        samples = []
        for _ in range(a.reps):
            run()
            s = hip.profile_read()
            assert [k for k, _ in s] == kinds, s
            samples.append([ms for _, ms in s])
        hip.profile_enable(0)
        return samples

    for G in [int(g) for g in a.groups.split(",")]:
        n_cand = n * G
        # the candidates: copy j of every block behind copy j - 1, candidate b * G + j = copy j of block b
        t_co = torch.empty(G * n_coeff, dtype=torch.int32, device="cuda")
        for j in range(G):
            keep = t_mag >= torch.clamp(t_top, max=j + 1)
            t_co[j * n_coeff:(j + 1) * n_coeff] = torch.where(keep, t_base, torch.zeros_like(t_base))
            del keep
        ctus = np.repeat(tus, G)
        ctus["coeff_offset"] += np.tile(np.arange(G, dtype=np.uint64) * np.uint64(n_coeff), n)
        t_tu = dev(ctus, np.uint8)
        t_first = torch.arange(n_cand + 1, dtype=torch.int32, device="cuda")
        t_gfirst = (torch.arange(n + 1, dtype=torch.int32, device="cuda") * G).contiguous()
        t_set = (torch.arange(n, dtype=torch.int32, device="cuda") * 37 % N_SETS).repeat_interleave(G).contiguous()
        t_bits = torch.zeros(n_cand, dtype=torch.int64, device="cuda")
        res = {"candidates": n_cand, "coefficients": int(G * n_coeff)}
        t_state = torch.zeros((N_SETS + n) * capi.NUM_CTX, dtype=torch.int32, device="cuda")
        t_rate = torch.zeros((N_SETS + n) * capi.NUM_CTX, dtype=torch.uint8, device="cuda")
        hip.ctx_init_device(N_SETS, t_qp.data_ptr(), t_init.data_ptr(), t_state.data_ptr(), t_rate.data_ptr())
        hip.synchronize()

        if a.leg in ("both", "estimate_only"):
            def estimate_only():
                hip.estimate_residual_device(n_cand, t_first.data_ptr(), t_tu.data_ptr(), t_co.data_ptr(), t_state.data_ptr(),
                                             t_rate.data_ptr(), t_set.data_ptr(), t_bits.data_ptr())

            samples = timed(estimate_only, [12])
            res["estimate_only"] = stats([s[0] for s in samples])
            only_bits = t_bits.clone()
        if a.leg in ("both", "round"):
            gen = torch.Generator(device="cuda").manual_seed(1234)
            t_dist = torch.randint(0, 4096, (n_cand,), dtype=torch.int64, device="cuda", generator=gen)
            t_out = (torch.arange(n, dtype=torch.int32, device="cuda") + N_SETS).contiguous()
            t_pick = torch.zeros(n, dtype=torch.int32, device="cuda")
            t_cost = torch.zeros(n, dtype=torch.int64, device="cuda")
            t_bits.zero_()

            def one_round():
                hip.search_round_device(n, t_gfirst.data_ptr(), n_cand, t_first.data_ptr(), t_tu.data_ptr(), t_co.data_ptr(),
                                        t_state.data_ptr(), t_rate.data_ptr(), t_set.data_ptr(), t_out.data_ptr(), t_dist.data_ptr(),
                                        LAMBDA_Q16, t_bits.data_ptr(), t_pick.data_ptr(), t_cost.data_ptr())

            samples = timed(one_round, [17, 16, 18])
            res["round"] = stats([sum(s) for s in samples])
            for k, name in enumerate(("estimate", "select", "commit")):
                res["round"][name] = stats([s[k] for s in samples])
            # what the round computed, against torch on the same buffers
            rate_cost = (t_bits.to(torch.float64) * LAMBDA_Q16 / 2.0 ** 31).floor().to(torch.int64)     # exact: the products stay below 2^53
            cost = (t_dist + rate_cost).view(n, G)
            want_cost, want_pick = cost.min(1)
            first_min = (cost == want_cost[:, None]).to(torch.int32).argmax(1)
            assert torch.equal(t_cost, want_cost) and torch.equal(t_pick.to(torch.int64), first_min + torch.arange(n, device="cuda") * G)
            res["round"]["picks_per_alternative"] = torch.bincount(first_min, minlength=G).tolist()
            res["round"]["sets_written"] = n
            if a.leg == "both":
                assert torch.equal(t_bits, only_bits), "the round's costs differ from the estimator's"
                res["round"]["over_estimate_only_same_commit"] = res["round"]["ms_median"] / res["estimate_only"]["ms_median"]
            del t_dist, t_out, t_pick, t_cost
        out["G%d" % G] = res
        del t_co, t_tu, t_first, t_gfirst, t_set, t_bits, t_state, t_rate
        torch.cuda.empty_cache()
    hip.close()

    merged = {}
    if os.path.exists(a.out):
        try:
            merged = json.load(open(a.out))
        except ValueError:
            merged = {}
    merged[a.label] = out
    # the expectation of the design: round <~ estimate_only(parent) * (1 + 1 / G), slack = the parent leg's own spread
    par = merged.get("parent", {})
    if a.label != "parent" and a.leg != "estimate_only":
        for key, res in out.items():
            if not key.startswith("G") or "round" not in res or "estimate_only" not in par.get(key, {}):
                continue
            G, p = int(key[1:]), par[key]["estimate_only"]
            bound = p["ms_median"] * (1.0 + 1.0 / G) + p["ms_spread"]
            res["round"]["over_parent_estimate_only"] = res["round"]["ms_median"] / p["ms_median"]
            res["round"]["expected_at_most"] = 1.0 + 1.0 / G
            res["round"]["bound_ms"] = bound
            res["round"]["within_expectation"] = res["round"]["ms_median"] <= bound
            res["round"]["ms_over_bound"] = max(0.0, res["round"]["ms_median"] - bound)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({a.label: out}))


if __name__ == "__main__":
    main()
