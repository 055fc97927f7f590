#!/usr/bin/env python3
"""One search round over candidates with side records against the round over plain block candidates.

Workload: that of tools/bench_search_round.py at G = 4 — the blocks of build_residual_tiles(N) (N = 4096), every block a GROUP
of 4 candidates of one block each (the block, then copies with the coefficients below a rising threshold zeroed), 64 start
sets shared by the groups, an out set per group, device buffers resident.  Three legs:
  round          cabac_hip_search_round_device — an entry point the parent commit has too: copy this file into a checkout
                 of the parent and run it there with --leg round --label parent, writing to the same --out
  unit_empty     cabac_hip_search_unit_round_device on the same candidates with empty side runs (d_tu_at NULL)
  unit_side24    the same with 24 side records per candidate (four in five context-coded on the contexts residual coding never
                 touches, the rest bypass bins) and the block at position 8
Times are HIP events from cabac_hip_profile_enable (the library's launches only), 3 warm-up + R timed repetitions; median,
minimum and spread (max - min) per leg and per part of a round.
Writes one JSON object (--out, default profiles/search_unit.json; merged with what the file holds under other labels).  When the
file holds a `parent` label, three ratios go in: unit_empty / round(parent) — "no slower" may be claimed below 1 + the parent's own
(median - min) / median —, unit_side24 / unit_empty, and round / round(parent), which shows whether the plain kernel moved.

  python tools/bench_search_unit.py [--tiles 4096] [--reps 10] [--leg all|round|unit] [--label NAME] [--out FILE]
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

N_SETS, G, N_SIDE, AT = 64, 4, 24, 8
LAMBDA_Q16 = int(1.5 * (1 << 16))


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms_spread": max(ms) - min(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--leg", default="all", choices=["all", "round", "unit"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_unit.json"))
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
    out = {"tiles": a.tiles, "groups": n, "G": G, "candidates": n_cand, "coefficients": int(G * n_coeff), "start_sets": N_SETS,
           "reps": a.reps, "lambda_q16": LAMBDA_Q16, "device": torch.cuda.get_device_name(0)}

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
        res = stats([sum(s) for s in samples])
        for k, name in enumerate(("estimate", "select", "commit")):
            res[name] = stats([s[k] for s in samples])
        return res

    def check_picks():
        """what the round picked, against torch on the same buffers (exact: the products stay below 2^53)"""
        rate_cost = (t_bits.to(torch.float64) * LAMBDA_Q16 / 2.0 ** 31).floor().to(torch.int64)
        cost = (t_dist + rate_cost).view(n, G)
        want_cost, _ = cost.min(1)
        first_min = (cost == want_cost[:, None]).to(torch.int32).argmax(1)
        assert torch.equal(t_cost, want_cost) and torch.equal(t_pick.to(torch.int64), first_min + torch.arange(n, device="cuda") * G)
        return torch.bincount(first_min, minlength=G).tolist()

    plain_bits = None
    if a.leg in ("all", "round"):
        def one_round():
            hip.search_round_device(n, t_gfirst.data_ptr(), n_cand, t_first.data_ptr(), t_tu.data_ptr(), t_co.data_ptr(),
                                    t_state.data_ptr(), t_rate.data_ptr(), t_set.data_ptr(), t_out.data_ptr(), t_dist.data_ptr(),
                                    LAMBDA_Q16, t_bits.data_ptr(), t_pick.data_ptr(), t_cost.data_ptr())

        out["round"] = timed(one_round, [17, 16, 18])
        out["round"]["picks_per_alternative"] = check_picks()
        plain_bits = t_bits.clone()
        plain_sets = (t_state[N_SETS * capi.NUM_CTX:].clone(), t_rate[N_SETS * capi.NUM_CTX:].clone())
    if a.leg in ("all", "unit"):
        t_flags = torch.zeros(n_cand, dtype=torch.int32, device="cuda")

        def unit_round(t_rf, t_rec, t_at):
            def run():
                hip.search_unit_round_device(n, t_gfirst.data_ptr(), n_cand, t_first.data_ptr(), t_tu.data_ptr(), t_co.data_ptr(),
                                             t_state.data_ptr(), t_rate.data_ptr(), t_set.data_ptr(), t_rf.data_ptr(),
                                             t_rec.data_ptr() if t_rec is not None else 0, t_at.data_ptr() if t_at is not None else 0,
                                             t_out.data_ptr(), t_dist.data_ptr(), LAMBDA_Q16, t_bits.data_ptr(), t_pick.data_ptr(),
                                             t_cost.data_ptr(), d_flags=t_flags.data_ptr())
            return run

        t_bits.zero_()
        out["unit_empty"] = timed(unit_round(torch.zeros(n_cand + 1, dtype=torch.int64, device="cuda"), None, None), [20, 21, 22])
        out["unit_empty"]["picks_per_alternative"] = check_picks()
        assert not t_flags.any()
        if plain_bits is not None:
            assert torch.equal(t_bits, plain_bits), "the costs with empty side runs differ from the plain round's"
            assert torch.equal(t_state[N_SETS * capi.NUM_CTX:], plain_sets[0]) and torch.equal(t_rate[N_SETS * capi.NUM_CTX:], plain_sets[1])
        # 24 side records per candidate: ids 0..85 and 292..356, one in five a bypass bin
        ids = torch.randint(0, 151, (n_cand * N_SIDE,), dtype=torch.int32, device="cuda", generator=gen)
        ids = torch.where(ids < 86, ids, ids + (292 - 86))
        ids = torch.where(torch.rand(n_cand * N_SIDE, device="cuda", generator=gen) < 0.2, torch.full_like(ids, capi.REC_EP), ids)
        t_rec = (ids | (torch.randint(0, 2, ids.shape, dtype=torch.int32, device="cuda", generator=gen) << 15)).to(torch.int16)
        del ids
        t_rf = (torch.arange(n_cand + 1, dtype=torch.int64, device="cuda") * N_SIDE).contiguous()
        t_at = torch.full((n_cand,), AT, dtype=torch.int32, device="cuda")
        out["unit_side24"] = timed(unit_round(t_rf, t_rec, t_at), [20, 21, 22])
        out["unit_side24"]["picks_per_alternative"] = check_picks()
        out["unit_side24"]["side_records"] = n_cand * N_SIDE
        assert not t_flags.any()
        if plain_bits is not None:                          # at least N_SIDE * 0.2 bypass bins dearer, and never cheaper
            assert bool((t_bits > plain_bits).all())
        out["unit_side24"]["over_unit_empty"] = out["unit_side24"]["ms_median"] / out["unit_empty"]["ms_median"]
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
    par = merged.get("parent", {}).get("round")
    if a.label != "parent" and par:
        margin = (par["ms_median"] - par["ms_min"]) / par["ms_median"]
        out["parent_round_min_to_median_spread"] = margin
        if "unit_empty" in out:
            out["unit_empty"]["over_parent_round"] = out["unit_empty"]["ms_median"] / par["ms_median"]
            out["unit_empty"]["no_slower_than_parent_round"] = out["unit_empty"]["over_parent_round"] <= 1.0 + margin
        if "round" in out:
            out["round"]["over_parent_round"] = out["round"]["ms_median"] / par["ms_median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({a.label: out}))


if __name__ == "__main__":
    main()
