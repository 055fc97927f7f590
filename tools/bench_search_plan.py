#!/usr/bin/env python3
"""The plan round (cabac_hip_search_plan_round_device: candidates given as plan + values + coefficients, resolved, costed, picked
and committed on the device) against cabac_hip_search_unit_round_device on the same content resolved on the host beforehand.

Workload: G groups (default 4096) of A candidates each (default 8), every candidate one worked transform unit
(tests/parse_plan_model.py::tu_plan — 24 entries and three guarded blocks) drawn from a pool of 4 cases per outcome of cbf_cb x
cbf_cr x cbf_y x ts x last_zero x violating with random side values and blocks; every candidate has its own coefficients in device
memory; group g starts from context set g and commits into it.  Two legs:
  plan_round  cabac_hip_search_plan_round_device on the plans, the real values (garbage where a value is not used) and all blocks
  floor       cabac_hip_search_unit_round_device — code the parent has too — fed what a host would have had to work out first:
              the bin records of the active side elements (tests' model: fill, then the oracle's binariser), the position of the
              blocks in record units and the CODED blocks alone; the skipped blocks are not handed over at all.  It leaves out the
              host's own resolve time and the sizes pass a host cannot do without a round trip
Both legs must give the same costs, picks and committed sets; that is checked before anything is timed.  Times are HIP events from
cabac_hip_profile_enable, per group of launches (kind 5 residual sizes pass, 29 plan resolve: count walk + scan + emit walk, 20
unit estimate, 21 select, 22 commit).  The legs alternate, 2 warm-up + R timed calls each, every call from the same start sets;
median, minimum and maximum per group and of the sum.  Writes one JSON object (--out, default profiles/search_plan.json).

  python tools/bench_search_plan.py [--groups 4096] [--alts 8] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import parse_elements_model as E  # noqa: E402
import parse_plan_model as PM  # noqa: E402
from entropy_coding_amd import capi  # noqa: E402
from test_parse_plan_model import TU_OUTCOMES  # noqa: E402

QP, SLOT = 32, 256                                                  # coefficients per block slot: the largest block of the pool


def dev(a, dt=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def pool(rng, per_outcome):
    """The cases the candidates are drawn from, each resolved by the tests' model: plan, real values, blocks, which blocks are
    coded, and the bin records of its active elements in front of (entries 0 .. 9) and behind (10 .. 23) its blocks"""
    cases = []
    for o in TU_OUTCOMES:
        for _ in range(per_outcome):
            plan, real, metas, blocks, at, guards = PM.tu_case(rng, *o)
            blocks = [np.clip(b, -32767, 32767) for b in blocks]
            values, infos, coded, active = PM.fill(plan, real, metas, blocks, at, guards)
            rec = [E.records_of([E.op_of(plan[i, 0], values[i])]) if active[i] else np.zeros(0, np.uint16) for i in range(PM.TU_LEN)]
            vin = np.array([v if on else 0xDEAD0000 + i for i, (v, on) in enumerate(zip(real, active))], np.uint64).astype(np.uint32)
            cases.append(dict(plan=plan, vin=vin, metas=metas, blocks=blocks, guards=guards, coded=coded,
                              before=np.concatenate(rec[:PM.TU_BLOCK_AT]), after=np.concatenate(rec[PM.TU_BLOCK_AT:])))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=4096)
    ap.add_argument("--alts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_plan.json"))
    a = ap.parse_args()
    assert a.reps >= 3
    rng = np.random.default_rng(2911)
    cases = pool(rng, 4)
    K, n_group, alts, L = len(cases), a.groups, a.alts, PM.TU_LEN
    n_cand = n_group * alts
    pick = rng.integers(0, K, n_cand)

    # ---- the plan round's input
    plan = np.stack([c["plan"] for c in cases])[pick]              # (n_cand, L, 2)
    vin = np.stack([c["vin"] for c in cases])[pick]
    pool_co = np.zeros((K, 3, SLOT), np.int32)
    pool_tu = np.zeros((K, 3), capi.TU_DTYPE)
    for k, c in enumerate(cases):
        for j, ((w, h, ch, fl), b) in enumerate(zip(c["metas"], c["blocks"])):
            assert w * h <= SLOT
            pool_co[k, j, :w * h] = b.reshape(-1)
            pool_tu[k, j]["log2_width"], pool_tu[k, j]["log2_height"] = int(np.log2(w)), int(np.log2(h))
            pool_tu[k, j]["channel"], pool_tu[k, j]["flags"] = ch, fl
    coeff = pool_co[pick].reshape(-1)                              # every candidate has its own coefficients
    tus = pool_tu[pick].reshape(-1)
    tus["coeff_offset"] = np.arange(3 * n_cand, dtype=np.uint64) * SLOT
    tu_at = np.full(3 * n_cand, PM.TU_BLOCK_AT, np.uint32)
    tu_guard = np.tile(np.array(cases[0]["guards"], np.uint32), n_cand)
    cand_first = np.arange(n_cand + 1, dtype=np.uint32) * 3
    ent_first = np.arange(n_cand + 1, dtype=np.uint64) * L
    group_first = np.arange(n_group + 1, dtype=np.uint32) * alts
    which = np.repeat(np.arange(n_group, dtype=np.uint32), alts)
    out_set = np.arange(n_group, dtype=np.uint32)
    dist = rng.integers(0, 3000, n_cand).astype(np.uint64)
    lam = int(1.7 * (1 << 16))

    # ---- the floor's input: what a host pass would have made of it
    len_b, len_a = np.array([len(c["before"]) for c in cases]), np.array([len(c["after"]) for c in cases])
    W = int((len_b + len_a).max())
    pool_rec, pool_len = np.zeros((K, W), np.uint16), len_b + len_a
    for k, c in enumerate(cases):
        pool_rec[k, :pool_len[k]] = np.concatenate([c["before"], c["after"]])
    cand_len = pool_len[pick]
    rec_first = np.concatenate([[0], np.cumsum(cand_len)]).astype(np.uint64)
    records = pool_rec[pick][np.arange(W)[None, :] < cand_len[:, None]]
    coded = np.array([c["coded"] for c in cases], bool)[pick]      # (n_cand, 3)
    tus_f = tus[coded.reshape(-1)]
    at_f = np.broadcast_to(len_b[pick][:, None], coded.shape)[coded].astype(np.uint32)
    cand_first_f = np.concatenate([[0], np.cumsum(coded.sum(1))]).astype(np.uint32)
    n_rec = int(rec_first[-1])

    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_gf, t_cf, t_ef, t_set, t_out, t_dist = (dev(group_first, np.int32), dev(cand_first, np.int32), dev(ent_first, np.int64),
                                              dev(which, np.int32), dev(out_set, np.int32), dev(dist, np.int64))
    t_plan, t_vin, t_tu, t_at, t_gd, t_co = dev(plan, np.int32), dev(vin, np.int32), dev(tus), dev(tu_at, np.int32), dev(tu_guard, np.int32), dev(coeff, np.int32)
    t_cff, t_rff, t_recf, t_tuf, t_atf = dev(cand_first_f, np.int32), dev(rec_first, np.int64), dev(records, np.int16), dev(tus_f), dev(at_f, np.int32)
    start_state = torch.zeros(n_group * capi.NUM_CTX, dtype=torch.int32, device="cuda")
    start_rate = torch.zeros(n_group * capi.NUM_CTX, dtype=torch.uint8, device="cuda")
    t_qp, t_init = dev(np.full(n_group, QP, np.int32), np.int32), dev(np.full(n_group, 2, np.uint32), np.int32)
    hip.ctx_init_device(n_group, t_qp.data_ptr(), t_init.data_ptr(), start_state.data_ptr(), start_rate.data_ptr())
    outs = [dict(state=start_state.clone(), rate=start_rate.clone(), bits=torch.zeros(n_cand, dtype=torch.int64, device="cuda"),
                 pick=torch.zeros(n_group, dtype=torch.int32, device="cuda"), cost=torch.zeros(n_group, dtype=torch.int64, device="cuda"))
            for _ in range(2)]
    cap = n_rec + 64                                               # the need is known here; the bound would be 63 records per entry
    t_rf = torch.zeros(n_cand + 1, dtype=torch.int64, device="cuda")
    t_rec = torch.zeros(cap, dtype=torch.int16, device="cuda")
    t_ato = torch.zeros(3 * n_cand, dtype=torch.int32, device="cuda")
    t_tuo = torch.zeros(3 * n_cand * capi.TU_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    t_flags = torch.zeros(n_cand, dtype=torch.int32, device="cuda")
    t_total = torch.zeros(1, dtype=torch.int64, device="cuda")

    def rewind(o):
        o["state"].copy_(start_state)
        o["rate"].copy_(start_rate)

    def plan_round():
        o = outs[0]
        hip.search_plan_round_device(n_group, t_gf.data_ptr(), n_cand, t_cf.data_ptr(), 3 * n_cand, t_tu.data_ptr(), t_co.data_ptr(),
                                     o["state"].data_ptr(), o["rate"].data_ptr(), t_set.data_ptr(), t_ef.data_ptr(), t_plan.data_ptr(),
                                     t_vin.data_ptr(), t_at.data_ptr(), t_gd.data_ptr(), t_out.data_ptr(), t_dist.data_ptr(), lam,
                                     o["bits"].data_ptr(), o["pick"].data_ptr(), o["cost"].data_ptr(), t_rf.data_ptr(), t_rec.data_ptr(), cap,
                                     t_ato.data_ptr(), t_tuo.data_ptr(), d_flags=t_flags.data_ptr(), d_total=t_total.data_ptr())

    def floor():
        o = outs[1]
        hip.search_unit_round_device(n_group, t_gf.data_ptr(), n_cand, t_cff.data_ptr(), t_tuf.data_ptr(), t_co.data_ptr(),
                                     o["state"].data_ptr(), o["rate"].data_ptr(), t_set.data_ptr(), t_rff.data_ptr(), t_recf.data_ptr(),
                                     t_atf.data_ptr(), t_out.data_ptr(), t_dist.data_ptr(), lam, o["bits"].data_ptr(), o["pick"].data_ptr(),
                                     o["cost"].data_ptr())

    plan_round()
    floor()
    hip.synchronize()
    assert int(t_total.cpu()[0]) == n_rec and not t_flags.any().item()
    assert bool(torch.equal(t_rf, t_rff)) and bool(torch.equal(t_rec[:n_rec], t_recf)), "the resolve is not the host's"
    for k in ("bits", "pick", "cost", "state", "rate"):
        assert bool(torch.equal(outs[0][k], outs[1][k])), "the two legs differ in " + k
    picked = outs[0]["pick"].cpu().numpy().view(np.uint32)

    legs = {"plan_round": (plan_round, ["5 sizes", "29 resolve", "20 estimate", "21 select", "22 commit"]),
            "floor": (floor, ["20 estimate", "21 select", "22 commit"])}
    samples = {k: {g: [] for g in v[1] + ["sum", "wall"]} for k, v in legs.items()}
    for rep in range(-2, a.reps):                                  # the legs alternate; the first two rounds warm up
        for i, (name, (run, groups)) in enumerate(legs.items()):
            rewind(outs[i])
            hip.synchronize()
            hip.profile_enable(16)
            t0 = time.perf_counter()
            run()
            hip.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            got = hip.profile_read()
            hip.profile_enable(0)
            assert [str(k) for k, _ in got] == [g.split()[0] for g in groups], got
            if rep >= 0:
                for g, (_, ms) in zip(groups, got):
                    samples[name][g].append(ms)
                samples[name]["sum"].append(sum(ms for _, ms in got))
                samples[name]["wall"].append(wall)
    hip.close()
    out = {"groups": n_group, "candidates": n_cand, "plan_entries": int(n_cand * L), "blocks": int(3 * n_cand),
           "coded_blocks": int(len(tus_f)), "side_records": n_rec, "distinct_picks_in_group": int(len(set((picked % alts).tolist()))),
           "reps": a.reps, "device": torch.cuda.get_device_name(0), "geometry": "one wave per candidate, four candidates per workgroup",
           "same_costs_picks_sets_as_floor": True}
    for name in legs:
        out[name] = {g: stats(v) for g, v in samples[name].items()}
    front = [x + y for x, y in zip(samples["plan_round"]["5 sizes"], samples["plan_round"]["29 resolve"])]
    out["plan_round"]["5 + 29"] = stats(front)
    med = lambda leg, g: out[leg][g]["ms_median"]
    out["plan_round_over_floor"] = med("plan_round", "sum") / med("floor", "sum")
    out["resolve_share_of_round"] = med("plan_round", "29 resolve") / med("plan_round", "sum")
    out["sizes_share_of_round"] = med("plan_round", "5 sizes") / med("plan_round", "sum")
    out["resolve_ns_per_candidate"] = med("plan_round", "29 resolve") * 1e6 / n_cand
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
