#!/usr/bin/env python3
"""What the host wait in the middle of the winner log's emit costs, and what a fixed workspace (include/cabac_hip_workspace.h)
makes of it.

Workload: tools/bench_search_plan.py's, cut down to what fits a minute — G groups (default 2048) of A candidates (default 4), every
candidate one worked transform unit of that tool's pool; group g is chain g of a winner log.  A SLICE is R positions (default 4):
cabac_hip_search_plan_round_device, then cabac_hip_search_log_append_device of the picks, nothing synchronised; then the log's emit,
cabac_hip_search_log_encode_device, into bytes.

Two figures, each on the default path and on the fixed path, alternating, 2 warm-up + 7 timed slices each, median / min / max:
  host_ms_in_emit   the wall time the host spends INSIDE the emit call, with the slice's rounds and appends queued in front of it
                    (on the default path the call drains them: it waits for the stream; on the fixed path it queues and returns)
  gpu_ms            the GPU time of the emit alone (the log is not consumed: the emit is run again on the drained stream), the sum
                    of its profile kinds by HIP events: 24 place, 5 residual passes, 10 splice (the gate is the scan's tail), 0 encode,
                    6 assemble
                    (gpu_ms_median_by_bracket lists them in the order of profile_kinds)
Two rows: the log's capacities at 1.25 x its content — the fixed emit walks its capacities, the default one its content, so this is
the row to compare — and at 4 x, which shows what a larger capacity costs.  Before anything is timed the fixed path's payload,
offsets and results are compared with the default path's.

  python tools/bench_workspace.py [--groups 2048] [--alts 4] [--rounds 4] [--reps 7] [--legs default,fixed] [--out FILE]
  CABAC_HIP_LIBRARY=<parent build> python tools/bench_workspace.py --legs default --out parent.json      (the parent's default path)
  python tools/bench_workspace.py --fold FILE --parent parent.json --bench-lines lines.txt
      folds the parent's run and `bench.py --full` lines ("parent <json>" / "change <json>", alternating runs) into FILE and states
      the comparisons: the fixed path's gpu_ms may exceed the parent's default path by no more than the parent's own spread."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def fold(a):
    out = json.load(open(a.fold))
    if a.parent:
        parent = json.load(open(a.parent))
        out["parent_default"] = {row: parent["emit"][row]["default"] for row in parent["emit"]}
        cmp_ = {}
        for row, legs in out["emit"].items():
            p = out["parent_default"][row]["gpu_ms"]
            spread = p["ms_max"] - p["ms_min"]
            over = legs["fixed"]["gpu_ms"]["ms_median"] - p["ms_median"]
            cmp_[row] = {"fixed_minus_parent_default_ms": over, "parent_spread_ms": spread, "within_parent_spread": over <= spread}
        out["gpu_ms_fixed_against_parent_default"] = cmp_
    if a.bench_lines:
        runs = {"parent": [], "change": []}
        for line in open(a.bench_lines):
            label, _, text = line.partition(" ")
            if label in runs and text.strip().startswith("{"):
                r = json.loads(text)
                runs[label].append({"kernel_ms.encode": r["kernel_ms"]["encode"], "kernel_ms.decode": r["kernel_ms"]["decode"],
                                    "residual.to_bytes": r["residual"]["to_bytes"]["coefficients_to_bytes_ms"]})
        table = {}
        for key in ("kernel_ms.encode", "kernel_ms.decode", "residual.to_bytes"):
            p, c = [r[key] for r in runs["parent"]], [r[key] for r in runs["change"]]
            table[key] = {"parent": p, "change": c, "parent_spread": max(p) - min(p),
                          "change_median_minus_parent_median": statistics.median(c) - statistics.median(p),
                          "within_parent_spread": statistics.median(c) - statistics.median(p) <= max(p) - min(p)}
        out["bench_full"] = {"runs_each": len(runs["parent"]), "order": "parent, change, parent, change, ...", "figures_ms": table}
    with open(a.fold, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("gpu_ms_fixed_against_parent_default", "bench_full") if k in out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=2048)
    ap.add_argument("--alts", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--legs", default="default,fixed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "workspace.json"))
    ap.add_argument("--fold", metavar="FILE")
    ap.add_argument("--parent", metavar="FILE")
    ap.add_argument("--bench-lines", metavar="FILE")
    a = ap.parse_args()
    if a.fold:
        return fold(a)
    assert a.reps >= 3

    import numpy as np
    import torch

    import bench_search_plan as BSP
    import parse_plan_model as PM
    from entropy_coding_amd import capi

    dev, SLOT, QP = BSP.dev, BSP.SLOT, BSP.QP
    legs = a.legs.split(",")
    rng = np.random.default_rng(2911)
    cases = BSP.pool(rng, 4)
    K, G, alts, L, R = len(cases), a.groups, a.alts, PM.TU_LEN, a.rounds
    n_cand = G * alts
    pick = rng.integers(0, K, n_cand)
    plan = np.stack([c["plan"] for c in cases])[pick]
    vin = np.stack([c["vin"] for c in cases])[pick]
    pool_co = np.zeros((K, 3, SLOT), np.int32)
    pool_tu = np.zeros((K, 3), capi.TU_DTYPE)
    for k, c in enumerate(cases):
        for j, ((w, h, ch, fl), b) in enumerate(zip(c["metas"], c["blocks"])):
            pool_co[k, j, :w * h] = b.reshape(-1)
            pool_tu[k, j]["log2_width"], pool_tu[k, j]["log2_height"] = int(np.log2(w)), int(np.log2(h))
            pool_tu[k, j]["channel"], pool_tu[k, j]["flags"] = ch, fl
    coeff = pool_co[pick].reshape(-1)
    tus = pool_tu[pick].reshape(-1)
    tus["coeff_offset"] = np.arange(3 * n_cand, dtype=np.uint64) * SLOT
    tu_at = np.full(3 * n_cand, PM.TU_BLOCK_AT, np.uint32)
    tu_guard = np.tile(np.array(cases[0]["guards"], np.uint32), n_cand)
    cand_first = np.arange(n_cand + 1, dtype=np.uint32) * 3
    ent_first = np.arange(n_cand + 1, dtype=np.uint64) * L
    group_first = np.arange(G + 1, dtype=np.uint32) * alts
    which = np.repeat(np.arange(G, dtype=np.uint32), alts)
    dist = rng.integers(0, 3000, n_cand).astype(np.uint64)
    lam = int(1.7 * (1 << 16))
    rec_cap = 64 * L * n_cand                                       # room for the resolved side records of one round

    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    have_ws = hasattr(hip.L, "cabac_hip_workspace_fix")
    assert have_ws or legs == ["default"], "this library has no fixed workspace: --legs default"
    t_gf, t_cf, t_ef, t_set = dev(group_first, np.int32), dev(cand_first, np.int32), dev(ent_first, np.int64), dev(which, np.int32)
    t_out, t_dist, t_chain = dev(np.arange(G, dtype=np.uint32), np.int32), dev(dist, np.int64), dev(np.arange(G, dtype=np.uint32), np.int32)
    t_plan, t_vin, t_tu, t_at = dev(plan, np.int32), dev(vin, np.int32), dev(tus), dev(tu_at, np.int32)
    t_gd, t_co = dev(tu_guard, np.int32), dev(coeff, np.int32)
    start_state = torch.zeros(G * capi.NUM_CTX, dtype=torch.int32, device="cuda")
    start_rate = torch.zeros(G * capi.NUM_CTX, dtype=torch.uint8, device="cuda")
    t_qp, t_init = dev(np.full(G, QP, np.int32), np.int32), dev(np.full(G, 2, np.uint32), np.int32)
    hip.ctx_init_device(G, t_qp.data_ptr(), t_init.data_ptr(), start_state.data_ptr(), start_rate.data_ptr())
    state, rate = start_state.clone(), start_rate.clone()
    t_bits = torch.zeros(n_cand, dtype=torch.int64, device="cuda")
    t_pick = torch.zeros(G, dtype=torch.int32, device="cuda")
    t_cost = torch.zeros(G, dtype=torch.int64, device="cuda")
    t_rf = torch.zeros(n_cand + 1, dtype=torch.int64, device="cuda")
    t_rec = torch.zeros(rec_cap, dtype=torch.int16, device="cuda")
    t_ato = torch.zeros(3 * n_cand, dtype=torch.int32, device="cuda")
    t_tuo = torch.zeros(3 * n_cand * capi.TU_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    desc = np.zeros(G, capi.DESC_DTYPE)
    desc["qp"], desc["init_id"] = QP, 2 | 0x100 | 0x200              # CABAC_SUB_FINISH | CABAC_SUB_ALIGN_RBSP
    t_desc = dev(desc)

    def queue_slice(log):
        """R positions: round, append — nothing synchronised"""
        state.copy_(start_state)
        rate.copy_(start_rate)
        log.reset()
        for _ in range(R):
            hip.search_plan_round_device(G, t_gf.data_ptr(), n_cand, t_cf.data_ptr(), 3 * n_cand, t_tu.data_ptr(), t_co.data_ptr(),
                                         state.data_ptr(), rate.data_ptr(), t_set.data_ptr(), t_ef.data_ptr(), t_plan.data_ptr(),
                                         t_vin.data_ptr(), t_at.data_ptr(), t_gd.data_ptr(), t_out.data_ptr(), t_dist.data_ptr(), lam,
                                         t_bits.data_ptr(), t_pick.data_ptr(), t_cost.data_ptr(), t_rf.data_ptr(), t_rec.data_ptr(), rec_cap,
                                         t_ato.data_ptr(), t_tuo.data_ptr())
            log.append_device(G, t_pick.data_ptr(), t_chain.data_ptr(), n_cand, t_cf.data_ptr(), t_tuo.data_ptr(), t_co.data_ptr(),
                              t_rf.data_ptr(), t_rec.data_ptr(), t_ato.data_ptr())

    # ---- the content of one slice, from a log with room for anything
    big = hip.search_log(G, R * G, R * G * 64 * L, 3 * R * G, 3 * R * G * SLOT)
    queue_slice(big)
    hip.synchronize()
    cnt = big.read()["counters"]
    content = {k: int(cnt[k]) for k in ("n_entry", "n_record", "n_tu", "n_coeff")}
    assert int(cnt["flags"]) == 0 and content["n_entry"] == R * G
    big.close()
    # no record codes more than 7 bits: the bytes of all substreams stay below the records of all expanded strings
    pay_cap = content["n_record"] + 33 * content["n_tu"] + 38 * content["n_coeff"] + 64 * G
    outs = {leg: dict(pay=torch.zeros(pay_cap, dtype=torch.uint8, device="cuda"), off=torch.zeros(G + 1, dtype=torch.int64, device="cuda"),
                      res=torch.zeros(2 * G, dtype=torch.int32, device="cuda")) for leg in legs}

    def emit(log, o):
        log.encode_device(t_desc.data_ptr(), o["pay"].data_ptr(), pay_cap, o["off"].data_ptr(), o["res"].data_ptr())

    result = {"workload": dict(groups=G, alts=alts, rounds=R, candidates_per_round=n_cand, chains=G, content=content),
              "reps": a.reps, "warmup": 2, "legs": legs, "device": torch.cuda.get_device_name(0), "emit": {}}
    for row, factor in (("capacity_1.25x", 1.25), ("capacity_4x", 4.0)):
        caps = {k: int(np.ceil(v * factor)) for k, v in content.items()}
        log = hip.search_log(G, caps["n_entry"], caps["n_record"], caps["n_tu"], caps["n_coeff"])
        sizes = None
        if have_ws:
            b_rec, b_slots = capi.workspace_bound(G, content["n_record"], content["n_tu"], content["n_coeff"])
            sizes = dict(n_sub=G, n_tu=caps["n_tu"], expanded_records=b_rec, slot_bytes=b_slots, log_records=caps["n_record"])

        def mode(leg):
            if have_ws:
                hip.workspace_fix(**sizes) if leg == "fixed" else hip.workspace_release()

        for leg in legs:                                            # the same bytes on both paths, before anything is timed
            mode(leg)
            queue_slice(log)
            emit(log, outs[leg])
            hip.synchronize()
        if len(legs) == 2:
            for k in ("off", "res", "pay"):
                assert bool(torch.equal(outs[legs[0]][k], outs[legs[1]][k])), "the two paths differ in " + k
            st = hip.workspace_status()
            assert int(st["n_voided"]) == 0 and int(st["n_calls"]) >= 1, st
        samples = {leg: {"host_ms_in_emit": [], "gpu_ms": [], "slice_wall_ms": [], "waits_in_emit": []} for leg in legs}
        kinds, brackets = {}, {}
        for rep in range(-2, a.reps):
            for leg in legs:
                mode(leg)
                hip.synchronize()
                t0 = time.perf_counter()
                queue_slice(log)
                w0 = hip.workspace_waits() if have_ws else 0
                t1 = time.perf_counter()
                emit(log, outs[leg])
                t2 = time.perf_counter()
                w1 = hip.workspace_waits() if have_ws else 0
                hip.synchronize()
                t3 = time.perf_counter()
                hip.profile_enable(64)                              # the emit alone, on the drained stream
                emit(log, outs[leg])
                hip.synchronize()
                got = hip.profile_read()
                hip.profile_enable(0)
                if rep >= 0:
                    s = samples[leg]
                    s["host_ms_in_emit"].append((t2 - t1) * 1e3)
                    s["slice_wall_ms"].append((t3 - t0) * 1e3)
                    s["gpu_ms"].append(sum(ms for _, ms in got))
                    brackets.setdefault(leg, []).append([ms for _, ms in got])
                    s["waits_in_emit"].append(w1 - w0)
                    kinds[leg] = [int(k) for k, _ in got]
        result["emit"][row] = {"log_capacities": caps}
        for leg in legs:
            s = samples[leg]
            result["emit"][row][leg] = {"host_ms_in_emit": stats(s["host_ms_in_emit"]), "gpu_ms": stats(s["gpu_ms"]),
                                        "slice_wall_ms": stats(s["slice_wall_ms"]), "profile_kinds": kinds[leg],
                                        "gpu_ms_median_by_bracket": [statistics.median(b) for b in zip(*brackets[leg])],
                                        "waits_in_emit": sorted(set(s["waits_in_emit"])) if have_ws else "not counted by this library"}
        log.close()
    hip.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
