#!/usr/bin/env python3
"""The plan rows (include/cabac_hip_plan_rows.h): the plan parse and the plan write from and into context sets and over WPP rows,
beside the plain plan parse and plan write.

Workload: build_residual_tiles(N) (N = 4096: the bench's residual leg), one substream per tile of 400 blocks, laid out as N / 16
pictures x 16 rows in LEVEL ORDER (level r = row r of every picture, row r linked to row r - 1 of its picture).  The plan of a tile
is one cbf bin (1) per block with the block behind it, guarded by that cbf, and the terminate bin; a "CTU" is 25 blocks, so every
row hands its contexts over at plan entry 25.  Device buffers resident; every payload is made by the device's own writer.  Legs:
  plan_write / plan_parse     the plain calls — code the parent has too: run with CABAC_HIP_LIBRARY naming a build of the parent
                              and --legs plain --label parent, alternating with --label this; both write to the same --out
  write_sets_noset / parse_sets_noset     the sets forms with no set (bytes and values checked equal to the plain calls')
  write_sets_shared / parse_sets_shared   from 64 shared sets, every substream writing an out set (the parse at entry 25)
  rows_write / rows_parse     16 levels of N / 16 rows each
Times are HIP events from cabac_hip_profile_enable per group of launches, 2 warm-up + R timed calls; median, minimum, maximum per
group and of the sum.  Every parse leg checks that values and coefficients come back.
Writes one JSON object (--out, default profiles/plan_rows.json; merged with what the file holds under other labels).

  python tools/bench_plan_rows.py [--tiles 4096] [--rows 16] [--reps 7] [--legs all|plain] [--label NAME] [--out FILE]
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

QP, CTU_BLOCKS, N_SHARED = 32, 25, 64
NO = capi.CTX_NO_SET


def dev(a, dt=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--legs", default="all", choices=["all", "plain"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_rows.json"))
    a = ap.parse_args()
    assert a.reps >= 3 and a.tiles % a.rows == 0

    tus, coeff, _ = build_residual_tiles(a.tiles)
    n, n_sub, n_row = len(tus), a.tiles, a.rows
    n_pic, per_tile = n_sub // n_row, n // n_sub
    assert per_tile * n_sub == n and per_tile > CTU_BLOCKS
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
    level_first = np.arange(0, n_sub + 1, n_pic, dtype=np.uint32)
    sync_from = np.concatenate([np.full(n_pic, NO, np.uint32), np.arange(n_sub - n_pic, dtype=np.uint32)])
    sync_at = np.full(n_sub, CTU_BLOCKS, np.uint32)

    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_desc, t_plan, t_vin = dev(desc), dev(plan, np.int32), dev(values, np.int32)
    t_first = (torch.arange(n_sub + 1, device="cuda", dtype=torch.int32) * per_tile).contiguous()
    t_tu, t_at, t_gd, t_co = dev(tus), dev(tu_at, np.int32), dev(tu_guard, np.int32), dev(coeff, np.int32)
    t_from, t_sat = dev(sync_from, np.int32), dev(sync_at, np.int32)
    cap = int(len(coeff)) + 64 * n_sub
    t_off = torch.zeros(n_sub + 1, dtype=torch.int64, device="cuda")
    t_res = torch.zeros(2 * n_sub, dtype=torch.int32, device="cuda")
    t_val = torch.zeros(n_sub * n_el, dtype=torch.int32, device="cuda")
    t_info = torch.zeros(n, dtype=torch.int32, device="cuda")
    t_dec = torch.zeros_like(t_co)
    # 64 shared start sets (the init sets of 64 qp / slice-type pairs) and one out set per substream
    t_qp, t_iid = dev(np.arange(N_SHARED, dtype=np.int32) % 52, np.int32), dev((np.arange(N_SHARED) % 3).astype(np.uint32), np.int32)
    n_sets = max(n_sub, N_SHARED)
    t_state = torch.zeros(n_sets * capi.NUM_CTX, dtype=torch.int32, device="cuda")
    t_rate = torch.zeros(n_sets * capi.NUM_CTX, dtype=torch.uint8, device="cuda")
    hip.ctx_init_device(N_SHARED, t_qp.data_ptr(), t_iid.data_ptr(), t_state.data_ptr(), t_rate.data_ptr())
    t_ostate, t_orate = torch.zeros_like(t_state), torch.zeros_like(t_rate)
    t_shared = dev((np.arange(n_sub) % N_SHARED).astype(np.uint32), np.int32)
    t_noset = dev(np.full(n_sub, NO, np.uint32), np.int32)
    t_own = dev(np.arange(n_sub, dtype=np.uint32), np.int32)
    pays = {k: torch.zeros(cap, dtype=torch.uint8, device="cuda") for k in ("plain", "noset", "shared", "rows")}

    w_args = lambda pay: (n_sub, t_desc.data_ptr(), t_plan.data_ptr(), t_vin.data_ptr(), t_first.data_ptr(), n, t_tu.data_ptr(), t_at.data_ptr(),
                          t_gd.data_ptr(), t_co.data_ptr(), pay.data_ptr(), cap, t_off.data_ptr(), t_res.data_ptr())
    sets_kw = dict(n_sets=n_sets, d_state=t_state.data_ptr(), d_rate=t_rate.data_ptr(), d_out_state=t_ostate.data_ptr(),
                   d_out_rate=t_orate.data_ptr())

    def parse_input(pay):
        """The payload in 16-aligned byte slots and the parse descriptors of it"""
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
        return dev(d), dev(buf), int(lens.sum())

    def p_args(t_d, t_b):
        return (n_sub, t_d.data_ptr(), t_b.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), t_at.data_ptr(), t_gd.data_ptr(),
                t_plan.data_ptr(), t_dec.data_ptr(), t_val.data_ptr(), t_res.data_ptr())

    def came_back(what):
        hip.synchronize()
        assert not t_res.cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any(), what
        assert bool(torch.equal(t_dec, t_co)) and bool(torch.equal(t_val, t_vin)), what + ": values or coefficients did not come back"
        t_dec.zero_()
        t_val.zero_()

    def timed(run):
        """-> {group: stats} with groups "<kind>#<occurrence>" and "sum" """
        samples = {}
        for rep in range(-2, a.reps):
            hip.synchronize()
            hip.profile_enable(64)
            run()
            hip.synchronize()
            got = hip.profile_read()
            hip.profile_enable(0)
            if rep < 0:
                continue
            by_kind = {}
            for k, ms in got:
                by_kind[k] = by_kind.get(k, 0.0) + ms
            for k, ms in by_kind.items():
                samples.setdefault("kind %d" % k, []).append(ms)
            samples.setdefault("launch groups", []).append(len(got))
            samples.setdefault("sum", []).append(sum(ms for _, ms in got))
        return {g: (stats(v) if g != "launch groups" else v[0]) for g, v in samples.items()}

    out = {"tiles": n_sub, "pictures": n_pic, "rows": n_row, "blocks": n, "plan_entries": int(n_sub * n_el), "reps": a.reps,
           "hand_over_entry": CTU_BLOCKS, "device": torch.cuda.get_device_name(0)}
    out["plan_write"] = timed(lambda: hip.write_plan_device(*w_args(pays["plain"]), t_val.data_ptr(), t_info.data_ptr()))
    d_plain, b_plain, out["coded_bytes"] = parse_input(pays["plain"])
    t_val.zero_()
    out["plan_parse"] = timed(lambda: hip.parse_plan_device(*p_args(d_plain, b_plain)))
    came_back("plan_parse")
    if a.legs == "all":
        out["write_sets_noset"] = timed(lambda: hip.plan_write_sets_device(*w_args(pays["noset"]), t_val.data_ptr(), t_info.data_ptr(),
                                                                           d_start_set=t_noset.data_ptr(), **sets_kw))
        hip.synchronize()
        out["sets_noset_bytes_equal_plain"] = bool(torch.equal(pays["noset"], pays["plain"]))
        assert out["sets_noset_bytes_equal_plain"]
        t_val.zero_()
        out["parse_sets_noset"] = timed(lambda: hip.plan_parse_sets_device(*p_args(d_plain, b_plain), d_start_set=t_noset.data_ptr(), **sets_kw))
        came_back("parse_sets_noset")
        out["write_sets_shared"] = timed(lambda: hip.plan_write_sets_device(*w_args(pays["shared"]), t_val.data_ptr(), t_info.data_ptr(),
                                                                            d_start_set=t_shared.data_ptr(), d_out_set=t_own.data_ptr(), **sets_kw))
        d_sh, b_sh, _ = parse_input(pays["shared"])
        t_val.zero_()
        out["parse_sets_shared"] = timed(lambda: hip.plan_parse_sets_device(*p_args(d_sh, b_sh), d_start_set=t_shared.data_ptr(),
                                                                            d_out_set=t_own.data_ptr(), d_out_at=t_sat.data_ptr(), **sets_kw))
        came_back("parse_sets_shared")
        out["rows_write"] = timed(lambda: hip.plan_write_rows_device(*w_args(pays["rows"]), level_first, t_from.data_ptr(), t_sat.data_ptr(),
                                                                     d_values_out=t_val.data_ptr(), d_tu_info=t_info.data_ptr()))
        d_rw, b_rw, out["rows_coded_bytes"] = parse_input(pays["rows"])
        t_val.zero_()
        out["rows_parse"] = timed(lambda: hip.plan_parse_rows_device(*p_args(d_rw, b_rw), level_first, t_from.data_ptr(), t_sat.data_ptr()))
        came_back("rows_parse")
        out["rows_parse_over_plan_parse"] = out["rows_parse"]["sum"]["ms_median"] / out["plan_parse"]["sum"]["ms_median"]
        out["rows_write_over_plan_write"] = out["rows_write"]["sum"]["ms_median"] / out["plan_write"]["sum"]["ms_median"]
    hip.close()

    merged = {}
    if os.path.exists(a.out):
        try:
            merged = json.load(open(a.out))
        except ValueError:
            merged = {}
    merged[a.label] = out
    par = merged.get("parent")
    if a.label != "parent" and par:
        for leg in ("plan_write", "plan_parse"):
            p = par[leg]["sum"]
            out[leg]["over_parent"] = out[leg]["sum"]["ms_median"] / p["ms_median"]
            out[leg]["inside_parent_spread"] = p["ms_min"] <= out[leg]["sum"]["ms_median"] <= p["ms_max"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({a.label: out}))


if __name__ == "__main__":
    main()
