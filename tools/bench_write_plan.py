#!/usr/bin/env python3
"""The plan write (cabac_hip_write_plan_device: plan + values + coefficients -> coded substreams, everything decided on the
device) against cabac_hip_encode_residual_device on the same content resolved on the host beforehand.

Workload: N substreams (default 4096) of U worked transform units each (default 64; tests/parse_plan_model.py::tu_plan — 24
entries and three guarded blocks per unit), every unit drawn from a pool of 4 cases per outcome of cbf_cb x cbf_cr x cbf_y x ts x
last_zero x violating with random side values and blocks; every unit has its own coefficients in device memory.  Two legs:
  plan_write  cabac_hip_write_plan_device on the plan, the real values (garbage where a value is not used) and all blocks
  floor       cabac_hip_encode_residual_device — code the parent has too — fed what a host would have had to work out first: the
              bin records of the active side elements (tests' model: fill, then the oracle's binariser) and one splice per CODED
              block; the skipped blocks are not handed over at all
Both legs must give the same payload, offsets and results; that is checked before anything is timed.  Times are HIP events from
cabac_hip_profile_enable, per group of launches (kind 5 residual passes, 10 splice plan / expand, 28 plan write: resolve + scan,
emit, stops in this order, 0 encode, 6 assembly); the host's one wait in the middle of either call lies between two groups and is
not in them.  The legs alternate, 2 warm-up + R timed calls each; median, minimum and maximum per group and of the sum.
Writes one JSON object (--out, default profiles/plan_write.json).

  python tools/bench_write_plan.py [--subs 4096] [--units 64] [--reps 7] [--out FILE]
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
    """The cases the units are drawn from, each resolved by the tests' model: plan, real values, blocks, which blocks are coded, and
    the bin records of its active elements in front of (entries 0 .. 9) and behind (10 .. 23) its blocks"""
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
    ap.add_argument("--subs", type=int, default=4096)
    ap.add_argument("--units", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_write.json"))
    a = ap.parse_args()
    assert a.reps >= 3
    rng = np.random.default_rng(2810)
    cases = pool(rng, 4)
    K, n_sub, per, L = len(cases), a.subs, a.units, PM.TU_LEN
    pick = rng.integers(0, K, (n_sub, per))
    n_unit, n_el = n_sub * per, per * L + 1

    # ---- the plan write's input
    plan = np.zeros((n_sub, n_el, 2), np.uint32)
    plan[:, :-1] = np.stack([c["plan"] for c in cases])[pick].reshape(n_sub, per * L, 2)
    plan[:, -1, 0] = capi.SE_TRM
    vin = np.ones((n_sub, n_el), np.uint32)
    vin[:, :-1] = np.stack([c["vin"] for c in cases])[pick].reshape(n_sub, per * L)
    pool_co = np.zeros((K, 3, SLOT), np.int32)
    pool_tu = np.zeros((K, 3), capi.TU_DTYPE)
    for k, c in enumerate(cases):
        for j, ((w, h, ch, fl), b) in enumerate(zip(c["metas"], c["blocks"])):
            assert w * h <= SLOT
            pool_co[k, j, :w * h] = b.reshape(-1)
            pool_tu[k, j]["log2_width"], pool_tu[k, j]["log2_height"] = int(np.log2(w)), int(np.log2(h))
            pool_tu[k, j]["channel"], pool_tu[k, j]["flags"] = ch, fl
    coeff = pool_co[pick].reshape(-1)                              # every unit has its own coefficients
    tus = pool_tu[pick].reshape(-1)
    tus["coeff_offset"] = np.arange(3 * n_unit, dtype=np.uint64) * SLOT
    tu_at = (np.tile(np.arange(per, dtype=np.uint32) * L + PM.TU_BLOCK_AT, n_sub)[:, None] + np.zeros(3, np.uint32)).reshape(-1)
    tu_guard = np.tile(np.array(cases[0]["guards"], np.uint32), n_unit)
    tile_first = np.arange(n_sub + 1, dtype=np.uint32) * (3 * per)
    desc = np.zeros(n_sub, capi.DESC_DTYPE)
    desc["rec_offset"], desc["n_records"], desc["qp"] = np.arange(n_sub, dtype=np.uint64) * n_el, n_el, QP
    desc["init_id"] = 2 | capi.SUB_FINISH | capi.SUB_ALIGN_RBSP

    # ---- the floor's input: what a host pass would have made of it
    len_b, len_a = np.array([len(c["before"]) for c in cases]), np.array([len(c["after"]) for c in cases])
    W = int((len_b + len_a).max())
    pool_rec, pool_len = np.zeros((K, W), np.uint16), len_b + len_a
    for k, c in enumerate(cases):
        pool_rec[k, :pool_len[k]] = np.concatenate([c["before"], c["after"]])
    unit_len = pool_len[pick]                                      # (n_sub, per)
    keep = np.arange(W)[None, None, :] < unit_len[:, :, None]
    sub_len = unit_len.sum(1) + 1                                  # + the terminate bin
    rec_off = np.concatenate([[0], np.cumsum(sub_len)]).astype(np.uint64)
    records = np.zeros(int(rec_off[-1]), np.uint16)
    body = np.ones(len(records), bool)
    body[(rec_off[1:] - 1).astype(np.int64)] = False
    records[body] = pool_rec[pick][keep]
    records[~body] = 0x8000 | 0x1FF                                # CABAC_REC_TRM, bin 1
    coded = np.array([c["coded"] for c in cases], bool)[pick]      # (n_sub, per, 3)
    unit_start = np.cumsum(unit_len, 1) - unit_len                 # within its substream
    at = np.broadcast_to((unit_start + len_b[pick])[:, :, None], coded.shape)[coded].astype(np.uint32)
    tus_f = tus[coded.reshape(-1)]
    splices = np.zeros(len(tus_f), capi.SPLICE_DTYPE)
    splices["at"], splices["tu"] = at, np.arange(len(tus_f), dtype=np.uint32)
    splice_first = np.concatenate([[0], np.cumsum(coded.reshape(n_sub, -1).sum(1))]).astype(np.uint32)
    desc_f = desc.copy()
    desc_f["rec_offset"], desc_f["n_records"] = rec_off[:-1], sub_len

    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_desc, t_plan, t_vin, t_first = dev(desc), dev(plan, np.int32), dev(vin, np.int32), dev(tile_first, np.int32)
    t_tu, t_at, t_gd, t_co = dev(tus), dev(tu_at, np.int32), dev(tu_guard, np.int32), dev(coeff, np.int32)
    t_descf, t_rec, t_sfirst, t_sp, t_tuf = dev(desc_f), dev(records, np.int16), dev(splice_first, np.int32), dev(splices), dev(tus_f)
    cap = 2 * len(records) + 64 * n_sub
    outs = [dict(pay=torch.zeros(cap, dtype=torch.uint8, device="cuda"), off=torch.zeros(n_sub + 1, dtype=torch.int64, device="cuda"),
                 res=torch.zeros(2 * n_sub, dtype=torch.int32, device="cuda")) for _ in range(2)]
    t_val = torch.zeros(n_sub * n_el, dtype=torch.int32, device="cuda")
    t_info = torch.zeros(3 * n_unit, dtype=torch.int32, device="cuda")

    def plan_write():
        o = outs[0]
        hip.write_plan_device(n_sub, t_desc.data_ptr(), t_plan.data_ptr(), t_vin.data_ptr(), t_first.data_ptr(), 3 * n_unit, t_tu.data_ptr(),
                              t_at.data_ptr(), t_gd.data_ptr(), t_co.data_ptr(), o["pay"].data_ptr(), cap, o["off"].data_ptr(),
                              o["res"].data_ptr(), t_val.data_ptr(), t_info.data_ptr())

    def floor():
        o = outs[1]
        hip.encode_residual_device(n_sub, t_descf.data_ptr(), t_rec.data_ptr(), t_sfirst.data_ptr(), t_sp.data_ptr(), len(tus_f), len(tus_f),
                                   t_tuf.data_ptr(), t_co.data_ptr(), o["pay"].data_ptr(), cap, o["off"].data_ptr(), o["res"].data_ptr())

    plan_write()
    floor()
    hip.synchronize()
    off = outs[0]["off"].cpu().numpy()
    assert bool(torch.equal(outs[0]["off"], outs[1]["off"])) and bool(torch.equal(outs[0]["res"], outs[1]["res"]))
    assert not outs[0]["res"].cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any()
    assert bool(torch.equal(outs[0]["pay"][:int(off[-1])], outs[1]["pay"][:int(off[-1])])), "the two legs code different bytes"

    legs = {"plan_write": (plan_write, ["5 sizes", "28 resolve+scan", "28 emit", "5 records", "0 encode", "28 stops", "6 assemble"]),
            "floor": (floor, ["5 sizes", "10 plan+scan", "10 expand", "5 records", "0 encode", "6 assemble"])}
    samples = {k: {g: [] for g in v[1] + ["sum", "wall"]} for k, v in legs.items()}
    for rep in range(-2, a.reps):                                  # the legs alternate; the first two rounds warm up
        for name, (run, groups) in legs.items():
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
    out = {"substreams": n_sub, "units_per_substream": per, "plan_entries": int(n_sub * n_el), "blocks": int(3 * n_unit),
           "coded_blocks": int(len(tus_f)), "expanded_records": int(len(records)) , "coded_bytes": int(off[-1]), "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "same_bytes_as_floor": True}
    for name in legs:
        out[name] = {g: stats(v) for g, v in samples[name].items()}
    own = [g for g in legs["plan_write"][1] if g.startswith("28")]
    kind28 = [sum(x) for x in zip(*[samples["plan_write"][g] for g in own])]
    out["plan_write"]["kind 28"] = stats(kind28)
    out["resolve_cost_ms_median"] = out["plan_write"]["sum"]["ms_median"] - out["floor"]["sum"]["ms_median"]
    out["plan_write_over_floor"] = out["plan_write"]["sum"]["ms_median"] / out["floor"]["sum"]["ms_median"]
    out["kind28_over_encode_kernel"] = out["plan_write"]["kind 28"]["ms_median"] / out["plan_write"]["0 encode"]["ms_median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
