#!/usr/bin/env python3
"""The plan write in pieces (include/cabac_hip_plan_continue.h) beside the one-call plan write with sets.

Workload: that of tools/bench_plan_resume.py — build_residual_tiles(N) (N = 4096: the bench's residual leg), one substream per tile
of 400 blocks; the plan of a tile is one cbf bin (1) per block with the block behind it, guarded by that cbf, and the terminate
bin.  Device buffers resident.  Legs, ALTERNATING in one run (rep by rep):
  parent_one_call  cabac_hip_plan_write_sets_device of the PARENT commit's build (--parent-library FILE: that build is loaded into
                   the same process beside this one), every substream from Ctx::init, writing an out set
  one_call         the same call of this build
  pieces_1         cabac_hip_plan_continue_write_device, one final piece from a fresh state: the cost of the form itself
  pieces_4         the same substreams in 4 equal pieces (100 cbfs and their blocks each; the terminate bin in the last): 4 calls,
                   state and contexts handed over in place
  pieces_16        in 16 equal pieces (25 blocks: the "CTU" of tools/bench_plan_rows.py)
  pieces_K_enc7    (--piece-encoder 7) the three pieces legs again under cabac_hip_piece_encoder_set(ctx, 7): the encode leg on
                   the lane-serial encoder, the one the one call's dispatch picks (include/cabac_hip_piece_encoder.h)
Before anything is timed every leg runs once and its bytes, results, values, info words and out sets are compared with the one
call's.  Two times per leg and round, 2 warm-up + R timed rounds, median / minimum / maximum:
  device   the sum of the HIP events of cabac_hip_profile_enable around the launches of the leg
  wall     the host's clock from the first call of the leg to the end of a synchronise behind the last
Every call of these forms waits for the stream once in the middle (the expanded length sizes the record scratch), so the device
idles while the host reads the totals and queues the second half: host_wait_share = (wall - device) / wall is that part of a
leg's time, reported per leg.

EXPECTATION, stated before the run: ONE piece costs at most 1.10 x the one-call form of the parent's build, device time, same run
(the standing bound of profiles/pieces.json and profiles/plan_resume.json).  Reported as met / MISSED with the 4- and 16-piece
ratios; the bound is no gate.  With --piece-encoder 7 the same is reported for pieces_1_enc7 ("expectation_enc7").  Without --parent-library the ratio is taken against this build's one_call and says so.

--label parent (with CABAC_HIP_LIBRARY naming a build of the parent): only the one_call leg, which the parent has too, is run and
stored under "parent"; a later run under another label reports its legs over that one as well.

Writes one JSON object (--out, default profiles/plan_continue.json; merged with what the file holds under other labels).

  python tools/bench_plan_continue.py [--tiles 4096] [--reps 7] [--parent-library FILE] [--piece-encoder 7] [--label NAME] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def other_build(path, stream):
    """A context of another build of the library, loaded beside this one"""
    mine, env = capi._lib, os.environ.get("CABAC_HIP_LIBRARY")
    capi._lib, os.environ["CABAC_HIP_LIBRARY"] = None, path
    try:
        return capi.CabacHip(0, stream=stream)
    finally:
        capi._lib = mine
        if env is None:
            del os.environ["CABAC_HIP_LIBRARY"]
        else:
            os.environ["CABAC_HIP_LIBRARY"] = env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--piece-encoder", type=int, default=4, choices=(4, 7), help="7: the pieces legs under setting 7 as well")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_continue.json"))
    a = ap.parse_args()
    assert a.reps >= 3
    only_plain = a.label == "parent"
    print("expectation: pieces_1 <= %.2f x the parent's one_call (device time, median of %d rounds, same run)" % (BOUND, a.reps), flush=True)

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

    stream = torch.cuda.current_stream().cuda_stream
    hip = capi.CabacHip(0, stream=stream)
    parent = other_build(a.parent_library, stream) if a.parent_library and not only_plain else None
    t_desc, t_plan, t_vin = dev(desc), dev(plan, np.int32), dev(values, np.int32)
    t_first = (torch.arange(n_sub + 1, device="cuda", dtype=torch.int32) * per_tile).contiguous()
    t_tu, t_at, t_gd, t_co = dev(tus), dev(tu_at, np.int32), dev(tu_guard, np.int32), dev(coeff, np.int32)
    cap = int(len(coeff)) + 64 * n_sub
    t_off = torch.zeros(n_sub + 1, dtype=torch.int64, device="cuda")
    t_res = torch.zeros(2 * n_sub, dtype=torch.int32, device="cuda")
    t_val = torch.zeros(n_sub * n_el, dtype=torch.int32, device="cuda")
    t_info = torch.zeros(n, dtype=torch.int32, device="cuda")
    t_state = torch.zeros(n_sub * capi.NUM_CTX, dtype=torch.int32, device="cuda")
    t_rate = torch.zeros(n_sub * capi.NUM_CTX, dtype=torch.uint8, device="cuda")
    t_noset = dev(np.full(n_sub, NO, np.uint32), np.int32)
    t_own = dev(np.arange(n_sub, dtype=np.uint32), np.int32)
    t_coder = torch.zeros(32 * n_sub, dtype=torch.uint8, device="cuda")
    pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    sets_kw = dict(n_sets=n_sub, d_state=t_state.data_ptr(), d_rate=t_rate.data_ptr(), d_out_set=t_own.data_ptr(),
                   d_out_state=t_state.data_ptr(), d_out_rate=t_rate.data_ptr())

    def one_call(ctx=hip):
        ctx.plan_write_sets_device(n_sub, t_desc.data_ptr(), t_plan.data_ptr(), t_vin.data_ptr(), t_first.data_ptr(), n, t_tu.data_ptr(),
                                   t_at.data_ptr(), t_gd.data_ptr(), t_co.data_ptr(), pay.data_ptr(), cap, t_off.data_ptr(), t_res.data_ptr(),
                                   t_val.data_ptr(), t_info.data_ptr(), d_start_set=t_noset.data_ptr(), **sets_kw)

    # the one call first: its payload is what every leg must give, and its lengths size the slots of the pieces
    one_call()
    hip.synchronize()
    want_res = t_res.cpu().numpy().view(capi.RESULT_DTYPE).copy()
    assert not want_res["flags"].any()
    off = t_off.cpu().numpy().copy()
    lens = np.diff(off).astype(np.uint64)
    slots = (lens + 15) // 16 * 16 + 16
    slot_at = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.uint64)
    want_pay = pay[:int(off[-1])].cpu().numpy().copy()
    want = [t.clone() for t in (t_val, t_info, t_state, t_rate)]
    t_slots = torch.zeros(int(slots.sum()), dtype=torch.uint8, device="cuda")

    # the pieces: piece p of substream s is the cbfs [p L, (p + 1) L) with their blocks (block k stands at entry k + 1, so it goes
    # with its cbf; positions relative to the piece), the last one with the terminate bin.  The blocks of a launch lie in substream
    # order, so every piece count has its own copy of the block descriptors, ordered (piece, substream, block).
    launches = {}
    tus_v = np.ascontiguousarray(tus).view(np.uint8).reshape(n_sub, per_tile, -1)
    if not only_plain:
        for P in PIECES:
            L = per_tile // P
            ls = []
            for p in range(P):
                dp = desc.copy()
                dp["rec_offset"] = desc["rec_offset"] + p * L
                dp["n_records"] = L + (1 if p == P - 1 else 0)
                dp["byte_offset"], dp["byte_capacity"] = slot_at, lens
                dp["init_id"] = 2 | ((capi.SUB_FINISH | capi.SUB_ALIGN_RBSP) if p == P - 1 else 0)
                t_tu_p = dev(tus_v[:, p * L:(p + 1) * L])
                t_at_p = dev(np.tile(np.arange(L, dtype=np.uint32) + 1, n_sub), np.int32)
                t_first_p = (torch.arange(n_sub + 1, device="cuda", dtype=torch.int32) * L).contiguous()
                t_info_p = torch.zeros(n_sub * L, dtype=torch.int32, device="cuda")
                ls.append((dev(dp), t_first_p, t_tu_p, t_at_p, t_info_p, p, L))
            launches[P] = ls

    def pieces(P, setting=4):
        hip.piece_encoder_set(setting)
        for t_dp, t_first_p, t_tu_p, t_at_p, t_info_p, p, L in launches[P]:
            hip.plan_continue_write_device(n_sub, t_dp.data_ptr(), t_plan.data_ptr(), t_vin.data_ptr(), t_first_p.data_ptr(), n_sub * L,
                                           t_tu_p.data_ptr(), t_at_p.data_ptr(), t_gd.data_ptr(), t_co.data_ptr(), t_slots.data_ptr(),
                                           t_res.data_ptr(), t_val.data_ptr(), t_info_p.data_ptr(),
                                           d_start_set=(t_noset if p == 0 else t_own).data_ptr(), **sets_kw,
                                           d_coder_in=t_coder.data_ptr(), d_coder_out=t_coder.data_ptr())

    legs = [("one_call", one_call)]
    if parent is not None:
        legs.insert(0, ("parent_one_call", lambda: one_call(parent)))
    if not only_plain:
        legs += [("pieces_%d" % P, (lambda P=P: pieces(P))) for P in PIECES]
        if a.piece_encoder == 7:
            legs += [("pieces_%d_enc7" % P, (lambda P=P: pieces(P, 7))) for P in PIECES]
    owner = {name: (parent if name == "parent_one_call" else hip) for name, _ in legs}

    def clear():
        for t in (pay, t_off, t_res, t_val, t_info, t_state, t_rate, t_coder, t_slots):
            t.zero_()

    # the outputs first: every leg gives what the one call gave
    for name, run in legs:
        clear()
        run()
        owner[name].synchronize()
        assert np.array_equal(t_res.cpu().numpy().view(capi.RESULT_DTYPE), want_res), name + ": not the one call's results"
        got = [t_val, t_info, t_state, t_rate]
        if name.startswith("pieces_"):
            P = int(name.split("_")[1])
            info = torch.cat([ls[4].view(n_sub, ls[6]) for ls in launches[P]], dim=1).reshape(-1)
            got = [t_val, info, t_state, t_rate]
            image = t_slots.cpu().numpy()
            for s in range(n_sub):
                assert np.array_equal(image[int(slot_at[s]):int(slot_at[s]) + int(lens[s])], want_pay[int(off[s]):int(off[s + 1])]), \
                    "%s: substream %d is not the one call's bytes" % (name, s)
            st = t_coder.cpu().numpy().view(capi.CODER_STATE_DTYPE)
            assert (st["kind"] == capi.CODER_CLOSED).all() and np.array_equal(st["bits"], want_res["n_bits"]), name
        else:
            assert np.array_equal(pay[:int(off[-1])].cpu().numpy(), want_pay) and np.array_equal(t_off.cpu().numpy(), off), name
        assert all(bool(torch.equal(x, y)) for x, y in zip(got, want)), name + ": not the one call's outputs"

    device, wall = {name: [] for name, _ in legs}, {name: [] for name, _ in legs}
    n_launch, per_kind = {}, {}
    for rep in range(-2, a.reps):
        for name, run in legs:                                      # alternating: every round runs every leg
            ctx = owner[name]
            clear()
            ctx.synchronize()
            ctx.profile_enable(128)
            t0 = time.perf_counter()
            run()
            ctx.synchronize()
            t1 = time.perf_counter()
            got = ctx.profile_read()
            ctx.profile_enable(0)
            n_launch[name] = len(got)
            if rep >= 0:
                device[name].append(sum(ms for _, ms in got))
                wall[name].append(1e3 * (t1 - t0))
                kinds = {}
                for k, ms in got:
                    kinds[k] = kinds.get(k, 0.0) + ms
                per_kind.setdefault(name, []).append(kinds)

    out = {"tiles": n_sub, "blocks": n, "plan_entries": int(n_sub * n_el), "coded_bytes": int(lens.sum()), "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "outputs_equal_one_call": True}
    for name, _ in legs:
        dv, wl = stats(device[name]), stats(wall[name])
        out[name] = {"device": dv, "wall": wl, "brackets": n_launch[name],
                     "host_wait_share": max(0.0, (wl["ms_median"] - dv["ms_median"]) / wl["ms_median"]),
                     "device_ms_median_by_kind": {str(k): statistics.median(r.get(k, 0.0) for r in per_kind[name])
                                                  for k in sorted(per_kind[name][0])}}
    merged = {}
    if os.path.exists(a.out):
        try:
            merged = json.load(open(a.out))
        except ValueError:
            merged = {}
    base_name = "parent_one_call" if parent is not None else None
    base = out[base_name]["device"] if base_name else (merged.get("parent") or {}).get("one_call", {}).get("device")
    against = "the parent's one_call, same run" if base_name else "the parent's one_call, its own run" if base else "this build's one_call (no parent build given)"
    base = base or out["one_call"]["device"]
    if not only_plain:
        for P in PIECES:
            out["pieces_%d_over_parent" % P] = out["pieces_%d" % P]["device"]["ms_median"] / base["ms_median"]
            out["pieces_%d_over_one_call" % P] = out["pieces_%d" % P]["device"]["ms_median"] / out["one_call"]["device"]["ms_median"]
            out["pieces_%d_wall_over_one_call_wall" % P] = out["pieces_%d" % P]["wall"]["ms_median"] / out["one_call"]["wall"]["ms_median"]
        out["one_call_over_parent"] = out["one_call"]["device"]["ms_median"] / base["ms_median"]
        out["one_call_inside_parent_spread"] = base["ms_min"] <= out["one_call"]["device"]["ms_median"] <= base["ms_max"]
        ratio = out["pieces_1_over_parent"]
        out["expectation"] = {"text": "pieces_1 <= %.2f x one_call (device time), against %s" % (BOUND, against), "bound": BOUND,
                              "ratio": ratio, "verdict": "met" if ratio <= BOUND else "MISSED"}
        print("expectation %s: pieces_1 / parent one_call = %.3f (pieces_4 %.3f, pieces_16 %.3f); host wait share of pieces_1 %.2f" %
              (out["expectation"]["verdict"], ratio, out["pieces_4_over_parent"], out["pieces_16_over_parent"], out["pieces_1"]["host_wait_share"]))
        if a.piece_encoder == 7:
            for P in PIECES:
                out["pieces_%d_enc7_over_parent" % P] = out["pieces_%d_enc7" % P]["device"]["ms_median"] / base["ms_median"]
                out["pieces_%d_enc7_over_one_call" % P] = out["pieces_%d_enc7" % P]["device"]["ms_median"] / out["one_call"]["device"]["ms_median"]
            ratio = out["pieces_1_enc7_over_parent"]
            out["expectation_enc7"] = {"text": "pieces_1_enc7 <= %.2f x one_call (device time), against %s" % (BOUND, against), "bound": BOUND,
                                       "ratio": ratio, "verdict": "met" if ratio <= BOUND else "MISSED"}
            print("expectation under setting 7 %s: pieces_1_enc7 / one_call = %.3f (pieces_4_enc7 %.3f, pieces_16_enc7 %.3f)" %
                  (out["expectation_enc7"]["verdict"], ratio, out["pieces_4_enc7_over_parent"], out["pieces_16_enc7_over_parent"]))
    merged[a.label] = out
    if not only_plain:
        hip.piece_encoder_set(4)
    hip.close()
    if parent is not None:
        parent.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({a.label: out}))


if __name__ == "__main__":
    main()
