#!/usr/bin/env python3
"""The plan parse (the element parse with computed entries: conditions on several values and on block results) against the
element parse.

Workload: build_residual_tiles(N) (N = 4096: the bench's residual leg), one substream per tile of 400 blocks, coded on the device
by cabac_hip_encode_residual_device, device buffers resident (tools/bench_parse_elements.py's workload).  Three legs:
  elements_guarded  cabac_hip_parse_elements_device: every block behind a cbf element of 1 that guards it, and per block one
                    UNARY_MAX (maxSymbol 5), an EXP_GOLOMB escape guarded by "prefix == 5" and a sign bin guarded by "prefix != 0"
                    (tools/bench_parse_elements.py's leg) — an entry point the parent commit has too: copy this file into a
                    checkout of the parent and run it there with --leg elements --label parent, writing to the same --out
  plan_same         cabac_hip_parse_plan_device on the very same plan and bytes
  plan_tu           the luma path of the tests' transform-unit plan around every block, 14 entries: cbf, an "any cbf" COND joined
                    by OR, cu_qp_delta behind it (the three elements above), the block behind its cbf, four BLOCK_INFO fields of
                    the block's info word (scanPosLast, MTS_VIOLATION, TS, NOT_CODED), an AND chain of four CONDs over them, and
                    an mts_idx-like UNARY_MAX (maxSymbol 4) behind the chain
Every leg checks that all coefficients and values come back.  Times are HIP events from cabac_hip_profile_enable (the library's
launch only), 3 warm-up + R timed repetitions; median, minimum and spread (max - min) per leg.
Writes one JSON object (--out, default profiles/parse_plan.json; merged with what the file holds under other labels).  When the
file holds a `parent` label, elements_guarded / elements_guarded(parent) goes in — "no slower" may be claimed below 1 + the parent's
own (median - min) / median.  plan_same / elements_guarded and plan_tu / plan_same are recorded; no bound is set on them.

  python tools/bench_parse_plan.py [--tiles 4096] [--reps 10] [--leg all|elements|plan] [--label NAME] [--out FILE]
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

N_SIDE, QP = 8, 32


def dev(a, dt=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms_spread": max(ms) - min(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--leg", default="all", choices=["all", "elements", "plan"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parse_plan.json"))
    a = ap.parse_args()
    assert a.reps >= 10

    tus, coeff, tile_first = build_residual_tiles(a.tiles)
    n, n_sub = len(tus), a.tiles
    per_tile = n // n_sub
    assert per_tile * n_sub == n
    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_tu, t_co = dev(tus), dev(coeff, np.int32)
    t_first = (torch.arange(n_sub + 1, device="cuda", dtype=torch.int32) * per_tile).contiguous()
    out = {"tiles": n_sub, "blocks": n, "coefficients": int(len(coeff)), "reps": a.reps, "device": torch.cuda.get_device_name(0)}

    def coded(t_records, rec_offset, n_rec, at):
        """The tiles coded by the device's own writer: tile s has the side records [rec_offset[s], + n_rec[s]) with block k of the
        tile spliced in front of record at[s * per_tile + k].  -> (parse descriptors without rec_offset / n_records, bytes in
        16-aligned slots, coded bytes)"""
        desc = np.zeros(n_sub, capi.DESC_DTYPE)
        desc["n_records"], desc["rec_offset"], desc["qp"] = n_rec, rec_offset, QP
        desc["init_id"] = 2 | capi.SUB_FINISH | capi.SUB_ALIGN_RBSP
        splices = np.zeros(n, capi.SPLICE_DTYPE)
        splices["tu"], splices["at"] = np.arange(n, dtype=np.uint32), at
        cap = int(len(coeff)) + 2 * int(np.sum(n_rec)) + 64 * n_sub     # far above the coded size
        t_pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        t_off = torch.zeros(n_sub + 1, dtype=torch.int64, device="cuda")
        t_res = torch.zeros(2 * n_sub, dtype=torch.int32, device="cuda")
        keep = [dev(desc), dev(splices)]
        hip.encode_residual_device(n_sub, keep[0].data_ptr(), t_records.data_ptr(), t_first.data_ptr(), keep[1].data_ptr(), n, n,
                                   t_tu.data_ptr(), t_co.data_ptr(), t_pay.data_ptr(), cap, t_off.data_ptr(), t_res.data_ptr())
        hip.synchronize()
        assert not t_res.cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any()
        off = t_off.cpu().numpy()
        pay = t_pay[:int(off[-1])].cpu().numpy()
        lens = np.diff(off).astype(np.uint64)
        slots = (lens + 15) // 16 * 16 + 16
        desc["byte_offset"] = np.concatenate([[0], np.cumsum(slots)[:-1]])
        desc["byte_capacity"] = lens
        desc["init_id"] = 2 | capi.SUB_FINISH
        buf = np.zeros(int(slots.sum()), np.uint8)
        for s in range(n_sub):
            buf[int(desc["byte_offset"][s]):int(desc["byte_offset"][s]) + int(lens[s])] = pay[int(off[s]):int(off[s + 1])]
        return desc, dev(buf), int(lens.sum())

    def timed(run, kind):
        for _ in range(3):
            run()
        hip.synchronize()
        hip.profile_enable(4)
        samples = []
        for _ in range(a.reps):
            run()
            s = hip.profile_read()
            assert [k for k, _ in s] == [kind], s
            samples.append(s[0][1])
        hip.profile_enable(0)
        return stats(samples)

    t_dec = torch.zeros_like(t_co)
    t_res = torch.zeros(2 * n_sub, dtype=torch.int32, device="cuda")

    def came_back():
        res = t_res.cpu().numpy().view(capi.RESULT_DTYPE)
        assert not res["flags"].any() and bool(torch.equal(t_dec, t_co)), "the coefficients did not come back"

    gen = np.random.default_rng(1234)
    # per block: cbf (1) -> block; a unary prefix (maxSymbol 5), its escape behind "== 5", a sign behind "!= 0"
    n_el = 4 * per_tile + 1
    pre = gen.integers(0, 6, n).astype(np.uint32)
    esc = np.where(pre == 5, gen.integers(0, 12, n), 0).astype(np.uint32)
    sign = np.where(pre != 0, gen.integers(0, 2, n), 0).astype(np.uint32)
    w0 = np.array([capi.element(capi.SE_CTX_BIN, ctx=0), capi.element(capi.SE_UNARY_MAX, ctx=1, ctx_n=2, max_symbol=5),
                   capi.element(capi.SE_EXP_GOLOMB, count=0), capi.element(capi.SE_EP_BINS, n=1)], np.uint32)
    gw = np.array([0, 0, capi.guard(1, capi.GUARD_EQ, 5), capi.guard(2, capi.GUARD_NE, 0)], np.uint32)
    gplan = np.zeros((n_sub, n_el, 2), np.uint32)
    gplan[:, :-1, 0], gplan[:, :-1, 1] = np.tile(w0, per_tile), np.tile(gw, per_tile)
    gplan[:, -1, 0] = capi.SE_TRM
    values = np.zeros((n_sub, n_el), np.uint32)
    values[:, :-1] = np.stack([np.ones(n, np.uint32), pre, esc, sign], 1).reshape(n_sub, 4 * per_tile)
    values[:, -1] = 1
    active = np.ones((n_sub, n_el), bool)
    active[:, :-1] = np.stack([np.ones(n, bool), np.ones(n, bool), pre == 5, pre != 0], 1).reshape(n_sub, 4 * per_tile)
    # the writer's side: the active elements through the device binariser, the blocks spliced behind their four elements
    se = np.stack([gplan[..., 0][active], values[active]], 1).astype(np.uint32)
    se_off = np.concatenate([[0], np.cumsum(active.sum(1))]).astype(np.uint64)
    ones = np.floor(np.log2(esc.astype(np.float64) + 1)).astype(np.int64)                  # exp_golomb_eqprob, count 0
    per_block = 1 + np.minimum(pre.astype(np.int64) + 1, 5) + np.where(pre == 5, 2 * ones + 1, 0) + (pre != 0)
    n_grec = per_block.reshape(n_sub, per_tile).sum(1) + 1
    g_off = np.concatenate([[0], np.cumsum(n_grec)]).astype(np.uint64)
    t_se, t_se_off, t_goff = dev(se, np.int32), dev(se_off, np.int64), dev(g_off[:-1], np.int64)
    t_cnt = torch.zeros(n_sub, dtype=torch.int32, device="cuda")
    t_grec = torch.zeros(int(g_off[-1]), dtype=torch.int16, device="cuda")
    hip.binarize_device(n_sub, t_se_off.data_ptr(), t_se.data_ptr(), t_goff.data_ptr(), t_cnt.data_ptr(), t_grec.data_ptr())
    hip.synchronize()
    assert np.array_equal(t_cnt.cpu().numpy().astype(np.int64), n_grec), "the binariser's record counts are not the expected ones"
    g_at = np.cumsum(per_block.reshape(n_sub, per_tile), 1).reshape(-1).astype(np.uint32)   # block k behind its own elements
    gdesc, t_gbytes, g_bytes = coded(t_grec, g_off[:-1], n_grec.astype(np.uint32), g_at)
    gdesc["n_records"], gdesc["rec_offset"] = n_el, np.arange(n_sub, dtype=np.uint64) * n_el
    t_gdesc, t_gplan = dev(gdesc), dev(gplan, np.int32)
    t_gat = dev(np.tile((np.arange(per_tile, dtype=np.uint32) + 1) * 4, n_sub), np.int32)
    t_guard = dev(np.full(n, capi.guard(4, capi.GUARD_EQ, 1), np.uint32), np.int32)
    t_gval = torch.zeros(n_sub * n_el, dtype=torch.int32, device="cuda")
    t_dec.zero_()

    def elements_guarded():
        hip.parse_elements_device(n_sub, t_gdesc.data_ptr(), t_gbytes.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), t_gat.data_ptr(),
                                  t_guard.data_ptr(), t_gplan.data_ptr(), t_dec.data_ptr(), t_gval.data_ptr(), t_res.data_ptr())
    t_info = torch.zeros(n, dtype=torch.int32, device="cuda")
    if a.leg in ("all", "elements"):
        out["elements_guarded"] = timed(elements_guarded, 26)
        came_back()
        assert np.array_equal(t_gval.cpu().numpy().view(np.uint32), values.reshape(-1)), "the values did not come back"
        out["elements_guarded"].update(elements=int(n_sub * n_el), skipped_elements=int((~active).sum()), coded_bytes=g_bytes)
    if a.leg in ("all", "plan"):
        # the very same plan and bytes through the new entry point
        t_gval.zero_()
        t_dec.zero_()

        def plan_same():
            hip.parse_plan_device(n_sub, t_gdesc.data_ptr(), t_gbytes.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), t_gat.data_ptr(),
                                  t_guard.data_ptr(), t_gplan.data_ptr(), t_dec.data_ptr(), t_gval.data_ptr(), t_res.data_ptr(),
                                  d_tu_info=t_info.data_ptr())
        out["plan_same"] = timed(plan_same, 27)
        came_back()
        assert np.array_equal(t_gval.cpu().numpy().view(np.uint32), values.reshape(-1)), "the values did not come back"
        out["plan_same"].update(elements=int(n_sub * n_el), coded_bytes=g_bytes)
        if "elements_guarded" in out:
            out["plan_same"]["over_elements_guarded"] = out["plan_same"]["ms_median"] / out["elements_guarded"]["ms_median"]
        # the luma path of the transform-unit plan around every block.  The info words are the parser's own (the run above)
        info = t_info.cpu().numpy().view(np.uint32)
        last, viol, ts = info & 0xFFFF, (info >> 16) & 1, (info >> 17) & 1
        assert not (info & capi.TU_INFO_NOT_CODED).any()
        mts_on = (ts == 0) & (last >= 1) & (viol == 0)
        mts = np.where(mts_on, gen.integers(0, 5, n), 0).astype(np.uint32)
        E, C, B = capi.element, capi.cond, capi.block_info
        NE, EQ, GE = capi.GUARD_NE, capi.GUARD_EQ, capi.GUARD_GE
        per = [(E(capi.SE_CTX_BIN, ctx=0), 0), C(1, NE, 0, capi.JOIN_OR, 1),
               (E(capi.SE_UNARY_MAX, ctx=1, ctx_n=2, max_symbol=5), capi.guard(1, NE, 0)),
               (E(capi.SE_EXP_GOLOMB, count=0), capi.guard(1, EQ, 5)), (E(capi.SE_EP_BINS, n=1), capi.guard(2, NE, 0)),
               (B(0, 0, 16), 0), (B(0, 16, 1), 0), (B(0, 17, 1), 0), (B(0, 18, 1), 0),
               C(1, EQ, 0), C(3, EQ, 0, capi.JOIN_AND, 1), C(6, GE, 1, capi.JOIN_AND, 1), C(6, EQ, 0, capi.JOIN_AND, 1),
               (E(capi.SE_UNARY_MAX, ctx=3, ctx_n=4, max_symbol=4), capi.guard(1, NE, 0))]
        n_per, block_at = len(per), 5                                        # the block lies in front of entry 5, behind its cbf
        n_tel = n_per * per_tile + 1
        tplan = np.zeros((n_sub, n_tel, 2), np.uint32)
        tplan[:, :-1] = np.tile(np.array(per, np.uint32), (per_tile, 1))
        tplan[:, -1, 0] = capi.SE_TRM
        one = np.ones(n, np.uint32)
        not_ts = (ts == 0).astype(np.uint32)
        c11 = not_ts & (last >= 1)
        tvalues = np.zeros((n_sub, n_tel), np.uint32)
        tvalues[:, :-1] = np.stack([one, one, pre, esc, sign, last, viol, ts, 0 * one, one, not_ts, c11, mts_on.astype(np.uint32), mts],
                                   1).reshape(n_sub, n_per * per_tile)
        tvalues[:, -1] = 1
        real = np.zeros(n_per, bool)
        real[[0, 2, 3, 4, 13]] = True
        tactive = np.ones((n_sub, n_tel), bool)
        always, never = np.ones(n, bool), np.zeros(n, bool)
        tactive[:, :-1] = np.stack([always, never, always, pre == 5, pre != 0] + [never] * 8 + [mts_on], 1).reshape(n_sub, n_per * per_tile)
        assert not tactive[:, :-1].reshape(n, n_per)[:, ~real].any()
        tse = np.stack([tplan[..., 0][tactive], tvalues[tactive]], 1).astype(np.uint32)
        tse_off = np.concatenate([[0], np.cumsum(tactive.sum(1))]).astype(np.uint64)
        after = np.where(mts_on, np.minimum(mts.astype(np.int64) + 1, 4), 0)             # the mts records lie behind the block
        t_nrec = (per_block + after).reshape(n_sub, per_tile).sum(1) + 1
        t_off = np.concatenate([[0], np.cumsum(t_nrec)]).astype(np.uint64)
        t_tse, t_tse_off, t_toff = dev(tse, np.int32), dev(tse_off, np.int64), dev(t_off[:-1], np.int64)
        t_trec = torch.zeros(int(t_off[-1]), dtype=torch.int16, device="cuda")
        hip.binarize_device(n_sub, t_tse_off.data_ptr(), t_tse.data_ptr(), t_toff.data_ptr(), t_cnt.data_ptr(), t_trec.data_ptr())
        hip.synchronize()
        assert np.array_equal(t_cnt.cpu().numpy().astype(np.int64), t_nrec), "the binariser's record counts are not the expected ones"
        both = (per_block + after).reshape(n_sub, per_tile)
        tu_rec_at = (np.cumsum(both, 1) - after.reshape(n_sub, per_tile)).reshape(-1).astype(np.uint32)
        tdesc, t_tbytes, t_bytes = coded(t_trec, t_off[:-1], t_nrec.astype(np.uint32), tu_rec_at)
        tdesc["n_records"], tdesc["rec_offset"] = n_tel, np.arange(n_sub, dtype=np.uint64) * n_tel
        t_tdesc, t_tplan = dev(tdesc), dev(tplan, np.int32)
        t_tat = dev(np.tile(np.arange(per_tile, dtype=np.uint32) * n_per + block_at, n_sub), np.int32)
        t_tguard = dev(np.full(n, capi.guard(block_at, EQ, 1), np.uint32), np.int32)
        t_tval = torch.zeros(n_sub * n_tel, dtype=torch.int32, device="cuda")
        t_dec.zero_()

        def plan_tu():
            hip.parse_plan_device(n_sub, t_tdesc.data_ptr(), t_tbytes.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), t_tat.data_ptr(),
                                  t_tguard.data_ptr(), t_tplan.data_ptr(), t_dec.data_ptr(), t_tval.data_ptr(), t_res.data_ptr())
        out["plan_tu"] = timed(plan_tu, 27)
        came_back()
        assert np.array_equal(t_tval.cpu().numpy().view(np.uint32), tvalues.reshape(-1)), "the values did not come back"
        out["plan_tu"].update(entries=int(n_sub * n_tel), computed_entries=int(n * 9), mts_coded=int(mts_on.sum()), coded_bytes=t_bytes)
        out["plan_tu"]["over_plan_same"] = out["plan_tu"]["ms_median"] / out["plan_same"]["ms_median"]
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
    par = merged.get("parent", {}).get("elements_guarded")
    if a.label != "parent" and par and "elements_guarded" in out:
        margin = (par["ms_median"] - par["ms_min"]) / par["ms_median"]
        out["parent_elements_guarded_min_to_median_spread"] = margin
        out["elements_guarded"]["over_parent_elements_guarded"] = out["elements_guarded"]["ms_median"] / par["ms_median"]
        out["elements_guarded"]["no_slower_than_parent_elements_guarded"] = out["elements_guarded"]["over_parent_elements_guarded"] <= 1.0 + margin
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({a.label: out}))


if __name__ == "__main__":
    main()
