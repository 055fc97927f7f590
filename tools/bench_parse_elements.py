#!/usr/bin/env python3
"""The element parse (the unit parse over a plan of syntax elements, with guards) against the unit parse.

Workload: build_residual_tiles(N) (N = 4096: the bench's residual leg), one substream per tile of 400 blocks, coded on the device
by cabac_hip_encode_residual_device, device buffers resident.  Three legs:
  unit_side8        cabac_hip_parse_unit_device with eight context-coded side records in front of every block and the terminate
                    bin behind the last (tools/bench_parse_unit.py's leg) — an entry point the parent commit has too: copy this
                    file into a checkout of the parent and run it there with --leg unit --label parent, writing to the same --out
  elements_side8    cabac_hip_parse_elements_device on the same bytes, the same side bins as unguarded single-bin elements
  elements_guarded  every block behind a cbf element of 1 that guards it, and per block one UNARY_MAX (maxSymbol 5), an
                    EXP_GOLOMB escape guarded by "prefix == 5" and a sign bin guarded by "prefix != 0" (cu_qp_delta's shape); the
                    records are the device binariser's
Every leg checks that all coefficients (and side bins / values) come back.  Times are HIP events from cabac_hip_profile_enable
(the library's launch only), 3 warm-up + R timed repetitions; median, minimum and spread (max - min) per leg.
Writes one JSON object (--out, default profiles/parse_elements.json; merged with what the file holds under other labels).  When
the file holds a `parent` label, unit_side8 / unit_side8(parent) goes in — "no slower" may be claimed below 1 + the parent's own
(median - min) / median.  elements_side8 / unit_side8 and elements_guarded / elements_side8 are recorded; no bound is set on them.

  python tools/bench_parse_elements.py [--tiles 4096] [--reps 10] [--leg all|unit|elements] [--label NAME] [--out FILE]
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
    ap.add_argument("--leg", default="all", choices=["all", "unit", "elements"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parse_elements.json"))
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

    # eight context-coded side records (contexts residual coding never touches) in front of every block, the terminate bin behind
    n_rec = N_SIDE * per_tile + 1
    gen = np.random.default_rng(1234)
    ids = gen.integers(0, 151, (n_sub, n_rec)).astype(np.uint16)
    ids = np.where(ids < 86, ids, ids + (292 - 86)).astype(np.uint16)
    rec = (ids | (gen.integers(0, 2, ids.shape).astype(np.uint16) << 15)).astype(np.uint16)
    rec[:, -1] = 0x81FF
    at = (np.arange(per_tile, dtype=np.uint32) + 1) * N_SIDE
    t_rec = dev(rec, np.int16)
    sdesc, t_sbytes, s_bytes = coded(t_rec, np.arange(n_sub, dtype=np.uint64) * n_rec, n_rec, np.tile(at, n_sub))
    t_sdesc, t_at = dev(sdesc), dev(np.tile(at, n_sub), np.int32)
    if a.leg in ("all", "unit"):
        t_bins = torch.zeros(n_sub * n_rec, dtype=torch.uint8, device="cuda")

        def unit_side():
            hip.parse_unit_device(n_sub, t_sdesc.data_ptr(), t_sbytes.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), t_at.data_ptr(),
                                  t_rec.data_ptr(), t_dec.data_ptr(), t_bins.data_ptr(), t_res.data_ptr())
        out["unit_side8"] = timed(unit_side, 25)
        came_back()
        assert bool(torch.equal(t_bins, (t_rec < 0).to(torch.uint8))), "the side bins did not come back"
        out["unit_side8"]["side_records"] = int(n_sub * n_rec)
        out["unit_side8"]["coded_bytes"] = s_bytes
    if a.leg in ("all", "elements"):
        # the same bytes, the side bins as single-bin elements
        plan = np.zeros((n_sub * n_rec, 2), np.uint32)
        plan[:, 0] = (ids.reshape(-1).astype(np.uint32) << 4) | capi.SE_CTX_BIN
        plan[n_rec - 1::n_rec, 0] = capi.SE_TRM
        t_plan = dev(plan, np.int32)
        t_val = torch.zeros(n_sub * n_rec, dtype=torch.int32, device="cuda")
        t_dec.zero_()

        def elements_side():
            hip.parse_elements_device(n_sub, t_sdesc.data_ptr(), t_sbytes.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), t_at.data_ptr(), 0,
                                      t_plan.data_ptr(), t_dec.data_ptr(), t_val.data_ptr(), t_res.data_ptr())
        out["elements_side8"] = timed(elements_side, 26)
        came_back()
        assert bool(torch.equal(t_val, (t_rec < 0).to(torch.int32))), "the side bins did not come back"
        out["elements_side8"]["elements"] = int(n_sub * n_rec)
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
        out["elements_guarded"] = timed(elements_guarded, 26)
        came_back()
        assert np.array_equal(t_gval.cpu().numpy().view(np.uint32), values.reshape(-1)), "the values did not come back"
        out["elements_guarded"].update(elements=int(n_sub * n_el), skipped_elements=int((~active).sum()), coded_bytes=g_bytes)
        out["elements_guarded"]["over_elements_side8"] = out["elements_guarded"]["ms_median"] / out["elements_side8"]["ms_median"]
        if "unit_side8" in out:
            out["elements_side8"]["over_unit_side8"] = out["elements_side8"]["ms_median"] / out["unit_side8"]["ms_median"]
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
    par = merged.get("parent", {}).get("unit_side8")
    if a.label != "parent" and par and "unit_side8" in out:
        margin = (par["ms_median"] - par["ms_min"]) / par["ms_median"]
        out["parent_unit_side8_min_to_median_spread"] = margin
        out["unit_side8"]["over_parent_unit_side8"] = out["unit_side8"]["ms_median"] / par["ms_median"]
        out["unit_side8"]["no_slower_than_parent_unit_side8"] = out["unit_side8"]["over_parent_unit_side8"] <= 1.0 + margin
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({a.label: out}))


if __name__ == "__main__":
    main()
