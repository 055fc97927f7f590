#!/usr/bin/env python3
"""The unit parse (spliced substreams read back: side records and blocks in one walk) against the block-only residual parser.

Workload: build_residual_tiles(N) (N = 4096: the bench's residual leg), one substream per tile of 400 blocks, coded on the device
by cabac_hip_encode_residual_device, device buffers resident.  Three legs:
  parse        cabac_hip_residual_parse_device — an entry point the parent commit has too: copy this file into a checkout of the
               parent and run it there with --leg parse --label parent, writing to the same --out
  unit_empty   cabac_hip_parse_unit_device on the same bytes with no side records
  unit_side8   the same blocks with eight context-coded side records (contexts residual coding never touches) in front of every
               block and the terminate bin behind the last
Every leg checks that all coefficients (and side bins) come back.  Times are HIP events from cabac_hip_profile_enable (the
library's launch only), 3 warm-up + R timed repetitions; median, minimum and spread (max - min) per leg.
Writes one JSON object (--out, default profiles/parse_unit.json; merged with what the file holds under other labels).  When the
file holds a `parent` label, the ratios go in: parse / parse(parent) — "no slower" may be claimed below 1 + the parent's own
(median - min) / median —, unit_empty / parse(parent) and unit_side8 / unit_empty.

  python tools/bench_parse_unit.py [--tiles 4096] [--reps 10] [--leg all|parse|unit] [--label NAME] [--out FILE]
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
    ap.add_argument("--leg", default="all", choices=["all", "parse", "unit"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parse_unit.json"))
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

    def coded(records, n_rec, at):
        """The tiles coded by the device's own writer: per tile n_rec side records with block k of the tile spliced in front of
        record at(k).  -> (parse descriptors, bytes in 16-aligned slots)"""
        desc = np.zeros(n_sub, capi.DESC_DTYPE)
        desc["n_records"], desc["rec_offset"], desc["qp"] = n_rec, np.arange(n_sub, dtype=np.uint64) * n_rec, QP
        desc["init_id"] = 2 | capi.SUB_FINISH | capi.SUB_ALIGN_RBSP
        splices = np.zeros(n, capi.SPLICE_DTYPE)
        splices["tu"], splices["at"] = np.arange(n, dtype=np.uint32), np.tile(at, n_sub)
        cap = int(len(coeff)) + 2 * n_sub * n_rec + 64 * n_sub     # far above the coded size: under a byte per coefficient and record
        t_pay = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        t_off = torch.zeros(n_sub + 1, dtype=torch.int64, device="cuda")
        t_res = torch.zeros(2 * n_sub, dtype=torch.int32, device="cuda")
        keep = [dev(desc), dev(records, np.int16), dev(splices)]
        hip.encode_residual_device(n_sub, keep[0].data_ptr(), keep[1].data_ptr(), t_first.data_ptr(), keep[2].data_ptr(), n, n, t_tu.data_ptr(),
                                   t_co.data_ptr(), t_pay.data_ptr(), cap, t_off.data_ptr(), t_res.data_ptr())
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

    # the block-only bytes: the blocks of a tile, then its terminate bin
    desc, t_bytes, n_bytes = coded(np.full(n_sub, 0x81FF, np.uint16), 1, np.zeros(per_tile, np.uint32))
    out["coded_bytes"] = n_bytes
    t_desc = dev(desc)
    if a.leg in ("all", "parse"):
        def parse():
            hip.residual_parse_device(n_sub, t_desc.data_ptr(), t_bytes.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), t_dec.data_ptr(),
                                      t_res.data_ptr())
        out["parse"] = timed(parse, 9)
        came_back()
    if a.leg in ("all", "unit"):
        t_dec.zero_()
        bare = desc.copy()
        bare["n_records"], bare["rec_offset"], bare["init_id"] = 0, 0, 2
        t_bare = dev(bare)

        def unit_empty():
            hip.parse_unit_device(n_sub, t_bare.data_ptr(), t_bytes.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), 0, 0, t_dec.data_ptr(),
                                  0, t_res.data_ptr())
        out["unit_empty"] = timed(unit_empty, 25)
        came_back()
        # eight context-coded side records in front of every block, the terminate bin behind the last
        n_rec = N_SIDE * per_tile + 1
        gen = np.random.default_rng(1234)
        ids = gen.integers(0, 151, (n_sub, n_rec)).astype(np.uint16)
        ids = np.where(ids < 86, ids, ids + (292 - 86)).astype(np.uint16)
        rec = (ids | (gen.integers(0, 2, ids.shape).astype(np.uint16) << 15)).astype(np.uint16)
        rec[:, -1] = 0x81FF
        at = (np.arange(per_tile, dtype=np.uint32) + 1) * N_SIDE
        sdesc, t_sbytes, s_bytes = coded(rec, n_rec, at)
        t_sdesc, t_rec, t_at = dev(sdesc), dev(rec, np.int16), dev(np.tile(at, n_sub), np.int32)
        t_bins = torch.zeros(n_sub * n_rec, dtype=torch.uint8, device="cuda")
        t_dec.zero_()

        def unit_side():
            hip.parse_unit_device(n_sub, t_sdesc.data_ptr(), t_sbytes.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), t_at.data_ptr(),
                                  t_rec.data_ptr(), t_dec.data_ptr(), t_bins.data_ptr(), t_res.data_ptr())
        out["unit_side8"] = timed(unit_side, 25)
        came_back()
        assert bool(torch.equal(t_bins, (t_rec < 0).to(torch.uint8))), "the side bins did not come back"
        out["unit_side8"]["side_records"] = int(n_sub * n_rec)
        out["unit_side8"]["coded_bytes"] = s_bytes
        out["unit_side8"]["over_unit_empty"] = out["unit_side8"]["ms_median"] / out["unit_empty"]["ms_median"]
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
    par = merged.get("parent", {}).get("parse")
    if a.label != "parent" and par:
        margin = (par["ms_median"] - par["ms_min"]) / par["ms_median"]
        out["parent_parse_min_to_median_spread"] = margin
        if "parse" in out:
            out["parse"]["over_parent_parse"] = out["parse"]["ms_median"] / par["ms_median"]
            out["parse"]["no_slower_than_parent_parse"] = out["parse"]["over_parent_parse"] <= 1.0 + margin
        if "unit_empty" in out:
            out["unit_empty"]["over_parent_parse"] = out["unit_empty"]["ms_median"] / par["ms_median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({a.label: out}))


if __name__ == "__main__":
    main()
