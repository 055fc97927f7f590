#!/usr/bin/env python3
"""The spliced rows (include/cabac_hip_splice_rows.h): cabac_hip_encode_residual_rows_device and
cabac_hip_encode_residual_sets_device beside the plain cabac_hip_encode_residual_device, on the same input, in the same process.

Workload: build_residual_tiles(N) (N = 4096: the bench's residual leg), one substream per tile of 400 blocks, laid out as N / 16
pictures x 16 rows in LEVEL ORDER (level r = row r of every picture, row r linked to row r - 1 of its picture).  The host records
of a tile are one cbf bin (1) per block, the block spliced in behind it, and the terminate bin; a "CTU" is 25 blocks, so every row
hands its contexts over at host record 25 with the 25 blocks in front of it.  Device buffers resident.  Legs, alternating within
every repetition so that drift of the machine touches all of them alike:
  plain        cabac_hip_encode_residual_device
  sets_noset   the sets form with no set (payload checked equal to the plain call's)
  rows         16 levels of N / 16 rows each, with and without d_sync_splice (payloads checked equal: no block begins a CTU here)
Times are HIP events from cabac_hip_profile_enable per profile kind, 2 warm-up + R timed repetitions; median, minimum, maximum per
kind and of the sum.  Writes one JSON object (--out, default profiles/splice_rows.json).

  python tools/bench_splice_rows.py [--tiles 4096] [--rows 16] [--reps 7] [--out FILE]
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

QP, CTU_BLOCKS = 32, 25
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_rows.json"))
    a = ap.parse_args()
    assert a.reps >= 3 and a.tiles % a.rows == 0

    tus, coeff, _ = build_residual_tiles(a.tiles)
    n, n_sub, n_row = len(tus), a.tiles, a.rows
    n_pic, per_tile = n_sub // n_row, n // n_sub
    assert per_tile * n_sub == n and per_tile > CTU_BLOCKS
    n_host = per_tile + 1
    records = np.full((n_sub, n_host), 0 | 0x8000, np.uint16)               # cbf = 1 on context 0 ...
    records[:, -1] = 0x1FF | 0x8000                                         # ... and the terminate bin
    splices = np.zeros(n, capi.SPLICE_DTYPE)
    splices["at"], splices["tu"] = np.tile(np.arange(per_tile, dtype=np.uint32) + 1, n_sub), np.arange(n, dtype=np.uint32)
    desc = np.zeros(n_sub, capi.DESC_DTYPE)
    desc["rec_offset"], desc["n_records"], desc["qp"] = np.arange(n_sub, dtype=np.uint64) * n_host, n_host, QP
    desc["init_id"] = 2 | capi.SUB_FINISH | capi.SUB_ALIGN_RBSP
    level_first = np.arange(0, n_sub + 1, n_pic, dtype=np.uint32)
    sync_from = np.concatenate([np.full(n_pic, NO, np.uint32), np.arange(n_sub - n_pic, dtype=np.uint32)])
    sync_at = np.full(n_sub, CTU_BLOCKS, np.uint32)

    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_desc, t_rec, t_sp = dev(desc), dev(records, np.int16), dev(splices)
    t_first = (torch.arange(n_sub + 1, device="cuda", dtype=torch.int32) * per_tile).contiguous()
    t_tu, t_co = dev(tus), dev(coeff, np.int32)
    t_from, t_at, t_spl = dev(sync_from, np.int32), dev(sync_at, np.int32), dev(sync_at, np.int32)
    t_noset = dev(np.full(n_sub, NO, np.uint32), np.int32)
    cap = int(len(coeff)) + 64 * n_sub
    t_off = torch.zeros(n_sub + 1, dtype=torch.int64, device="cuda")
    t_res = torch.zeros(2 * n_sub, dtype=torch.int32, device="cuda")
    pays = {k: torch.zeros(cap, dtype=torch.uint8, device="cuda") for k in ("plain", "sets_noset", "rows", "rows_null")}
    head = (n_sub, t_desc.data_ptr(), t_rec.data_ptr(), t_first.data_ptr(), t_sp.data_ptr(), n, n, t_tu.data_ptr(), t_co.data_ptr())
    tail = lambda pay: (pay.data_ptr(), cap, t_off.data_ptr(), t_res.data_ptr())
    legs = {
        "plain": lambda: hip.encode_residual_device(*head, *tail(pays["plain"])),
        "sets_noset": lambda: hip.encode_residual_sets_device(*head, *tail(pays["sets_noset"]), d_start_set=t_noset.data_ptr()),
        "rows": lambda: hip.encode_residual_rows_device(*head, *tail(pays["rows"]), level_first, t_from.data_ptr(), t_at.data_ptr(),
                                                        t_spl.data_ptr()),
        "rows_null": lambda: hip.encode_residual_rows_device(*head, *tail(pays["rows_null"]), level_first, t_from.data_ptr(),
                                                             t_at.data_ptr()),
    }
    samples = {leg: {} for leg in legs}
    for rep in range(-2, a.reps):
        for leg, run in legs.items():
            hip.synchronize()
            hip.profile_enable(64)
            run()
            hip.synchronize()
            got = hip.profile_read()
            hip.profile_enable(0)
            assert not t_res.cpu().numpy().view(capi.RESULT_DTYPE)["flags"].any(), leg
            if rep < 0:
                continue
            by_kind = {}
            for k, ms in got:
                by_kind[k] = by_kind.get(k, 0.0) + ms
            s = samples[leg]
            for k, ms in by_kind.items():
                s.setdefault("kind %d" % k, []).append(ms)
            s.setdefault("launch groups", []).append(len(got))
            s.setdefault("sum", []).append(sum(ms for _, ms in got))
    out = {"tiles": n_sub, "pictures": n_pic, "rows": n_row, "blocks": n, "host_records": int(n_sub * n_host), "reps": a.reps,
           "hand_over_record": CTU_BLOCKS, "device": torch.cuda.get_device_name(0), "coded_bytes": int(t_off[-1].item())}
    for leg, s in samples.items():
        out[leg] = {g: (stats(v) if g != "launch groups" else v[0]) for g, v in s.items()}
    out["sets_noset_bytes_equal_plain"] = bool(torch.equal(pays["sets_noset"], pays["plain"]))
    out["rows_null_bytes_equal_rows"] = bool(torch.equal(pays["rows_null"], pays["rows"]))
    out["rows_bytes_differ_from_plain"] = not bool(torch.equal(pays["rows"], pays["plain"]))
    assert out["sets_noset_bytes_equal_plain"] and out["rows_null_bytes_equal_rows"] and out["rows_bytes_differ_from_plain"]
    out["rows_over_plain"] = out["rows"]["sum"]["ms_median"] / out["plain"]["sum"]["ms_median"]
    hip.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
