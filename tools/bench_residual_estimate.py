#!/usr/bin/env python3
"""Costing transform blocks on the device: the fused residual estimator against the composed path.

Workload: build_residual_tiles(N) (N = 4096: the bench's residual leg), one block per candidate, 64 start sets
(ctx_init of 64 (qp, init) pairs), device buffers resident.
  composed  cabac_hip_residual_device sizes pass + prefix sum (torch.cumsum) + records pass + cabac_hip_estimate_from_device —
            entry points every commit since the estimator has; run this leg on the parent commit as well
  fused     cabac_hip_estimate_residual_device
Times are HIP events from cabac_hip_profile_enable (the library's launches only: the composed path's prefix sum and
descriptor fill are NOT counted, which favours it), 3 warm-up + R timed repetitions, median and min.
Writes one JSON object (--out, default profiles/residual_estimate.json; merged with what the file holds under other labels).

  python tools/bench_residual_estimate.py [--tiles 4096] [--reps 10] [--leg both|composed|fused] [--label NAME] [--out FILE]
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

N_SETS = 64


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(-1).copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--leg", default="both", choices=["both", "composed", "fused"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_estimate.json"))
    a = ap.parse_args()

    tus, coeff, _ = build_residual_tiles(a.tiles)
    n = len(tus)
    hip = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_tu, t_co = dev(tus, np.uint8), dev(coeff, np.int32)
    t_qp = torch.arange(N_SETS, dtype=torch.int32, device="cuda") % 52 + 10
    t_init = (torch.arange(N_SETS, dtype=torch.int32, device="cuda") % 3).contiguous()
    t_state = torch.zeros(N_SETS * capi.NUM_CTX, dtype=torch.int32, device="cuda")
    t_rate = torch.zeros(N_SETS * capi.NUM_CTX, dtype=torch.uint8, device="cuda")
    hip.ctx_init_device(N_SETS, t_qp.data_ptr(), t_init.data_ptr(), t_state.data_ptr(), t_rate.data_ptr())
    t_set = (torch.arange(n, dtype=torch.int32, device="cuda") * 37 % N_SETS).contiguous()
    t_first = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    hip.synchronize()
    out = {"tiles": a.tiles, "blocks": n, "coefficients": int(len(coeff)), "start_sets": N_SETS, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}

    def timed(run):
        for _ in range(3):
            run()
        hip.synchronize()
        hip.profile_enable(8)
        samples = []
        for _ in range(a.reps):
            run()
            samples.append(hip.profile_read())
        hip.profile_enable(0)
        return samples

    # ---- composed: sizes pass, prefix sum, records pass, estimator over the records --------------------------------
    t_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    hip.residual_device(n, t_tu.data_ptr(), t_co.data_ptr(), 0, t_cnt.data_ptr(), 0, 0)
    hip.synchronize()
    n_bins = int(t_cnt.to(torch.int64).sum().item())
    out["bins"] = n_bins
    composed_bits = None
    if a.leg in ("both", "composed"):
        t_rec = torch.zeros(n_bins + 16, dtype=torch.int16, device="cuda")
        t_desc = torch.zeros(n * 4, dtype=torch.int64, device="cuda")           # cabac_substream_desc: 32 bytes
        t_roff = torch.zeros(n, dtype=torch.int64, device="cuda")
        t_bits = torch.zeros(n, dtype=torch.int64, device="cuda")
        t_flags = torch.zeros(n, dtype=torch.int32, device="cuda")

        def composed():
            hip.residual_device(n, t_tu.data_ptr(), t_co.data_ptr(), 0, t_cnt.data_ptr(), 0, 0)
            c64 = t_cnt.to(torch.int64)
            torch.cumsum(c64, 0, out=t_roff)
            t_roff.sub_(c64)
            d = t_desc.view(n, 4)
            d[:, 0] = t_roff                    # rec_offset
            d[:, 2] = c64                       # n_records (low word), byte_capacity 0
            hip.residual_device(n, t_tu.data_ptr(), t_co.data_ptr(), t_roff.data_ptr(), t_cnt.data_ptr(), 0, t_rec.data_ptr())
            hip.estimate_from_device(n, t_desc.data_ptr(), t_rec.data_ptr(), t_state.data_ptr(), t_rate.data_ptr(), t_set.data_ptr(),
                                     t_bits.data_ptr(), t_flags.data_ptr())

        samples = timed(composed)
        assert all([k for k, _ in s] == [5, 5, 4] for s in samples), samples[0]
        assert not t_flags.any().item()
        composed_bits = t_bits.clone()
        tot = [sum(ms for _, ms in s) for s in samples]
        out["composed"] = {
            "ms_median": statistics.median(tot), "ms_min": min(tot),
            "sizes_pass_ms_median": statistics.median(s[0][1] for s in samples),
            "records_pass_ms_median": statistics.median(s[1][1] for s in samples),
            "estimate_ms_median": statistics.median(s[2][1] for s in samples),
            "gbins_per_s": n_bins / statistics.median(tot) / 1e6,
            # coefficients read twice, descriptors twice, 2 B per bin written and read back, offsets / counts / substream descriptors
            "bytes_per_coefficient": (2 * 4 * len(coeff) + 2 * 16 * n + 4 * n_bins + (4 + 8 + 32 + 8 + 4) * n) / len(coeff),
        }
        del t_rec
    # ---- fused ------------------------------------------------------------------------------------------------------
    if a.leg in ("both", "fused"):
        t_fb = torch.zeros(n, dtype=torch.int64, device="cuda")

        def fused():
            hip.estimate_residual_device(n, t_first.data_ptr(), t_tu.data_ptr(), t_co.data_ptr(), t_state.data_ptr(), t_rate.data_ptr(),
                                         t_set.data_ptr(), t_fb.data_ptr())

        samples = timed(fused)
        assert all([k for k, _ in s] == [12] for s in samples), samples[0]
        tot = [s[0][1] for s in samples]
        out["fused"] = {
            "ms_median": statistics.median(tot), "ms_min": min(tot),
            "gcoefficients_per_s": len(coeff) / statistics.median(tot) / 1e6,
            "gbins_per_s": n_bins / statistics.median(tot) / 1e6,
            # coefficients once, descriptors (ordering pre-pass + walk), candidate bounds, set index, order, result
            "bytes_per_coefficient": (4 * len(coeff) + 2 * 16 * n + (8 + 4 + 12 + 8) * n) / len(coeff),
        }
        if composed_bits is not None:
            assert torch.equal(t_fb, composed_bits), "fused and composed costs differ"
            out["fused"]["equal_to_composed"] = True
            out["fused"]["speedup_median_over_composed_median"] = out["composed"]["ms_median"] / out["fused"]["ms_median"]
            out["fused"]["median_below_composed_min"] = out["fused"]["ms_median"] < out["composed"]["ms_min"]
    hip.close()

    merged = {}
    if os.path.exists(a.out):
        try:
            merged = json.load(open(a.out))
        except ValueError:
            merged = {}
    merged[a.label] = out
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({a.label: out}))


if __name__ == "__main__":
    main()
