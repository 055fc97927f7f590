#!/usr/bin/env python3
"""Sparse coefficient transport (include/cabac_hip_sparse.h) beside the dense 16-bit forms it stands in for.

Workload: the benchmark's residual tiles, workload.build_residual_tiles(256) replicated to 4 096 tiles (as bench.py's residual
leg does), at three densities chosen on the CPU (--calibrate prints the share of non-zeros a density parameter gives): the
default, one near 25 % and one near 60 % non-zeros.  Every large host buffer is pinned.  Per density, in one process:
  wall    cabac_hip_encode_batch_residual16 against cabac_hip_sparse_encode_batch, and cabac_hip_residual_parse_batch16 against
          cabac_hip_sparse_parse_batch: 3 warm-up calls each, then the dense and the sparse form alternate, R repetitions each;
          median and spread (min .. max).  The dense form measured here is the baseline, not figures of earlier runs.
  bytes   what each form moves each way, computed from shapes.
  gpu     HIP-event times of the profile ring for one call of each form: kind 41 (coefficient expand) and 42 (coefficient
          compact) beside 5 (the binariser's two passes) and 9 (the parser).
  device  cabac_hip_sparse_expand_device / _compact_device on resident buffers alternating with a device-to-device
          hipMemcpyAsync of the same dense buffer, R repetitions, medians: the expand (zeroing included) writes the buffer once
          where the copy also reads it; the compact reads it at most twice.
  host    single-thread wall time of cabac_hip_sparse_pack_host / _unpack_host on the same blocks: whether a caller who must pack
          still wins.
Writes one JSON object (--out, default profiles/sparse_transport.json) with the three acceptance checks of the default density.

  python tools/bench_sparse_transport.py [--reps 20] [--tiles 4096] [--out FILE]
  python tools/bench_sparse_transport.py --calibrate            # CPU only
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from entropy_coding_amd import capi  # noqa: E402
from entropy_coding_amd import workload as W  # noqa: E402

# density parameter of build_residual_tiles -> share of non-zero coefficients (--calibrate, 64 tiles): the default 0.12 gives
# 3.2 %; the other two were chosen to land near 25 % and 60 %
DENSITIES = [("default", 0.12), ("quarter", 1.1), ("dense", 3.25)]
UNIQUE = 256


def share_of_nonzeros(density, tiles=64):
    tus, coeff, _ = W.build_residual_tiles(tiles, density=density)
    return float(np.count_nonzero(coeff)) / len(coeff), len(tus), len(coeff)


def calibrate():
    for d in (0.12, 0.5, 0.8, 1.0, 1.2, 1.5, 2.0, 2.5, 3.0, 4.0, 6.0):
        share, n_tu, n_coeff = share_of_nonzeros(d)
        print("density %-5g  non-zero %.4f  (%d blocks, %d coefficients)" % (d, share, n_tu, n_coeff))


def med(xs):
    return {"median_ms": round(statistics.median(xs) * 1e3, 4), "min_ms": round(min(xs) * 1e3, 4), "max_ms": round(max(xs) * 1e3, 4),
            "spread_ms": round((max(xs) - min(xs)) * 1e3, 4)}


def pinned(shape, dtype, fill=None):
    p = capi.PinnedArray(shape, dtype)
    if fill is not None:
        p.array[...] = fill
    return p


def ring(hip, call):
    """HIP-event milliseconds per profile kind of one call"""
    hip.profile_enable(256)
    hip.profile_read()
    call()
    out = {}
    for kind, ms in hip.profile_read():
        out[int(kind)] = out.get(int(kind), 0.0) + float(ms)
    hip.profile_enable(0)
    return out


def run_density(hip, name, density, n_tiles, reps):
    import torch
    copies = max(n_tiles // UNIQUE, 1)
    n_tiles = copies * UNIQUE
    tus, coeff, tile_first = W.build_residual_tiles(UNIQUE, density=density)
    assert int(coeff.min()) >= -32768 and int(coeff.max()) <= 32767
    per_tile = len(tus) // UNIQUE
    n_u, c_u = len(tus), len(coeff)
    all_tus = np.tile(tus, copies)
    all_tus["coeff_offset"] += np.repeat(np.arange(copies, dtype=np.uint64) * np.uint64(c_u), n_u)
    n_tu, n_coeff = len(all_tus), c_u * copies
    keep = []
    dense = pinned((n_coeff,), np.int16)
    keep.append(dense)
    for r in range(copies):
        dense.array[r * c_u:(r + 1) * c_u] = coeff
    share = float(np.count_nonzero(coeff)) / c_u

    # ---- host: pack / unpack, single thread
    ent_first = pinned((n_tu + 1,), np.uint32)
    keep.append(ent_first)
    need = int(np.count_nonzero(dense.array))                       # (nothing lies outside the coded regions of these tiles)
    entries = pinned((max(need, 1),), np.uint32)
    keep.append(entries)
    t_pack, t_unpack = [], []
    back = np.zeros(n_coeff, np.int16)
    for _ in range(3):
        t0 = time.perf_counter()
        _, ent, st = capi.sparse_pack_host(all_tus, dense.array, entries=entries.array, ent_first=ent_first.array)
        t_pack.append(time.perf_counter() - t0)
        assert int(st["n_entries"]) == need and int(st["flags"]) == 0
        t0 = time.perf_counter()
        st = capi.sparse_unpack_host(all_tus, ent_first.array, ent, back)
        t_unpack.append(time.perf_counter() - t0)
    assert np.array_equal(back, dense.array)
    del back
    n_entries = need

    # ---- encode: dense 16-bit against sparse, alternating
    sp_desc = np.zeros(n_tiles, capi.DESC_DTYPE)
    sp_desc["n_records"], sp_desc["rec_offset"], sp_desc["qp"] = 1, np.arange(n_tiles, dtype=np.uint64), 32
    sp_desc["init_id"] = 2 | capi.SUB_FINISH | capi.SUB_ALIGN_RBSP
    sp_first = (np.arange(n_tiles + 1, dtype=np.uint32) * per_tile).astype(np.uint32)
    sp_list = np.zeros(n_tu, capi.SPLICE_DTYPE)
    sp_list["tu"] = np.arange(n_tu, dtype=np.uint32)
    sp_rec = np.full(n_tiles, 0x81FF, np.uint16)
    pay_cap = n_coeff + (1 << 20)                                   # a byte per coefficient: above what the densest of the three codes to
    pay_d, pay_s = pinned((pay_cap,), np.uint8, 0), pinned((pay_cap,), np.uint8, 0)
    keep += [pay_d, pay_s]

    def enc_dense():
        return hip.encode_batch_residual(sp_desc, sp_rec, sp_first, sp_list, all_tus, dense.array, pay_d.array)

    def enc_sparse():
        return hip.sparse_encode_batch(sp_desc, sp_rec, sp_first, sp_list, all_tus, ent_first.array, entries.array[:n_entries], n_coeff,
                                       pay_s.array)

    for _ in range(3):
        off_d, res_d = enc_dense()
        off_s, res_s = enc_sparse()
    total = int(off_d[-1])
    assert np.array_equal(off_d, off_s) and np.array_equal(res_d, res_s) and np.array_equal(pay_d.array[:total], pay_s.array[:total])
    t_ed, t_es = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        enc_dense()
        t_ed.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        enc_sparse()
        t_es.append(time.perf_counter() - t0)
    gpu_ed, gpu_es = ring(hip, enc_dense), ring(hip, enc_sparse)

    # ---- parse: the coded tiles back to blocks, dense 16-bit against sparse, alternating
    nb = np.diff(off_d.astype(np.int64))
    slot = (nb + 15) // 16 * 16 + 16
    ddesc = sp_desc.copy()
    ddesc["byte_capacity"] = nb
    ddesc["byte_offset"] = np.concatenate([[0], np.cumsum(slot)[:-1]])
    h_in = pinned((int(slot.sum()),), np.uint8, 0)
    keep.append(h_in)
    for s in range(n_tiles):
        h_in.array[int(ddesc["byte_offset"][s]):int(ddesc["byte_offset"][s]) + int(nb[s])] = pay_d.array[int(off_d[s]):int(off_d[s + 1])]
    h_first = sp_first
    co_back = pinned((n_coeff,), np.int16, 0)
    ent_back, first_back = pinned((max(n_entries, 1),), np.uint32, 0), pinned((n_tu + 1,), np.uint32, 0)
    keep += [co_back, ent_back, first_back]

    def par_dense():
        return hip.residual_parse_batch(ddesc, h_in.array, h_first, all_tus, n_coeff, int16=True, coeff=co_back.array)

    def par_sparse():
        return hip.sparse_parse_batch(ddesc, h_in.array, h_first, all_tus, n_coeff, entries=ent_back.array, ent_first=first_back.array)

    for _ in range(3):
        par_dense()
        got = par_sparse()
    assert np.array_equal(co_back.array, dense.array)               # the coded blocks come back (hidden signs arranged by the workload)
    assert np.array_equal(got[0], ent_first.array) and np.array_equal(got[1], entries.array[:n_entries])
    t_pd, t_ps = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        par_dense()
        t_pd.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        par_sparse()
        t_ps.append(time.perf_counter() - t0)
    gpu_pd, gpu_ps = ring(hip, par_dense), ring(hip, par_sparse)

    # ---- device forms on resident buffers, alternating with a device-to-device copy of the dense buffer
    dev = capi.CabacHip(0, stream=torch.cuda.current_stream().cuda_stream)
    t_tu = torch.from_numpy(all_tus.view(np.uint8).reshape(-1).copy()).cuda()
    t_co = torch.from_numpy(dense.array.copy()).cuda()
    t_co2 = torch.empty_like(t_co)
    t_first = torch.zeros(n_tu + 1, dtype=torch.int32, device="cuda")
    t_ent = torch.zeros(max(n_entries, 1), dtype=torch.int32, device="cuda")
    t_st = torch.zeros(16, dtype=torch.uint8, device="cuda")
    hiprt = ctypes.CDLL("libamdhip64.so")
    hiprt.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream

    def timed(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    def copy():
        assert hiprt.hipMemcpyAsync(t_co2.data_ptr(), t_co.data_ptr(), 2 * n_coeff, 3, stream) == 0    # hipMemcpyDeviceToDevice

    def compact():
        dev.sparse_compact_device(n_tu, t_tu.data_ptr(), t_co.data_ptr(), 2, n_coeff, t_first.data_ptr(), t_ent.data_ptr(), n_entries,
                                  t_st.data_ptr())

    def expand():
        dev.sparse_expand_device(n_tu, t_tu.data_ptr(), t_first.data_ptr(), t_ent.data_ptr(), n_entries, t_co2.data_ptr(), 2, n_coeff,
                                 t_st.data_ptr())

    for _ in range(3):
        copy(), compact(), expand()
    torch.cuda.synchronize()
    assert torch.equal(t_co, t_co2)                                 # expand of compact: these tiles have nothing outside the coded regions
    t_copy, t_compact, t_expand = [], [], []
    for _ in range(reps):
        t_copy.append(timed(copy))
        t_compact.append(timed(compact))
        t_expand.append(timed(expand))
    dev.close()
    for k in keep:
        k.close()

    def kinds(d, names):
        return {label: round(d.get(k, 0.0), 4) for k, label in names.items()}

    out = {
        "density_parameter": density, "nonzero_share": round(share, 4), "tiles": n_tiles, "blocks": n_tu, "coefficients": n_coeff,
        "entries": n_entries, "entries_per_block": round(n_entries / n_tu, 2), "payload_bytes": total,
        "encode_wall": {"dense16": med(t_ed), "sparse": med(t_es)},
        "parse_wall": {"dense16": med(t_pd), "sparse": med(t_ps)},
        "bytes": {"encode_up_dense16": 2 * n_coeff, "encode_up_sparse": 4 * n_entries + 4 * (n_tu + 1),
                  "parse_down_dense16": 2 * n_coeff, "parse_down_sparse": 4 * n_entries + 4 * (n_tu + 1) + 16,
                  "either_form_also_moves": {"block_descriptors_up": 16 * n_tu, "tu_info_down": 4 * n_tu, "payload": total}},
        "gpu_ms_one_call": {
            "encode_dense16": kinds(gpu_ed, {5: "binariser"}), "encode_sparse": kinds(gpu_es, {5: "binariser", 41: "expand_kind_41"}),
            "parse_dense16": kinds(gpu_pd, {9: "parser"}), "parse_sparse": kinds(gpu_ps, {9: "parser", 42: "compact_kind_42"})},
        "device_forms": {"d2d_copy": med(t_copy), "expand": med(t_expand), "compact": med(t_compact),
                         "copy_gbs_read_plus_write": round(4 * n_coeff / statistics.median(t_copy) / 1e9, 1)},
        "host_single_thread": {"pack_host": med(t_pack), "unpack_host": med(t_unpack)},
    }
    print(name, json.dumps(out), flush=True)
    return out


def verdicts(r):
    """the three acceptance checks, on the default density"""
    def faster(wall):
        gain = wall["dense16"]["median_ms"] - wall["sparse"]["median_ms"]
        return {"passed": bool(gain > wall["dense16"]["spread_ms"]), "gain_ms": round(gain, 4), "dense_spread_ms": wall["dense16"]["spread_ms"]}
    d = r["device_forms"]
    copy, expand, compact = d["d2d_copy"]["median_ms"], d["expand"]["median_ms"], d["compact"]["median_ms"]
    return {"sparse_encode_faster_than_dense_by_more_than_its_spread": faster(r["encode_wall"]),
            "sparse_parse_faster_than_dense_by_more_than_its_spread": faster(r["parse_wall"]),
            "expand_no_longer_than_the_d2d_copy": {"passed": bool(expand <= copy), "expand_ms": expand, "copy_ms": copy,
                                                   "ratio": round(expand / copy, 3)},
            "compact_no_longer_than_twice_the_d2d_copy": {"passed": bool(compact <= 2 * copy), "compact_ms": compact, "copy_ms": copy,
                                                          "ratio": round(compact / copy, 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_transport.json"))
    ap.add_argument("--calibrate", action="store_true")
    ap.add_argument("--only", default=None, help="one of: " + ", ".join(n for n, _ in DENSITIES))
    a = ap.parse_args()
    if a.calibrate:
        return calibrate()
    import torch
    hip = capi.CabacHip(0)
    result = {"tool": "tools/bench_sparse_transport.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "densities": {}}
    for name, density in DENSITIES:
        if a.only in (None, name):
            result["densities"][name] = run_density(hip, name, density, a.tiles, a.reps)
    if "default" in result["densities"]:
        result["accept_at_the_default_density"] = verdicts(result["densities"]["default"])
    hip.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result.get("accept_at_the_default_density", {}), indent=1))


if __name__ == "__main__":
    main()
