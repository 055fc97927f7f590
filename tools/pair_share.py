#!/usr/bin/env python3
"""Which 16-bin steps of a synthetic batch can the quad decoder decode with its pairs variant (decode_kernel_v4, L = 16)?

Host only: the records of the whole batch, grouped four substreams to a wave in descriptor order as the kernel groups
them.  A wave's step qualifies iff none of its four rows has a terminate or an align record, a context more than twice,
or — for a pick every `cadence` bins — a context twice inside an aligned group of `cadence` bins.

  python3 tools/pair_share.py [--workload C4] [--json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from entropy_coding_amd import workload  # noqa: E402

NUM_CTX, REC_ALIGN, REC_TRM = 379, 0x1FD, 0x1FF


def row_steps(ids):
    """ids: (rows, steps, 16) record ids.  Per row and step: has a repeat, has a context more than twice, has a special
    record, and per cadence 2 / 4 whether two occurrences share an aligned group."""
    ctx = ids < NUM_CTX
    others = np.zeros(ids.shape, np.int8)
    near = {2: np.zeros(ids.shape[:2], bool), 4: np.zeros(ids.shape[:2], bool)}
    for a in range(16):
        for b in range(a + 1, 16):
            eq = (ids[..., a] == ids[..., b]) & ctx[..., a]
            others[..., a] += eq
            others[..., b] += eq
            for c in near:
                if a // c == b // c:
                    near[c] |= eq
    special = ((ids == REC_TRM) | (ids == REC_ALIGN)).any(-1)
    return (others > 0).any(-1), (others > 1).any(-1), special, near


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    cfg = workload.CONFIGS[a.workload]
    desc, records, _ = workload.build_batch(cfg)
    n_sub = len(desc)
    tot = {"wave_steps": 0, "row_steps": 0, "row_repeat": 0, "no_repeat": 0, "special": 0, "twice_1": 0, "twice_2": 0, "twice_4": 0}
    for w0 in range(0, n_sub, 256):          # 64 waves at a time
        d = desc[w0:w0 + 256]
        n_max = int(d["n_records"].max())
        steps = (n_max + 15) // 16
        ids = np.full((len(d) + (-len(d)) % 4, steps * 16), 0x1F0, np.uint16)   # past a row's end: the id of "nothing"
        for k, row in enumerate(d):
            o, n = int(row["rec_offset"]), int(row["n_records"])
            ids[k, :n] = records[o:o + n] & 0x1FF
        lens = np.zeros(len(ids), np.int64)
        lens[:len(d)] = d["n_records"]
        ids = ids.reshape(len(ids), steps, 16)
        rep, many, special, near = row_steps(ids)
        live_row = (np.arange(steps)[None, :] * 16) < lens[:, None]
        wave = lambda x: x.reshape(-1, 4, steps).any(1)   # noqa: E731
        live = wave(live_row)
        tot["wave_steps"] += int(live.sum())
        tot["row_steps"] += int(live_row.sum())
        tot["row_repeat"] += int((rep & live_row).sum())
        tot["no_repeat"] += int((~wave(rep | special) & live).sum())
        tot["special"] += int((wave(special) & live).sum())
        tot["twice_1"] += int((~wave(many | special) & live).sum())
        tot["twice_2"] += int((~wave(many | special | near[2]) & live).sum())
        tot["twice_4"] += int((~wave(many | special | near[4]) & live).sum())
    n = tot["wave_steps"]
    out = {"workload": a.workload, "substreams": n_sub, "wave_steps": n,
           "share_rows_with_a_repeat": tot["row_repeat"] / tot["row_steps"],
           "share_special": tot["special"] / n,
           "share_no_repeat": tot["no_repeat"] / n,
           "share_pairs_pick_every_bin": tot["twice_1"] / n,
           "share_pairs_pick_every_2nd": tot["twice_2"] / n,
           "share_pairs_pick_every_4th": tot["twice_4"] / n}
    if a.json:
        print(json.dumps(out))
    else:
        for k, v in out.items():
            print("%-30s %s" % (k, ("%.4f" % v) if isinstance(v, float) else v))


if __name__ == "__main__":
    main()
