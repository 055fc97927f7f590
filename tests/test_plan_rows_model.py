"""CPU: tests/plan_rows_model.py pinned to what it is composed from — one level without links is parse_plan_model's own
expectation, rows written by the model decode from the model's start contexts to their own bins, and the hand-over set at or
behind the end of the plan is the set the decoder leaves."""
import numpy as np

import ctx_sets_model as CS
import helpers as H
import parse_plan_model as PM
import plan_rows_model as R
from test_parse_plan_model import TU_OUTCOMES


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_one_level_without_links_is_the_plan_models_own_expectation():
    rng = np.random.default_rng(0x9051)
    rows = [R.tu_row(rng, [TU_OUTCOMES[int(rng.integers(0, len(TU_OUTCOMES)))] for _ in range(n)]) for n in (1, 3, 2)]
    out, ok = R.rows(rows, [0, 3], [R.NO_SET] * 3, [0, 5, 10 ** 6])
    assert all(ok)
    for row, w in zip(rows, out):
        u = PM.build(rng, row["plan"], row["real"], row["metas"], row["blocks"], row["at"], row["guards"], qp=row["qp"])
        assert np.array_equal(w["data"], u["data"]) and w["values"] == [v & 0xFFFFFFFF for v in u["values"]] and w["infos"] == u["infos"]
        assert R.read_row(row, w)[:2] == PM.want_walk(u)                       # what the parser reports: bits read, flags


def test_rows_decode_from_their_start_contexts_and_hand_over_what_the_decoder_leaves():
    rows, level_first, sync_from, sync_at = R.batch(0x9052)
    out, ok = R.rows(rows, level_first, sync_from, sync_at)
    assert all(ok) and all(w is not None for w in out)
    linked = 0
    for s, (row, w) in enumerate(zip(rows, out)):
        n_bits, flags, left = R.read_row(row, w)                  # asserts the bins are the string's own
        assert flags == 0 and 0 < n_bits <= w["n_bits"]            # bits read; the writer's count includes the RBSP alignment
        assert _same(left, w["left"])
        f = int(sync_from[s])
        if f != R.NO_SET:
            linked += 1
            assert _same(w["start"], out[f]["handed"])
            assert not _same(w["start"], CS.init_set(row["qp"], 2)) or int(sync_at[f]) == 0
        # k >= n: the contexts the decoder leaves
        for k in (len(row["plan"]), len(row["plan"]) + 5):
            at = R.handover_index(row, w["values"], k)
            assert at == len(w["string"]) and _same(CS.advance_from(w["string"][:at], w["start"]), left)
    assert linked == 8


def test_the_hand_over_index_counts_entries_and_the_blocks_in_front_of_them():
    rng = np.random.default_rng(0x9053)
    row = R.tu_row(rng, [(1, 1, 1, 0, 0, 0), (1, 0, 1, 0, 0, 0), (0, 1, 1, 1, 0, 0)])
    values, infos, coded, string = R.filled(row)
    assert len(row["plan"]) == 3 * PM.TU_LEN + 1 and all(coded[:3])
    idx = [R.handover_index(row, values, k) for k in range(len(row["plan"]) + 2)]
    assert idx[0] == 0 and idx[-1] == idx[-2] == len(string) and all(a <= b for a, b in zip(idx, idx[1:]))
    # the three blocks lie in front of entry TU_BLOCK_AT: arriving there, their records are behind the walk
    n_block = sum(len(PM.M.block_records(m, b, None)) for m, b in zip(row["metas"][:3], row["blocks"][:3]))
    assert idx[PM.TU_BLOCK_AT] - idx[PM.TU_BLOCK_AT - 1] >= n_block > 0
    # computed entries contribute no record
    assert idx[PM.TU_BLOCK_AT + 4] == idx[PM.TU_BLOCK_AT]
    # a zero-bin marker contributes none either and shifts what follows by one entry
    rng = np.random.default_rng(0x9053)
    marked = R.tu_row(rng, [(1, 1, 1, 0, 0, 0), (1, 0, 1, 0, 0, 0), (0, 1, 1, 1, 0, 0)], marker=True)
    v2, _, _, s2 = R.filled(marked)
    assert np.array_equal(s2, string) and len(marked["plan"]) == len(row["plan"]) + 2
    assert R.handover_index(marked, v2, PM.TU_LEN) == R.handover_index(marked, v2, PM.TU_LEN + 1) == idx[PM.TU_LEN]
