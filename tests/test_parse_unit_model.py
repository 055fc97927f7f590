"""CPU: tests/parse_unit_model.py — the consistency check the GPU tests of the unit parse rest on — against the encoder's input
on valid streams, against the oracle's block parser on damaged block-only streams, and the expanded strings' bytes against the
compiled reference's encoder where it is built."""
import numpy as np
import pytest

import helpers as H
import parse_unit_model as M

STYLES = ["regular", "ts_flag_0", "ts_flag_1", "ts", "bdpcm", "sbt"]
DAMAGED_SEED = 7


def _infos(unit):
    return [H.TU_INFO_TS if m[3] & H.TU_TRANSFORM_SKIP else 0 for m in unit["metas"]]


def _n_bits(unit):
    orc = H.load_oracle()
    string, _, _ = M.expand(unit["side"], list(zip(unit["metas"], unit["blocks"])), unit["at"])
    rc, bins, nread = orc.decode_records(string, unit["qp"], 2, unit["data"], flags=1 if unit["finish"] else 0)
    assert rc == 0 and np.array_equal(bins, string >> 15)
    return nread


@pytest.mark.parametrize("style", STYLES)
def test_consistent_accepts_the_input_of_a_valid_stream_and_nothing_next_to_it(style):
    rng = np.random.default_rng(0x51 + STYLES.index(style))
    for n in range(6):
        unit = M.make_unit(rng, [style] * 3, int(rng.integers(0, 20)), at=[None, "random"][n & 1], ts_side=(n in (3, 5)))
        B = (unit["side"] >> 15).astype(np.uint8)
        n_bits = _n_bits(unit)
        args = (unit["data"], unit["qp"], unit["side"], unit["metas"], unit["at"])
        assert M.consistent(*args, unit["blocks"], B, n_bits, finish=unit["finish"], infos=_infos(unit)) == (True, 0)
        assert M.consistent(*args, unit["blocks"], B, n_bits + 1, finish=unit["finish"], infos=_infos(unit))[0] is False
        # one coefficient changed (kept non-zero, inside the coded region) ...
        k = int(rng.integers(0, 3))
        c = unit["blocks"][k].copy()
        ys, xs = np.nonzero(c)
        j = int(rng.integers(0, len(ys)))
        c[ys[j], xs[j]] += 1 if c[ys[j], xs[j]] > 0 else -1
        wrong = [c if i == k else b for i, b in enumerate(unit["blocks"])]
        assert M.consistent(*args, wrong, B, n_bits, finish=unit["finish"], infos=_infos(unit))[0] is False
        # ... or one side bin
        j = int(rng.integers(0, len(B)))
        B2 = B.copy()
        B2[j] ^= 1
        assert M.consistent(*args, unit["blocks"], B2, n_bits, finish=unit["finish"], infos=_infos(unit))[0] is False


def test_consistent_accepts_the_oracle_s_parse_of_damaged_block_only_streams():
    """The block-only analogue of the damaged corpus of tests/test_gpu_parse_unit.py (same seed): what orc.residual_decode makes
    of the bytes is consistent, n_bits included, and the substreams that cannot be judged stay within 1 in 20."""
    orc = H.load_oracle()
    units = M.damaged_units(DAMAGED_SEED, 200, block_only=True)
    skipped = refused = 0
    for u in units:
        rc, want, nbits = orc.residual_decode(u["data"], u["qp"], u["metas"], finish=False)
        if rc != 0:
            refused += 1
            continue
        try:
            ok, rc2 = M.consistent(u["data"], u["qp"], np.zeros(0, np.uint16), u["metas"], None, want, np.zeros(0, np.uint8), nbits)
        except M.Skip:
            skipped += 1
            continue
        assert ok and rc2 == 0
    print("damaged block-only corpus: %d skipped, %d refused by the oracle's parser" % (skipped, refused))
    assert skipped <= len(units) // 20 and refused <= 2


def test_expansion_follows_the_clipping_rule():
    rng = np.random.default_rng(3)
    unit = M.make_unit(rng, ["regular"] * 3, 10, at=[7, 2, 0xFFFFFFFF], trm=False)
    string, spans, is_side = M.expand(unit["side"], list(zip(unit["metas"], unit["blocks"])), unit["at"])
    n = [len(M.block_records(m, c)) for m, c in zip(unit["metas"], unit["blocks"])]
    assert spans == [(7, 7 + n[0]), (7 + n[0], 7 + n[0] + n[1]), (10 + n[0] + n[1], 10 + sum(n))]   # 7, held at 7, clipped to 10
    assert np.array_equal(string[is_side], unit["side"])


@pytest.mark.skipif(not H.ref_available(), reason="compiled reference not built")
def test_expanded_strings_code_to_the_reference_encoder_s_bytes():
    ref = H.load_ref()
    rng = np.random.default_rng(0x77)
    for n in range(6):
        unit = M.make_unit(rng, [STYLES[n % 6], "regular"], 12)
        string, _, _ = M.expand(unit["side"], list(zip(unit["metas"], unit["blocks"])), unit["at"])
        assert np.array_equal(ref.encode_records(string, unit["qp"], 2, 3)[0], unit["data"])
