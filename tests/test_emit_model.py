"""tests/emit_model.py against the CPU oracle, and the census of the batches that tests/test_gpu_encode_emission.py sends to the
device.  The census is a condition on the INPUTS: every event of the output stage that the GPU tests are there for is reached
by a substream of every batch, by construction — nothing here is measured, and no substream is left out of a comparison."""
import ctypes

import numpy as np
import pytest

import emit_model as M
import helpers as H


def _oracle_tight(slots):
    """The oracle run on the composed descriptors, into a buffer full of the sentinel."""
    orc = H.load_oracle()
    out = slots.fresh()
    res = np.zeros(len(slots.desc), H.RESULT_DTYPE)
    orc.lib.orc_encode_batch(slots.desc.ctypes.data, 0, len(slots.desc), slots.records.ctypes.data_as(H.u16p),
                             out.ctypes.data_as(H.u8p), res.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return out, res


# ------------------------------------------------------------------ the coder and the replay
def test_simplest_instance():
    """From the start state with P = 256: 1,0,0,0,0,0,0,0 repeated keeps P - low cycling through 2, 4, .., 256."""
    orc = H.load_oracle()
    recs = ([M.EP1] + [M.EP0] * 7) * 5
    cross = recs + [M.EP1, M.EP1]                      # the first brings P - low back to 2, the second crosses
    assert bytes(orc.encode_records(np.array(cross, np.uint16), 30, 0, 3)[0]) == bytes.fromhex("800000000030")
    assert bytes(orc.encode_records(np.array(recs, np.uint16), 30, 0, 3)[0]) == bytes.fromhex("7fffffffffc0")
    assert bytes(M.finished_bytes(M.code(cross))[0]) == bytes.fromhex("800000000030")
    c, d = M.Coder(), []
    for r in recs:
        d.append(256 * (1 << c.S) - c.low)
        c.put(r)
    assert d[:9] == [256, 2, 4, 8, 16, 32, 64, 128, 256]


def test_model_equals_oracle():
    """Every generated substream: the complete bytes of the (9 + S)-bit value but the last two (finish() owns them) are the
    oracle's; so is the whole stream as finish() and the byte alignment leave it; the replay in 16-bit units stores the same
    bytes; 8 pos + 16 nbuf + pend of the replay is the oracle's CABAC_SUB_PROBE count, and the number of shifts."""
    orc = H.load_oracle()
    fams = M.all_families() + [(n, r, len(r)) for n, r in M.capacity_cases() if M.is_free(r)]
    assert len(fams) > 600
    for name, r, n_head in fams:
        want, n_bits = orc.encode_records(r, 27, 2, 3)
        if n_head != len(r):
            assert not M.is_free(r[n_head:]) and M.is_free(r[:n_head]), name      # a tail with context bins: the oracle alone
            continue
        c = M.code(r)
        sb = M.stream_bytes(c)
        assert len(sb) >= 2 or len(r) < 8, name
        assert np.array_equal(sb[:-2], want[:max(len(sb) - 2, 0)]), name
        fb, fn = M.finished_bytes(c)
        assert fn == n_bits and np.array_equal(fb, want), name
        rp = M.Replay(r)
        assert bytes(rp.out) == bytes(want) and rp.n_bits == n_bits and rp.pos == len(want), name
        probe = orc.encode_records(r, 27, 2, 4)[1]
        assert probe == rp.probe_bits == c.S == rp.shifts, name


def test_long_runs_are_as_long_as_asked():
    for name, r in M.family_long():
        K = int(name.split("K")[1])
        rp = M.Replay(r)
        if "sibling" in name:
            assert rp.max_run == 0 and (K < 2 or "fin_nocarry_run" in rp.ev), name
        else:
            assert rp.max_run >= K - 1 and (K < 2 or {"carry_run", "fin_carry_run"} & rp.ev), name


# ------------------------------------------------------------------ the composer
@pytest.mark.parametrize("which", ["carries", "capacity", "probe"])
def test_composer_predicts_the_oracle(which):
    """The oracle run with the tight descriptors: flags, n_bits (the full count; overflow iff N > cap), the prefix of every
    slot, the sentinel everywhere outside the slots."""
    slots = {"carries": M.carries_batch, "capacity": M.capacity_batch, "probe": M.probe_batch}[which]()[0]
    d = slots.desc
    assert (d["byte_offset"] % 16 == 0).all() and int(d["byte_offset"][0]) >= M.GUARD
    assert (d["byte_offset"][1:].astype(np.int64) >= d["byte_offset"][:-1].astype(np.int64) + d["byte_capacity"][:-1]).all()
    assert slots.total >= int(d["byte_offset"][-1]) + int(d["byte_capacity"][-1]) + M.GUARD
    assert (d["byte_capacity"] % 16 != 0).any() and (d["byte_capacity"] % 2 == 1).any()
    out, res = _oracle_tight(slots)
    slots.check(out, res)
    over = (slots.results["flags"] & H.RES_OVERFLOW) != 0
    assert np.array_equal(over, slots.n_bytes > slots.caps) or which == "probe"
    if which == "capacity":
        assert over.any() and (~over).any()
    # and the check can fail: one byte outside a slot, one inside a prefix
    bad = out.copy()
    bad[int(d["byte_offset"][3]) + int(d["byte_capacity"][3])] ^= 1
    with pytest.raises(AssertionError):
        slots.check(bad, res)
    k = int(np.flatnonzero(np.minimum(slots.n_bytes, slots.caps) > 0)[0])
    bad = out.copy()
    bad[int(d["byte_offset"][k])] ^= 0x80
    with pytest.raises(AssertionError):
        slots.check(bad, res)


# ------------------------------------------------------------------ the census
BATCH_SIZES = {"carries": (M.SMALL, 1025, 1040, 4097), "capacity": (M.SMALL, 1025, 4097), "probe": (M.SMALL, 1025, 4097)}


@pytest.mark.parametrize("n_sub", BATCH_SIZES["carries"])
def test_census_carries(n_sub):
    """Every emission event in every batch of test_carries_and_runs (and test_host_path_chunks); the carry into a run and the
    step of seven units at each of the eight positions s mod 8 — the substreams of one v7 output wave — and next to plain
    substreams; whole blocks of sixteen plain substreams exist."""
    slots, recs, names = M.carries_batch(n_sub)
    cen = M.census(recs, slots.caps)
    print(M.format_census("carries[%s]" % (n_sub or len(recs)), cen, M.EMISSION_EVENTS))
    for ev in M.EMISSION_EVENTS:
        assert cen.get(ev), ev
    for ev in ("carry_run", "step7", "carry_nbuf1", "ff_start"):
        assert {s % 8 for s in cen[ev]} == set(range(8)), ev
    for ev in ("carry_run", "ff_start"):
        assert {s % 16 for s in cen[ev]} == set(range(16)), ev
    assert len(names) == len(M.all_families()) and len(recs) == (n_sub or len(recs))
    for s in names:                                           # a case shares its four with a plain substream
        assert any(t not in names for t in range(s & ~3, (s & ~3) + 4) if t < len(recs)), s
    assert any(all(16 * b + t not in names for t in range(16)) for b in range(len(recs) // 16))
    if n_sub in (1025, 4097):                                 # one live substream in the last workgroup
        assert len(recs) % 16 == 1 and M.is_free(recs[-1]) and "carry_run" in M.Replay(recs[-1]).ev
    assert not (slots.results["flags"]).any() and (slots.caps % 2 == 1).sum() > len(recs) // 4


@pytest.mark.parametrize("n_sub", BATCH_SIZES["capacity"])
def test_census_capacity(n_sub):
    """test_every_capacity: every capacity 0 .. N + 2 of every case, hence every byte phase: room 0, -1 and -2 in a step, the
    overflow from the first unit, the single byte of quad_put16 at pos == cap - 1, cuts inside a run and inside finish()."""
    slots, recs, names = M.capacity_batch(n_sub)
    cen = M.census(recs, slots.caps)
    print(M.format_census("capacity[%s]" % (n_sub or len(recs)), cen, M.CAPACITY_EVENTS + M.EMISSION_EVENTS))
    for ev in M.CAPACITY_EVENTS + ("carry_run", "ff_extend", "step7", "fin_nocarry_run"):
        assert cen.get(ev), ev
    by_case = {}
    for s, name in names.items():
        by_case.setdefault(name.split("/cap")[0], []).append(int(slots.caps[s]))
    assert len(by_case) >= 12
    for case, caps in by_case.items():
        N = int(slots.n_bytes[[s for s, n in names.items() if n.startswith(case + "/")][0]])
        assert sorted(caps) == list(range(N + 3)), case
    cut_in_run = cut_in_finish = 0
    for s, name in names.items():
        if M.is_free(recs[s]):
            rp = M.Replay(recs[s], finish=False)
            cap = int(slots.caps[s])
            cut_in_finish += rp.pos <= cap < int(slots.n_bytes[s])
            full = bytes(M.Replay(recs[s]).out)
            cut_in_run += 2 <= cap < len(full) - 2 and full[cap - 2:cap + 2] in (b"\xff" * 4, b"\x00" * 4)
    assert cut_in_run and cut_in_finish


@pytest.mark.parametrize("n_sub", BATCH_SIZES["probe"])
def test_census_probe(n_sub):
    """test_probe_with_outstanding_runs: every probed substream ends with 0xFFFF units outstanding (nbuf >= 2)."""
    slots, recs, flags = M.probe_batch(n_sub)
    probed = np.flatnonzero(flags & M.PROBE)
    assert len(probed) >= 30 and (flags & H.SUB_FINISH).sum() > len(probed)
    runs = [M.Replay(recs[s], finish=False).nbuf - 1 for s in probed]
    print("probe[%s]: %d probed, outstanding runs %d .. %d units" % (n_sub or len(recs), len(probed), min(runs), max(runs)))
    assert min(runs) >= 1 and max(runs) >= 30          # from one unit to more than three steps can produce
    assert {int(s) % 8 for s in probed} == set(range(8))
