"""CPU: tests/splice_rows_model.py — the hand-over pair of include/cabac_hip_splice_rows.h — against the parts it is composed of
and against the literal definition in the header: one level with no link is the plain model, both ends of the clip when a block
sits at the hand-over position, the ends of a substream, blocks without records, and the rows' bytes decoded back into the bins
by ctx_sets_model.decode_wpp with the expanded records and the expanded index."""
import numpy as np

import ctx_sets_model as CS
import helpers as H
import search_emit_model as E
import splice_rows_model as M
import search_unit_model as U

BIN = 0x8000
SEED = 0x5B11CE


def literal_index(side_len, ats, recs, k, m):
    """The header's definition, element by element: for i = 0 .. n first every block spliced at at == i, then host record i; the
    hand-over index counts the records of the string that belong to the k host records and the m splices in front."""
    n_front = 0
    for i in range(side_len + 1):
        for j, at in enumerate(ats):
            if at == i and j < m and recs[j] is not None:
                n_front += len(recs[j])
        if i < side_len and i < k:
            n_front += 1
    return n_front


def hand_made():
    """12 host records; blocks of 3, 5 (at 4, twice at one position), 0 (rejected, at 4), 2 (at 9) and 4 (at 12) records"""
    side = np.arange(12, dtype=np.uint16) + 1
    recs = [np.full(3, 100, np.uint16), np.full(5, 101, np.uint16), None, np.full(2, 102, np.uint16), np.full(4, 103, np.uint16)]
    return M.Sub(side, [4, 4, 4, 9, 12], recs)


def test_clip_pair_and_index_follow_the_definition():
    sub = hand_made()
    assert sub.string.tolist()[:6] == [1, 2, 3, 4, 100, 100] and len(sub.string) == 12 + 14
    n = len(sub.side)
    # both ends of the clip where blocks sit at at == k
    assert M.clip_pair(sub.ats, n, 4, 0) == (4, 0) and M.clip_pair(sub.ats, n, 4, 10 ** 6) == (4, 3) and M.clip_pair(sub.ats, n, 4) == (4, 3)
    assert [sub.index(4, m) for m in (0, 1, 2, 3, 4, None)] == [4, 7, 12, 12, 12, 12]       # the rejected block adds nothing
    assert sub.string[sub.index(4, 0)] == 100 and sub.string[sub.index(4)] == 5
    # no block at k: the pair has one value whatever m says
    assert [sub.index(6, m) for m in (0, 3, 99, None)] == [14, 14, 14, 14]
    assert M.clip_pair(sub.ats, n, 3, 2) == (3, 0) and M.clip_pair(sub.ats, n, 5, 0) == (5, 3)
    # k == 0 and k >= n
    assert sub.index(0, 0) == 0 and sub.index(0) == 0
    assert sub.index(12, 4) == 22 and sub.index(12) == 26 and sub.index(10 ** 6) == 26 and sub.index(0xFFFFFFFF, 0xFFFFFFFF) == 26
    assert sub.index(10 ** 6, 0) == 22                                                      # clipped to n = 12, then the lower end
    head = M.Sub(sub.side, [0, 0, 4], [np.full(2, 7, np.uint16), None, np.full(1, 8, np.uint16)])
    assert [head.index(0, m) for m in (0, 1, 2, None)] == [0, 2, 2, 2]
    for s in (sub, head):
        for k in list(range(14)) + [10 ** 6]:
            for m in list(range(7)) + [None]:
                kk, mm = M.clip_pair(s.ats, len(s.side), k, m)
                assert s.index(k, m) == literal_index(len(s.side), s.ats, s.recs, kk, mm), (k, m)
                # and the index is where that block begins, or where that host record stands, in U.expand's own string
                if mm < len(s.ats) and s.ats[mm] == kk:
                    assert s.index(k, m) == s.spans[mm][0]


def test_one_level_without_links_is_the_plain_model():
    B = M.rows_batch(SEED)
    subs, n = B["subs"], len(B["subs"])
    rng = np.random.default_rng(1)
    qp, init = rng.integers(20, 45, n), rng.integers(0, 3, n)
    want, want_bits = M.encode_plain(subs, qp, init)
    none = np.full(n, M.NO_SET, np.uint32)
    chunks, res, _, _ = M.encode_rows(subs, qp, init, [0, n], none, B["sync_at"], B["splice"]["lower"])
    assert not res["flags"].any() and np.array_equal(res["n_bits"], want_bits)
    assert all(np.array_equal(a, b) for a, b in zip(chunks, want))
    chunks, res, written = M.encode_sets(subs, qp, init, [], None, None)
    assert np.array_equal(res["n_bits"], want_bits) and all(np.array_equal(a, b) for a, b in zip(chunks, want)) and not written


def test_rows_batch_holds_what_the_gpu_test_is_about():
    B = M.rows_batch(SEED)
    subs, case, n_pic = B["subs"], B["case"], int(B["level_first"][1])
    n = len(subs)
    rng = np.random.default_rng(2)
    qp, init = rng.integers(20, 45, n), rng.integers(0, 3, n)
    assert sorted(set(int(x) for x in B["sync_at"] if x not in (0, 10 ** 6))) and (B["sync_at"] == 0).any() and (B["sync_at"] == 10 ** 6).any()
    # more than 64 splices in front of a point; a rejected and an empty block in front of one
    assert int(B["splice"]["lower"][2]) > 64
    assert subs[1].recs[0] is None and subs[1].infos[0] == H.TU_INFO_BAD_DESC and subs[1].recs[1] is None and subs[1].infos[1] & H.TU_INFO_EMPTY
    assert subs[1].ats[1] < B["sync_at"][1]
    without = M.Sub(subs[1].side, subs[1].ats[2:], subs[1].recs[2:])
    assert without.index(int(B["sync_at"][1]), int(B["splice"]["lower"][1]) - 2) == subs[1].index(int(B["sync_at"][1]), int(B["splice"]["lower"][1]))
    assert np.array_equal(without.string, subs[1].string)
    # the CTU that begins with two blocks: lower, middle, upper give three different rows below; NULL is the upper end
    p, c = B["probe"], B["child"]
    k = int(B["sync_at"][p])
    assert subs[p].ats.count(k) >= 2 and int(B["sync_from"][c]) == p
    out = {name: M.encode_rows(subs, qp, init, B["level_first"], B["sync_from"], B["sync_at"], sp) for name, sp in B["splice"].items()}
    out["null"] = M.encode_rows(subs, qp, init, B["level_first"], B["sync_from"], B["sync_at"], None)
    idx = [int(out[name][2][p]) for name in ("lower", "middle", "upper")]
    assert idx[0] < idx[1] < idx[2] and int(out["null"][2][p]) == idx[2]
    rows = [out[name][0][c].tobytes() for name in ("lower", "middle", "upper")]
    assert len(set(rows)) == 3 and out["null"][0][c].tobytes() == rows[2]
    # the links matter: every linked row differs from the same row coded alone; the unlinked one in the middle does not
    alone, _ = M.encode_plain(subs, qp, init)
    u = 2 * n_pic + 1
    assert int(B["sync_from"][u]) == M.NO_SET and np.array_equal(out["lower"][0][u], alone[u])
    linked = [s for s in range(n) if int(B["sync_from"][s]) != M.NO_SET]
    assert len(linked) == n - n_pic - 1 and all(not np.array_equal(out["lower"][0][s], alone[s]) for s in linked)
    assert case.n_cand == n


def test_rows_bytes_decode_back_into_the_bins():
    B = M.rows_batch(SEED)
    subs, n = B["subs"], len(B["subs"])
    rng = np.random.default_rng(3)
    qp, init = rng.integers(20, 45, n), rng.integers(0, 3, n)
    for sp in (B["splice"]["lower"], None):
        chunks, res, idx, _ = M.encode_rows(subs, qp, init, B["level_first"], B["sync_from"], B["sync_at"], sp)
        desc, total = H.make_desc([len(s.string) for s in subs], qp, init, H.SUB_FINISH, capacities=[len(c) + 16 for c in chunks])
        records = np.concatenate([s.string for s in subs]).astype(np.uint16)
        data = np.zeros(total, np.uint8)
        for s, c in enumerate(chunks):
            data[int(desc[s]["byte_offset"]):int(desc[s]["byte_offset"]) + len(c)] = c
        bins, dres = CS.decode_wpp(desc, records, data, B["level_first"], B["sync_from"], idx)
        assert not dres["flags"].any() and np.array_equal(bins, records >> 15)
        # with the host positions in place of the expanded indices the rows below a block do not come back
        bins2, _ = CS.decode_wpp(desc, records, data, B["level_first"], B["sync_from"], B["sync_at"])
        assert not np.array_equal(bins2, bins)


def test_same_level_link_refuses_that_row_alone():
    B = M.rows_batch(SEED)
    subs, n, n_pic = B["subs"], len(B["subs"]), int(B["level_first"][1])
    qp, init = np.full(n, 30), np.zeros(n, np.int64)
    good = M.encode_rows(subs, qp, init, B["level_first"], B["sync_from"], B["sync_at"], None)
    sf = B["sync_from"].copy()
    bad = 3 * n_pic + 1
    sf[bad] = bad - 1
    chunks, res, _, _ = M.encode_rows(subs, qp, init, B["level_first"], sf, B["sync_at"], None)
    assert tuple(res[bad]) == (0, M.RES_BAD_SET) and len(chunks[bad]) == 0
    for s in range(n):
        if s != bad:
            assert np.array_equal(chunks[s], good[0][s]) and tuple(res[s]) == tuple(good[1][s])


def test_marked_log_is_the_log_model_with_cursors_noted():
    from test_gpu_search_emit import Cands  # noqa: F401  (the tests' candidate arrays; imported lazily there too)
    rng = np.random.default_rng(0x10C)
    K = 4
    log, plain = M.MarkedLog(K), E.LogModel(K)
    chain = np.arange(K, dtype=np.uint32)
    for r in range(3):
        case, gf, _ = E.search_round(rng, K, 3)
        pick = gf[:-1].copy()
        args = (pick, chain, case.cand_first, case.tus, case.coeff, case.rec_first, case.records, case.tu_at)
        assert log.append(*args) and plain.append(*args)
        if r == 0:
            log.mark([0, 2, 0xFFFFFFFF, K + 3])
            first = log.pairs()
        if r == 1:
            log.mark([2])                                            # replaces the earlier mark of chain 2
    at, sp = log.pairs()
    assert at[0] == first[0][0] and sp[0] == first[1][0] and (at[2], sp[2]) == (log.log.chain_rec[2] - log.log.entries[-2][2], sp[2])
    assert at[2] >= first[0][2] and at[1] == M.END and sp[3] == M.END
    subs = log.subs()
    strings = plain.strings()[0]
    assert all(np.array_equal(s.string, w) for s, w in zip(subs, strings))
    # a mark is always consistent: clipping changes nothing
    for k in (0, 2):
        assert M.clip_pair(subs[k].ats, len(subs[k].side), at[k], sp[k]) == (int(at[k]), int(sp[k]))
    # the marked index is the length of the string of the entries in front of the mark
    spans = plain.strings()[2]
    assert subs[0].index(at[0], sp[0]) == [e for c, b, e in spans if c == 0][0]
    assert subs[2].index(at[2], sp[2]) == [e for c, b, e in spans if c == 2][1]
    assert subs[1].index(at[1], sp[1]) == len(strings[1])
    # one level, no link: the model's emit
    qp, init = [30, 31, 32, 33], [0, 1, 2, 0]
    chunks, res, _, _ = log.encode_rows(qp, init, [0, K], np.full(K, M.NO_SET, np.uint32))
    pay, off = M.payload_of(chunks)
    want = plain.emit(qp, init, 3)
    assert np.array_equal(pay, want[0]) and np.array_equal(off, want[1]) and np.array_equal(res["n_bits"], want[2])
    log.reset()
    assert log.pairs()[0].tolist() == [M.END] * K and not log.log.entries
