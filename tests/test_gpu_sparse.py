"""GPU: the sparse coefficient transport (include/cabac_hip_sparse.h) — cabac_hip_sparse_expand_device / _compact_device against
tests/sparse_model.py (status word, firsts, entries, every element of the dense array and the sentinels around it), the scan and
grid edges, the capacity, S1 and S2 on the device, the waits counter, and the two host-pointer forms against their dense
counterparts (S3: cabac_hip_encode_batch_residual16, S4: cabac_hip_residual_parse_batch16)."""
import numpy as np
import pytest

import helpers as H
import parse_corpus as PC
import sparse_model as M
import test_gpu_residual_parse as P
from entropy_coding_amd import capi

pytestmark = pytest.mark.gpu

SENT = {np.int16: 0x5A5A, np.int32: 0x5A5A5A5A}
FRONT = 3            # sentinel elements in front of the dense array: its base is then not 16-byte aligned either
GUARD = 8


@pytest.fixture(scope="module")
def hip():
    h = H.gpu_ctx()
    yield h
    h.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _filled(n_bytes, byte):
    import torch
    return torch.full((max(n_bytes, 16),), byte, dtype=torch.uint8, device="cuda")


def _status(t):
    return M.status_dict(t.cpu().numpy()[:16].view(capi.SPARSE_STATUS_DTYPE)[0])


def dev_compact(hip, tus, coeff, capacity=None):
    """compact_device on `coeff` (sentinels in front and behind) against the model; returns (firsts, entries, status)."""
    dtype = coeff.dtype.type
    w_first, w_ent, w_st = M.pack(tus, coeff, capacity)
    cap = w_st["n_entries"] if capacity is None else capacity
    padded = np.concatenate([np.full(FRONT, SENT[dtype], dtype), coeff, np.full(GUARD, SENT[dtype], dtype)])
    t_tu, t_co = _dev(tus), _dev(padded)
    t_first, t_ent, t_st = _filled(4 * (len(tus) + 1 + GUARD), 0xA5), _filled(4 * (cap + GUARD), 0xA5), _filled(16, 0x77)
    hip.sparse_compact_device(len(tus), t_tu.data_ptr(), t_co.data_ptr() + FRONT * coeff.itemsize, coeff.itemsize, len(coeff),
                              t_first.data_ptr(), t_ent.data_ptr(), cap, t_st.data_ptr())
    hip.synchronize()
    st = _status(t_st)
    assert st == w_st, (st, w_st)
    first, ent = t_first.cpu().numpy().view(np.uint32), t_ent.cpu().numpy().view(np.uint32)
    assert np.array_equal(first[:len(tus) + 1], w_first) and np.all(first[len(tus) + 1:len(tus) + 1 + GUARD] == 0xA5A5A5A5)
    k = min(cap, w_st["n_entries"])
    assert np.array_equal(ent[:k], w_ent[:k]), np.nonzero(ent[:k] != w_ent[:k])[0][:8]
    assert np.all(ent[cap:cap + GUARD] == 0xA5A5A5A5)               # nothing past the capacity
    assert np.array_equal(t_co.cpu().numpy().view(dtype), padded)   # the input is input
    return w_first, w_ent[:k], w_st


def dev_expand(hip, tus, first, entries, n_total, dtype, n_entries=None):
    """expand_device into an array of sentinels (in front, in the gaps, behind) against the model on the same array."""
    n_entries = len(entries) if n_entries is None else n_entries
    want = np.full(FRONT + n_total + GUARD, SENT[dtype], dtype)
    w_st = M.unpack(tus, first, entries, want[FRONT:FRONT + n_total], n_entries)
    t_tu, t_first, t_ent = _dev(tus), _dev(np.asarray(first, np.uint32)), _dev(np.asarray(entries, np.uint32))
    t_co = _dev(np.full(FRONT + n_total + GUARD, SENT[dtype], dtype))
    t_st = _filled(16, 0x77)
    hip.sparse_expand_device(len(tus), t_tu.data_ptr(), t_first.data_ptr(), t_ent.data_ptr() if len(entries) else 0, n_entries,
                             t_co.data_ptr() + FRONT * np.dtype(dtype).itemsize, np.dtype(dtype).itemsize, n_total, t_st.data_ptr())
    hip.synchronize()
    st = _status(t_st)
    assert st == w_st, (st, w_st)
    got = t_co.cpu().numpy().view(dtype)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    return got[FRONT:FRONT + n_total], w_st


def both_ways(hip, tus, coeff):
    """compact, then expand what it gave: S2 on the device"""
    first, ent, st = dev_compact(hip, tus, coeff)
    back, _ = dev_expand(hip, tus, first, ent, len(coeff), coeff.dtype.type)
    for tu in tus:
        if int(tu["log2_width"]) > 6 or int(tu["log2_height"]) > 6:
            continue
        w, h, off = 1 << int(tu["log2_width"]), 1 << int(tu["log2_height"]), int(tu["coeff_offset"])
        if off + w * h > len(coeff):
            continue
        a = coeff[off:off + w * h].reshape(h, w).copy()
        a[32:, :] = 0
        a[:, 32:] = 0
        if coeff.dtype == np.int32:
            a = a.astype(np.int16).astype(np.int32)                 # stored truncated
        assert np.array_equal(a, back[off:off + w * h].reshape(h, w))
    return first, ent, st


# ------------------------------------------------------------------------------------------------ expand and compact
@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_every_shape_empty_sparse_and_full(hip, dtype):
    rng = np.random.default_rng(141)
    for density in (0.0, 0.1, 1.0):
        tus, n_total = M.layout(M.ALL_SHAPES)
        first, ent, st = both_ways(hip, tus, M.fill(rng, tus, n_total, dtype, density=density))
        assert st["flags"] == 0 and (density or st["n_entries"] == 0)


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_single_entries_at_the_first_and_the_last_coded_position(hip, dtype):
    tus, n_total = M.layout(M.ALL_SHAPES)
    for last in (False, True):
        coeff = np.zeros(n_total, dtype)
        for tu in tus:
            w, h, off = 1 << int(tu["log2_width"]), 1 << int(tu["log2_height"]), int(tu["coeff_offset"])
            coeff[off + ((min(h, 32) - 1) * w + min(w, 32) - 1 if last else 0)] = -3
        first, ent, st = both_ways(hip, tus, coeff)
        assert st["n_entries"] == len(tus) and np.all(ent >> 16 == 0xFFFD)


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_junk_outside_the_coded_region_odd_offsets_and_gaps(hip, dtype):
    rng = np.random.default_rng(142)
    shapes = [(6, 6), (0, 1), (6, 2), (1, 1), (2, 6), (0, 0), (6, 0), (1, 0), (0, 6), (0, 1), (6, 5), (1, 1), (5, 6)] + M.mixed_shapes(rng, 60)
    tus, n_total = M.layout(shapes, rng, gaps=True, odd=True)
    assert any(int(t["coeff_offset"]) & 1 and 1 <= int(t["log2_width"]) + int(t["log2_height"]) <= 2 for t in tus)
    both_ways(hip, tus, M.fill(rng, tus, n_total, dtype, density=0.35, junk=True))


def test_int16_boundaries_and_a_wide_level_that_raises_range(hip):
    tus, n_total = M.layout([(2, 2), (2, 2), (2, 2)])
    c32 = np.zeros(n_total, np.int32)
    c32[[0, 5, 16, 47]] = [-32768, 32767, -1, 1]
    assert both_ways(hip, tus, c32)[2]["flags"] == 0
    assert both_ways(hip, tus, c32.astype(np.int16))[2]["flags"] == 0
    c32[20] = 40000
    first, ent, st = dev_compact(hip, tus, c32)
    assert st["flags"] == M.RANGE and st["first_bad"] == 1 and int(ent[int(first[1]) + 1]) == 4 | ((40000 & 0xFFFF) << 16)
    c32[40] = -32769
    assert dev_compact(hip, tus, c32)[2] == dict(n_entries=6, flags=M.RANGE, first_bad=1)


def test_each_bad_flag_alone_with_first_bad(hip):
    rng = np.random.default_rng(145)
    tus, n_total = M.layout([(2, 2)] * 40)                          # more than one workgroup of sixteen blocks
    coeff = M.fill(rng, tus, n_total, np.int16, density=0.6, sentinel=False)
    for t in range(20, 25):                                         # one entry each, at positions of their own: a list that runs
        coeff[16 * t:16 * t + 16] = 0                               # into its neighbours' then holds no position twice
        coeff[16 * t + t - 18] = t
    first, ent, _ = M.pack(tus, coeff)
    e = ent.copy()
    for t in (33, 19):                                              # BAD_POS in two blocks: the lowest is reported
        assert int(first[t + 1]) > int(first[t])
        e[int(first[t])] = (e[int(first[t])] & 0xFFFF0000) | 16
    assert dev_expand(hip, tus, first, e, n_total, np.int16)[1] == dict(n_entries=len(ent), flags=M.BAD_POS, first_bad=19)
    f = first.copy()
    f[22] = f[23] + 1                                               # descends
    assert dev_expand(hip, tus, f, ent, n_total, np.int16)[1]["first_bad"] == 22
    st = dev_expand(hip, tus, first, ent, n_total, np.int16, n_entries=int(first[38]) - 1)[1]   # passes n_entries
    assert st == dict(n_entries=int(first[38]) - 1, flags=M.BAD_FIRST, first_bad=37)
    for field, value in (("log2_width", 7), ("coeff_offset", n_total - 15), ("coeff_offset", 2 ** 64 - 4)):
        bad = tus.copy()
        bad[17][field] = value
        assert dev_expand(hip, bad, first, ent, n_total, np.int16)[1] == dict(n_entries=len(ent), flags=M.BAD_BLOCK, first_bad=17)
        assert dev_compact(hip, bad, coeff)[2]["flags"] == M.BAD_BLOCK


def test_no_block_and_refusals(hip):
    assert dev_compact(hip, np.zeros(0, capi.TU_DTYPE), np.zeros(0, np.int16))[2] == dict(n_entries=0, flags=0, first_bad=M.NO_BAD)
    assert dev_expand(hip, np.zeros(0, capi.TU_DTYPE), [0], [], 0, np.int16)[1] == dict(n_entries=0, flags=0, first_bad=M.NO_BAD)
    t = _filled(64, 0)
    with pytest.raises(capi.CabacHipError):                         # firsts are 32-bit
        hip.sparse_compact_device(1, t.data_ptr(), t.data_ptr(), 2, 1 << 32, t.data_ptr(), t.data_ptr(), 4, t.data_ptr())
    with pytest.raises(capi.CabacHipError):
        hip.sparse_expand_device(1, t.data_ptr(), t.data_ptr(), t.data_ptr(), 4, t.data_ptr(), 3, 16, t.data_ptr())


# ------------------------------------------------------------------------------------------------ scan and grid edges
@pytest.mark.parametrize("n_tu", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_scan_and_grid_edges(hip, n_tu):
    rng = np.random.default_rng(150 + n_tu)
    tus, n_total = M.layout(M.mixed_shapes(rng, n_tu, max_log2=6 if n_tu == 4097 else 4), rng, gaps=True)
    coeff = M.fill(rng, tus, n_total, np.int16, density=0.08, junk=False)
    first, ent, st = dev_compact(hip, tus, coeff)
    dev_expand(hip, tus, first, ent, n_total, np.int16)


def test_overflow_writes_nothing_past_the_capacity(hip):
    rng = np.random.default_rng(151)
    tus, n_total = M.layout(M.mixed_shapes(rng, 100), rng, gaps=True)
    coeff = M.fill(rng, tus, n_total, np.int16, density=0.5)
    need = M.pack(tus, coeff)[2]["n_entries"]
    for cap in (need - 1, 0):
        first, ent, st = dev_compact(hip, tus, coeff, capacity=cap)  # (the guard words behind the capacity are checked there)
        assert st["flags"] == M.OVERFLOW and st["n_entries"] == need and int(first[-1]) == need


def test_s1_and_s2_on_random_blocks_of_the_corpus(hip):
    rng = np.random.default_rng(152)
    for dtype in (np.int16, np.int32):
        blocks = [PC.random_tu(rng, PC.MIXED_STYLES[int(rng.integers(0, len(PC.MIXED_STYLES)))]) for _ in range(200)]
        tus, n_total = M.layout([(int(np.log2(m[0])), int(np.log2(m[1]))) for m, _ in blocks], rng, gaps=True, odd=True)
        coeff = np.full(n_total, SENT[dtype], dtype)
        for tu, (m, c) in zip(tus, blocks):
            coeff[int(tu["coeff_offset"]):int(tu["coeff_offset"]) + c.size] = np.clip(c, -32768, 32767).ravel()
        first, ent, st = both_ways(hip, tus, coeff)                 # S2
        shuffled = ent.copy()
        for t in range(len(tus)):
            lo, hi = int(first[t]), int(first[t + 1])
            shuffled[lo:hi] = rng.permutation(shuffled[lo:hi])
        again, _ = dev_expand(hip, tus, first, shuffled, n_total, dtype)
        f2, e2, _ = dev_compact(hip, tus, again.copy())             # S1
        assert np.array_equal(f2, first) and np.array_equal(e2, ent)


def test_a_second_call_of_the_same_size_does_not_wait(hip):
    rng = np.random.default_rng(153)
    tus, n_total = M.layout(M.mixed_shapes(rng, 3000), rng)
    coeff = M.fill(rng, tus, n_total, np.int16, density=0.1, sentinel=False)
    first, ent, _ = M.pack(tus, coeff)
    t_tu, t_co, t_first, t_ent, t_st = _dev(tus), _dev(coeff), _dev(first), _dev(ent), _filled(16, 0)
    def run():
        hip.sparse_compact_device(len(tus), t_tu.data_ptr(), t_co.data_ptr(), 2, n_total, t_first.data_ptr(), t_ent.data_ptr(), len(ent), t_st.data_ptr())
        hip.sparse_expand_device(len(tus), t_tu.data_ptr(), t_first.data_ptr(), t_ent.data_ptr(), len(ent), t_co.data_ptr(), 2, n_total, t_st.data_ptr())
    run()
    before = hip.workspace_waits()
    run()
    assert hip.workspace_waits() == before
    hip.synchronize()
    assert np.array_equal(t_co.cpu().numpy().view(np.int16), coeff) and np.array_equal(t_ent.cpu().numpy().view(np.uint32), ent)


# ------------------------------------------------------------------------------------------------ S3 and S4
STYLES = ["regular", "ts", "bdpcm", "sbt", "ts_flag_0", "ts_flag_1", "hiding", "chroma"]


def _styled(rng, style):
    """one block -> (w, h, channel, flags), int16-range coefficients"""
    if style == "hiding":                                           # sign hiding + dependent quantisation
        w, h, c = P.random_regular(rng)
        m = (w, h, 0, H.TU_SIGN_HIDING | H.TU_DEP_QUANT)
    elif style == "chroma":
        w, h, c = P.random_regular(rng)
        m = (w, h, 1, int(rng.integers(0, 2)))
    else:
        m, c = PC.random_tu(rng, style)
    return m, np.clip(c, -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def spliced():
    """10 substreams, 208 blocks of every style, host records around the splices; block 77 is empty"""
    rng = np.random.default_rng(160)
    host, splices, first, metas, blocks = [], [], [0], [], []
    for s in range(10):
        n_host = [0, 40, 200][s % 3] if s else 60
        rec = H.random_records(rng, n_host, ctx_frac=0.6, end_trm=False) if n_host else np.zeros(0, np.uint16)
        rec = np.concatenate([rec, PC.TRM_END])
        n_blocks = 28 if s == 3 else 20
        for at in np.sort(rng.integers(0, len(rec), size=n_blocks)):
            m, c = _styled(rng, STYLES[len(metas) % len(STYLES)])
            if len(metas) == 77:
                c = np.zeros_like(c)
            if m[3] & H.TU_TS_FLAG:                                 # the flag is the caller's record in the splice form
                m = (m[0], m[1], m[2], m[3] & ~H.TU_TS_FLAG)
            splices.append((int(at), len(metas)))
            metas.append(m)
            blocks.append(c)
        host.append(rec)
        first.append(len(splices))
    offsets, n_total = P.scattered_layout(rng, metas)
    tus = np.zeros(len(metas), H.TU_DTYPE)
    coeff = np.zeros(n_total, np.int16)
    for t, (m, c) in enumerate(zip(metas, blocks)):
        tus[t]["coeff_offset"], tus[t]["log2_width"], tus[t]["log2_height"] = int(offsets[t]), int(np.log2(m[0])), int(np.log2(m[1]))
        tus[t]["channel"], tus[t]["flags"] = m[2], m[3]
        coeff[int(offsets[t]):int(offsets[t]) + c.size] = c.ravel()
    desc, _ = H.make_desc([len(r) for r in host], rng.integers(0, 64, size=10), rng.integers(0, 3, size=10), H.SUB_FINISH | H.SUB_ALIGN_RBSP)
    desc["byte_offset"] = 0
    desc["byte_capacity"] = 0
    ent_first, entries, st = M.pack(tus, coeff)
    assert len(metas) >= 200 and st["flags"] == 0
    return dict(desc=desc, records=np.concatenate(host), first=np.array(first, np.uint32), splices=np.array(splices, capi.SPLICE_DTYPE),
                tus=tus, coeff=coeff, ent_first=ent_first, entries=entries, metas=metas, blocks=blocks)


def test_s3_sparse_encode_equals_the_dense_form_on_the_expanded_blocks(spliced):
    c = spliced
    hip = capi.CabacHip(0)
    expanded = np.zeros(len(c["coeff"]), np.int16)                  # the model's expand of the lists
    M.unpack(c["tus"], c["ent_first"], c["entries"], expanded)
    assert np.array_equal(expanded, c["coeff"])
    pay_d, pay_s = np.full(1 << 18, 0xEE, np.uint8), np.full(1 << 18, 0xEE, np.uint8)
    off_d, res_d, info_d, cnt_d = hip.encode_batch_residual(c["desc"], c["records"], c["first"], c["splices"], c["tus"], expanded, pay_d,
                                                            check=False, with_info=True, with_counts=True)
    for rep in range(2):                                            # the same ctx again: staging is reused
        pay_s[:] = 0xEE
        off_s, res_s, info_s, cnt_s = hip.sparse_encode_batch(c["desc"], c["records"], c["first"], c["splices"], c["tus"], c["ent_first"],
                                                              c["entries"], len(c["coeff"]), pay_s, check=False, with_info=True,
                                                              with_counts=True)
        assert np.array_equal(off_s, off_d) and np.array_equal(res_s, res_d) and np.array_equal(info_s, info_d)
        assert np.array_equal(cnt_s, cnt_d) and np.array_equal(pay_s, pay_d) and int(off_d[-1]) > 1000
    assert int(info_d[77]) & H.TU_INFO_EMPTY and np.count_nonzero(info_d & H.TU_INFO_EMPTY) == 1
    # the return code: an empty block makes both forms answer CABAC_HIP_ERR_SUBSTREAM
    with pytest.raises(capi.CabacHipError) as e_d:
        hip.encode_batch_residual(c["desc"], c["records"], c["first"], c["splices"], c["tus"], expanded, pay_d)
    with pytest.raises(capi.CabacHipError) as e_s:
        hip.sparse_encode_batch(c["desc"], c["records"], c["first"], c["splices"], c["tus"], c["ent_first"], c["entries"], len(c["coeff"]), pay_s)
    assert e_d.value.status == e_s.value.status == -5
    hip.close()


def test_s3_refusals_touch_no_output_and_the_fixed_workspace_refuses_the_call(spliced):
    c = spliced
    hip = capi.CabacHip(0)
    n = len(c["desc"])

    def refused(tus=c["tus"], ent_first=c["ent_first"], entries=c["entries"], word=None):
        pay = np.full(1 << 18, 0xEE, np.uint8)
        off, res = np.full(n + 1, 0x7777, np.uint64), np.zeros(n, capi.RESULT_DTYPE)
        res["n_bits"] = 0x7777
        with pytest.raises(capi.CabacHipError) as e:
            hip.sparse_encode_batch(c["desc"], c["records"], c["first"], c["splices"], tus, ent_first, entries, len(c["coeff"]), pay,
                                    offsets=off, results=res)
        assert e.value.status == -2 and (word is None or word in str(e.value)), str(e.value)
        assert np.all(pay == 0xEE) and np.all(off == 0x7777) and np.all(res["n_bits"] == 0x7777)

    e = c["entries"].copy()
    t = 100
    w, h = c["metas"][t][:2]
    assert int(c["ent_first"][t + 1]) > int(c["ent_first"][t])
    e[int(c["ent_first"][t])] = (e[int(c["ent_first"][t])] & 0xFFFF0000) | (w * h)
    refused(entries=e, word="block 100")                            # pos out of block
    f = c["ent_first"].copy()
    f[50] = f[49] - 1
    refused(ent_first=f, word="block 49: ent_first descends")      # descending firsts
    tu = c["tus"].copy()
    tu[9]["max_log2_tr_range"] = 16
    refused(tus=tu, word="block 9")
    # a fixed workspace: refused like the other host-pointer forms of the splice pipeline; works again after the release
    rec, slots = capi.workspace_bound(n, len(c["records"]), len(c["tus"]), len(c["coeff"]))
    hip.workspace_fix(n, len(c["tus"]), rec, slots)
    refused(word="workspace")
    hip.workspace_release()
    pay = np.zeros(1 << 18, np.uint8)
    off, res = hip.sparse_encode_batch(c["desc"], c["records"], c["first"], c["splices"], c["tus"], c["ent_first"], c["entries"],
                                       len(c["coeff"]), pay, check=False)
    assert int(off[-1]) > 1000
    hip.close()


@pytest.fixture(scope="module")
def parsed(spliced):
    """the blocks of `spliced` (without the empty one) coded as block-only substreams by the oracle: what the parser reads"""
    orc = H.load_oracle()
    rng = np.random.default_rng(161)
    keep = [t for t in range(len(spliced["metas"])) if t != 77]
    subs, qps = [], rng.integers(0, 64, size=10)
    for s in range(10):
        mine = keep[s::10]
        metas = [spliced["metas"][t] for t in mine]
        blocks = [spliced["blocks"][t].astype(np.int32) for t in mine]
        subs.append((metas, blocks, PC.encode(orc, metas, blocks, qps[s])))
    return subs, qps


def _sparse_vs_dense(hip, desc, buf, tile_first, tus, total):
    coeff, res_d, info_d = hip.residual_parse_batch(desc, buf, tile_first, tus, total, check=False, with_info=True, int16=True)
    first, ent, res_s, info_s, st = hip.sparse_parse_batch(desc, buf, tile_first, tus, total, check=False)
    assert np.array_equal(res_s, res_d) and np.array_equal(info_s, info_d)
    w_first, w_ent, w_st = M.pack(tus, coeff)                       # the compact of the dense form's coefficients
    assert M.status_dict(st) == w_st and np.array_equal(first, w_first) and np.array_equal(ent, w_ent)
    back = np.zeros(total, np.int16)
    M.unpack(tus, first, ent, back)
    assert np.array_equal(back, coeff)                              # the dense form zeroes what the parser does not write
    return coeff, first, ent, res_s, st


def test_s4_sparse_parse_equals_the_dense_form(parsed):
    subs, qps = parsed
    hip = capi.CabacHip(0)
    rng = np.random.default_rng(162)
    metas = [m for s in subs for m in s[0]]
    desc, buf, tile_first, tus, offsets, total = P.pack(subs, qps, layout=P.scattered_layout(rng, metas))
    coeff, first, ent, res, st = _sparse_vs_dense(hip, desc, buf, tile_first, tus, total)
    assert not res["flags"].any() and int(st["n_entries"]) > 1000
    t = 0
    for s in subs:                                                  # and they are the coded blocks
        for m, c in zip(s[0], s[1]):
            if not m[3] & H.TU_SIGN_HIDING:
                assert np.array_equal(coeff[int(offsets[t]):int(offsets[t]) + c.size], c.ravel()), t
            t += 1
    # a truncated stream: the same CABAC_RES_UNDERRUN, no entries behind the stop
    cut = desc.copy()
    cut["byte_capacity"][4] = cut["byte_capacity"][4] // 3
    coeff, first, ent, res, st = _sparse_vs_dense(hip, cut, buf, tile_first, tus, total)
    assert int(res["flags"][4]) & H.RES_UNDERRUN and not res["flags"][np.arange(10) != 4].any()
    # a block the parser refuses: the substream stops there, and the blocks behind the stop have no entries
    stop = tus.copy()
    k = int(tile_first[6]) + 5
    stop[k]["channel"] = 2
    coeff, first, ent, res, st = _sparse_vs_dense(hip, desc, buf, tile_first, stop, total)
    assert int(res["flags"][6]) & H.RES_BAD_RECORD and not res["flags"][np.arange(10) != 6].any()
    assert first[k] == first[int(tile_first[7])] and first[k] > first[int(tile_first[6])] and first[-1] > first[int(tile_first[7])]
    with pytest.raises(capi.CabacHipError) as e:                    # ... and the flagged call answers as the dense form does
        hip.sparse_parse_batch(cut, buf, tile_first, tus, total)
    assert e.value.status == -5
    # a capacity that is too small: the need is reported, firsts / results / info are delivered, no entries; then success with it
    need = int(M.pack(tus, hip.residual_parse_batch(desc, buf, tile_first, tus, total, int16=True)[0])[2]["n_entries"])
    small = np.full(need + 4, 0xA5A5A5A5, np.uint32)
    with pytest.raises(capi.CabacHipError) as e:
        hip.sparse_parse_batch(desc, buf, tile_first, tus, total, entries=small, entry_capacity=need - 1)
    assert e.value.status == -2 and int(e.value.sparse_status["n_entries"]) == need and int(e.value.sparse_status["flags"]) == M.OVERFLOW
    assert np.all(small == 0xA5A5A5A5) and int(e.value.sparse_outputs[0][-1]) == need and not e.value.sparse_outputs[1]["flags"].any()
    first, ent, res, info, st = hip.sparse_parse_batch(desc, buf, tile_first, tus, total, entries=small, entry_capacity=need)
    assert len(ent) == need and np.all(small[need:] == 0xA5A5A5A5) and int(st["flags"]) == 0
    # with a workspace fixed the call works: it is not one of the pipeline's forms
    hip.workspace_fix(10, len(tus), *capi.workspace_bound(10, 100, len(tus), total))
    _sparse_vs_dense(hip, desc, buf, tile_first, tus, total)
    waits = hip.workspace_waits()                                   # a call of a size seen before: the two waits and no other
    hip.sparse_parse_batch(desc, buf, tile_first, tus, total)
    assert hip.workspace_waits() == waits + 2
    hip.workspace_release()
    hip.close()
