"""GPU: WPP substreams (include/cabac_hip_ctx_sets.h, part 2) — 3 pictures x 4 rows in level order, ragged rows, row r of a
picture starting from the contexts its row r - 1 has after sync_at records (0, 21 — inside a 16-bin step —, exactly n_records,
beyond n_records), one picture whose row 2 links to nothing.  Expectation: tests/ctx_sets_model.py, level by level on the CPU;
tests/test_ctx_sets_model.py asserts for these seeds that the links change the bytes of at least one row of every picture and
that the batch decodes back to its bins, so nothing here can pass with the links ignored.  Device and host-pointer forms, under
the forced geometries encode 4 / 6 / 7 and decode 4 / 8 / 1 and under the dispatch."""
import numpy as np
import pytest
import torch

import ctx_sets_model as M
import helpers as H
from entropy_coding_amd import capi
from test_ctx_sets_model import WPP_SEEDS
from test_gpu_ctx_sets import SENT8, SENT32, dev, host, ptr, same_coded_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[(0, 0), (4, 4), (6, 8), (7, 1)], ids=["dispatch", "enc4-dec4", "enc6-dec8", "enc7-dec1"])
def hip(request):
    c = H.gpu_ctx()
    c.set_variant(*request.param)
    yield c
    c.close()


def device_encode(hip, desc, records, total, level_first, sync_from, sync_at):
    d = [dev(a) for a in (desc, np.concatenate([records, np.zeros(8, np.uint16)]), sync_from, sync_at)]
    d_bytes = torch.full((total + 16,), SENT8, dtype=torch.uint8, device="cuda")
    d_res = dev(np.full(2 * len(desc), SENT32, np.uint32))
    hip.encode_wpp_device(len(desc), ptr(d[0]), ptr(d[1]), ptr(d_bytes), ptr(d_res), level_first, ptr(d[2]), ptr(d[3]))
    hip.synchronize()
    return host(d_bytes, np.uint8), host(d_res, H.RESULT_DTYPE)


def device_decode(hip, desc, records, data, level_first, sync_from, sync_at):
    d = [dev(a) for a in (desc, np.concatenate([records, np.zeros(8, np.uint16)]), sync_from, sync_at,
                          np.concatenate([data, np.zeros(16, np.uint8)]))]
    d_bins = torch.full((len(records) + 16,), SENT8, dtype=torch.uint8, device="cuda")
    d_res = dev(np.full(2 * len(desc), SENT32, np.uint32))
    hip.decode_wpp_device(len(desc), ptr(d[0]), ptr(d[1]), ptr(d[4]), ptr(d_bins), ptr(d_res), level_first, ptr(d[2]), ptr(d[3]))
    hip.synchronize()
    return host(d_bins, np.uint8), host(d_res, H.RESULT_DTYPE)


@pytest.mark.parametrize("seed", WPP_SEEDS)
def test_wpp_encode_and_decode_device_and_batch_forms(hip, seed):
    desc, records, total, level_first, sync_from, sync_at = case = M.wpp_batch(seed)
    ref_b, ref_r = M.encode_wpp(*case)
    got_b, got_r = device_encode(hip, *case)
    assert np.array_equal(got_r, ref_r), (got_r, ref_r)
    same_coded_bytes(desc, got_b, ref_b, ref_r)
    # decoding those bytes gives the records' bins
    bins_w, dres_w = M.decode_wpp(desc, records, ref_b, level_first, sync_from, sync_at)
    bins, dres = device_decode(hip, desc, records, ref_b, level_first, sync_from, sync_at)
    assert np.array_equal(dres, dres_w) and not dres["flags"].any()
    assert np.array_equal(bins[:len(records)], records >> 15) and np.array_equal(bins_w, records >> 15)
    # the host-pointer forms agree with the device forms
    hb, hr = hip.encode_wpp_batch(desc, records, total, level_first, sync_from, sync_at)
    assert np.array_equal(hr, got_r)
    same_coded_bytes(desc, hb, got_b, got_r)
    hbins, hdres = hip.decode_wpp_batch(desc, records, hb, level_first, sync_from, sync_at)
    assert np.array_equal(hbins, bins[:len(records)]) and np.array_equal(hdres, dres)


def test_wpp_one_level_is_the_plain_call(hip):
    desc, records, total, _, sync_from, sync_at = M.wpp_batch(WPP_SEEDS[0])
    none = np.full(len(desc), M.NO_SET, np.uint32)
    got_b, got_r = device_encode(hip, desc, records, total, np.array([0, len(desc)], np.uint32), none, sync_at)
    ref_b, ref_r, _ = M.encode_sets(desc, records, total, [], None)
    assert np.array_equal(got_r, ref_r)
    same_coded_bytes(desc, got_b, ref_b, ref_r)


def test_wpp_batch_forms_refuse_malformed_input(hip):
    desc, records, total, level_first, sync_from, sync_at = M.wpp_batch(WPP_SEEDS[0])
    n_pic = int(level_first[1])
    data = np.zeros(total, np.uint8)

    def refused(lf, sf, names):
        for call in (lambda: hip.encode_wpp_batch(desc, records, total, lf, sf, sync_at),
                     lambda: hip.decode_wpp_batch(desc, records, data, lf, sf, sync_at)):
            with pytest.raises(capi.CabacHipError) as e:
                call()
            assert e.value.status == -2 and names in str(e.value), str(e.value)

    bad = level_first.copy()
    bad[2] = bad[1] - 1                                           # not non-decreasing
    refused(bad, sync_from, "level_first")
    bad = level_first.copy()
    bad[-1] -= 1                                                  # does not end at n_sub
    refused(bad, sync_from, "level_first")
    sf = sync_from.copy()
    sf[n_pic + 1] = n_pic + 2                                     # into the same level
    refused(level_first, sf, "substream %d " % (n_pic + 1))
    sf = sync_from.copy()
    sf[n_pic + 1] = 3 * n_pic                                     # into a later level
    refused(level_first, sf, "substream %d " % (n_pic + 1))
    sf = sync_from.copy()
    sf[2 * n_pic] = len(desc)                                     # beyond the batch
    refused(level_first, sf, "substream %d " % (2 * n_pic))
    # and the ctx still works
    hb, hr = hip.encode_wpp_batch(desc, records, total, level_first, sync_from, sync_at)
    assert np.array_equal(hr, M.encode_wpp(desc, records, total, level_first, sync_from, sync_at)[1])


def test_wpp_device_form_flags_a_same_level_link_and_keeps_the_other_pictures(hip):
    desc, records, total, level_first, sync_from, sync_at = M.wpp_batch(WPP_SEEDS[0])
    n_pic = int(level_first[1])
    good_b, good_r = M.encode_wpp(desc, records, total, level_first, sync_from, sync_at)
    sf = sync_from.copy()
    sf[n_pic] = n_pic + 1                                         # picture 0, row 1 -> a substream of its own level
    got_b, got_r = device_encode(hip, desc, records, total, level_first, sf, sync_at)
    assert tuple(got_r[n_pic]) == (0, M.RES_BAD_SET)
    o, c = int(desc[n_pic]["byte_offset"]), int(desc[n_pic]["byte_capacity"])
    assert (got_b[o:o + c] == SENT8).all()
    others = [s for s in range(len(desc)) if s % n_pic != 0]
    assert np.array_equal(got_r[others], good_r[others])
    same_coded_bytes(desc, got_b, good_b, good_r, others)
    bins, dres = device_decode(hip, desc, records, good_b, level_first, sf, sync_at)
    assert tuple(dres[n_pic]) == (0, M.RES_BAD_SET)
    for s in others:
        a, n = int(desc[s]["rec_offset"]), int(desc[s]["n_records"])
        assert np.array_equal(bins[a:a + n], records[a:a + n] >> 15) and dres[s]["flags"] == 0
