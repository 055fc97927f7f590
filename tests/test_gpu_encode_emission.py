"""The encoder's output stage on the device (csrc/cabac_kernels_v4.hip: quad_flush_lead, quad_list_units, quad_emit_units,
quad_flush_list, quad_enc_finish; shared by encode variants 4, 6 and 7): carries into 0xFFFF runs, runs resolved without a
carry, steps of seven units, slots of every capacity, and nothing written outside a slot.

The inputs are constructed by tests/emit_model.py, and tests/test_emit_model.py shows on the CPU which events of the output
stage each batch reaches (the census).  Here the device codes the batch into a buffer full of a sentinel, and the whole buffer
is compared with the image the composer predicts from the oracle's roomy coding: per slot the first min(capacity, N) bytes,
the sentinel everywhere outside the slots; bytes of a slot behind min(capacity, N) are open.  n_bits and flags are compared
exactly, and the result words behind the batch stay as they were.

Geometries: variant 7 under 1 024 substreams (encode_kernel_v7<1>) and with 1 025 (encode_kernel_v7<4>, one live substream
in the last workgroup), variant 6 small (encode_kernel_v6<1, 2>) and with 4 097 (encode_kernel_v6<4, 1>), variant 4 as the
control."""
import os

import numpy as np
import pytest

import emit_model as M
import helpers as H

RES_FILL = 0x5A5A5A5A
GEOMETRIES = [(7, M.SMALL), (7, 1025), (6, M.SMALL), (6, 4097), (4, M.SMALL)]


@pytest.fixture(scope="module", params=GEOMETRIES, ids=["v7x1", "v7x4", "v6x1", "v6x4", "v4"])
def enc(request):
    c = H.gpu_ctx()   # raises without a GPU: there is no fallback
    c.set_variant(request.param[0], 0)
    yield c, request.param[1]
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _run(hip, slots, sets=False):
    """The batch through the device-pointer call -> (the whole byte buffer, results, the result words behind the batch)."""
    n = len(slots.desc)
    d_desc, d_rec = _dev(slots.desc), _dev(np.concatenate([slots.records, np.zeros(8, np.uint16)]))
    d_bytes = _dev(slots.fresh())
    d_res = _dev(np.full(2 * n + 16, RES_FILL, np.uint32))
    if sets:
        import ctx_sets_model as CS
        from test_gpu_residual_estimate import make_sets
        state, rate = CS.pack(make_sets(np.random.default_rng(4420), 1)[0])
        d_state, d_rate = _dev(state.astype(np.uint32)), _dev(rate.astype(np.uint8))
        d_start = _dev(np.full(n, CS.NO_SET, np.uint32))
        hip.encode_sets_device(n, d_desc.data_ptr(), d_rec.data_ptr(), d_bytes.data_ptr(), d_res.data_ptr(), 1,
                               d_state.data_ptr(), d_rate.data_ptr(), d_start.data_ptr())
    else:
        hip.encode_device(n, d_desc.data_ptr(), d_rec.data_ptr(), d_bytes.data_ptr(), d_res.data_ptr())
    hip.synchronize()
    res = d_res.cpu().numpy().view(np.uint32)
    return d_bytes.cpu().numpy(), res[:2 * n].view(H.RESULT_DTYPE), res[2 * n:]


def _check(hip, slots, sets=False):
    got_b, got_r, behind = _run(hip, slots, sets)
    assert (behind == RES_FILL).all()
    slots.check(got_b, got_r)


@pytest.mark.gpu
def test_carries_and_runs(enc):
    """All families (the grid of lane, post and unit phase; long runs; drives started mid-stream; ends 0 .. 15 bins behind the
    crossing; TRM 1 x n; crossings with random tails), three in four beside a plain substream in their output wave, in slots of
    N + 1 and N + 3 bytes."""
    hip, n_sub = enc
    _check(hip, M.carries_batch(n_sub)[0])


@pytest.mark.gpu
def test_every_capacity(enc):
    """A dozen substreams of 20 .. 70 coded bytes, each once per capacity 0 .. N + 2: flags, n_bits (the full count), the
    prefix [0, min(capacity, N)) and every byte outside the slots."""
    hip, n_sub = enc
    slots = M.capacity_batch(n_sub)[0]
    assert (slots.results["flags"] == H.RES_OVERFLOW).sum() > 300
    _check(hip, slots)


@pytest.mark.gpu
def test_probe_with_outstanding_runs(enc):
    """CABAC_SUB_PROBE where the records end with 0xFFFF units outstanding (the siblings, TRM 1 x n), beside finished
    substreams: n_bits is the oracle's count; the finished ones are compared byte for byte, and nothing leaves a slot."""
    hip, n_sub = enc
    _check(hip, M.probe_batch(n_sub)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("variant, n_sub", [(7, 1025), (6, M.SMALL)], ids=["v7x4", "v6x1"])
def test_carries_from_context_sets(variant, n_sub):
    """The same batch through cabac_hip_encode_sets_device with every start NO_SET (Ctx::init): the kernels' CtxSets
    instantiations are code objects of their own."""
    hip = H.gpu_ctx()
    try:
        hip.set_variant(variant, 0)
        _check(hip, M.carries_batch(n_sub)[0], sets=True)
    finally:
        hip.close()


@pytest.mark.gpu
def test_host_path_chunks():
    """1 040 substreams through cabac_hip_encode_batch in three chunks: the chunks of a big batch run the big geometry
    (encode_kernel_v7<4>) on a short grid.  Per substream the bytes and the results are the oracle's."""
    from entropy_coding_amd import capi
    slots = M.carries_batch(1040)[0]
    before = os.environ.get("CABAC_HIP_CHUNKS")
    os.environ["CABAC_HIP_CHUNKS"] = "3"   # read when the ctx sets up its streams
    try:
        hip = capi.CabacHip(0)
        try:
            hip.set_variant(7, 0)
            out, res = hip.encode_batch(slots.desc, slots.records, slots.total, out=slots.fresh())
        finally:
            hip.close()
    finally:
        if before is None:
            del os.environ["CABAC_HIP_CHUNKS"]
        else:
            os.environ["CABAC_HIP_CHUNKS"] = before
    assert np.array_equal(res["n_bits"], slots.results["n_bits"]) and np.array_equal(res["flags"], slots.results["flags"])
    for s in range(len(slots.desc)):
        o, n = int(slots.desc[s]["byte_offset"]), int(slots.n_bytes[s])
        assert n > 0 and np.array_equal(out[o:o + n], slots.image[o:o + n]), s
