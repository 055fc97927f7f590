"""GPU: the unit parse (include/cabac_hip_parse_unit.h; the side-walking instantiation of csrc/cabac_residual_parse.hip) — spliced
substreams read back on the device — against the encoder's input, the two identities of the header (the residual parser, the bin
decoder) and tests/parse_unit_model.py's consistency check, which tests/test_parse_unit_model.py pins to the oracle.  Everything is
bit-exact: == on integers.  Every output sits between guard words that are checked, every test has its own bounded input, and
nothing is run again after a failure."""
import numpy as np
import pytest

import helpers as H
import parse_unit_model as M
import search_unit_model as U
from entropy_coding_amd import capi
from test_gpu_residual_estimate import dev

pytestmark = pytest.mark.gpu

G = 64                                                     # guard elements on either side of every output
BIN_GUARD, WORD_GUARD = 0xEE, -0x11223345
MIXED = ["regular", "regular", "ts_flag_0", "ts_flag_1", "ts", "bdpcm", "sbt"]


@pytest.fixture(scope="module")
def hip():
    c = H.gpu_ctx()
    yield c
    c.close()


def sentinel(int16):
    return 0x5A5A if int16 else 0x5A5A5A5A


def t_or_dummy(a, dt):
    import torch
    a = np.ascontiguousarray(a)
    return dev(a, dt) if a.size else torch.zeros(16, dtype=torch.uint8, device="cuda")


class Out:
    """The four outputs of a call, each between G guard elements."""

    def __init__(self, P, int16):
        import torch
        self.P, self.int16 = P, int16
        self.n_sub, self.n_tu, self.n_rec = len(P["desc"]), P["n_tu"], len(P["records"])
        self.co = torch.full((P["total"] + 2 * G,), sentinel(int16), dtype=torch.int16 if int16 else torch.int32, device="cuda")
        self.bins = torch.full((self.n_rec + 2 * G,), BIN_GUARD, dtype=torch.uint8, device="cuda")
        self.info = torch.full((self.n_tu + 2 * G,), WORD_GUARD, dtype=torch.int32, device="cuda")
        self.res = torch.full((2 * self.n_sub + 2 * G,), WORD_GUARD, dtype=torch.int32, device="cuda")

    def ptrs(self):
        return (self.co.data_ptr() + G * (2 if self.int16 else 4), self.bins.data_ptr() + G, self.info.data_ptr() + 4 * G,
                self.res.data_ptr() + 4 * G)

    def read(self):
        """-> (coefficient buffer as int32, side bins, info, results); the guards are checked here"""
        co, bins, info, res = self.co.cpu().numpy(), self.bins.cpu().numpy(), self.info.cpu().numpy(), self.res.cpu().numpy()
        for a, g in ((co, sentinel(self.int16)), (bins, BIN_GUARD), (info, WORD_GUARD), (res, WORD_GUARD)):
            assert (a[:G] == g).all() and (a[len(a) - G:] == g).all(), "a guard word was written"
        return (co[G:len(co) - G].astype(np.int32), bins[G:len(bins) - G], info[G:len(info) - G].view(np.uint32),
                res[G:len(res) - G].view(H.RESULT_DTYPE))


def run_unit(hip, units, int16=False, capacities=None, null_at=False, mutate=None, blocks_of="unit"):
    """parse_unit_device over `units` (parse_unit_model.pack) -> dict(P, co, bins [per unit], info, res, blocks [per unit])."""
    P = M.pack(units, capacities)
    if mutate:
        mutate(P)
    out = Out(P, int16)
    t_desc, t_buf = dev(P["desc"], np.uint8), dev(P["bytes"])
    t_first, t_tu = dev(P["tile_first"].view(np.int32)), t_or_dummy(P["tus"][:P["n_tu"]], np.uint8)
    t_at = None if (null_at or P["tu_at"] is None) else t_or_dummy(P["tu_at"].view(np.int32), None)
    t_rec = t_or_dummy(P["records"].view(np.int16), None)
    p_co, p_bins, p_info, p_res = out.ptrs()
    hip.parse_unit_device(len(units), t_desc.data_ptr(), t_buf.data_ptr(), t_first.data_ptr(), t_tu.data_ptr() if P["n_tu"] else 0,
                          t_at.data_ptr() if t_at is not None else 0, t_rec.data_ptr() if len(P["records"]) else 0,
                          p_co if P["n_tu"] else 0, p_bins if len(P["records"]) else 0, p_res, d_tu_info=p_info, int16=int16)
    hip.synchronize()
    co, bins, info, res = out.read()
    blocks, per_bins, t = [], [], 0
    for s, u in enumerate(units):
        bl = []
        for m in u["metas"]:
            w, h = m[0], m[1]
            bl.append(co[int(P["offsets"][t]): int(P["offsets"][t]) + w * h].reshape(h, w))
            t += 1
        blocks.append(bl)
        r0 = int(P["desc"]["rec_offset"][s])
        per_bins.append(bins[r0:r0 + len(u["side"])])
    return dict(P=P, co=co, bins=per_bins, all_bins=bins, info=info, res=res, blocks=blocks)


def assert_untouched_outside(r, units, int16, parsed=None):
    """Nothing but the coded top-left min(w, 32) x min(h, 32) of the parsed blocks was written.  parsed[s]: the number of blocks
    of unit s that were parsed (default: all)."""
    mask = np.zeros(len(r["co"]), bool)
    t = 0
    for s, u in enumerate(units):
        for k, m in enumerate(u["metas"]):
            w, h = m[0], m[1]
            if parsed is None or k < parsed[s]:
                blk = np.zeros((h, w), bool)
                blk[:min(h, 32), :min(w, 32)] = True
                mask[int(r["P"]["offsets"][t]): int(r["P"]["offsets"][t]) + w * h] = blk.ravel()
            t += 1
    want = np.int32(np.int16(sentinel(int16))) if int16 else np.int32(sentinel(int16))
    assert (r["co"][~mask] == want).all(), "a coefficient outside the coded regions was written"


def coded(c):
    return np.asarray(c)[:min(c.shape[0], 32), :min(c.shape[1], 32)]


def as_read(meta, c):
    """The block a reader gets back: the block itself, but with sign-data hiding the hidden signs as the parity rule infers them
    (they depend on the block's own levels only) — the oracle's parse of the block coded alone."""
    if not (meta[3] & H.TU_SIGN_HIDING) or (meta[3] & H.TU_TRANSFORM_SKIP):
        return c
    orc = H.load_oracle()
    data = orc.encode_records(np.concatenate([M.block_records(meta, c), M.TRM_END]), 30, 2, 3)[0]
    rc, blocks, _ = orc.residual_decode(data, 30, [meta])
    assert rc == 0
    return blocks[0]


def want_info(unit):
    """tu_info as cabac_hip_residual_parse_device reports the blocks of a valid unit"""
    orc = H.load_oracle()
    out = []
    for m, c in zip(unit["metas"], unit["blocks"]):
        if m[3] & H.TU_TRANSFORM_SKIP:
            out.append(H.TU_INFO_TS)
        else:
            _, last, viol = orc.residual_records(c, m[2], m[3], max_log2_range=m[4] if len(m) > 4 and m[4] else 15)
            out.append(last | (H.TU_INFO_MTS_VIOLATION if viol else 0))
    return out


def want_walk(unit):
    """(n_bits, flags) of a valid unit: orc.decode_records of its expanded string"""
    orc = H.load_oracle()
    string, _, _ = M.expand(unit["side"], list(zip(unit["metas"], unit["blocks"])), unit["at"])
    rc, bins, nread = orc.decode_records(string, unit["qp"], 2, unit["data"], flags=1 if unit["finish"] else 0)
    assert rc in (0, -5) and np.array_equal(bins, string >> 15)
    return nread, {0: 0, -5: H.RES_BAD_STOP}[rc]


def assert_valid(r, units, int16, what=""):
    """Every unit came back as it was coded: coefficients, side bins, tu_info, n_bits and flags."""
    t = 0
    for s, u in enumerate(units):
        n_bits, flags = want_walk(u)
        assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (n_bits, flags), (what, s)
        assert np.array_equal(r["bins"][s], (u["side"] >> 15).astype(np.uint8)), (what, s)
        for k, (c, got) in enumerate(zip(u["blocks"], r["blocks"][s])):
            assert np.array_equal(coded(got), coded(as_read(u["metas"][k], c))), (what, s, k)
        info = want_info(u)
        assert r["info"][t:t + len(info)].tolist() == info, (what, s)
        t += len(info)
    assert_untouched_outside(r, units, int16)


def with_(unit, **kw):
    u = dict(unit)
    u.update(kw)
    return u


# ---------------------------------------------------------------------------------------------- 1. identity I1
def run_block_parser(hip, units, int16):
    """cabac_hip_residual_parse_device on the same arrays -> (coefficient buffer, info, results)"""
    import torch
    P = M.pack(units)
    t_desc, t_buf = dev(P["desc"], np.uint8), dev(P["bytes"])
    t_first, t_tu = dev(P["tile_first"].view(np.int32)), t_or_dummy(P["tus"], np.uint8)
    t_co = torch.full((max(P["total"], 1),), sentinel(int16), dtype=torch.int16 if int16 else torch.int32, device="cuda")
    t_res = torch.full((2 * len(units),), WORD_GUARD, dtype=torch.int32, device="cuda")
    t_info = torch.full((max(P["n_tu"], 1),), WORD_GUARD, dtype=torch.int32, device="cuda")
    hip.residual_parse_device(len(units), t_desc.data_ptr(), t_buf.data_ptr(), t_first.data_ptr(), t_tu.data_ptr(), t_co.data_ptr(),
                              t_res.data_ptr(), d_tu_info=t_info.data_ptr(), int16=int16)
    hip.synchronize()
    return (t_co.cpu().numpy().astype(np.int32)[:P["total"]], t_info.cpu().numpy().view(np.uint32)[:P["n_tu"]],
            t_res.cpu().numpy().view(H.RESULT_DTYPE))


def _i1_units(rng, n_sub, small):
    units = []
    for s in range(n_sub):
        if small:
            styles, shapes = ["regular"], [(4, 4)]
        elif s % 16 == 5:
            styles, shapes = [], None                                     # an empty substream
        elif s % 8 == 3:
            styles, shapes = ["regular"] * 2, [(64, 64), (64, 8)]
        else:
            styles, shapes = [MIXED[int(rng.integers(0, len(MIXED)))] for _ in range(int(rng.integers(1, 5)))], None
        u = M.make_unit(rng, styles, 0, at=[0] * len(styles), shapes=shapes)     # blocks, then the run [TRM]
        if s % 7 == 2:                                                    # damaged: the identities hold for any bytes
            d = u["data"].copy()
            d[int(rng.integers(0, len(d)))] ^= 1 << int(rng.integers(0, 8))
            u["data"] = d
        units.append(u)
    return units


@pytest.mark.parametrize("int16", [False, True])
@pytest.mark.parametrize("n_sub,small", [(64, False), (1030, True)])
def test_i1_without_side_records_it_is_the_residual_parser(hip, int16, n_sub, small):
    """No side records, no CABAC_SUB_FINISH: every output equals cabac_hip_residual_parse_device's.  With CABAC_SUB_FINISH that
    call equals this one with the run [CABAC_REC_TRM] behind the blocks, its BAD_STOP being "side bin 0, or BAD_STOP here".
    64 substreams of mixed styles with 64-wide blocks, empty and damaged ones (one wave per workgroup), and 1 030 of one 4 x 4
    block (four waves per workgroup)."""
    rng = np.random.default_rng(0x11 + n_sub)
    units = _i1_units(rng, n_sub, small)
    caps = np.array([len(u["data"]) for u in units])
    if not small:
        caps[5] = 0                                                       # an empty substream without a byte
    bare = [with_(u, side=np.zeros(0, np.uint16), at=None, finish=False) for u in units]
    for u, c in zip(bare, caps):
        u["data"] = u["data"][:c]
    want_co, want_info_, want_res = run_block_parser(hip, bare, int16)
    r = run_unit(hip, bare, int16)
    assert np.array_equal(r["co"], want_co) and np.array_equal(r["info"], want_info_) and np.array_equal(r["res"], want_res)
    assert (r["res"]["flags"] == 0).sum() > n_sub // 2
    # with the stop check
    closed = [with_(u, data=u["data"][:c]) for u, c in zip(units, caps)]
    want_co, want_info_, want_res = run_block_parser(hip, [with_(u, side=np.zeros(0, np.uint16), at=None) for u in closed], int16)
    r = run_unit(hip, closed, int16)
    assert np.array_equal(r["co"], want_co) and np.array_equal(r["info"], want_info_)
    assert np.array_equal(r["res"]["n_bits"], want_res["n_bits"])
    for s in range(n_sub):
        mine, theirs = int(r["res"]["flags"][s]), int(want_res["flags"][s])
        if mine & (H.RES_UNDERRUN | H.RES_BAD_RECORD) or theirs & (H.RES_UNDERRUN | H.RES_BAD_RECORD):
            assert mine == theirs, s
            continue
        stop = (mine & H.RES_BAD_STOP) or int(r["bins"][s][0]) == 0
        assert (mine & ~H.RES_BAD_STOP) == (theirs & ~H.RES_BAD_STOP) and bool(stop) == bool(theirs & H.RES_BAD_STOP), s
    assert (want_res["flags"] == 0).sum() > n_sub // 2 and (small or (want_res["flags"] != 0).any())


# ---------------------------------------------------------------------------------------------- 2. identity I2
@pytest.mark.parametrize("finish", [False, True])
def test_i2_without_blocks_it_is_the_bin_decoder(hip, finish):
    """Runs of 0, 1, 63, 64, 65, 129 and 1 000 records with bypass, terminate and align records among them, intact and damaged:
    side bins and results equal cabac_hip_decode_device's wherever that call sets no flag."""
    import torch
    orc = H.load_oracle()
    rng = np.random.default_rng(0x12)
    units = []
    for rep in range(2):
        for n in (0, 1, 63, 64, 65, 129, 1000):
            rec = H.random_records(rng, n - 1, ctx_frac=0.6, end_trm=True, trm0_frac=0.02) if n else np.zeros(0, np.uint16)
            if n >= 63:
                rec[int(rng.integers(0, n - 1))] = H.REC_ALIGN
                rec[int(rng.integers(0, n - 1))] = H.REC_TRM              # a terminate bin of 0 inside the run
            u = dict(metas=[], blocks=[], side=rec.astype(np.uint16), at=None, qp=int(rng.integers(0, 64)), finish=finish)
            u["data"] = orc.encode_records(rec if n else M.TRM_END, u["qp"], 2, 3)[0]
            if rep:
                d = u["data"].copy()
                d[int(rng.integers(0, len(d)))] ^= 1 << int(rng.integers(0, 8))
                u["data"] = d
            units.append(u)
    r = run_unit(hip, units)
    P = r["P"]
    t_desc, t_buf, t_rec = dev(P["desc"], np.uint8), dev(P["bytes"]), dev(P["records"].view(np.int16))
    t_bins = torch.full((len(P["records"]),), BIN_GUARD, dtype=torch.uint8, device="cuda")
    t_res = torch.zeros(2 * len(units), dtype=torch.int32, device="cuda")
    hip.decode_device(len(units), t_desc.data_ptr(), t_rec.data_ptr(), t_buf.data_ptr(), t_bins.data_ptr(), t_res.data_ptr())
    hip.synchronize()
    want_bins, want_res = t_bins.cpu().numpy(), t_res.cpu().numpy().view(H.RESULT_DTYPE)
    clean = 0
    for s, u in enumerate(units):
        if int(want_res["flags"][s]):
            continue
        clean += 1
        r0 = int(P["desc"]["rec_offset"][s])
        assert np.array_equal(r["bins"][s], want_bins[r0:r0 + len(u["side"])]), s
        assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (int(want_res["n_bits"][s]), 0), s
        if s < 7:                                                         # intact: the bins that were coded
            assert np.array_equal(r["bins"][s], (u["side"] >> 15).astype(np.uint8)), s
    assert clean >= 6                                                     # the intact runs of one record and more, at the least


# ---------------------------------------------------------------------------------------------- 3. round trip through the writer
def device_encode(hip, units, int16=False):
    """cabac_hip_encode_residual_device over the units (FINISH | ALIGN_RBSP) -> the coded bytes of every unit"""
    import torch
    n = len(units)
    P = M.pack([with_(u, data=np.zeros(0, np.uint8)) for u in units])
    desc = P["desc"].copy()
    desc["init_id"] = 2 | H.SUB_FINISH | H.SUB_ALIGN_RBSP
    splices, first, t = [], [0], 0
    for u in units:
        pos = U.positions(u["at"] if u["at"] is not None else [None] * len(u["metas"]), len(u["side"]))
        for p in pos:
            splices.append((p, t))
            t += 1
        if pos:                                                           # the helper gives the parse's view of the list back
            order, at = capi.splices_to_tu_at(np.array(splices[first[-1]:], capi.SPLICE_DTYPE))
            assert order.tolist() == list(range(first[-1], t)) and at.tolist() == pos
        first.append(len(splices))
    coeff = np.concatenate([np.asarray(c, np.int32).ravel() for u in units for c in u["blocks"]] + [np.zeros(0, np.int32)])
    cap = 64 * n + sum(len(u["data"]) for u in units)
    t_desc, t_rec, t_first = dev(desc, np.uint8), t_or_dummy(P["records"].view(np.int16), None), dev(np.array(first, np.uint32).view(np.int32))
    t_sp = t_or_dummy(np.array(splices, capi.SPLICE_DTYPE), np.uint8)
    t_tu = t_or_dummy(P["tus"][:P["n_tu"]], np.uint8)
    t_co = t_or_dummy(coeff.astype(np.int16 if int16 else np.int32), None)
    t_pay = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
    t_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    t_res = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    hip.encode_residual_device(n, t_desc.data_ptr(), t_rec.data_ptr(), t_first.data_ptr(), t_sp.data_ptr() if t else 0, t, t,
                               t_tu.data_ptr() if t else 0, t_co.data_ptr() if t else 0, t_pay.data_ptr(), cap, t_off.data_ptr(),
                               t_res.data_ptr(), int16=int16)
    hip.synchronize()
    assert not t_res.cpu().numpy().view(H.RESULT_DTYPE)["flags"].any()
    pay, off = t_pay.cpu().numpy(), t_off.cpu().numpy()
    return [pay[int(off[s]):int(off[s + 1])].copy() for s in range(n)]


def _roundtrip_units(rng):
    """Runs R + [TRM] with blocks at 0, at 64 (three of them), at 128 and at the end of R; all blocks at the end of a short R; one
    block in an empty R; a run without blocks."""
    return [M.make_unit(rng, ["regular", "ts", "sbt", "bdpcm", "regular", "regular"], 130, at=[0, 64, 64, 64, 128, 130]),
            M.make_unit(rng, ["regular"] * 3, 7, at=[7, 7, 7], shapes=[(8, 8), (4, 4), (64, 16)]),
            M.make_unit(rng, ["regular"], 0, at=[0]),
            M.make_unit(rng, [], 20, at=[])]


@pytest.mark.parametrize("int16", [False, True])
def test_round_trip_through_the_device_s_own_writer(hip, int16):
    """encode_residual_device -> parse_unit_device: coefficients, side bins, tu_info, n_bits and flags, for blocks at 0, at
    n_records, three at one position, exactly at records 64 and 128, with d_tu_at NULL, and with a d_tu_at that decreases or
    passes the end (clipped, not refused)."""
    rng = np.random.default_rng(0x13)
    units = _roundtrip_units(rng)
    for u, data in zip(units, device_encode(hip, units, int16)):
        assert np.array_equal(data, u["data"])                            # the writer's bytes are the oracle's
        u["data"] = data
    assert_valid(run_unit(hip, units, int16), units, int16, "as coded")
    # the run without its terminate bin: blocks AT n_records, and raw positions that go backwards or pass the end
    short = [with_(u, side=u["side"][:-1], finish=False) for u in units]
    raw = [[0, 64, 10, 64, 128, 0xFFFFFFFF], [7, 0, 9], [3], []]
    r = run_unit(hip, [with_(u, at=a) for u, a in zip(short, raw)], int16)
    assert_valid(r, short, int16, "clipped positions")
    # d_tu_at == NULL: every block behind the run
    behind = short[1:]
    r = run_unit(hip, [with_(u, at=None) for u in behind], int16, null_at=True)
    assert_valid(r, behind, int16, "null positions")


# ---------------------------------------------------------------------------------------------- 4. transform_skip_flag both ways
def test_transform_skip_flag_as_a_side_record_and_read_by_the_parser(hip):
    rng = np.random.default_rng(0x14)
    styles = ["ts_flag_1", "ts_flag_0", "ts_flag_1", "ts_flag_0", "regular", "ts_flag_1"]
    units = [M.make_unit(rng, styles, 9, ts_side={0, 1, 5}), M.make_unit(rng, styles[::-1], 3, ts_side={2, 3})]
    for u in units:
        ids = u["side"] & 0x1FF
        assert ((ids == 310) | (ids == 311)).sum() >= 2                    # flags in the run ...
        assert sum(bool(m[3] & H.TU_TS_FLAG) for m in u["metas"]) >= 2      # ... and flags the parser reads
        assert any(m[3] & H.TU_TS_FLAG and m[3] & H.TU_TRANSFORM_SKIP for m in u["metas"])
    assert_valid(run_unit(hip, units), units, False)


# ---------------------------------------------------------------------------------------------- 5. one store
EDGE_IDS = [0, 85, 86, 291, 292, 309, 310, 311, 312, 356, 357, 378]


def test_side_records_and_blocks_share_one_context_store(hip):
    """Side records on contexts the blocks use too (SigCoeffGroup 86, LastX 246.., TransformSkipFlag 310, the transform-skip
    sets) in front of and between the blocks, thirty each with a skewed bin so that the states move far, and on the edges of every
    id range: with two stores, or an id in the wrong slot, the blocks behind them decode to something else."""
    rng = np.random.default_rng(0x15)
    shared = [86, 87, 246, 247, 249, 269, 90, 91, 150, 214, 310, 357, 360, 373]
    run = []
    for k in range(3):
        for cid in shared:
            run += [cid | 0x8000 if (cid + k) & 1 else cid] * 30
        run += [c | (int(rng.integers(0, 2)) << 15) for c in EDGE_IDS] * 3
    n = len(run) // 3
    styles = ["regular", "ts_flag_1", "regular", "ts", "ts_flag_0", "regular"]
    base = M.make_unit(rng, styles, 0, at=[0] * 6, trm=False)
    metas = [(m[0], m[1], 0) + tuple(m[3:]) for m in base["metas"]]       # luma: the contexts named above
    unit = dict(metas=metas, blocks=base["blocks"], side=np.concatenate([np.array(run, np.uint16), M.TRM_END]),
                at=[n, n, 2 * n, 2 * n, 3 * n, 3 * n], qp=30, finish=True)
    unit["data"] = M.encode_unit(unit)
    # A reader whose side walk keeps a store of its own, modelled on the CPU: the side records moved to contexts no block uses.
    # It reads other bins for the blocks, so this input tells the two apart.
    orc = H.load_oracle()
    string, spans, is_side = M.expand(unit["side"], list(zip(unit["metas"], unit["blocks"])), unit["at"])
    apart = string.copy()
    ids = apart & 0x1FF
    apart[is_side & (ids >= 86) & (ids < 379)] = 1
    rc, bins, _ = orc.decode_records(apart, 30, 2, unit["data"])
    assert not np.array_equal(bins[~is_side], (string >> 15)[~is_side])
    assert_valid(run_unit(hip, [unit]), [unit], False)


# ---------------------------------------------------------------------------------------------- 6. the winner log
def test_winner_log_round_trip(hip):
    """Three chains, four rounds, a head and a tail entry each: search_log_encode_device, then the log's view turned into
    chain-relative positions (chain_rec_first + at) — the parse returns the logged coefficients and records."""
    import search_emit_model as E
    from test_gpu_search import t_u32
    from test_gpu_search_emit import RBSP, Cands, Tail, encode_log, make_rounds, start_sets
    rng = np.random.default_rng(0x16)
    K, lam = 3, int(1.7 * (1 << 16))
    qp, init = rng.integers(18, 42, K), np.full(K, 2)
    rounds, tail = make_rounds(rng, K, 4), Tail(K)
    head_rec = U.side_run(rng, 3 * K)
    head = Cands(np.zeros(K + 1, np.uint32), np.zeros(0, H.TU_DTYPE), np.zeros(0, np.int32), 3 * np.arange(K + 1, dtype=np.uint64), head_rec, None)
    model = E.LogModel(K)
    t_state, t_rate, sets, keep = start_sets(hip, qp, init)
    ident = np.arange(K, dtype=np.uint32)
    t_chain, t_head = t_u32(ident), t_u32(ident)
    log = hip.search_log(K, 6 * K, 6 * K * 30, 6 * K * 2, 6 * K * 2 * 256)
    head.append(log, t_head, t_chain, K)
    assert head.model_append(model, ident, ident)
    for rd in rounds:
        rd.enqueue(hip, log, t_state, t_rate, t_chain, lam)
        sets = rd.model(model, sets, lam)
    tail.cands.append(log, tail.t_pick, t_chain, K)
    assert tail.cands.model_append(model, tail.pick, ident)
    got, want = encode_log(hip, log, model, qp, init, RBSP)
    pay, off = got[0], got[1]
    a = log.read()
    log.close()
    ent = a["entries"]
    assert len(ent) == 6 * K
    units = []
    for ch in range(K):
        mine = [e for e in ent if int(e["chain"]) == ch]                   # in the order they were appended
        side, at, metas, blocks = [], [], [], []
        for e in mine:
            assert int(e["chain_rec_first"]) == len(side) and int(e["chain_tu_first"]) == len(metas)
            side += a["records"][int(e["rec_first"]):int(e["rec_first"]) + int(e["n_rec"])].tolist()
            for t in range(int(e["tu_first"]), int(e["tu_first"]) + int(e["n_tu"])):
                d = a["tu"][t]
                w, h = 1 << int(d["log2_width"]), 1 << int(d["log2_height"])
                metas.append((w, h, int(d["channel"]), int(d["flags"])))
                blocks.append(a["coeff"][int(d["coeff_offset"]):int(d["coeff_offset"]) + w * h].reshape(h, w).astype(np.int32))
                at.append(int(e["chain_rec_first"]) + int(a["tu_at"][t]))
        units.append(dict(metas=metas, blocks=blocks, side=np.array(side, np.uint16), at=at, qp=int(qp[ch]), finish=True,
                          data=pay[int(off[ch]):int(off[ch + 1])].copy()))
        assert np.array_equal(units[-1]["data"], M.encode_unit(units[-1]))
    assert sum(len(u["metas"]) for u in units) >= 6 and all(int(u["side"][-1]) == 0x81FF for u in units)
    assert_valid(run_unit(hip, units), units, False)
    del keep


# ---------------------------------------------------------------------------------------------- 7. damaged input
DAMAGED_SEED = 7                                                       # tests/test_parse_unit_model.py: the block-only analogue skips 0 of 200


def test_damaged_input_parses_to_a_consistent_result(hip):
    """200 substreams of regular blocks up to 8 x 8 with side records between them, one to three flipped bits, zero-padded so
    that the input cannot run out: guards intact, flags within {BAD_STOP}, and what came back is the reader's walk
    (parse_unit_model.consistent) for every substream that can be judged — all but 1 in 20 at the most."""
    units = M.damaged_units(DAMAGED_SEED, 200)
    r = run_unit(hip, units)
    assert_untouched_outside(r, units, False)
    skipped = changed = 0
    for s, u in enumerate(units):
        fl = int(r["res"]["flags"][s])
        assert (fl & ~H.RES_BAD_STOP) == 0, s
        try:
            ok, rc = M.consistent(u["data"], u["qp"], u["side"], u["metas"], u["at"], r["blocks"][s], r["bins"][s],
                                  int(r["res"]["n_bits"][s]), finish=True)
        except M.Skip:
            skipped += 1
            continue
        assert ok and {0: 0, -5: H.RES_BAD_STOP}[rc] == fl, s
        changed += not all(np.array_equal(coded(a), coded(b)) for a, b in zip(r["blocks"][s], u["blocks"]))
    print("damaged corpus: %d of %d skipped, %d decoded to other blocks" % (skipped, len(units), changed))
    assert skipped <= len(units) // 20
    assert changed > 0                                                    # the damage does reach the blocks


# ---------------------------------------------------------------------------------------------- 8. refusals on the device
def test_a_bad_side_record_stops_its_substream_and_no_other(hip):
    orc = H.load_oracle()
    rng = np.random.default_rng(0x18)
    units = [M.make_unit(rng, ["regular", "ts", "regular"], 12, at=[2, 6, 10], shapes=None) for _ in range(8)]
    bad_s, bad_i = 3, 7                                                  # behind block 1 (at 6), in front of block 2 (at 10)
    bad = units[bad_s]
    assert U.positions(bad["at"], len(bad["side"])) == [2, 6, 10]

    def mutate(P):
        P["records"][int(P["desc"]["rec_offset"][bad_s]) + bad_i] = 0x1FC | 0x8000
    r = run_unit(hip, units, mutate=mutate)
    good = [s for s in range(8) if s != bad_s]
    for s in good:                                                        # the seven neighbours
        n_bits, flags = want_walk(units[s])
        assert (int(r["res"]["n_bits"][s]), int(r["res"]["flags"][s])) == (n_bits, 0) and flags == 0
        assert np.array_equal(r["bins"][s], (units[s]["side"] >> 15).astype(np.uint8))
        assert all(np.array_equal(coded(a), coded(b)) for a, b in zip(r["blocks"][s], units[s]["blocks"]))
    # the stopped one: everything in front of the record, nothing behind it
    string, spans, is_side = M.expand(bad["side"], list(zip(bad["metas"], bad["blocks"])), bad["at"])
    cut = int(np.flatnonzero(np.cumsum(is_side) == bad_i + 1)[0])         # the bad record's place in the expanded string
    rc, _, n_bits = orc.decode_records(string[:cut], bad["qp"], 2, bad["data"])
    assert rc == 0 and (int(r["res"]["n_bits"][bad_s]), int(r["res"]["flags"][bad_s])) == (n_bits, H.RES_BAD_RECORD)
    assert np.array_equal(r["bins"][bad_s][:bad_i], (bad["side"][:bad_i] >> 15).astype(np.uint8))
    assert (r["bins"][bad_s][bad_i:] == BIN_GUARD).all()
    assert all(np.array_equal(coded(r["blocks"][bad_s][k]), coded(bad["blocks"][k])) for k in (0, 1))
    t0 = int(r["P"]["tile_first"][bad_s])
    assert r["info"][t0:t0 + 2].tolist() == want_info(bad)[:2] and r["info"][t0 + 2] == np.uint32(WORD_GUARD & 0xFFFFFFFF)
    assert_untouched_outside(r, units, False, parsed=[2 if s == bad_s else 3 for s in range(8)])


def test_no_bytes_and_a_refused_start(hip):
    """byte_capacity 0: CABAC_RES_UNDERRUN with nothing read; a first byte 0xFF: CABAC_RES_BAD_STOP with nothing parsed."""
    rng = np.random.default_rng(0x19)
    units = [M.make_unit(rng, [], 5, at=[]), M.make_unit(rng, ["regular"], 5, at=[2]), M.make_unit(rng, ["regular"], 5, at=[2])]
    units[1]["data"] = np.concatenate([[0xFF], units[1]["data"][1:]]).astype(np.uint8)
    poison = [None]

    def mutate(P):                                                        # whatever lies at a substream without bytes is not read
        P["desc"]["byte_capacity"][0] = 0
        P["bytes"][int(P["desc"]["byte_offset"][0]):int(P["desc"]["byte_offset"][0]) + 16] = 0xFF
        poison[0] = True
    r = run_unit(hip, units, mutate=mutate)
    assert poison[0] and int(r["res"]["flags"][0]) == H.RES_UNDERRUN
    assert (int(r["res"]["n_bits"][1]), int(r["res"]["flags"][1])) == (8, H.RES_BAD_STOP)
    assert (r["bins"][1] == BIN_GUARD).all() and r["info"][0] == np.uint32(WORD_GUARD & 0xFFFFFFFF)
    n_bits, flags = want_walk(units[2])
    assert (int(r["res"]["n_bits"][2]), int(r["res"]["flags"][2])) == (n_bits, 0)
    assert np.array_equal(coded(r["blocks"][2][0]), coded(units[2]["blocks"][0]))
    assert_untouched_outside(r, units, False, parsed=[0, 0, 1])


# ---------------------------------------------------------------------------------------------- 9. the batch form
@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("int16", [False, True])
def test_batch_form_gives_the_device_form_s_results(hip, pinned, int16):
    rng = np.random.default_rng(0x1A)
    units = _roundtrip_units(rng)
    r = run_unit(hip, units, int16)
    assert_valid(r, units, int16)
    P = r["P"]
    cdt = np.int16 if int16 else np.int32
    keep = []

    def buf(a):
        if not pinned:
            return a.copy()
        keep.append(capi.PinnedArray((max(len(a), 1),), a.dtype))
        keep[-1].array[:len(a)] = a
        return keep[-1].array[:len(a)]
    coeff = buf(np.full(P["total"], sentinel(int16), cdt))
    bins = buf(np.full(len(P["records"]), BIN_GUARD, np.uint8))
    host = capi.CabacHip(0)
    co, sb, res, info = host.parse_unit_batch(P["desc"], buf(P["bytes"]), P["tile_first"], P["tus"][:P["n_tu"]], P["tu_at"], buf(P["records"]),
                                              P["total"], int16=int16, coeff=coeff, side_bins=bins, with_info=True)
    assert np.array_equal(res, r["res"]) and np.array_equal(info, r["info"]) and np.array_equal(sb, r["all_bins"])
    if int16:                                                             # output only: zero where nothing is written
        mask = r["co"] != np.int32(np.int16(sentinel(True)))
        assert np.array_equal(co.astype(np.int32)[mask], r["co"][mask]) and not co[~mask].any()
    else:
        assert np.array_equal(co, r["co"])
    host.close()
    for k in keep:
        k.close()


def test_batch_form_refuses_what_the_header_says(hip):
    rng = np.random.default_rng(0x1B)
    units = _roundtrip_units(rng)
    P = M.pack(units)
    host = capi.CabacHip(0)

    def call(desc=None, tile_first=None, tu_at=None, records=None):
        coeff, bins = np.full(P["total"], 0x5A5A5A5A, np.int32), np.full(len(P["records"]), BIN_GUARD, np.uint8)
        with pytest.raises(capi.CabacHipError) as e:
            host.parse_unit_batch(P["desc"] if desc is None else desc, P["bytes"], P["tile_first"] if tile_first is None else tile_first,
                                  P["tus"][:P["n_tu"]], P["tu_at"] if tu_at is None else tu_at, P["records"] if records is None else records,
                                  P["total"], coeff=coeff, side_bins=bins)
        assert e.value.status == -2
        assert (coeff == 0x5A5A5A5A).all() and (bins == BIN_GUARD).all()  # no output touched
        return str(e.value)
    d = P["desc"].copy()
    d["n_records"][3] += 1                                                # the last run leaves n_records_total
    assert "n_records_total" in call(desc=d)
    d = P["desc"].copy()
    d["rec_offset"][0] = len(P["records"]) + 1
    assert "n_records_total" in call(desc=d)
    tf = P["tile_first"].copy()
    tf[2] = tf[1] - 1
    assert "tile_first" in call(tile_first=tf)
    at = P["tu_at"].copy()
    at[2] = 10                                                            # 0, 64, 10: decreases inside substream 0
    assert "decreases" in call(tu_at=at)
    at = P["tu_at"].copy()
    at[5] = 132                                                           # the run has 131 records
    assert "exceeds" in call(tu_at=at)
    rec = P["records"].copy()
    rec[int(P["desc"]["rec_offset"][1]) + 4] = 0x1FC
    msg = call(records=rec)
    assert "substream 1" in msg and "record 4" in msg
    co, sb, res = host.parse_unit_batch(P["desc"], P["bytes"], P["tile_first"], P["tus"][:P["n_tu"]], P["tu_at"], P["records"], P["total"])
    assert not res["flags"].any()                                         # and the ctx still works
    host.close()


# ---------------------------------------------------------------------------------------------- 10. stream order
def test_stream_order_on_the_default_stream(hip):
    """Fill -> call -> read on torch's default stream (stream=0 -> CABAC_HIP_STREAM_DEFAULT), no host synchronisation between."""
    import torch
    assert torch.cuda.current_stream().cuda_stream == 0
    rng = np.random.default_rng(0x1C)
    units = _roundtrip_units(rng)
    P = M.pack(units)
    own = capi.CabacHip(0, stream=0)
    src = [dev(P["desc"], np.uint8), dev(P["bytes"]), dev(P["tile_first"].view(np.int32)), dev(P["tus"][:P["n_tu"]], np.uint8),
           dev(P["tu_at"].view(np.int32)), dev(P["records"].view(np.int16))]
    torch.cuda.synchronize()
    for _ in range(2):
        big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
        big.fill_(0xA5)                                                   # a long fill in front, then the operands are produced ON the stream
        ops = [torch.zeros_like(s) for s in src]
        for o, s in zip(ops, src):
            o.copy_(s)
        out = Out(P, False)
        p_co, p_bins, p_info, p_res = out.ptrs()
        own.parse_unit_device(len(units), *[o.data_ptr() for o in ops], p_co, p_bins, p_res, d_tu_info=p_info)
        co, bins, info, res = out.read()
        assert not res["flags"].any()
        t = 0
        for s, u in enumerate(units):
            r0 = int(P["desc"]["rec_offset"][s])
            assert np.array_equal(bins[r0:r0 + len(u["side"])], (u["side"] >> 15).astype(np.uint8))
            for c in u["blocks"]:
                h, w = c.shape
                assert np.array_equal(coded(co[int(P["offsets"][t]):int(P["offsets"][t]) + w * h].reshape(h, w)), coded(c))
                t += 1
        del big, ops
    own.close()
