"""GPU: what the host-pointer forms of the parser family (cabac_hip_residual_parse_batch, cabac_hip_parse_unit_batch,
cabac_hip_parse_elements_batch, cabac_hip_parse_plan_batch, cabac_hip_plan_parse_rows_batch) refuse, in which order and in which
words; what such a call keeps of the caller's arrays and what it overwrites; and the event bracket of the single-launch device
calls (cabac_hip_last_kernel_ms, cabac_hip_profile_read).  The library functions are called directly, so that every output array is
the test's own.  Every expected status, message, value and kind below is a literal."""
import numpy as np
import pytest

import helpers as H
import parse_elements_model as E
import parse_plan_model as PM
import parse_unit_model as M
import plan_rows_model as R
from entropy_coding_amd import capi
from test_gpu_residual_estimate import dev

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (8, 8)]                                          # every substream: one block of each
N_SUB = 3
CO32, CO16, INFO, VALUE, BIN, RES = 0x5A5A5A5A, 0x5A5A, 0xA5A5A5A5, 0x3C3C3C3C, 0xEE, 0xEE
FORMS = ["residual", "unit", "elements", "plan", "rows"]
ERR_INVALID, ERR_SUBSTREAM = -2, -5


# ---------------------------------------------------------------------------------------------- inputs
def _arrays(P, **more):
    A = dict(desc=P["desc"], bytes=P["bytes"], tile_first=P["tile_first"], tus=P["tus"], tu_at=P["tu_at"], total=P["total"],
             n_tu=P["n_tu"], offsets=P["offsets"])
    A.update(more)
    return A


@pytest.fixture(scope="module")
def corpus():
    """form -> its valid host arrays: 3 substreams of a 4 x 4 and an 8 x 8 block each; the unit form with 6 side records and
    the terminate bin, the element / plan / rows forms with a plan of 6 one-bin and bypass elements and the terminate bin."""
    rng = np.random.default_rng(0x2B0)
    blocks_only = [M.make_unit(rng, ["regular"] * 2, 0, qp=30, at=None, shapes=SHAPES) for _ in range(N_SUB)]
    units = [M.make_unit(rng, ["regular"] * 2, 6, qp=30, at=[1, 4], shapes=SHAPES) for _ in range(N_SUB)]
    planned = []
    for u in units:
        plan, values = E.close(*E.random_plan(rng, 6, kinds=[E.CTX_BIN, E.EP_BINS], guard_frac=0.0))
        planned.append(E.make_unit(rng, plan, values, u["metas"], u["blocks"], at=[1, 4], guards=None, qp=30))
    Pb, Pu, Pe = M.pack(blocks_only), M.pack(units), PM.pack(planned)
    plan_arrays = _arrays(Pe, plan=Pe["plan"], tu_guard=None)
    rows = dict(level_first=np.array([0, N_SUB], np.uint32), sync_from=np.full(N_SUB, R.NO_SET, np.uint32),
                sync_at=np.zeros(N_SUB, np.uint32))
    return dict(residual=_arrays(Pb), unit=_arrays(Pu, records=Pu["records"]), elements=plan_arrays, plan=plan_arrays,
                rows=dict(plan_arrays, **rows))


@pytest.fixture()
def host():
    c = capi.CabacHip(0)
    yield c
    c.close()


def outputs(A, int16=False):
    """Every output array of a call, filled with its sentinel."""
    res = np.zeros(N_SUB, capi.RESULT_DTYPE)
    res.view(np.uint8)[:] = RES
    return dict(coeff=np.full(A["total"], CO16 if int16 else CO32, np.int16 if int16 else np.int32),
                info=np.full(A["n_tu"], INFO, np.uint32), res=res, bins=np.full(len(A.get("records", ())), BIN, np.uint8),
                values=np.full(len(A.get("plan", ())), VALUE, np.uint32))


def untouched(out, int16=False):
    return ((out["coeff"] == (CO16 if int16 else CO32)).all() and (out["info"] == INFO).all() and (out["bins"] == BIN).all() and
            (out["values"] == VALUE).all() and (out["res"].view(np.uint8) == RES).all())


def call(host, form, A, out, int16=False):
    """-> (status, last error) of the form's library function on the arrays A and the outputs out"""
    L, h = host.L, host.h

    def p(a):
        return None if a is None else np.ascontiguousarray(a).ctypes.data
    for a in list(A.values()) + list(out.values()):
        assert a is None or not isinstance(a, np.ndarray) or a.flags.c_contiguous
    d, by, cb = A["desc"], A["bytes"], 2 if int16 else 4
    head = (h, len(d), p(d), p(by), len(by), p(A["tile_first"]), p(A["tus"]))
    if form == "residual":
        fn = L.cabac_hip_residual_parse_batch16 if int16 else L.cabac_hip_residual_parse_batch
        rc = fn(*head, p(out["coeff"]), A["total"], p(out["info"]), p(out["res"]))
    elif form == "unit":
        rc = L.cabac_hip_parse_unit_batch(*head, p(A["tu_at"]), p(A["records"]), len(A["records"]), p(out["coeff"]), cb, A["total"],
                                          p(out["bins"]), p(out["info"]), p(out["res"]))
    else:
        fn = dict(elements=L.cabac_hip_parse_elements_batch, plan=L.cabac_hip_parse_plan_batch, rows=L.cabac_hip_plan_parse_rows_batch)[form]
        tail = (len(A["level_first"]) - 1, p(A["level_first"]), p(A["sync_from"]), p(A["sync_at"])) if form == "rows" else ()
        rc = fn(*head, p(A["tu_at"]), p(A["tu_guard"]), p(A["plan"]), len(A["plan"]), p(out["coeff"]), cb, A["total"], p(out["values"]),
                p(out["info"]), p(out["res"]), *tail)
    return rc, L.cabac_hip_last_error(h).decode()


def changed(A, **kw):
    B = dict(A)
    B.update(kw)
    return B


# the defects: each returns the arrays with ONE thing wrong
def bad_tile_first(A):                                             # substream 0: tile_first[0] > tile_first[1]
    tf = A["tile_first"].copy()
    tf[0] = tf[1] + 1
    return changed(A, tile_first=tf)


def bad_bytes(A, s=2):                                             # substream s: its byte range ends past bytes_total
    d = A["desc"].copy()
    d["byte_capacity"][s] = len(A["bytes"])
    return changed(A, desc=d)


def bad_init_id(A, s=1):
    d = A["desc"].copy()
    d["init_id"][s] |= 3
    return changed(A, desc=d)


def bad_coeff(A):                                                  # the last block begins where the coefficients end
    tus = A["tus"].copy()
    tus["coeff_offset"][A["n_tu"] - 1] = A["total"]
    return changed(A, tus=tus)


def bad_tu_at(A, s=1):                                             # substream s: 4, 1
    at = A["tu_at"].copy()
    t = int(A["tile_first"][s])
    at[t], at[t + 1] = 4, 1
    return changed(A, tu_at=at)


def bad_entry(A, s=1, i=2):                                        # element i of substream s: kind 15
    plan = A["plan"].copy()
    plan[int(A["desc"]["rec_offset"][s]) + i] = (0xF, 0)
    return changed(A, plan=plan)


def bad_record(A, s=1, i=4):                                       # record i of substream s: an id that is none
    rec = A["records"].copy()
    rec[int(A["desc"]["rec_offset"][s]) + i] = 0x1FC
    return changed(A, records=rec)


def refused(host, form, A, message):
    out = outputs(A)
    rc, msg = call(host, form, A, out)
    assert (rc, msg) == (ERR_INVALID, message)
    assert untouched(out), "a refused call wrote an output"


def still_works(host, form, A):
    out = outputs(A)
    rc, _ = call(host, form, A, out)
    assert rc == 0 and not out["res"]["flags"].any() and not (out["info"] == INFO).any()


# ---------------------------------------------------------------------------------------------- (a) common defects
@pytest.mark.parametrize("form", FORMS)
def test_common_defects(host, corpus, form):
    A = corpus[form]
    still_works(host, form, A)
    refused(host, form, bad_tile_first(A), "tile_first must not decrease")
    refused(host, form, bad_bytes(A), "bytes out of range")
    refused(host, form, bad_init_id(A), "init_id must be 0..2")
    refused(host, form, bad_coeff(A), "coefficients out of range")
    still_works(host, form, A)


# ---------------------------------------------------------------------------------------------- (b) precedence
@pytest.mark.parametrize("form", FORMS)
def test_substream_checks_come_before_the_block_loop(host, corpus, form):
    refused(host, form, bad_coeff(bad_tile_first(corpus[form])), "tile_first must not decrease")


@pytest.mark.parametrize("form", FORMS)
def test_the_lower_substream_wins(host, corpus, form):
    refused(host, form, bad_init_id(bad_bytes(corpus[form], s=1), s=0), "init_id must be 0..2")


@pytest.mark.parametrize("form", ["unit", "elements", "plan", "rows"])
def test_positions_are_checked_before_the_entries(host, corpus, form):
    A = bad_tu_at(corpus[form])
    refused(host, form, bad_record(A) if form == "unit" else bad_entry(A), "tu_at decreases inside a substream")


def test_rows_plan_checks_come_before_the_level_checks(host, corpus):
    A = changed(bad_entry(corpus["rows"]), level_first=np.array([0, N_SUB - 1], np.uint32))
    refused(host, "rows", A, "bad plan entry: substream 1, element 2 of its plan (word0 0xf, word1 0x0): kind above 10")
    refused(host, "rows", changed(corpus["rows"], level_first=np.array([0, N_SUB - 1], np.uint32)), "level_first must run from 0 to n_sub")


# ---------------------------------------------------------------------------------------------- (c) each form's own wording
def test_wording_of_the_element_parse(host, corpus):
    refused(host, "elements", bad_entry(corpus["elements"]),
            "bad plan entry: substream 1, element 2 of its plan (word0 0xf, guard 0x0): kind above 8")


def test_wording_of_the_plan_parse(host, corpus):
    refused(host, "plan", bad_entry(corpus["plan"]),
            "bad plan entry: substream 1, element 2 of its plan (word0 0xf, word1 0x0): kind above 10")


def test_wording_of_the_unit_parse(host, corpus):
    refused(host, "unit", bad_record(corpus["unit"]), "bad side record: substream 1, record 4 of its run (id 0x1fc)")


# ---------------------------------------------------------------------------------------------- (d) kept and overwritten
def stopped(A, s=1):
    """Substream s begins with the byte 0xFF: refused as a whole (CABAC_RES_BAD_STOP), nothing of it is parsed."""
    by = A["bytes"].copy()
    by[int(A["desc"]["byte_offset"][s])] = 0xFF
    return changed(A, bytes=by)


@pytest.mark.parametrize("int16", [False, True])
@pytest.mark.parametrize("form", ["residual", "unit", "elements", "plan"])
def test_what_a_call_keeps_and_what_it_overwrites(host, corpus, form, int16):
    A = corpus[form]
    valid = outputs(A, int16)
    assert call(host, form, A, valid, int16)[0] == 0
    out = outputs(A, int16)
    rc, msg = call(host, form, stopped(A), out, int16)
    assert (rc, msg) == (ERR_SUBSTREAM, "substream flag set (see results[].flags)")
    assert out["res"]["flags"].tolist() == [0, H.RES_BAD_STOP, 0]
    t0, t1 = int(A["tile_first"][1]), int(A["tile_first"][2])
    mine = np.zeros(A["n_tu"], bool)
    mine[t0:t1] = True
    print("info words of the stopped substream:", form, int16, [hex(int(x)) for x in out["info"][mine]])
    # the info words: the element and plan forms upload the caller's first, so the stopped substream's come back as they went in;
    # the residual and unit forms do not, and the words are what the device buffer held: the previous call's
    assert np.array_equal(out["info"][~mine], valid["info"][~mine])
    if form in ("elements", "plan"):
        assert (out["info"][mine] == INFO).all()
    else:
        assert np.array_equal(out["info"][mine], valid["info"][mine]) and not (out["info"] == INFO).any()
    # the coefficients: int32 blocks keep the caller's values, int16 blocks are output only and zero where nothing is written
    c0, c1 = int(A["offsets"][t0]), int(A["offsets"][t1]) if t1 < A["n_tu"] else A["total"]
    assert (out["coeff"][c0:c1] == (0 if int16 else CO32)).all()
    assert np.array_equal(out["coeff"][:c0], valid["coeff"][:c0]) and np.array_equal(out["coeff"][c1:], valid["coeff"][c1:])
    r0, r1 = int(A["desc"]["rec_offset"][1]), int(A["desc"]["rec_offset"][1]) + int(A["desc"]["n_records"][1])
    if form == "unit":                                             # unwritten side bins keep the caller's values
        assert (out["bins"][r0:r1] == BIN).all() and not (out["bins"][:r0] == BIN).any() and not (out["bins"][r1:] == BIN).any()
    if form in ("elements", "plan"):                               # and so do unwritten values
        assert (out["values"][r0:r1] == VALUE).all() and not (out["values"][:r0] == VALUE).any()


# ---------------------------------------------------------------------------------------------- (e) the bracket
class Device:
    """A tiny batch of everything the single-launch device calls take, on the device."""

    def __init__(self, corpus):
        import torch
        rng = np.random.default_rng(0x2B1)
        self.keep = []
        z = self.zeros
        # two substreams of bin records, coded
        recs = [H.random_records(rng, 60), H.random_records(rng, 40)]
        desc, total = H.make_desc([len(r) for r in recs], [30, 27], [2, 2], H.SUB_FINISH | H.SUB_ALIGN_RBSP)
        self.n, self.total = 2, total
        self.desc, self.rec = self.up(desc, np.uint8), self.up(np.concatenate(recs).view(np.int16))
        self.bytes, self.back, self.pay = z(total + 64), z(total + 64), z(total + 64)
        self.res, self.bins, self.bits, self.flags = z(64), z(256), z(64), z(64)
        self.off, self.counts = z(64), z(64)
        # context sets: one per substream, as cabac_hip_ctx_init_device makes them
        self.qp, self.init = self.up(np.array([30, 27], np.int32)), self.up(np.array([2, 2], np.uint32).view(np.int32))
        self.state, self.rate, self.out_state, self.out_rate = z(2 * 379 * 4), z(2 * 379), z(2 * 379 * 4), z(2 * 379)
        self.set = self.up(np.array([0, 1], np.uint32).view(np.int32))
        self.no_set = self.up(np.array([capi.SEARCH_NO_SET] * 2, np.uint32).view(np.int32))
        # syntax elements of one substream: a context bin and the terminate bin
        self.se, self.se_off = self.up(np.array([[5 << 4, 1], [3, 1]], np.uint32).view(np.int32)), self.up(np.array([0, 2], np.uint64).view(np.int64))
        # the parsers' inputs
        self.P = {f: {k: self.up(v, np.uint8) for k, v in corpus[f].items() if isinstance(v, np.ndarray) and v.size}
                  for f in ("residual", "unit", "plan")}
        self.A = corpus
        self.coeff, self.info, self.side, self.values, self.pres = z(4 * 512), z(64), z(64), z(256), z(64)
        # candidates: the residual corpus' blocks as one candidate per substream
        self.cand_first = self.P["residual"]["tile_first"]
        self.tu_bits, self.rec_first = z(8 * 8), z(8 * 8)
        self.co_in = self.up(np.concatenate([b.reshape(-1) for b in self._blocks(corpus)]).astype(np.int32))
        self.group_first = self.up(np.array([0, N_SUB], np.uint32).view(np.int32))
        self.pick, self.cost = z(16), z(16)
        # a payload of one segment for the emulation prevention
        self.nal_in, self.nal_off = self.up(np.array([0, 0, 1, 7, 0, 0, 0, 9], np.uint8)), self.up(np.array([0, 8], np.uint64).view(np.int64))
        self.nal, self.nal_noff, self.nal_back, self.nal_boff, self.nal_st = z(64), z(64), z(64), z(64), z(64)
        torch.cuda.synchronize()

    @staticmethod
    def _blocks(corpus):
        # the coefficient array a writer would hand in: zeros are enough for a launch, but a block must not be empty
        A = corpus["residual"]
        co = np.zeros(A["total"], np.int32)
        for t in range(A["n_tu"]):
            co[int(A["offsets"][t])] = 3
        return [co]

    def up(self, a, dt=None):
        self.keep.append(dev(a, dt))
        return self.keep[-1].data_ptr()

    def zeros(self, n):
        import torch
        self.keep.append(torch.zeros(n, dtype=torch.uint8, device="cuda"))
        return self.keep[-1].data_ptr()

    def calls(self, hip):
        """[(name, the call, the kind its bracket records)] in the order of the library's source"""
        d, P, n3 = self, self.P, N_SUB
        Pr, Pu, Pp = P["residual"], P["unit"], P["plan"]
        plan_args = (n3, Pp["desc"], Pp["bytes"], Pp["tile_first"], Pp["tus"], Pp["tu_at"], 0, Pp["plan"], d.coeff, d.values, d.pres)
        return [
            ("encode_device", lambda: hip.encode_device(d.n, d.desc, d.rec, d.bytes, d.res), 0),
            ("decode_device", lambda: hip.decode_device(d.n, d.desc, d.rec, d.bytes, d.bins, d.res), 1),
            ("estimate_device", lambda: hip.estimate_device(d.n, d.desc, d.rec, d.bits, d.flags), 4),
            ("estimate_from_device", lambda: hip.estimate_from_device(d.n, d.desc, d.rec, d.state, d.rate, d.set, d.bits, d.flags), 4),
            ("assemble_device", lambda: hip.assemble_device(d.n, d.desc, d.res, d.bytes, d.pay, d.total, d.off), 6),
            ("split_device", lambda: hip.split_device(d.n, d.desc, d.off, d.pay, d.back), 7),
            ("count_emulations_device", lambda: hip.count_emulations_device(d.n, d.desc, d.res, d.bytes, d.counts), 8),
            ("binarize_device", lambda: hip.binarize_device(1, d.se_off, d.se, 0, d.counts, 0), 2),
            ("residual_device", lambda: hip.residual_device(self.A["residual"]["n_tu"], Pr["tus"], d.co_in, 0, d.counts, d.info, 0), 5),
            ("residual_parse_device", lambda: hip.residual_parse_device(n3, Pr["desc"], Pr["bytes"], Pr["tile_first"], Pr["tus"], d.coeff,
                                                                        d.pres, d_tu_info=d.info), 9),
            ("residual_parse16_device", lambda: hip.residual_parse_device(n3, Pr["desc"], Pr["bytes"], Pr["tile_first"], Pr["tus"], d.coeff,
                                                                          d.pres, d_tu_info=d.info, int16=True), 9),
            ("parse_unit_device", lambda: hip.parse_unit_device(n3, Pu["desc"], Pu["bytes"], Pu["tile_first"], Pu["tus"], Pu["tu_at"],
                                                                Pu["records"], d.coeff, d.side, d.pres, d_tu_info=d.info), 25),
            ("parse_elements_device", lambda: hip.parse_elements_device(*plan_args, d_tu_info=d.info), 26),
            ("parse_plan_device", lambda: hip.parse_plan_device(*plan_args, d_tu_info=d.info), 27),
            ("estimate_residual_device", lambda: hip.estimate_residual_device(n3, d.cand_first, Pr["tus"], d.co_in, d.state, d.rate, d.set3(),
                                                                              d.bits, d.tu_bits, d.info), 12),
            ("nal_escape_device", lambda: hip.nal_escape_device(1, d.nal_off, d.nal_in, 8, d.nal, 32, d.nal_noff, d.nal_st), 13),
            ("nal_unescape_device", lambda: hip.nal_unescape_device(1, d.nal_noff, d.nal, 32, d.nal_back, 32, d.nal_boff, d.nal_st), 14),
            ("estimate_residual_ctx_device", lambda: hip.estimate_residual_ctx_device(n3, d.cand_first, Pr["tus"], d.co_in, d.state, d.rate,
                                                                                      d.set3(), d.bits, d.no_set3(), d.out_state,
                                                                                      d.out_rate), 15),
            ("search_select_device", lambda: hip.search_select_device(1, d.group_first, d.bits, 0, 1 << 16, d.pick, d.cost), 16),
            ("estimate_unit_device", lambda: hip.estimate_unit_device(n3, d.cand_first, Pr["tus"], d.co_in, d.state, d.rate, d.set3(),
                                                                      d.rec_first, 0, 0, d.bits), 19),
            ("encode_sets_device", lambda: hip.encode_sets_device(d.n, d.desc, d.rec, d.bytes, d.res), 30),
            ("decode_sets_device", lambda: hip.decode_sets_device(d.n, d.desc, d.rec, d.bytes, d.bins, d.res), 31),
            ("ctx_advance_device", lambda: hip.ctx_advance_device(d.n, d.desc, d.rec, 0, 0, 0, 0, 0, 0, 0), 32),
            ("plan_parse_sets_device", lambda: hip.plan_parse_sets_device(*plan_args, d_tu_info=d.info), 34),
        ]

    def set3(self):
        if not hasattr(self, "_set3"):
            self._set3 = self.up(np.array([0, 1, 0], np.uint32).view(np.int32))
            self._no_set3 = self.up(np.array([capi.SEARCH_NO_SET] * 3, np.uint32).view(np.int32))
        return self._set3

    def no_set3(self):
        self.set3()
        return self._no_set3


@pytest.fixture(scope="module")
def device(corpus):
    hip = H.gpu_ctx()
    d = Device(corpus)
    d.set3()
    hip.ctx_init_device(2, d.qp, d.init, d.state, d.rate)
    hip.synchronize()
    yield hip, d
    hip.close()


def pick(calls, *names):
    by_name = {c[0]: c for c in calls}
    return [by_name[n] for n in names]


def test_ring_off_the_ctx_pair_times_the_launch(device):
    hip, d = device
    hip.profile_enable(0)
    for name, run, _ in pick(d.calls(hip), "encode_device", "parse_plan_device", "ctx_advance_device"):
        run()
        assert hip.last_kernel_ms() > 0, name


def test_a_full_ring_falls_back_to_the_ctx_pair(device):
    hip, d = device
    first, second, third = pick(d.calls(hip), "encode_device", "parse_plan_device", "ctx_advance_device")
    hip.profile_enable(2)
    first[1]()
    assert hip.last_kernel_ms() == -1.0                            # the ring took the launch
    second[1]()
    assert hip.last_kernel_ms() == -1.0
    third[1]()
    assert hip.last_kernel_ms() > 0                                # the ring is full: the ctx's own pair
    got = hip.profile_read()
    assert [k for k, _ in got] == [0, 27] and all(ms > 0 for _, ms in got)
    hip.profile_enable(0)


def test_kind_of_every_single_launch_device_call(device):
    hip, d = device
    hip.profile_enable(1)
    calls = d.calls(hip)
    assert [k for _, _, k in calls] == [0, 1, 4, 4, 6, 7, 8, 2, 5, 9, 9, 25, 26, 27, 12, 13, 14, 15, 16, 19, 30, 31, 32, 34]
    for name, run, kind in calls:
        run()
        got = hip.profile_read()
        assert [k for k, _ in got] == [kind], name
    hip.profile_enable(0)
