"""GPU: the host-pointer forms outside the parser family — cabac_hip_estimate_batch, cabac_hip_residual_batch, the spliced encode
(plain, rows, probes, sparse), the plan write (plain, rows), cabac_hip_estimate_residual_batch, the three search rounds, the NAL
forms, the WPP forms and the probe forms: what each refuses, in which order and in which words; what a refused call has and has not
written; that a valid call returns what the `_device` call makes of the same arrays on the same ctx; and how many blocking runtime
calls (cabac_hip_workspace_waits) a second, identical call issues.  The library functions are called directly, so that every output
array is the test's own, filled with 0xEE bytes.  Every expected status, message and wait count below is a literal."""
import numpy as np
import pytest

import helpers as H
import parse_elements_model as E
import parse_plan_model as PM
import parse_unit_model as M
import search_plan_model as SP
import search_unit_model as U
import write_plan_model as W
from entropy_coding_amd import capi
from test_gpu_residual_estimate import dev, make_sets, pack_sets

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (8, 8)]                                          # every substream: one block of each
N_SUB, N_TU, N_CAND, N_GROUP = 3, 6, 4, 2
ERR_INVALID, ERR_SUBSTREAM = -2, -5
NO_SET = 0xFFFFFFFF
CAP = 4096                                                         # bytes of every payload / NAL buffer
LAMBDA = 1 << 16

# cabac_hip_workspace_waits of a second, identical call (every buffer exists), read off the build before the staging was shared
WAITS = {
    "estimate": 1, "residual": 2, "splice plain": 14, "splice rows": 16, "splice probes": 17, "splice sparse": 15,
    "write plan": 18, "write rows": 20, "estimate residual": 1, "search plain": 2, "search unit": 2, "search plan": 3,
    "nal escape": 2, "nal unescape": 2, "encode nal": 2, "wpp encode": 7, "wpp decode": 8, "written bits": 1, "estimate probes": 1,
    "parse unit": 1, "sparse parse": 2,
}


# ---------------------------------------------------------------------------------------------- plumbing
def S(n, dtype):
    a = np.zeros(n, dtype)
    a.view(np.uint8)[:] = 0xEE
    return a


def clean(a):
    return bool((a.view(np.uint8) == 0xEE).all())


def p(a):
    if a is None:
        return None
    assert a.flags.c_contiguous
    return a.ctypes.data


def ptrs(null, **arrays):
    q = {k: p(v) for k, v in arrays.items()}
    if null:
        assert null in q
        q[null] = None
    return q


def changed(A, **kw):
    B = dict(A)
    B.update(kw)
    return B


def edit(A, name, idx, value, field=None):
    a = A[name].copy()
    if field:
        a[field][idx] = value
    else:
        a[idx] = value
    return changed(A, **{name: a})


def last_error(host):
    return host.L.cabac_hip_last_error(host.h).decode()


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(0x57A6)
    A = {}
    # the spliced encode and the unit parse: 3 substreams of a 4 x 4 and an 8 x 8 block in 6 side records and the terminate bin
    units = [M.make_unit(rng, ["regular"] * 2, 6, qp=30, at=[1, 4], shapes=SHAPES) for _ in range(N_SUB)]
    Pu = M.pack(units)
    A.update(desc=Pu["desc"], records=Pu["records"], tus=Pu["tus"][:N_TU].copy(), tu_at=Pu["tu_at"], bytes=Pu["bytes"],
             tile_first=Pu["tile_first"], splice_first=Pu["tile_first"].copy())
    A["coeff"] = np.concatenate([b.reshape(-1) for u in units for b in u["blocks"]]).astype(np.int32)
    A["coeff16"] = A["coeff"].astype(np.int16)
    sp = np.zeros(N_TU, capi.SPLICE_DTYPE)
    sp["at"], sp["tu"] = Pu["tu_at"], np.arange(N_TU)
    A["splices"] = sp
    A["ent_first"], A["entries"], _ = capi.sparse_pack_host(A["tus"], A["coeff16"])
    A["entries"] = A["entries"].copy()
    A["probe_first"], A["probe_at"] = np.array([0, 2, 4, 6], np.uint32), np.array([2, 5] * 3, np.uint32)
    A["level_first"], A["sync_from"], A["sync_at"] = np.array([0, 1, 3], np.uint32), np.array([NO_SET, 0, 0], np.uint32), np.array([2, 0, 0], np.uint32)
    # the plan write: the same blocks in a plan of 6 one-bin and bypass elements and the terminate bin
    planned = []
    for u in units:
        plan, values = E.close(*E.random_plan(rng, 6, kinds=[E.CTX_BIN, E.EP_BINS], guard_frac=0.0))
        planned.append(E.make_unit(rng, plan, values, u["metas"], u["blocks"], at=[1, 4], guards=None, qp=30))
    Pe = PM.pack(planned)
    pdesc = Pe["desc"].copy()
    pdesc["init_id"] = W.SUB_FLAGS
    A.update(pdesc=pdesc, plan=Pe["plan"], values_in=np.array([v for u in planned for v in u["values"]], np.uint32), ptu_at=Pe["tu_at"])
    # the search rounds: the six blocks as 4 candidates in 2 groups, 2 context sets; side runs of 3 records; plans of 3 elements
    blocks, metas = [b for u in units for b in u["blocks"]], [m for u in units for m in u["metas"]]
    cands, t = [], 0
    for n_blk, at in ((2, [1, 2]), (2, [0, 3]), (1, [2]), (1, [1])):
        plan, values = E.random_plan(rng, 3, kinds=[E.CTX_BIN, E.EP_BINS], guard_frac=0.0)
        cands.append(SP.cand(plan, values, metas[t:t + n_blk], blocks[t:t + n_blk], at=at))
        t += n_blk
    Ps = SP.pack(cands)
    state, rate = pack_sets(make_sets(rng, 2))
    A.update(cand_first=Ps["cand_first"], ctus=Ps["tus"], ccoeff=Ps["coeff"], ctu_at=Ps["tu_at"], cplan=Ps["plan"], cvalues=Ps["values"],
             ent64=Ps["ent_first"], state=state.astype(np.uint32), rate=rate, set=np.array([0, 0, 1, 1], np.uint32),
             group_first=np.array([0, 2, 4], np.uint32), out_set=np.array([0, 1], np.uint32), dist=np.array([5, 9, 3, 7], np.uint64),
             side=U.side_run(rng, 12).astype(np.uint16), rec_first=np.array([0, 3, 6, 9, 12], np.uint64))
    # the bin codec's forms: 3 substreams of 61, 41 and 51 records
    recs = [H.random_records(rng, n) for n in (60, 40, 50)]
    A["cdesc"], A["ctotal"] = H.make_desc([len(r) for r in recs], [30, 27, 33], [2, 1, 0], H.SUB_FINISH | H.SUB_ALIGN_RBSP)
    A["crec"] = np.concatenate(recs).astype(np.uint16)
    A["wsync_at"] = np.array([10, 0, 0], np.uint32)
    # two NAL segments of 30 and 25 bytes, one start code in the first
    pay = rng.integers(1, 256, 55).astype(np.uint8)
    pay[10:13] = (0, 0, 1)
    A["nal_pay"], A["nal_off"] = pay, np.array([0, 30, 55], np.uint64)
    # the same blocks with nothing around them, for the sparse parse
    alone = [M.make_unit(rng, ["regular"] * 2, 0, qp=30, at=None, shapes=SHAPES) for _ in range(N_SUB)]
    A["blocks_only"] = dict(M.pack(alone), coeff16=np.concatenate([b.reshape(-1) for u in alone for b in u["blocks"]]).astype(np.int16))
    return A


@pytest.fixture()
def host():
    c = capi.CabacHip(0)
    yield c
    c.close()


def refused(run, message, wrote=(), **kw):
    """The call is refused in these words and has written nothing but the outputs named; -> its outputs"""
    rc, msg, out = run(**kw)
    assert (rc, msg) == (ERR_INVALID, message)
    for k, a in out.items():
        assert k in wrote or clean(a), "a refused call wrote %s" % k
    return out


def waits_of_second_call(host, name, run):
    rc, _, first = run()
    assert rc == 0
    w0 = host.workspace_waits()
    rc, _, out = run()
    delta = host.workspace_waits() - w0
    print("waits:", name, delta)
    assert rc == 0 and all(np.array_equal(first[k], out[k]) for k in out)
    assert delta == WAITS[name], name
    return out


class Dev:
    """Device copies of host arrays, and zeroed device buffers, alive as long as the object"""

    def __init__(self):
        self.keep = []

    def up(self, a):
        if a is None:
            return None
        self.keep.append(dev(a, np.uint8))
        return self.keep[-1].data_ptr()

    def z(self, nbytes, like=None):
        import torch
        t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda") if like is None else dev(like, np.uint8)
        self.keep.append(t)
        return t

    @staticmethod
    def get(t, dtype, n=None):
        a = t.cpu().numpy().view(dtype)
        return a if n is None else a[:n]


def synced(host, rc):
    import torch
    assert rc == 0, last_error(host)
    host.synchronize()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- cabac_hip_estimate_batch
def estimate(host, A, null=None):
    out = dict(bits=S(N_SUB, np.uint64), flags=S(N_SUB, np.uint32))
    q = ptrs(null, desc=A["cdesc"], records=A["crec"], **out)
    rc = host.L.cabac_hip_estimate_batch(host.h, N_SUB, q["desc"], q["records"], len(A["crec"]), q["bits"], q["flags"])
    return rc, last_error(host), out


def test_estimate_batch(host, corpus):
    A = corpus
    refused(lambda: estimate(host, A, null="bits"), "null")
    refused(lambda: estimate(host, edit(A, "cdesc", 1, 1000, "n_records")), "records out of range")
    refused(lambda: estimate(host, edit(A, "cdesc", 1, A["cdesc"]["init_id"][1] | 3, "init_id")), "init_id must be 0..2")
    both = edit(edit(A, "cdesc", 2, 1000, "n_records"), "cdesc", 0, A["cdesc"]["init_id"][0] | 3, "init_id")
    refused(lambda: estimate(host, both), "init_id must be 0..2")          # the lower substream wins
    out = waits_of_second_call(host, "estimate", lambda: estimate(host, A))
    import torch
    D = Dev()
    bits, flags = D.z(8 * N_SUB), D.z(4 * N_SUB)
    torch.cuda.synchronize()
    synced(host, host.L.cabac_hip_estimate_device(host.h, N_SUB, D.up(A["cdesc"]), D.up(A["crec"]), bits.data_ptr(), flags.data_ptr()))
    assert np.array_equal(out["bits"], D.get(bits, np.uint64)) and np.array_equal(out["flags"], D.get(flags, np.uint32)) and not out["flags"].any()


# ---------------------------------------------------------------------------------------------- cabac_hip_residual_batch
def residual(host, A, null=None, cap=CAP, n_coeff=None):
    out = dict(offsets=S(N_TU + 1, np.uint64), info=S(N_TU, np.uint32), records=S(cap, np.uint16))
    q = ptrs(null, tus=A["tus"], coeff=A["coeff"], **out)
    rc = host.L.cabac_hip_residual_batch(host.h, N_TU, q["tus"], q["coeff"], len(A["coeff"]) if n_coeff is None else n_coeff, q["offsets"],
                                         q["info"], q["records"], cap)
    return rc, last_error(host), out


def test_residual_batch(host, corpus):
    A = corpus
    refused(lambda: residual(host, A, null="offsets"), "null")
    out = refused(lambda: residual(host, A, n_coeff=len(A["coeff"]) - 1), "coefficients out of range", wrote=("offsets",))
    assert out["offsets"][0] == 0 and clean(out["offsets"][1:])            # offsets[0] is written before anything is looked at
    out = waits_of_second_call(host, "residual", lambda: residual(host, A))
    n_rec = int(out["offsets"][N_TU])
    assert n_rec > 0 and clean(out["records"][n_rec:]) and not (out["info"] & (H.TU_INFO_EMPTY | H.TU_INFO_BAD_DESC)).any()
    short = refused(lambda: residual(host, A, cap=n_rec - 1), "records_capacity too small", wrote=("offsets", "info"))
    assert np.array_equal(short["offsets"], out["offsets"]) and np.array_equal(short["info"], out["info"])
    import torch
    D = Dev()
    cnt, info, rec = D.z(4 * N_TU), D.z(4 * N_TU), D.z(2 * n_rec)
    d_tu, d_co, d_off = D.up(A["tus"]), D.up(A["coeff"]), D.up(out["offsets"])
    torch.cuda.synchronize()
    synced(host, host.L.cabac_hip_residual_device(host.h, N_TU, d_tu, d_co, d_off, cnt.data_ptr(), info.data_ptr(), rec.data_ptr()))
    assert np.array_equal(np.diff(out["offsets"]), D.get(cnt, np.uint32)) and np.array_equal(out["info"], D.get(info, np.uint32))
    assert np.array_equal(out["records"][:n_rec], D.get(rec, np.uint16))


# ---------------------------------------------------------------------------------------------- the spliced encode
def splice(host, A, kind="plain", null=None, coeff_bytes=4, cap=CAP, n_tu=N_TU):
    L, h = host.L, host.h
    out = dict(payload=S(cap, np.uint8), offsets=S(N_SUB + 1, np.uint64), res=S(N_SUB, capi.RESULT_DTYPE), info=S(N_TU, np.uint32),
               counts=S(N_SUB * capi.BIN_COUNT_WORDS, np.uint32), bits=S(len(A["probe_at"]), np.uint32))
    coeff = A["coeff16"] if coeff_bytes == 2 else A["coeff"]
    q = ptrs(null, desc=A["desc"], records=A["records"], first=A["splice_first"], splices=A["splices"], tus=A["tus"], coeff=coeff,
             level_first=A["level_first"], sync_from=A["sync_from"], sync_at=A["sync_at"], probe_first=A["probe_first"],
             probe_at=A["probe_at"], ent_first=A["ent_first"], entries=A["entries"], **out)
    head = (h, N_SUB, q["desc"], q["records"], len(A["records"]), q["first"], q["splices"], n_tu, q["tus"])
    tail = (q["payload"], cap, q["offsets"], q["res"], q["info"], q["counts"])
    if kind == "plain":
        rc = L.cabac_hip_encode_batch_residual(*head, q["coeff"], len(coeff), *tail)
    elif kind == "sparse":
        rc = L.cabac_hip_sparse_encode_batch(*head, q["ent_first"], q["entries"], len(A["entries"]), len(coeff), *tail)
    elif kind == "rows":
        rc = L.cabac_hip_encode_residual_rows_batch(*head, q["coeff"], coeff_bytes, len(coeff), *tail, len(A["level_first"]) - 1,
                                                    q["level_first"], q["sync_from"], q["sync_at"], None)
    else:
        rc = L.cabac_hip_encode_residual_probes_batch(*head, q["coeff"], coeff_bytes, len(coeff), *tail, q["probe_first"], q["probe_at"],
                                                      None, len(A["probe_at"]), q["bits"])
    if kind != "probes":
        assert clean(out.pop("bits"))
    return rc, last_error(host), out


def offsets0_alone(out):
    return out["offsets"][0] == 0 and clean(out["offsets"][1:])


@pytest.mark.parametrize("kind", ["plain", "rows", "probes", "sparse"])
def test_splice_refusals(host, corpus, kind):
    A = corpus
    # the plain and the probe form write payload_offsets[0] once the pointers, coeff_bytes and the probe list are through
    early = ("offsets",) if kind in ("plain", "probes") else ()
    pre = "substream %u: " if kind == "rows" else "%.0s"

    def run(B=A, **kw):
        return lambda: splice(host, B, kind, **kw)

    def late(B, message, **kw):
        out = refused(run(B, **kw), message, wrote=early)
        assert not early or offsets0_alone(out)
    refused(run(null="offsets"), "null")
    refused(run(null="splices"), "null")
    if kind in ("rows", "probes"):
        refused(run(coeff_bytes=3), "coeff_bytes must be 4 or 2")
    bad_rec = edit(A, "desc", 1, 1000, "n_records")
    bad_init = edit(A, "desc", 1, A["desc"]["init_id"][1] | 3, "init_id")
    late(bad_rec, (pre % 1) + "records out of range")
    late(bad_init, (pre % 1) + "init_id must be 0..2")
    late(edit(A, "splice_first", 0, 3), (pre % 0) + "splice_first must not decrease")
    late(edit(A, "splice_first", N_SUB, N_TU - 1), "every block must be spliced exactly once")
    late(edit(A, "tus", N_TU - 1, len(A["coeff"]), "coeff_offset"), "coefficients out of range")      # the check on the device
    late(edit(bad_rec, "desc", 0, A["desc"]["init_id"][0] | 3, "init_id"), (pre % 0) + "init_id must be 0..2")
    late(edit(bad_rec, "splice_first", N_SUB, N_TU - 1), (pre % 1) + "records out of range")
    if kind == "rows":
        levels = changed(A, level_first=np.array([0, 1, 2], np.uint32))
        refused(run(levels), "level_first must run from 0 to n_sub")
        refused(run(changed(A, level_first=np.array([0, 2, 1, 3], np.uint32))), "level_first decreases at level 2")
        refused(run(edit(A, "sync_from", 2, 2)), "substream 2 (level 1) links to 2 in the same or a later level")
        refused(run(edit(A, "sync_from", 2, 7)), "substream 2 links to 7, beyond the batch")
        refused(run(changed(bad_rec, level_first=np.array([0, 1, 2], np.uint32))), "level_first must run from 0 to n_sub")
    if kind == "probes":
        refused(run(edit(A, "probe_first", 2, 1)), "substream 1: probe_first must not decrease")
        refused(run(edit(A, "probe_at", 1, 1)), "substream 0: probe positions go backwards")
        refused(run(edit(A, "probe_first", 2, 1), coeff_bytes=3), "coeff_bytes must be 4 or 2")
        refused(run(edit(bad_rec, "probe_first", 2, 1)), "substream 1: probe_first must not decrease")
    if kind == "sparse":
        refused(run(null="ent_first"), "null")
        refused(run(edit(A, "ent_first", 2, int(A["ent_first"][3]) + 1)), "block 2: ent_first descends")
        refused(run(edit(bad_rec, "ent_first", 2, int(A["ent_first"][3]) + 1)), "records out of range")
    rc, _, out = splice(host, A, kind, coeff_bytes=2 if kind == "sparse" else 4)
    assert rc == 0
    late(A, "payload_capacity too small", cap=int(out["offsets"][N_SUB]) - 1)
    rc, _, again = splice(host, A, kind, coeff_bytes=2 if kind == "sparse" else 4)
    assert rc == 0 and all(np.array_equal(out[k], again[k]) for k in out)


@pytest.mark.parametrize("kind", ["plain", "rows", "probes", "sparse"])
def test_splice_valid_call_is_the_device_call(host, corpus, kind):
    import torch
    A, L, h = corpus, host.L, host.h
    cb = 2 if kind == "sparse" else 4
    out = waits_of_second_call(host, "splice " + kind, lambda: splice(host, A, kind, coeff_bytes=cb))
    assert not out["res"]["flags"].any() and out["offsets"][0] == 0
    D = Dev()
    pay, off, res, info = D.z(CAP), D.z(8 * (N_SUB + 1)), D.z(8 * N_SUB), D.z(4 * N_TU)
    cnt, bits = D.z(4 * N_SUB * capi.BIN_COUNT_WORDS), D.z(4 * len(A["probe_at"]))
    head = (h, N_SUB, D.up(A["desc"]), D.up(A["records"]), D.up(A["splice_first"]), D.up(A["splices"]), N_TU, N_TU, D.up(A["tus"]),
            D.up(A["coeff16"] if cb == 2 else A["coeff"]))
    tail = (pay.data_ptr(), CAP, off.data_ptr(), res.data_ptr(), info.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    if kind == "plain":
        rc = L.cabac_hip_encode_residual_device(*head, *tail)
    elif kind == "sparse":
        rc = L.cabac_hip_encode_residual16_device(*head, *tail)
    elif kind == "rows":
        rc = L.cabac_hip_encode_residual_rows_device(*head, cb, *tail, len(A["level_first"]) - 1, p(A["level_first"]), D.up(A["sync_from"]),
                                                     D.up(A["sync_at"]), None)
    else:
        rc = L.cabac_hip_encode_residual_probes_device(*head, cb, *tail, D.up(A["probe_first"]), D.up(A["probe_at"]), None,
                                                       len(A["probe_at"]), bits.data_ptr())
    synced(host, rc)
    n_pay = int(out["offsets"][N_SUB])
    assert np.array_equal(out["offsets"], D.get(off, np.uint64)) and np.array_equal(out["res"], D.get(res, capi.RESULT_DTYPE))
    assert n_pay > 0 and np.array_equal(out["payload"][:n_pay], D.get(pay, np.uint8, n_pay)) and clean(out["payload"][n_pay:])
    assert np.array_equal(out["info"], D.get(info, np.uint32)) and np.array_equal(out["counts"], D.get(cnt, np.uint32))
    if kind == "probes":
        assert np.array_equal(out["bits"], D.get(bits, np.uint32))


# ---------------------------------------------------------------------------------------------- the plan write
def write_plan(host, A, rows=False, null=None, coeff_bytes=4, cap=CAP):
    L, h = host.L, host.h
    n_el = len(A["plan"])
    out = dict(payload=S(cap, np.uint8), offsets=S(N_SUB + 1, np.uint64), res=S(N_SUB, capi.RESULT_DTYPE), values=S(n_el, np.uint32),
               info=S(N_TU, np.uint32))
    q = ptrs(null, desc=A["pdesc"], plan=A["plan"], values_in=A["values_in"], tile_first=A["tile_first"], tus=A["tus"], tu_at=A["ptu_at"],
             coeff=A["coeff"], level_first=A["level_first"], sync_from=A["sync_from"], sync_at=A["sync_at"], **out)
    args = (h, N_SUB, q["desc"], q["plan"], q["values_in"], n_el, q["tile_first"], q["tus"], q["tu_at"], None, q["coeff"], coeff_bytes,
            len(A["coeff"]), q["payload"], cap, q["offsets"], q["res"], q["values"], q["info"])
    if rows:
        rc = L.cabac_hip_plan_write_rows_batch(*args, len(A["level_first"]) - 1, q["level_first"], q["sync_from"], q["sync_at"])
    else:
        rc = L.cabac_hip_write_plan_batch(*args)
    return rc, last_error(host), out


@pytest.mark.parametrize("rows", [False, True])
def test_write_plan_refusals(host, corpus, rows):
    A = corpus

    def run(B=A, **kw):
        return lambda: write_plan(host, B, rows, **kw)
    refused(run(null="offsets"), "null")
    refused(run(null="values_in"), "null")
    refused(run(coeff_bytes=3), "coeff_bytes must be 4 or 2")
    bad_first = edit(A, "tile_first", 0, 3)
    refused(run(bad_first), "tile_first must not decrease")
    refused(run(edit(A, "pdesc", 1, A["pdesc"]["init_id"][1] | 3, "init_id")), "init_id must be 0..2")
    refused(run(edit(A, "pdesc", N_SUB - 1, 8, "n_records")), "a plan leaves n_elements_total")
    refused(run(edit(A, "plan", (9, 0), 0xF)), "bad plan entry: substream 1, element 2 of its plan (word0 0xf, word1 0x0): kind above 10")
    bad_coeff = edit(A, "tus", N_TU - 1, len(A["coeff"]), "coeff_offset")
    refused(run(bad_coeff), "coefficients out of range")
    refused(run(edit(bad_coeff, "tile_first", 0, 3)), "tile_first must not decrease")
    refused(run(bad_first, coeff_bytes=3), "coeff_bytes must be 4 or 2")
    if rows:
        levels = np.array([0, 1, 2], np.uint32)
        refused(run(changed(A, level_first=levels)), "level_first must run from 0 to n_sub")
        refused(run(edit(A, "sync_from", 2, 2)), "substream 2 (level 1) links to 2 in the same or a later level")
        refused(run(changed(bad_coeff, level_first=levels)), "coefficients out of range")      # the plan's checks come first
    rc, _, out = write_plan(host, A, rows)
    assert rc == 0
    refused(run(cap=int(out["offsets"][N_SUB]) - 1), "payload_capacity too small")


@pytest.mark.parametrize("rows", [False, True])
def test_write_plan_valid_call_is_the_device_call(host, corpus, rows):
    import torch
    A, L, h = corpus, host.L, host.h
    out = waits_of_second_call(host, "write rows" if rows else "write plan", lambda: write_plan(host, A, rows))
    assert not out["res"]["flags"].any() and out["offsets"][0] == 0
    D = Dev()
    pay, off, res, info = D.z(CAP), D.z(8 * (N_SUB + 1)), D.z(8 * N_SUB), D.z(4 * N_TU)
    values = D.z(0, like=A["values_in"])
    args = (h, N_SUB, D.up(A["pdesc"]), D.up(A["plan"]), D.up(A["values_in"]), D.up(A["tile_first"]), N_TU, D.up(A["tus"]), D.up(A["ptu_at"]),
            None, D.up(A["coeff"]), 4, pay.data_ptr(), CAP, off.data_ptr(), res.data_ptr(), values.data_ptr(), info.data_ptr())
    torch.cuda.synchronize()
    if rows:
        rc = L.cabac_hip_plan_write_rows_device(*args, len(A["level_first"]) - 1, p(A["level_first"]), D.up(A["sync_from"]), D.up(A["sync_at"]))
    else:
        rc = L.cabac_hip_write_plan_device(*args)
    synced(host, rc)
    n_pay = int(out["offsets"][N_SUB])
    assert np.array_equal(out["offsets"], D.get(off, np.uint64)) and np.array_equal(out["res"], D.get(res, capi.RESULT_DTYPE))
    assert n_pay > 0 and np.array_equal(out["payload"][:n_pay], D.get(pay, np.uint8, n_pay)) and clean(out["payload"][n_pay:])
    assert np.array_equal(out["info"], D.get(info, np.uint32)) and np.array_equal(out["values"], D.get(values, np.uint32))


# ---------------------------------------------------------------------------------------------- cabac_hip_estimate_residual_batch
def estimate_residual(host, A, null=None, coeff_bytes=4, n_coeff=None):
    out = dict(bits=S(N_CAND, np.uint64), tu_bits=S(N_TU, np.uint64), info=S(N_TU, np.uint32))
    q = ptrs(null, cand_first=A["cand_first"], tus=A["ctus"], coeff=A["ccoeff"], state=A["state"], rate=A["rate"], set=A["set"], **out)
    rc = host.L.cabac_hip_estimate_residual_batch(host.h, N_CAND, q["cand_first"], q["tus"], q["coeff"], coeff_bytes,
                                                  len(A["ccoeff"]) if n_coeff is None else n_coeff, q["state"], q["rate"], 2, q["set"],
                                                  q["bits"], q["tu_bits"], q["info"])
    return rc, last_error(host), out


def test_estimate_residual_batch(host, corpus):
    A = corpus

    def run(B=A, **kw):
        return lambda: estimate_residual(host, B, **kw)
    refused(run(null="set"), "null")
    refused(run(null="tus"), "null")
    refused(run(coeff_bytes=3), "coeff_bytes must be 4 or 2")
    bad_first = edit(A, "cand_first", 2, 1)
    refused(run(bad_first), "cand_first is not non-decreasing")
    refused(run(edit(A, "set", 3, 2)), "set out of range")
    refused(run(n_coeff=len(A["ccoeff"]) - 1), "coefficients out of range")
    refused(run(edit(bad_first, "set", 0, 2)), "set out of range")                 # candidate by candidate: the lower one wins
    refused(run(edit(bad_first, "set", 3, 2)), "cand_first is not non-decreasing")
    refused(run(bad_first, n_coeff=0), "cand_first is not non-decreasing")
    out = waits_of_second_call(host, "estimate residual", run())
    import torch
    D = Dev()
    bits, tu_bits, info = D.z(8 * N_CAND), D.z(8 * N_TU), D.z(4 * N_TU)
    args = (host.h, N_CAND, D.up(A["cand_first"]), D.up(A["ctus"]), D.up(A["ccoeff"]), D.up(A["state"]), D.up(A["rate"]), D.up(A["set"]),
            bits.data_ptr(), tu_bits.data_ptr(), info.data_ptr())
    torch.cuda.synchronize()
    synced(host, host.L.cabac_hip_estimate_residual_device(*args))
    assert np.array_equal(out["bits"], D.get(bits, np.uint64)) and out["bits"].all()
    assert np.array_equal(out["tu_bits"], D.get(tu_bits, np.uint64)) and np.array_equal(out["info"], D.get(info, np.uint32))


# ---------------------------------------------------------------------------------------------- the search rounds
def search(host, A, kind="plain", null=None, coeff_bytes=4, n_coeff=None):
    L, h = host.L, host.h
    n_ent = len(A["cplan"])
    out = dict(bits=S(N_CAND, np.uint64), pick=S(N_GROUP, np.uint32), cost=S(N_GROUP, np.uint64), tu_bits=S(N_TU, np.uint64),
               info=S(N_TU, np.uint32), flags=S(N_CAND, np.uint32), values=S(n_ent, np.uint32))
    state, rate = A["state"].copy(), A["rate"].copy()
    q = ptrs(null, group_first=A["group_first"], cand_first=A["cand_first"], tus=A["ctus"], coeff=A["ccoeff"], state=state, rate=rate,
             set=A["set"], out_set=A["out_set"], dist=A["dist"], side=A["side"], rec_first=A["rec_first"], tu_at=A["ctu_at"],
             plan=A["cplan"], values_in=A["cvalues"], ent_first=A["ent64"], **out)
    head = (h, N_GROUP, q["group_first"], N_CAND, q["cand_first"], q["tus"], q["coeff"], coeff_bytes,
            len(A["ccoeff"]) if n_coeff is None else n_coeff, q["state"], q["rate"], 2, q["set"])
    tail = (q["out_set"], q["dist"], LAMBDA, q["bits"], q["pick"], q["cost"], q["tu_bits"], q["info"])
    if kind == "plain":
        rc = L.cabac_hip_search_round_batch(*head, *tail)
    elif kind == "unit":
        rc = L.cabac_hip_search_unit_round_batch(*head, q["side"], len(A["side"]), q["rec_first"], q["tu_at"], *tail)
    else:
        rc = L.cabac_hip_search_plan_round_batch(*head, q["plan"], q["values_in"], n_ent, q["ent_first"], q["tu_at"], None, *tail,
                                                 q["flags"], q["values"])
    if kind != "plan":
        assert clean(out.pop("flags")) and clean(out.pop("values"))
    out["state"], out["rate"] = state, rate
    return rc, last_error(host), out


def search_refused(host, A, kind, message, **kw):
    rc, msg, out = search(host, A, kind, **kw)
    assert (rc, msg) == (ERR_INVALID, message)
    state, rate = out.pop("state"), out.pop("rate")
    assert np.array_equal(state, A["state"]) and np.array_equal(rate, A["rate"]) and all(clean(a) for a in out.values())


@pytest.mark.parametrize("kind", ["plain", "unit", "plan"])
def test_search_round_refusals(host, corpus, kind):
    A = corpus
    search_refused(host, A, kind, "null", null="group_first")
    search_refused(host, A, kind, "null", null="pick")
    search_refused(host, A, kind, "null", null="tus")
    search_refused(host, A, kind, "coeff_bytes must be 4 or 2", coeff_bytes=3)
    bad_first = edit(A, "cand_first", 2, 1)
    search_refused(host, bad_first, kind, "cand_first is not non-decreasing")
    search_refused(host, edit(A, "set", 3, 2), kind, "set out of range")
    bad_group = edit(A, "group_first", 1, 5)
    search_refused(host, bad_group, kind, "group_first is not non-decreasing")
    search_refused(host, edit(A, "group_first", 2, 3), kind, "group_first[n_group] must be n_cand")
    search_refused(host, A, kind, "coefficients out of range", n_coeff=len(A["ccoeff"]) - 1)
    in_place = edit(A, "set", 2, 0)
    message = "in-place rule: set 0 is the out set of group 0 and the start set of candidate 2 of another group"
    search_refused(host, in_place, kind, message)
    search_refused(host, edit(A, "out_set", 1, 2), kind, "out set out of range")
    search_refused(host, edit(A, "out_set", 1, 0), kind, "two groups name the same out set")
    # the order: candidates, groups, coefficients, the in-place rule, then what the form adds
    search_refused(host, edit(bad_group, "cand_first", 2, 1), kind, "cand_first is not non-decreasing")
    search_refused(host, bad_group, kind, "group_first is not non-decreasing", n_coeff=0)
    search_refused(host, in_place, kind, "coefficients out of range", n_coeff=0)
    if kind == "unit":
        search_refused(host, A, kind, "null", null="rec_first")
        search_refused(host, edit(A, "rec_first", 1, 7), kind, "rec_first is not non-decreasing")
        search_refused(host, edit(A, "rec_first", N_CAND, 13), kind, "rec_first ends past n_records_total")
        search_refused(host, edit(A, "ctu_at", 0, 3), kind, "tu_at decreases inside a candidate")
        bad_side = edit(A, "side", 4, 0x1FC)
        search_refused(host, bad_side, kind, "bad side record: candidate 1, record 1 of its run (id 0x1fc)")
        search_refused(host, edit(bad_side, "set", 2, 0), kind, message)
    if kind == "plan":
        search_refused(host, A, kind, "null", null="ent_first")
        bad_ent = edit(A, "ent64", 1, 7)
        search_refused(host, bad_ent, kind, "ent_first is not non-decreasing")
        search_refused(host, edit(A, "cplan", (4, 0), 0xF), kind,
                       "bad plan entry: candidate 1, element 1 of its plan (word0 0xf, word1 0x0): kind above 10")
        search_refused(host, edit(bad_ent, "set", 2, 0), kind, message)
    rc, _, out = search(host, A, kind)
    assert rc == 0


@pytest.mark.parametrize("kind", ["plain", "unit", "plan"])
def test_search_round_valid_call_is_the_device_call(host, corpus, kind):
    import torch
    A, L, h = corpus, host.L, host.h
    out = waits_of_second_call(host, "search " + kind, lambda: search(host, A, kind))
    assert (out["pick"] != NO_SET).all() and not np.array_equal(out["state"], A["state"])
    D = Dev()
    bits, pick, cost, tu_bits, info = D.z(8 * N_CAND), D.z(4 * N_GROUP), D.z(8 * N_GROUP), D.z(8 * N_TU), D.z(4 * N_TU)
    flags, values = D.z(4 * N_CAND), D.z(0, like=A["cvalues"])
    state, rate = D.z(0, like=A["state"]), D.z(0, like=A["rate"])
    head = (h, N_GROUP, D.up(A["group_first"]), N_CAND, D.up(A["cand_first"]))
    blocks = (D.up(A["ctus"]), D.up(A["ccoeff"]), 4, state.data_ptr(), rate.data_ptr(), D.up(A["set"]))
    tail = (D.up(A["out_set"]), D.up(A["dist"]), LAMBDA, bits.data_ptr(), pick.data_ptr(), cost.data_ptr(), tu_bits.data_ptr(), info.data_ptr())
    torch.cuda.synchronize()
    if kind == "plain":
        rc = L.cabac_hip_search_round_device(*head, *blocks, *tail)
    elif kind == "unit":
        rc = L.cabac_hip_search_unit_round_device(*head, *blocks, D.up(A["rec_first"]), D.up(A["side"]), D.up(A["ctu_at"]), *tail, None)
    else:
        rec_first, rec, at_out, tu_out = D.z(8 * (N_CAND + 1)), D.z(2 * 4096), D.z(4 * N_TU), D.z(A["ctus"].nbytes)
        rc = L.cabac_hip_search_plan_round_device(*head, N_TU, *blocks, D.up(A["ent64"]), D.up(A["cplan"]), D.up(A["cvalues"]),
                                                  D.up(A["ctu_at"]), None, *tail, flags.data_ptr(), rec_first.data_ptr(), rec.data_ptr(),
                                                  4096, at_out.data_ptr(), tu_out.data_ptr(), values.data_ptr(), None)
    synced(host, rc)
    for name, t, dt in (("bits", bits, np.uint64), ("pick", pick, np.uint32), ("cost", cost, np.uint64), ("tu_bits", tu_bits, np.uint64),
                        ("info", info, np.uint32), ("state", state, np.uint32), ("rate", rate, np.uint8)):
        assert np.array_equal(out[name], D.get(t, dt)), name
    if kind == "plan":
        assert np.array_equal(out["flags"], D.get(flags, np.uint32)) and np.array_equal(out["values"], D.get(values, np.uint32))


# ---------------------------------------------------------------------------------------------- emulation prevention
def nal_escape(host, A, null=None, cap=CAP):
    out = dict(nal=S(cap, np.uint8), nal_off=S(3, np.uint64), status=S(1, capi.NAL_STATUS_DTYPE))
    q = ptrs(null, offsets=A["nal_off"], payload=A["nal_pay"], **out)
    rc = host.L.cabac_hip_nal_escape_batch(host.h, 2, q["offsets"], q["payload"], q["nal"], cap, q["nal_off"], q["status"])
    return rc, last_error(host), out


def nal_unescape(host, A, nal, nal_off, null=None, cap=CAP):
    out = dict(payload=S(cap, np.uint8), offsets=S(3, np.uint64), loc=S(16, np.uint32), status=S(1, capi.NAL_STATUS_DTYPE))
    q = ptrs(null, nal_off=nal_off, nal=nal, **out)
    rc = host.L.cabac_hip_nal_unescape_batch(host.h, 2, q["nal_off"], q["nal"], q["payload"], cap, q["offsets"], q["loc"], 16, 0, q["status"])
    return rc, last_error(host), out


def test_nal_escape_and_unescape_batch(host, corpus):
    import torch
    A, L, h = corpus, host.L, host.h
    refused(lambda: nal_escape(host, A, null="status"), "null")
    refused(lambda: nal_escape(host, A, null="payload"), "null")
    refused(lambda: nal_escape(host, edit(A, "nal_off", 0, 1)), "offsets[0] must be 0")
    refused(lambda: nal_escape(host, edit(A, "nal_off", 1, 60)), "offsets are not ascending")
    esc = waits_of_second_call(host, "nal escape", lambda: nal_escape(host, A))
    st = esc["status"][0]
    assert (int(st["out_bytes"]), int(st["n_changed"]), int(st["flags"])) == (56, 1, 0) and esc["nal_off"].tolist() == [0, 31, 56]
    assert esc["nal"][10:14].tolist() == [0, 0, 3, 1] and clean(esc["nal"][56:])
    nal, nal_off = esc["nal"][:56].copy(), esc["nal_off"]
    refused(lambda: nal_unescape(host, A, nal, nal_off, null="offsets"), "null")
    refused(lambda: nal_unescape(host, A, nal, np.array([0, 40, 31], np.uint64)), "offsets are not ascending")
    une = waits_of_second_call(host, "nal unescape", lambda: nal_unescape(host, A, nal, nal_off))
    assert np.array_equal(une["payload"][:55], A["nal_pay"]) and clean(une["payload"][55:]) and une["offsets"].tolist() == [0, 30, 55]
    assert une["loc"][0] == 12 and clean(une["loc"][1:])
    D = Dev()
    d_nal, d_noff, d_st = D.z(CAP), D.z(24), D.z(16)
    cap = min(CAP, int(L.cabac_hip_nal_escape_bound(55)))
    torch.cuda.synchronize()
    synced(host, L.cabac_hip_nal_escape_device(h, 2, D.up(A["nal_off"]), D.up(A["nal_pay"]), 55, d_nal.data_ptr(), cap, d_noff.data_ptr(), d_st.data_ptr()))
    assert np.array_equal(esc["nal"][:56], D.get(d_nal, np.uint8, 56)) and np.array_equal(esc["nal_off"], D.get(d_noff, np.uint64))
    assert np.array_equal(esc["status"], D.get(d_st, capi.NAL_STATUS_DTYPE))
    d_pay, d_off, d_loc = D.z(CAP), D.z(24), D.z(64)
    synced(host, L.cabac_hip_nal_unescape_device(h, 2, d_noff.data_ptr(), d_nal.data_ptr(), 56, d_pay.data_ptr(), 56, d_off.data_ptr(),
                                                 d_loc.data_ptr(), 16, 0, d_st.data_ptr()))
    assert np.array_equal(une["payload"][:55], D.get(d_pay, np.uint8, 55)) and np.array_equal(une["offsets"], D.get(d_off, np.uint64))
    assert une["loc"][0] == D.get(d_loc, np.uint32)[0] and np.array_equal(une["status"], D.get(d_st, capi.NAL_STATUS_DTYPE))


def encode_nal(host, A, null=None, cap=CAP):
    out = dict(nal=S(cap, np.uint8), nal_off=S(N_SUB + 1, np.uint64), res=S(N_SUB, capi.RESULT_DTYPE), status=S(1, capi.NAL_STATUS_DTYPE))
    q = ptrs(null, desc=A["cdesc"], records=A["crec"], **out)
    rc = host.L.cabac_hip_encode_batch_nal(host.h, N_SUB, q["desc"], q["records"], len(A["crec"]), q["nal"], cap, q["nal_off"], q["res"],
                                           q["status"])
    return rc, last_error(host), out


def test_encode_batch_nal(host, corpus):
    import torch
    A, L, h = corpus, host.L, host.h
    refused(lambda: encode_nal(host, A, null="status"), "null")
    refused(lambda: encode_nal(host, A, null="res"), "null")

    def cleared(B, message):                                       # the status and nal_offsets[0] are cleared in front of the checks
        out = refused(lambda: encode_nal(host, B), message, wrote=("status", "nal_off"))
        assert out["status"].tobytes() == bytes(16) and out["nal_off"][0] == 0 and clean(out["nal_off"][1:])
    bad_rec = edit(A, "cdesc", 1, 1000, "n_records")
    cleared(bad_rec, "records out of range")
    cleared(edit(A, "cdesc", 1, A["cdesc"]["init_id"][1] | 3, "init_id"), "init_id must be 0..2")
    cleared(edit(A, "cdesc", 1, 8, "byte_offset"), "byte_offset must be 16-byte aligned")
    cleared(edit(bad_rec, "cdesc", 0, A["cdesc"]["init_id"][0] | 3, "init_id"), "init_id must be 0..2")
    out = waits_of_second_call(host, "encode nal", lambda: encode_nal(host, A))
    n_nal = int(out["status"][0]["out_bytes"])
    assert n_nal == int(out["nal_off"][N_SUB]) > 0 and not out["res"]["flags"].any() and clean(out["nal"][n_nal:])
    short = refused(lambda: encode_nal(host, A, cap=n_nal - 1), "nal_capacity too small (status->out_bytes is the size needed)",
                    wrote=("status", "nal_off", "res"))
    assert int(short["status"][0]["out_bytes"]) == n_nal and np.array_equal(short["nal_off"], out["nal_off"])
    assert np.array_equal(short["res"], out["res"])
    D = Dev()
    total = A["ctotal"]
    d_desc, d_rec = D.up(A["cdesc"]), D.up(A["crec"])
    slots, res, pay, off, nal, noff, st = D.z(total), D.z(8 * N_SUB), D.z(total), D.z(8 * (N_SUB + 1)), D.z(CAP), D.z(8 * (N_SUB + 1)), D.z(16)
    cap = min(CAP, int(L.cabac_hip_nal_escape_bound(total)))
    torch.cuda.synchronize()
    assert L.cabac_hip_encode_device(h, N_SUB, d_desc, d_rec, slots.data_ptr(), res.data_ptr()) == 0
    assert L.cabac_hip_assemble_device(h, N_SUB, d_desc, res.data_ptr(), slots.data_ptr(), pay.data_ptr(), total, off.data_ptr()) == 0
    synced(host, L.cabac_hip_nal_escape_device(h, N_SUB, off.data_ptr(), pay.data_ptr(), total, nal.data_ptr(), cap, noff.data_ptr(), st.data_ptr()))
    assert np.array_equal(out["nal"][:n_nal], D.get(nal, np.uint8, n_nal)) and np.array_equal(out["nal_off"], D.get(noff, np.uint64))
    assert np.array_equal(out["res"], D.get(res, capi.RESULT_DTYPE)) and np.array_equal(out["status"], D.get(st, capi.NAL_STATUS_DTYPE))


# ---------------------------------------------------------------------------------------------- the WPP forms
def wpp(host, A, decode=False, data=None, null=None):
    L, h = host.L, host.h
    total, n_rec = A["ctotal"], len(A["crec"])
    out = dict(res=S(N_SUB, capi.RESULT_DTYPE))
    out.update(bins=S(n_rec, np.uint8)) if decode else out.update(bytes=S(total, np.uint8))
    q = ptrs(null, desc=A["cdesc"], records=A["crec"], data=data, level_first=A["level_first"], sync_from=A["sync_from"],
             sync_at=A["wsync_at"], **out)
    rows = (len(A["level_first"]) - 1, q["level_first"], q["sync_from"], q["sync_at"])
    if decode:
        rc = L.cabac_hip_decode_wpp_batch(h, N_SUB, q["desc"], q["records"], n_rec, q["data"], total, q["bins"], q["res"], *rows)
    else:
        rc = L.cabac_hip_encode_wpp_batch(h, N_SUB, q["desc"], q["records"], n_rec, q["bytes"], total, q["res"], *rows)
    return rc, last_error(host), out


def test_wpp_batch(host, corpus):
    import torch
    A, L, h = corpus, host.L, host.h
    enc = waits_of_second_call(host, "wpp encode", lambda: wpp(host, A))
    assert not enc["res"]["flags"].any()
    data = enc["bytes"]
    for decode in (False, True):
        def run(B=A, **kw):
            return lambda: wpp(host, B, decode, data, **kw)
        refused(run(null="sync_at"), "null")
        refused(run(null="res"), "null")
        bad_rec = edit(A, "cdesc", 1, 1000, "n_records")
        refused(run(bad_rec), "records out of range")
        refused(run(edit(A, "cdesc", 1, A["cdesc"]["init_id"][1] | 3, "init_id")), "init_id must be 0..2")
        refused(run(edit(A, "cdesc", 2, 1 << 20, "byte_capacity")), "bytes out of range")
        refused(run(changed(A, level_first=np.array([0, 1, 2], np.uint32))), "level_first must run from 0 to n_sub")
        refused(run(edit(A, "sync_from", 2, 2)), "substream 2 (level 1) links to 2 in the same or a later level")
        refused(run(changed(bad_rec, level_first=np.array([0, 1, 2], np.uint32))), "records out of range")
    dec = waits_of_second_call(host, "wpp decode", lambda: wpp(host, A, True, data))
    assert not dec["res"]["flags"].any() and np.array_equal(dec["bins"], (A["crec"] >> 15).astype(np.uint8))
    D = Dev()
    total = A["ctotal"]
    d_desc, d_rec, d_from, d_at = D.up(A["cdesc"]), D.up(A["crec"]), D.up(A["sync_from"]), D.up(A["wsync_at"])
    slots, res, bins, res2 = D.z(total + 4), D.z(8 * N_SUB), D.z(len(A["crec"]) + 8), D.z(8 * N_SUB)
    rows = (len(A["level_first"]) - 1, p(A["level_first"]), d_from, d_at)
    torch.cuda.synchronize()
    synced(host, L.cabac_hip_encode_wpp_device(h, N_SUB, d_desc, d_rec, slots.data_ptr(), res.data_ptr(), *rows))
    assert np.array_equal(enc["bytes"], D.get(slots, np.uint8, total)) and np.array_equal(enc["res"], D.get(res, capi.RESULT_DTYPE))
    synced(host, L.cabac_hip_decode_wpp_device(h, N_SUB, d_desc, d_rec, slots.data_ptr(), bins.data_ptr(), res2.data_ptr(), *rows))
    assert np.array_equal(dec["bins"], D.get(bins, np.uint8, len(A["crec"]))) and np.array_equal(dec["res"], D.get(res2, capi.RESULT_DTYPE))


# ---------------------------------------------------------------------------------------------- the probe forms
def probes(host, A, estimate=False, null=None, start_set=None):
    L, h = host.L, host.h
    n_probe = len(A["probe_at"])
    out = dict(values=S(n_probe, np.uint64 if estimate else np.uint32), flags=S(N_SUB, np.uint32))
    q = ptrs(null, desc=A["cdesc"], records=A["crec"], probe_first=A["probe_first"], probe_at=A["probe_at"], state=A["state"], rate=A["rate"],
             start_set=start_set, **out)
    fn = L.cabac_hip_estimate_probes_batch if estimate else L.cabac_hip_written_bits_batch
    sets = (2, q["state"], q["rate"], q["start_set"]) if start_set is not None else (0, None, None, None)
    rc = fn(h, N_SUB, q["desc"], q["records"], len(A["crec"]), q["probe_first"], q["probe_at"], n_probe, *sets, q["values"], q["flags"])
    return rc, last_error(host), out


@pytest.mark.parametrize("estimate", [False, True])
def test_probes_batch(host, corpus, estimate):
    import torch
    A, L, h = corpus, host.L, host.h

    def run(B=A, **kw):
        return lambda: probes(host, B, estimate, **kw)
    refused(run(null="values"), "null")
    refused(run(null="probe_first"), "null")
    bad_rec = edit(A, "cdesc", 1, 1000, "n_records")
    refused(run(bad_rec), "records out of range")
    refused(run(edit(A, "cdesc", 1, A["cdesc"]["init_id"][1] | 3, "init_id")), "init_id must be 0..2")
    refused(run(start_set=np.array([0, 2, NO_SET], np.uint32)), "substream 1: start set >= n_sets")
    bad_list = edit(A, "probe_first", 2, 1)
    refused(run(bad_list), "substream 1: probe_first must not decrease")
    refused(run(edit(A, "probe_first", 0, 1)), "probe_first must start at 0")
    refused(run(edit(A, "probe_at", 1, 1)), "substream 0: probe positions go backwards")
    refused(run(edit(bad_list, "cdesc", 1, 1000, "n_records")), "records out of range")      # the descriptors come first
    start = np.array([1, NO_SET, 0], np.uint32)
    out = waits_of_second_call(host, "estimate probes" if estimate else "written bits", run(start_set=start))
    assert not out["flags"].any() and not clean(out["values"])
    D = Dev()
    n_probe = len(A["probe_at"])
    values, flags = D.z(8 * n_probe), D.z(4 * N_SUB)
    fn = L.cabac_hip_estimate_probes_device if estimate else L.cabac_hip_written_bits_device
    args = (h, N_SUB, D.up(A["cdesc"]), D.up(A["crec"]), D.up(A["probe_first"]), D.up(A["probe_at"]), n_probe, 2, D.up(A["state"]),
            D.up(A["rate"]), D.up(start), values.data_ptr(), flags.data_ptr())
    torch.cuda.synchronize()
    synced(host, fn(*args))
    assert np.array_equal(out["values"], D.get(values, out["values"].dtype, n_probe)) and np.array_equal(out["flags"], D.get(flags, np.uint32))


# ---------------------------------------------------------------------------------------------- the two parsers' own slots
def parse_unit(host, A):
    n_rec, total = len(A["records"]), len(A["coeff"])
    out = dict(coeff=S(total, np.int32), bins=S(n_rec, np.uint8), info=S(N_TU, np.uint32), res=S(N_SUB, capi.RESULT_DTYPE))
    q = ptrs(None, desc=A["desc"], bytes=A["bytes"], tile_first=A["tile_first"], tus=A["tus"], tu_at=A["tu_at"], records=A["records"], **out)
    rc = host.L.cabac_hip_parse_unit_batch(host.h, N_SUB, q["desc"], q["bytes"], len(A["bytes"]), q["tile_first"], q["tus"], q["tu_at"],
                                           q["records"], n_rec, q["coeff"], 4, total, q["bins"], q["info"], q["res"])
    return rc, last_error(host), out


def test_parse_unit_batch_is_the_device_call(host, corpus):
    import torch
    A = corpus
    out = waits_of_second_call(host, "parse unit", lambda: parse_unit(host, A))
    assert not out["res"]["flags"].any() and np.array_equal(out["coeff"], A["coeff"])
    assert np.array_equal(out["bins"], (A["records"] >> 15).astype(np.uint8))
    D = Dev()
    coeff, bins, info, res = D.z(4 * len(A["coeff"])), D.z(len(A["records"])), D.z(4 * N_TU), D.z(8 * N_SUB)
    args = (host.h, N_SUB, D.up(A["desc"]), D.up(A["bytes"]), D.up(A["tile_first"]), D.up(A["tus"]), D.up(A["tu_at"]), D.up(A["records"]),
            coeff.data_ptr(), 4, bins.data_ptr(), info.data_ptr(), res.data_ptr())
    torch.cuda.synchronize()
    synced(host, host.L.cabac_hip_parse_unit_device(*args))
    assert np.array_equal(out["coeff"], D.get(coeff, np.int32)) and np.array_equal(out["bins"], D.get(bins, np.uint8))
    assert np.array_equal(out["info"], D.get(info, np.uint32)) and np.array_equal(out["res"], D.get(res, capi.RESULT_DTYPE))


def sparse_parse(host, P, cap=None):
    n_coeff = P["total"]
    cap = n_coeff if cap is None else cap
    out = dict(ent_first=S(N_TU + 1, np.uint32), entries=S(max(cap, 1), np.uint32), info=S(N_TU, np.uint32), res=S(N_SUB, capi.RESULT_DTYPE),
               status=S(1, capi.SPARSE_STATUS_DTYPE))
    q = ptrs(None, desc=P["desc"], bytes=P["bytes"], tile_first=P["tile_first"], tus=P["tus"], **out)
    rc = host.L.cabac_hip_sparse_parse_batch(host.h, N_SUB, q["desc"], q["bytes"], len(P["bytes"]), q["tile_first"], q["tus"], q["ent_first"],
                                             q["entries"], cap, n_coeff, q["info"], q["res"], q["status"])
    return rc, last_error(host), out


def test_sparse_parse_batch(host, corpus):
    P = corpus["blocks_only"]
    want_first, want, _ = capi.sparse_pack_host(P["tus"][:N_TU], P["coeff16"])
    out = waits_of_second_call(host, "sparse parse", lambda: sparse_parse(host, P))
    n_ent = len(want)
    assert int(out["status"][0]["n_entries"]) == n_ent > 0 and np.array_equal(out["ent_first"], want_first)
    assert np.array_equal(out["entries"][:n_ent], want) and clean(out["entries"][n_ent:]) and not out["res"]["flags"].any()
    short = refused(lambda: sparse_parse(host, P, cap=n_ent - 1), "entry_capacity too small (status->n_entries is the size needed)",
                    wrote=("ent_first", "info", "res", "status"))
    assert int(short["status"][0]["n_entries"]) == n_ent and np.array_equal(short["ent_first"], out["ent_first"])
