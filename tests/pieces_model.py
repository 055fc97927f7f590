"""The expectation of include/cabac_hip_pieces.h, on the CPU, as compositions of what the oracle already answers
(tests/ctx_sets_model.py: encode_from with the flags for finish() and for the probe, decode_from on prefixes, advance_from for the
sets between pieces) and, for context-free strings, a replay of the emission piece by piece (tests/emit_model.py's Replay, whose
output stage this one inherits): it yields pos, buf and nbuf behind every piece and therefore the exact bytes_final.

A piece hands over every whole 16-bit unit it has: all sixteen places of its last step run their flush checks, so pend < 16
behind a piece, and the next piece starts at place 0 of a step.  Which units are stored, buffered or outstanding behind a piece
therefore depends on where the cuts were (a carry that arrives later lands on the buffered unit); the bytes in the end do not."""
import numpy as np

import ctx_sets_model as M
import emit_model as E
import helpers as H

CODER_FRESH, CODER_ENC, CODER_DEC, CODER_CLOSED = 0, 1, 2, 3
RES_BAD_STATE = 0x80
STICKY = H.RES_OVERFLOW | H.RES_BAD_RECORD | H.RES_UNDERRUN | M.RES_BAD_SET
# events of a run of 0xFFFF units that was handed over from an earlier piece
CROSS_EVENTS = ("carry_run", "ff_extend", "fin_carry_run", "fin_nocarry_run")


def pieces_of(n, cuts):
    """[(first, end)] of the consecutive runs of n records cut at `cuts` (ascending, repeats allowed: empty pieces)."""
    edges = [0] + [int(c) for c in cuts] + [int(n)]
    assert all(a <= b for a, b in zip(edges, edges[1:]))
    return list(zip(edges[:-1], edges[1:]))


def equal_cuts(n, size):
    return list(range(size, n, size))


# ---------------------------------------------------------------------------------------------- what every piece reports
def encode_pieces(rec, cuts, ctx, cap=None, align=True):
    """One substream coded in pieces from the contexts `ctx`: [(n_bits, flags, contexts behind the piece)] per piece and the bytes
    of the whole.  Non-final pieces: what CABAC_SUB_PROBE answers for the records so far; the last: finish()."""
    rec = np.ascontiguousarray(rec, np.uint16)
    out = []
    spans = pieces_of(len(rec), cuts)
    for first, end in spans[:-1]:
        rc, _, nbits, left = M.encode_from(rec[:end], ctx, 4)
        assert rc >= 0
        out.append((nbits, 0, left))
    rc, data, nbits, left = M.encode_from(rec, ctx, 3 if align else 1, cap)
    assert rc >= 0
    out.append((nbits, 0, left))
    return out, data


def decode_pieces(rec, cuts, ctx, data, finish=True):
    """[(n_bits read, flags, contexts behind the piece)] per piece and the bins of the whole: decode_from on the prefixes."""
    rec = np.ascontiguousarray(rec, np.uint16)
    out = []
    spans = pieces_of(len(rec), cuts)
    bins = None
    for k, (first, end) in enumerate(spans):
        last = k == len(spans) - 1
        rc, b, nread, left = M.decode_from(rec[:end], ctx, data, 1 if (last and finish) else 0)
        assert rc in (0, -5)
        out.append((nread, H.RES_BAD_STOP if rc == -5 else 0, left))
        bins = b
    return out, bins


def contexts_between(rec, cuts, ctx):
    """The set every piece starts from: advance_from over the records in front of it."""
    return [M.advance_from(np.ascontiguousarray(rec[:first], np.uint16), ctx) for first, _ in pieces_of(len(rec), cuts)]


# ---------------------------------------------------------------------------------------------- the emission, piece by piece
class PieceReplay(E.Replay):
    """emit_model.Replay continued across pieces (context-free records): feed(piece) runs the piece's steps from place 0 and leaves
    pos / buf / nbuf / pend / low as the kernel's state behind it; finish() is the last piece's.  Events of a run that was
    outstanding when a piece began are also noted as ("cross", event); a run outstanding over two hand-overs as "run3"."""

    def __init__(self, cap=None):      # (not Replay.__init__: that one codes a whole substream)
        self.cap = cap
        self.out = bytearray()
        self.pos = 0
        self.buf, self.nbuf = 0, 0
        self.ev = set()
        self.max_run = 0
        self.max_units = 0
        self.low, self.pend = 0, 0
        self.coder = E.Coder()
        self.handed = 0                 # hand-overs the run outstanding now has been through
        self.n_pieces = 0

    def _flush_lead(self, lead):
        if self.handed and self.nbuf >= 2:      # the run that was outstanding when the piece began is still there
            if lead >> 16:
                self.ev.add(("cross", "carry_run"))
            if lead == 0xFFFF:
                self.ev.add(("cross", "ff_extend"))
        super()._flush_lead(lead)
        if lead != 0xFFFF:
            self.handed = 0

    def feed(self, records):
        n = len(records)
        self.handed = self.handed + 1 if (self.n_pieces and self.nbuf >= 2) else 0
        if self.handed >= 2:
            self.ev.add("run3")
        self.n_pieces += 1
        for base in range(0, n, 16):
            for i in range(16):
                if base + i < n:
                    before = self.coder.low
                    sh = self.coder.put(records[base + i])
                    self.low = (self.low << sh) + (self.coder.low - (before << sh))
                    self.pend += sh
                if i & 3 == 3:
                    while self.pend >= 16:              # quad_flush16, one unit at a time
                        sh = 9 + self.pend - 16
                        lead = self.low >> sh
                        assert lead < (2 << 16)
                        self.low &= (1 << sh) - 1
                        self.pend -= 16
                        self._flush_lead(lead)
        assert self.pend < 16, "a piece leaves no whole unit inside low"
        self.probe_bits = 8 * self.pos + 16 * self.nbuf + self.pend
        self.shifts = self.coder.S
        assert self.probe_bits == self.shifts
        return self

    def finish(self):
        if self.handed and self.nbuf >= 2:      # the run came from an earlier piece
            carry = (self.low >> (9 + self.pend)) & 1
            self.ev.add(("cross", "fin_carry_run" if carry else "fin_nocarry_run"))
        self._finish()
        return self

    def state(self):
        """The documented words of cabac_coder_state behind a non-final piece, and the private ones."""
        return dict(kind=CODER_ENC, flags=0, bits=self.probe_bits, bytes_final=self.pos,
                    priv=(self.low, self.coder.rng | (self.pend << 16), self.buf, self.nbuf))


def replay_pieces(rec, cuts, cap=None, finish=True):
    """-> (PieceReplay behind the last piece, [state behind every non-final piece])."""
    rp = PieceReplay(cap)
    states = []
    spans = pieces_of(len(rec), cuts)
    for k, (first, end) in enumerate(spans):
        rp.feed(rec[first:end])
        if k < len(spans) - 1:
            states.append(rp.state())
    if finish:
        rp.finish()
    return rp, states


def cross_census(cases):
    """{event: [case indices]} over (records, cuts) cases: the CROSS_EVENTS that happen to a run handed over, and "run3"."""
    got = {}
    for k, (rec, cuts) in enumerate(cases):
        rp, _ = replay_pieces(rec, cuts)
        for ev in rp.ev:
            if ev == "run3":
                got.setdefault("run3", []).append(k)
            elif isinstance(ev, tuple):
                got.setdefault(ev[1], []).append(k)
    return got


def overflows_at(rec, cuts, cap):
    """The index of the first piece that reports CABAC_RES_OVERFLOW for a context-free string in a slot of `cap` bytes, or None:
    a non-final piece as soon as bytes_final + 2 * nbuf > cap, the final one when the finished substream does not fit."""
    rp = PieceReplay(cap)
    spans = pieces_of(len(rec), cuts)
    for k, (first, end) in enumerate(spans[:-1]):
        rp.feed(rec[first:end])
        if rp.pos + 2 * rp.nbuf > cap:
            return k
    rp.feed(rec[spans[-1][0]:spans[-1][1]])
    rp.finish()
    return len(spans) - 1 if rp.pos > cap else None
