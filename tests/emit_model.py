"""The encoder's output stage, restated for the tests (no GPU, no HIP): an exact big-integer coder for the records whose
arithmetic needs no context state (bypass, terminate, align), a replay of the emission in 16-bit units as the kernels do it
(csrc/cabac_kernels_v4.hip: the posts of quad_enc_step, quad_flush_lead, quad_list_units' room, quad_put16, quad_enc_finish),
generators that CONSTRUCT carries into 0xFFFF runs, and a composer that lays substreams into slots of arbitrary capacity
with sentinels around them.

The coder.  low = 0, range = 510, S = 0 (shifts so far).  EP b: low = 2 low + b range, one shift.  TRM 0: range -= 2, and
one doubling if that leaves it under 256.  TRM 1: low += range - 2, low <<= 7, range = 256, seven shifts.  ALIGN: range =
256.  low + range <= 2^(9 + S) throughout, so the stream is the (9 + S)-bit value of low, top first; finish() writes its top
S + 1 bits (it drops the eight below them), the stop bit of the byte alignment follows.

Driving at a point.  A boundary P strictly inside [low, low + range) — the next multiple of 2^m above low for the largest
m <= 8 that is inside — and at each bin a record whose sub-interval still holds P (P doubled per shift).  While low < P the
stream is P - 1 followed by ones: 0xFFFF units for as long as the drive goes on.  A record that lands at or above P then
sends a carry through all of them; one that falls below P, or the end of the substream, resolves them without."""
import functools

import numpy as np

import helpers as H

EP0, EP1 = np.uint16(H.REC_EP), np.uint16(H.REC_EP | H.REC_BIN)
TRM0, TRM1 = np.uint16(H.REC_TRM), np.uint16(H.REC_TRM | H.REC_BIN)
ALIGN = np.uint16(H.REC_ALIGN)
FREE = (EP0, EP1, TRM0, TRM1, ALIGN)           # the context-free records
FIN = H.SUB_FINISH | H.SUB_ALIGN_RBSP
PROBE = 0x400                                  # CABAC_SUB_PROBE
SENTINEL = 0xA5
GUARD = 64

# the events of the census
EMISSION_EVENTS = ("carry_nbuf1", "carry_run", "ff_start", "ff_extend", "carry_held", "post2_carry", "step7",
                   "fin_carry_nbuf1", "fin_carry_run", "fin_nocarry_run")
CAPACITY_EVENTS = ("room0", "room-1", "room-2", "overflow_first", "partial_put16")


# ------------------------------------------------------------------ the exact coder
class Coder:
    def __init__(self):
        self.low, self.rng, self.S = 0, 510, 0

    def copy(self):
        c = Coder()
        c.low, c.rng, c.S = self.low, self.rng, self.S
        return c

    def put(self, rec):
        """One record; -> its shift."""
        rid, b = int(rec) & 0x1FF, int(rec) >> 15
        if rid == H.REC_EP:
            self.low = 2 * self.low + b * self.rng
            sh = 1
        elif rid == H.REC_TRM and b:
            self.low = (self.low + self.rng - 2) << 7
            self.rng, sh = 256, 7
        elif rid == H.REC_TRM:
            self.rng -= 2
            sh = 0
            if self.rng < 256:
                self.low, self.rng, sh = 2 * self.low, 2 * self.rng, 1
        elif rid == H.REC_ALIGN:
            self.rng, sh = 256, 0
        else:
            raise ValueError("record %#x needs a context" % int(rec))
        self.S += sh
        assert 256 <= self.rng <= 510 and self.low + self.rng <= 1 << (9 + self.S)
        return sh


def code(records):
    c = Coder()
    for r in records:
        c.put(r)
    return c


def stream_bytes(c):
    """The complete bytes of the (9 + S)-bit value of low, top first."""
    n = (9 + c.S) // 8
    return np.frombuffer((c.low >> ((9 + c.S) - 8 * n)).to_bytes(n, "big"), np.uint8) if n else np.zeros(0, np.uint8)


def finished_bytes(c):
    """(bytes, n_bits) of finish() and the byte alignment: the top S + 1 bits of the value, the stop bit, zero pad."""
    nb = c.S + 2
    n = (nb + 7) // 8
    v = (((c.low >> 8) << 1) | 1) << (8 * n - nb)
    return np.frombuffer(v.to_bytes(n, "big"), np.uint8), 8 * n


# ------------------------------------------------------------------ the emission, as the kernels do it
class Replay:
    """records (context-free) -> the bytes the output stage stores, its final state, and the events it went through.
    cap: the slot's capacity (None: roomy); the bytes are collected without a bound either way, pos counts as the kernels'."""

    def __init__(self, records, cap=None, finish=True):
        self.cap = cap
        self.out = bytearray()
        self.pos = 0
        self.buf, self.nbuf = 0, 0
        self.ev = set()
        self.max_run = 0            # the longest 0xFFFF run a carry went through
        self.max_units = 0
        low, rng_c, pend = 0, Coder(), 0
        n = len(records)
        for base in range(0, n, 16):
            leads = []
            for i in range(16):
                if base + i < n:                       # (bins past the end are no-ops: no shift, nothing added)
                    before = rng_c.low
                    sh = rng_c.put(records[base + i])
                    low = (low << sh) + (rng_c.low - (before << sh))
                    pend += sh
                if i & 3 == 3:                         # the post after bins 3, 7, 11, 15
                    if pend >= 16:
                        keep, nun = pend & 15, pend >> 4
                        assert nun <= 2
                        v = low >> (9 + keep)
                        assert v < (2 << (16 * nun))
                        post = [v >> 16, v & 0xFFFF] if nun == 2 else [v]
                        if nun == 2 and post[0] >> 16:
                            self.ev.add("post2_carry")
                        leads += post
                        low &= (1 << (9 + keep)) - 1
                        pend = keep
                    elif low >> (9 + pend):
                        self.ev.add("carry_held")      # nothing is cut: the carry waits for a whole unit
            m = len(leads)
            assert m <= 8
            self.max_units = max(self.max_units, m)
            if m >= 7:
                self.ev.add("step7")
            if cap is not None and m:
                room = cap - self.pos - 2 * m          # quad_list_units
                if room in (0, -1, -2):
                    self.ev.add("room%d" % room)
            for lead in leads:
                self._flush_lead(lead)
        self.pend, self.low = pend, low
        assert pend < 16
        self.probe_bits = 8 * self.pos + 16 * self.nbuf + pend
        self.shifts = rng_c.S
        if finish:
            self._finish()

    def _put16(self, unit):
        assert 0 <= unit <= 0xFFFF
        if self.cap is not None:
            if self.pos == 0 and self.cap < 2:
                self.ev.add("overflow_first")
            if self.pos == self.cap - 1:
                self.ev.add("partial_put16")
        self.out += bytes([unit >> 8, unit & 0xFF])
        self.pos += 2

    def _put_byte(self, b):
        self.out.append(b)
        self.pos += 1

    def _flush_lead(self, lead):
        carry, is_ff = lead >> 16, lead == 0xFFFF
        if carry:
            assert self.nbuf >= 1
            self.ev.add("carry_nbuf1" if self.nbuf == 1 else "carry_run")
            self.max_run = max(self.max_run, self.nbuf - 1)
        if is_ff:
            assert self.nbuf >= 1          # the first unit of a stream is below 0xFF00: low + range <= 510 / 512
            self.ev.add("ff_start" if self.nbuf == 1 else "ff_extend")
            self.nbuf += 1
            return
        if self.nbuf > 0:
            self._put16(self.buf + carry)
            for _ in range(self.nbuf - 1):
                self._put16((0xFFFF + carry) & 0xFFFF)
        self.buf, self.nbuf = lead & 0xFFFF, 1

    def _finish(self):
        total = 9 + self.pend
        low = self.low
        if (low >> total) & 1:
            self.ev.add("fin_carry_nbuf1" if self.nbuf == 1 else "fin_carry_run")
            self.max_run = max(self.max_run, self.nbuf - 1)
            assert self.nbuf >= 1
            self._put16(self.buf + 1)
            for _ in range(1, self.nbuf):
                self._put16(0)
            low -= 1 << total
        else:
            if self.nbuf >= 2:
                self.ev.add("fin_nocarry_run")
            if self.nbuf > 0:
                self._put16(self.buf)
            for _ in range(1, self.nbuf):
                self._put16(0xFFFF)
        nb = self.pend + 1
        v = low >> 8
        while nb >= 8:
            self._put_byte((v >> (nb - 8)) & 0xFF)
            nb -= 8
        held = ((v & ((1 << nb) - 1)) << (8 - nb)) if nb else 0
        self._put_byte(held | (1 << (7 - nb)))           # the stop bit and the zero pad
        self.n_bits = 8 * self.pos


# ------------------------------------------------------------------ driving at a point
def pick_point(c):
    for m in range(8, -1, -1):
        P = ((c.low >> m) + 1) << m
        if c.low < P < c.low + c.rng:
            return P
    raise AssertionError("low + 1 is always inside")


def _after(c, rec):
    t = c.copy()
    return t, t.put(rec)


def _keeps(c, P, rec):
    t, sh = _after(c, rec)
    return t.low < (P << sh) < t.low + t.rng


def _stuck(c, P, rec):
    t, sh = _after(c, rec)
    return 2 * ((P << sh) - t.low) == t.rng


def drive(c, recs, shifts, menu, rng, away=False):
    """Pick P and keep it strictly inside for at least `shifts` shifts, then until a bypass 1 would cross it (away: until a
    bypass 0 would fall below it), with records of `menu` chosen by `rng`.  A record that does not shift is followed by a
    bypass bin, so the drive always moves.  Ends early where no record keeps P inside (P on the split point: both hold
    then).  -> P, scaled to the present shift count."""
    P, s0, moved = pick_point(c), c.S, True
    for _ in range(shifts * 2 + 400):
        d = P - c.low
        assert 0 < d < c.rng
        if c.S - s0 >= shifts and (2 * d >= c.rng if away else 2 * d <= c.rng):
            return P
        opts = [r for r in (menu if moved else (EP0, EP1)) if _keeps(c, P, r)]
        if not opts:
            assert 2 * d == c.rng                      # the stuck case: bypass 1 crosses, bypass 0 falls away
            return P
        if c.S - s0 < shifts:                          # not into the stuck case before the run is as long as asked, if avoidable
            free = [r for r in opts if not _stuck(c, P, r)]
            opts = free or opts
        r = opts[int(rng.integers(0, len(opts)))]
        sh = c.put(r)
        recs.append(r)
        P <<= sh
        moved = sh > 0
    raise AssertionError("the drive did not come to an end")


def head(f, e, shifts, seed, menu=(EP0, EP1), prefix=(), cross=True, away=False, cross_rec=EP1):
    """f leading TRM 0 (they take a bin slot each and shift nothing while range >= 258), `prefix`, e leading bypass bins, the
    drive, and the crossing (cross) or the fall-away (away) or nothing.  -> (records list, coder)."""
    rng = np.random.default_rng(seed)
    c, recs = Coder(), []
    for r in [TRM0] * f + list(prefix) + [EP1 if rng.integers(0, 2) else EP0 for _ in range(e)]:
        c.put(r)
        recs.append(r)
    P = drive(c, recs, shifts, menu, rng, away=away and not cross)
    if cross:
        sh = c.put(cross_rec)
        recs.append(cross_rec)
        assert c.low >= P << sh                        # the carry: every bit of P - 1 below the boundary flips
    elif away:
        sh = c.put(EP0)
        recs.append(EP0)
        assert c.low + c.rng <= P << sh                # P - 1 and the ones behind it are final
    return recs, c


def free_records(rng, n, trm1=True):
    """n random context-free records."""
    menu = [EP0, EP1, EP0, EP1, TRM0, ALIGN] + ([TRM1] if trm1 else [])
    return [menu[int(k)] for k in rng.integers(0, len(menu), n)]


def _arr(recs):
    return np.array(recs, np.uint16)


# ------------------------------------------------------------------ the families
def family_grid():
    """f x e x K in {1, 3}: the crossing in every lane and post, at every unit phase; every eighth also without the crossing."""
    out = []
    for K in (1, 3):
        for f in range(16):
            for e in range(16):
                seed = 5000 + (K * 16 + f) * 16 + e
                recs, _ = head(f, e, 16 * K + 16, seed)
                tail = free_records(np.random.default_rng(seed + 10000), 6 + (f + e) % 23, trm1=False)
                out.append(("grid/K%d/f%d/e%d" % (K, f, e), _arr(recs + tail + [TRM1])))
                if (f + e) % 8 == 0:
                    recs, _ = head(f, e, 16 * K + 16, seed, cross=False, away=bool(f & 1))
                    out.append(("grid-sibling/K%d/f%d/e%d" % (K, f, e), _arr(recs + (tail + [TRM1] if f & 1 else []))))
    return out


def family_long():
    out = []
    for K in (0, 2, 8, 40, 300):
        recs, _ = head(K % 16, (3 * K) % 16, 16 * K, 6000 + K)
        out.append(("long/K%d" % K, _arr(recs + [EP0, EP1, EP1, TRM1])))
        recs, _ = head(K % 16, (3 * K) % 16, 16 * K, 6000 + K, cross=False)
        out.append(("long-sibling/K%d" % K, _arr(recs)))
    return out


def family_mid():
    """Drives started mid-stream, behind a random context-free prefix; menus with and without TRM 1."""
    out = []
    for t in range(4):
        for name, menu in (("ep", (EP0, EP1, TRM0, ALIGN)), ("trm1", (EP0, EP1, TRM0, TRM1, ALIGN))):
            rng = np.random.default_rng(7000 + t)
            prefix = free_records(rng, 20 + 17 * t)
            recs, _ = head(0, t, 16 * (2 + t), 7100 + t, menu=menu, prefix=prefix)
            out.append(("mid/%s/%d" % (name, t), _arr(recs + free_records(rng, 9, trm1=False) + [TRM1])))
        recs, _ = head(0, t, 16 * (2 + t), 7100 + t, menu=(EP0, EP1, TRM0, ALIGN), prefix=prefix, cross=False, away=True)
        out.append(("mid-sibling/%d" % t, _arr(recs + free_records(rng, 9, trm1=False) + [TRM1])))
    return out


def family_ends():
    """The substream ends 0 .. 15 bins after the crossing: finish() meets the carry inside low, on buf, or on a run."""
    out = []
    for after in range(16):
        recs, _ = head(after % 5, (7 * after) % 16, 16 * (1 + after % 3) + 16, 8000 + after)
        out.append(("ends/%d" % after, _arr(recs + [EP0] * after)))
    return out


def family_trm1():
    """TRM 1 x n: seven 0xFFFF units per 16-bin step.  Two dozen of them, so that they fall on every position of an output wave."""
    out = []
    for k in range(24):
        n = (16, 17, 64)[k % 3]
        lead = k // 3 if n == 64 else 16 * (k // 3 % 2)     # (sixteen TRM 1 of the 16 and the 17 stay in one step)
        out.append(("trm1/%d/%d" % (n, k), _arr([TRM0] * lead + [TRM1] * n)))
    return out


def family_burst():
    """The crossing made by a TRM 1 with more TRM 1 behind it: posts of two units, the carry on top of them."""
    out = []
    for k in range(8):
        recs, _ = head(2 * k, 5 * k % 16, 32, 9500 + k, cross_rec=TRM1)
        out.append(("burst/%d" % k, _arr(recs + [TRM1] * 3 + [EP0, EP1] * k)))
    return out


def family_tails():
    """A crossing followed by ordinary random records, context bins included: the model builds the head, the oracle codes it all."""
    out = []
    for t in range(8):
        recs, _ = head(t, 2 * t, 16 * (1 + t % 4) + 16, 9000 + t)
        tail = H.random_records(np.random.default_rng(9100 + t), 30 + 11 * t)
        out.append(("tails/%d" % t, np.concatenate([_arr(recs), tail]).astype(np.uint16), len(recs)))
    return out


def all_families():
    """[(name, records, n_head)]: n_head records from the front are context-free (all of them but in the tails family)."""
    out = []
    for fam in (family_trm1, family_grid, family_long, family_mid, family_ends, family_burst, family_tails):
        for item in fam():
            out.append(item if len(item) == 3 else (item[0], item[1], len(item[1])))
    return out


def is_free(records):
    ids = np.asarray(records) & 0x1FF
    return bool((ids >= H.REC_ALIGN).all())


def census(recs, caps=None, flags=None):
    """{event: [substreams that reach it]} over the context-free substreams of a batch, each replayed with its capacity; a
    substream under CABAC_SUB_PROBE is replayed without finish()."""
    got = {}
    for s, r in enumerate(recs):
        if not is_free(r):
            continue
        fin = flags is None or not (int(flags[s]) & PROBE)
        rp = Replay(r, None if caps is None else int(caps[s]), finish=fin)
        for ev in rp.ev:
            got.setdefault(ev, []).append(s)
    return got


def format_census(name, cen, events):
    return "%s: " % name + ", ".join("%s %d" % (ev, len(cen.get(ev, ()))) for ev in events)


# ------------------------------------------------------------------ the layout of a batch
def plain_slot(s):
    """Where the plain substreams of a batch stand: every eighth block of sixteen is all plain (whole output waves on the fast
    path in every geometry), and in the other blocks one substream of every four, at a position that moves from block to
    block — a case substream always shares its output wave (four substreams, eight in v7) with plain ones."""
    b = s >> 4
    return b % 8 == 7 or (s & 3) == b % 3


def layout(cases, plain, n_sub=None, filler=None, last=None):
    """Cases into the case slots in order, plain substreams into the plain slots; then filler up to n_sub - 1 and `last` as the
    final substream.  -> (records list, slot of every case)."""
    recs, where, ci, pi = [], [], 0, 0
    while ci < len(cases):
        if plain_slot(len(recs)):
            recs.append(plain[pi])
            pi += 1
        else:
            where.append(len(recs))
            recs.append(cases[ci])
            ci += 1
    if n_sub is not None:
        assert len(recs) < n_sub
        recs += list(filler[:n_sub - 1 - len(recs)]) + [last]
        assert len(recs) == n_sub
    return recs, where


# ------------------------------------------------------------------ the slots
_roomy_cache = {}


def roomy(rec, qp, init_id):
    """The oracle's coding of one substream with room to spare (finish and byte alignment): (bytes, n_bits)."""
    key = (np.asarray(rec, np.uint16).tobytes(), int(qp), int(init_id))
    if key not in _roomy_cache:
        _roomy_cache[key] = H.load_oracle().encode_records(rec, int(qp), int(init_id), 3)
    return _roomy_cache[key]


class Slots:
    """recs laid into slots of the given capacities — NOT rounded — at 16-aligned offsets, GUARD bytes in front, the gap up to
    the next offset behind every slot, at least GUARD behind the last one; everything filled with SENTINEL.
      desc, records, total     the batch
      image, fixed             the expected buffer and which of its bytes are promised: per slot the first min(cap, N) bytes
                               of the roomy coding (N = ceil(n_bits / 8)), the sentinel everywhere outside [offset, offset + cap);
                               slot bytes behind min(cap, N) are open
      results                  n_bits the full count, CABAC_RES_OVERFLOW iff N > cap"""

    def __init__(self, recs, caps, qps, inits, flags=None):
        n = len(recs)
        caps = np.asarray(caps, np.int64)
        assert len(caps) == n and (caps >= 0).all()
        flags = np.full(n, FIN, np.uint32) if flags is None else np.asarray(flags, np.uint32)
        lens = np.array([len(r) for r in recs], np.uint64)
        d = np.zeros(n, H.DESC_DTYPE)
        d["n_records"] = lens
        d["rec_offset"] = np.concatenate([[0], np.cumsum(lens)[:-1]])
        off = np.zeros(n, np.int64)
        at = GUARD
        for s in range(n):
            off[s] = at
            at = (at + int(caps[s]) + 15) // 16 * 16
        d["byte_offset"], d["byte_capacity"] = off, caps
        d["qp"], d["init_id"] = qps, np.asarray(inits, np.uint32) | flags
        self.desc, self.total = d, at + GUARD
        self.records = np.concatenate(recs).astype(np.uint16) if n else np.zeros(0, np.uint16)
        self.caps, self.flags = caps, flags
        self.image = np.full(self.total, SENTINEL, np.uint8)
        self.fixed = np.ones(self.total, bool)
        self.results = np.zeros(n, H.RESULT_DTYPE)
        self.n_bytes = np.zeros(n, np.int64)
        for s in range(n):
            o, cap = int(off[s]), int(caps[s])
            self.fixed[o:o + cap] = False
            if int(flags[s]) & PROBE:              # nothing is flushed, the bytes are unspecified: the count only
                self.results[s]["n_bits"] = H.load_oracle().encode_records(recs[s], int(d["qp"][s]), int(inits[s]), 4)[1]
                continue
            b, n_bits = roomy(recs[s], d["qp"][s], inits[s])
            N = (n_bits + 7) // 8
            assert N == len(b)
            k = min(cap, N)
            self.image[o:o + k] = b[:k]
            self.fixed[o:o + k] = True
            self.results[s]["n_bits"] = n_bits
            self.results[s]["flags"] = H.RES_OVERFLOW if N > cap else 0
            self.n_bytes[s] = N

    def fresh(self):
        return np.full(self.total, SENTINEL, np.uint8)

    def check(self, got_bytes, got_results):
        """got_bytes: the whole buffer after the run; got_results: RESULT_DTYPE."""
        assert len(got_bytes) == self.total
        bad = np.flatnonzero(got_results["flags"] != self.results["flags"])
        assert bad.size == 0, ("flags", bad[:8], got_results["flags"][bad[:8]], self.results["flags"][bad[:8]])
        bad = np.flatnonzero(got_results["n_bits"] != self.results["n_bits"])
        assert bad.size == 0, ("n_bits", bad[:8], got_results["n_bits"][bad[:8]], self.results["n_bits"][bad[:8]])
        diff = np.flatnonzero((got_bytes != self.image) & self.fixed)
        if diff.size:
            at = int(diff[0])
            s = int(np.searchsorted(self.desc["byte_offset"].astype(np.int64), at, side="right")) - 1
            raise AssertionError("byte %d differs (%#x, expected %#x): substream %d at offset %d, capacity %d, %d bytes coded; %d bytes differ"
                                 % (at, got_bytes[at], self.image[at], s, int(self.desc["byte_offset"][max(s, 0)]) if s >= 0 else -1,
                                    int(self.caps[max(s, 0)]), int(self.n_bytes[max(s, 0)]), diff.size))


# ------------------------------------------------------------------ the batches of the tests
SMALL = None          # the batch as the layout leaves it: under 1 024 substreams
POOL = np.arange(H.NUM_CTX)


@functools.lru_cache(None)
def _plain_pool():
    """Ordinary random substreams, context bins included, 40 .. 120 records: several steps each, on the fast path."""
    rng = np.random.default_rng(4400)
    return [H.random_records(rng, int(rng.integers(40, 120))) for _ in range(400)]


@functools.lru_cache(None)
def _filler():
    """What pads a batch to a big geometry: short random substreams, at most 49 records."""
    rng = np.random.default_rng(4401)
    return [H.random_records(rng, int(rng.integers(0, 49))) for _ in range(4200)]


def _qp_init(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(20, 45, n), rng.integers(0, 3, n)


@functools.lru_cache(None)
def carries_batch(n_sub=SMALL):
    """All families in the layout above, roomy ODD capacities (N + 1 and N + 3, N the coded bytes).  n_sub: padded with filler
    to that many substreams, the last one a copy of a grid case (a carry into a run).  -> (Slots, records list, names by substream)."""
    fams = all_families()
    cases = [f[1] for f in fams]
    recs, where = layout(cases, _plain_pool(), n_sub, _filler(), cases[len(cases) // 2])
    assert n_sub is not None or len(recs) < 1024
    names = {s: fams[i][0] for i, s in enumerate(where)}
    qps, inits = _qp_init(len(recs), 4402)
    caps = [len(roomy(r, qps[s], inits[s])[0]) + (1 if s % 2 == 0 else 3) for s, r in enumerate(recs)]
    return Slots(recs, caps, qps, inits), recs, names


def capacity_cases():
    """About a dozen substreams of 20 .. 70 coded bytes."""
    rng = np.random.default_rng(4403)
    out = []
    recs, _ = head(2, 5, 16 * 3 + 16, 4404)                                     # a crossing into a 3-unit run
    out.append(("cross3", _arr(recs + free_records(rng, 120, trm1=False) + [TRM1])))
    recs, _ = head(2, 5, 16 * 3 + 16, 4404, cross=False, away=True)             # its sibling
    out.append(("sibling3", _arr(recs + free_records(rng, 120, trm1=False) + [TRM1])))
    out.append(("trm1x17", _arr([TRM1] * 17 + free_records(rng, 60, trm1=False))))
    out.append(("trm1x64", _arr([TRM1] * 64)))
    recs, _ = head(9, 11, 32, 4405)                                             # a grid member
    out.append(("grid", _arr(recs + free_records(rng, 200, trm1=False) + [TRM1])))
    recs, _ = head(3, 0, 16 * 8, 4406)                                          # the cut falls inside a long run
    out.append(("cross8", _arr(recs + free_records(rng, 90, trm1=False) + [TRM1])))
    recs, _ = head(1, 7, 16 * 11, 4407, cross=False)                            # finish() resolves the run
    out.append(("end-in-run", _arr(recs)))
    recs, _ = head(6, 2, 32, 4408, cross_rec=TRM1)
    out.append(("burst", _arr(recs + [TRM1] * 3 + free_records(rng, 150, trm1=False))))
    out.append(("free-random", _arr(free_records(rng, 260))))
    out.append(("free-random-ep", _arr(free_records(rng, 330, trm1=False))))
    out.append(("random", H.random_records(rng, 180)))                          # context bins: the oracle alone knows them
    out.append(("random-ep", H.random_records(rng, 240, ctx_frac=0.3)))
    return out


@functools.lru_cache(None)
def capacity_batch(n_sub=SMALL):
    """Every case once per capacity 0 .. N + 2.  -> (Slots, records list, names by substream)."""
    recs, caps, names = [], [], {}
    for name, r in capacity_cases():
        N = len(roomy(r, 30, 1)[0])
        assert 20 <= N <= 70, (name, N)
        for cap in range(N + 3):
            names[len(recs)] = "%s/cap%d" % (name, cap)
            recs.append(r)
            caps.append(cap)
    n_case = len(recs)
    assert n_case < 1024
    qps, inits = [30] * n_case, [1] * n_case
    if n_sub is not None:
        fill = _filler()[:n_sub - n_case]
        q2, i2 = _qp_init(len(fill), 4409)
        caps += [len(roomy(r, q2[k], i2[k])[0]) + 1 for k, r in enumerate(fill)]
        recs, qps, inits = recs + fill, qps + list(q2), inits + list(i2)
        assert len(recs) == n_sub
    return Slots(recs, caps, qps, inits), recs, names


@functools.lru_cache(None)
def probe_batch(n_sub=SMALL):
    """The siblings and TRM 1 x n under CABAC_SUB_PROBE (0xFFFF units outstanding when the records end) beside finished
    substreams.  -> (Slots, records list, flags)."""
    cases = [f[1] for f in all_families() if "sibling" in f[0] or f[0].startswith("trm1/")]
    cases = [c for c in cases if Replay(c, finish=False).nbuf >= 2]
    assert len(cases) >= 40
    recs, where = layout(cases, _plain_pool(), n_sub, _filler(), cases[0])
    flags = np.full(len(recs), FIN, np.uint32)
    flags[where] = PROBE
    flags[where[::5]] = FIN                       # some of the cases finished as well
    qps, inits = _qp_init(len(recs), 4410)
    caps = [len(roomy(r, qps[s], inits[s])[0]) + 1 + s % 3 for s, r in enumerate(recs)]
    return Slots(recs, caps, qps, inits, flags), recs, flags
