"""Built edges of the segmented decompress pipeline (lz4_seg_*.hip) for jobs WITH HISTORY — existing output out[0, E) and a prefix
of P bytes — and the host model of its stages for them.  Plain Python and numpy: no GPU, no library.  The builders, the parse and the
history-free model are seg_stage_cases.py's; here:

  * HBlk: a block built sequence by sequence on the virtual stream prefix ++ existing ++ output (decompress.rs:80-99);
  * HLayout / HModel: the model with E and P, from the rule in DESIGN (d) — every position is absolute (a job's first output byte is E), a
    source in out[0, E) is a source like any other (the ring is primed with the history's tail; older: class 7), a source wholly in the prefix
    is class 13 and depends on nothing, a source that starts in the prefix and ends in the output stands alone in its sub-batch (class 8); existing
    output of 65 535 bytes or more hides the prefix;
  * the cases, each named for its edge, and census(): the named edges a model run reaches.  tests/test_seg_history_cases_cpu.py requires
    every edge and compares every case with the oracle; tests/test_gpu_seg_history.py compares the device's stage dumps with the model."""
import functools

import numpy as np

import seg_stage_cases as S
from seg_stage_cases import CHUNK, RESIDUES, RINGS, TILE  # noqa: F401

PREFIX_REACH = 65535                                       # kSegPrefixReach: no offset reaches the prefix from here on
E_LIST = tuple(sorted({1, 15, 16, 17, 4095, 65535, 65536} | {R + d for R in RINGS for d in (-1, 0, 1)} | {3 * R for R in RINGS}))
E_RESIDUES = tuple(4096 + k for k in range(2, 15))         # with E_LIST: every residue of (E + rb) & 15 at rb = 0, and so at any rb
M_AT_EDGE = (4, 19, 64, 65)


def _bytes(seed, n):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


class HBlk(S.Blk):
    """A block whose output continues `existing` behind `prefix`: o holds existing ++ the block's bytes (positions are absolute), offsets may
    reach through out[0 ..] into the prefix's tail."""

    def __init__(self, seed=1, prefix=b"", existing=b""):
        super().__init__(seed)
        self.prefix, self.E = bytes(prefix), len(existing)
        self.o = bytearray(existing)

    def seq(self, L, off, M, fill=None, lit=None):
        lit = self._lits(L, fill) if lit is None else lit
        assert len(lit) == L
        self.o += lit
        reach = len(self.o) + (len(self.prefix) if self.E < PREFIX_REACH else 0)
        assert 1 <= off <= reach and off <= 0xFFFF and M >= 4, (off, M, len(self.o), len(self.prefix))
        self.c += S._seq(lit, off, M)
        P = len(self.prefix)
        for _ in range(M):                                 # copy_overlapping on the virtual stream, byte by byte (the cases are small)
            s = len(self.o) - off
            self.o.append(self.o[s] if s >= 0 else self.prefix[P + s])
        return self

    def raw(self, data, out=b""):
        """Compressed bytes as they are (a damaged sequence), with what they would add to the output."""
        self.c += data; self.o += out
        return self


# ------------------------------------------------------------------------------------------------------------------------------ the model
class HLayout(S.Layout):
    """S.Layout for a job with E bytes of existing output and a prefix of P bytes (P as the kernels see it: 0 from E = 65 535 on)."""

    def __init__(self, n, toks, E=0, P=0):
        self.E, self.Pfx = E, (0 if E >= PREFIX_REACH else P)
        super().__init__(n, toks)

    def _levels(self):
        """Absolute positions first, then the levels: as S.Layout._levels, but a source that starts in the prefix depends on nothing."""
        E, act = self.E, self.act
        self.tile_out = self.tile_out + E
        self.outb += E
        self.lo = np.where(act, self.lo + E, 0); self.mo = np.where(act, self.mo + E, 0); self.endp = np.where(act, self.endp + E, 0)
        has = act & (self.M > 0)
        self.pre = has & (self.off > self.mo) if self.Pfx else np.zeros(self.ntok, bool)
        self.strad = self.pre & (self.off - self.mo < self.M)      # ... and ends in the output
        N = self.ntok
        self.lvl_lo = np.where(has, 1, 0).astype(np.int64); self.lvl_hi = self.lvl_lo.copy()
        self.reads = np.zeros(N, bool); self.ilo = np.zeros(N, np.int64); self.ihi = np.zeros(N, np.int64)
        self.exact = np.ones(self.nbatch, bool)
        if not N:
            return
        b0 = (np.arange(N) // 64) * 64
        ob = self.lo[b0]
        s0 = self.mo - self.off
        e0 = s0 + np.minimum(self.M, self.off)
        aslot = np.nonzero(act)[0]
        ends, mos = self.endp[aslot], self.mo[aslot]
        first = np.searchsorted(aslot, b0)
        a = np.maximum(np.searchsorted(ends, s0, side="right") - first, 0)       # lanes of the batch that end at or before the source
        bb = np.maximum(np.searchsorted(mos, e0, side="left") - first, 0)        # lanes whose match starts before the source's end
        bb = np.minimum(bb, np.arange(N) - b0)
        dep = has & ~self.pre & (e0 > ob) & (bb >= 1) & (a <= bb - 1)
        self.reads, self.ilo, self.ihi = dep, np.where(dep, a, 0), np.where(dep, bb - 1, 0)
        for q in np.nonzero(dep)[0].tolist():
            b = q - q % 64
            i0, i1 = b + int(self.ilo[q]), b + int(self.ihi[q])
            self.lvl_lo[q] = 1 + int(self.lvl_lo[i0:i1 + 1].max())
            self.lvl_hi[q] = 1 + int(self.lvl_hi[b:i1 + 1].max())
            if i1 - i0 > 1:
                self.exact[q // 64] = False

    def records(self, R, rb):
        if not self.Pfx:
            return super().records(R, rb)                  # (absolute positions are all a job without a reachable prefix needs)
        N, span = self.ntok, R // 8
        sub = np.zeros(N, np.int64); giant = np.zeros(N, bool); oe = np.zeros(N, np.int64); sob = np.zeros(N, np.int64)
        for b in range(self.nbatch):
            s, nb = b * 64, int(self.nb[b])
            endp, lo, strad = self.endp[s:s + nb], self.lo[s:s + nb], self.strad[s:s + nb]
            a = sidx = 0
            while a < nb:
                so = int(lo[a])
                e = a + int(np.searchsorted(endp[a:], so + span, side="right"))
                st = np.nonzero(strad[a:e])[0]
                if len(st):                                # a sub-batch ends in front of such a source, and the source is one of its own
                    e = a + int(st[0])
                g = e == a
                if g:
                    e = a + 1
                sub[s + a:s + e] = sidx; giant[s + a:s + e] = g; oe[s + a:s + e] = int(endp[e - 1]); sob[s + a:s + e] = so
                a = e; sidx += 1
            sub[s + nb:s + 64] = sidx - 1
        act, M, off, mo = self.act, self.M, self.off, self.mo
        fpw = ((oe + rb + 15) & ~15) + 3 * span + 64
        lov = np.maximum(fpw - R, 0)
        sy, dy = mo - off + rb, mo + rb
        di, si = dy & (R - 1), sy & (R - 1)
        wrap = (di + M > R) | (si + M > R)
        size = np.where(M < 8, 1, np.where(M <= 16, 2, np.where(M <= 32, 3, 4)))
        rle = (off == 1) | (off == 2) | (off == 4)
        cls = np.where(sy < lov, 7, np.where((M > 64) | wrap, 6, np.where(off < M, np.where(rle, 8 + size, 5), size)))
        cls = np.where(self.pre, 13, cls)
        cls = np.where(giant, 8, np.where(M != 0, cls, 0))
        cls = np.where(act, cls, 0)
        fl = (np.isin(cls, (1, 9)) * 1 | np.isin(cls, (2, 3, 4, 10, 11, 12)) * 2 | np.isin(cls, (3, 4, 11, 12)) * 4 | np.isin(cls, (4, 12)) * 8 |
              np.isin(cls, (5, 6)) * 16 | np.isin(cls, (9, 10, 11, 12)) * 32)
        last = (np.arange(N) // 64) * 64 + np.maximum(np.repeat(self.nb, 64) - 1, 0)
        return dict(sub=sub, cls=cls, fl=fl, giant=giant & act, oe=oe, sob=sob, lov=lov, sy=sy, di=di, si=si, wrap=wrap,
                    w0=np.where(act, M, 0), w1=np.where(act, mo, self.endp[last] if N else 0) + rb, w2_low=sub | (fl << 8), w3=np.where(act, off, 0))


def record_stage_failure(toks, limit, cap, E, P):
    """Does the records stage give the job up (decompress.rs:72-74, :83-89 on prefix ++ output, our buffer)?"""
    o = E
    for _, L, M, off, _ in toks:
        if o > cap or cap - o < L:
            return True
        mo = o + L
        if M and (mo + M > limit or off == 0 or off > mo + P or cap - mo < M):
            return True
        o = mo + M
    return False


class HModel:
    """Everything the stages should hold for one case with history (S.Model's attributes; .P is the parse, as there)."""

    def __init__(self, case):
        c = case["input"]
        self.E, plen = len(case["existing"]), len(case["prefix"])
        self.plen = 0 if self.E >= PREFIX_REACH else plen
        self.P = S.Parse(c)
        self.seam = S.Seam(c, self.P)
        self.toks, self.chain_err = self.P.chain(0)
        self.n = len(c)
        self.nch, self.ntile = S.seg_nch(self.n), S.seg_ntile(self.n)
        limit, cap = case["limit"], case["out_cap"]
        out_total = self.E + sum(t[1] + t[2] for t in self.toks)
        assert not self.seam.failed and not self.chain_err
        self.gives_up = "scan" if out_total > cap else "records" if record_stage_failure(self.toks, limit, cap, self.E, self.plen) else None
        self.layout = HLayout(self.n, self.toks, self.E, plen)


# ------------------------------------------------------------------------------------------------------------------------------ the cases
def _case(name, b, **kw):
    c, o = b.end(kw.pop("tail", 5))
    d = dict(name=name, input=c, output=o, prefix=b.prefix, existing=bytes(o[:b.E]), status=S.OK, limit=max(len(o), 1), out_cap=len(o) + 64)
    d.update(kw)
    return d


def _damaged(name, b, status, gives_up, **kw):
    """A block whose last sequence is the damage (nothing behind it)."""
    d = dict(name=name, input=bytes(b.c), prefix=b.prefix, existing=bytes(b.o[:b.E]), status=status, gives_up=gives_up,
             limit=b.opos + (1 << 16), out_cap=b.opos + (1 << 16) + 64)
    d.update(kw)
    return d


def existing_cases():
    out = []
    spans = [R // 8 for R in RINGS]
    m_cycle = M_AT_EDGE + (spans[-1] + 1,)                 # (larger than a sub-batch under every ring)
    for k, E in enumerate(E_LIST + E_RESIDUES):
        b = HBlk(200 + k, existing=_bytes(1000 + k, E))
        M0 = m_cycle[k % len(m_cycle)]
        b.seq(0, 1, M0)                                    # the first sequence has no literals: the match is at mo = E, its source starts at E - 1
        if E >= 8:
            b.seq(3, b.opos + 3 - E + 8, 8)                # a source that ends exactly at E
        if E >= 5:
            b.seq(2, b.opos + 2 - (E + 1) + 6, 6)          # ... that ends one byte behind E: one byte of the block, five of the history
        b.seq(1, b.opos + 1 - (E - 1), 4)                  # ... that starts at E - 1: one byte of the history, three of the block
        if b.opos + 2 <= 0xFFFF:
            b.seq(2, b.opos + 2, 7)                        # off == mo: the source is byte 0 of `out`
        for far in (20000, 30000, 45000, 60000, 65535):    # history in front of what a ring holds at the block's start, where E reaches that far
            if far <= b.opos + 1:
                b.seq(1, far, 6 + far % 9)
        for _ in range(12):
            b.near(int(b.rng.integers(0, 9)), 4 + int(b.rng.integers(0, 30)), reach=min(E + 40, 0xFFFF))
        out.append(_case(f"existing: E = {E}, first match of {M0} at E from E - 1", b, E_named=E))
    # every M of the edge list right at E for one E (the cycle above spreads them over the E list)
    for M0 in m_cycle:
        b = HBlk(300 + M0 % 97, existing=_bytes(1300 + M0 % 97, 777))
        b.seq(0, 1, M0); b.near(3, 9); b.near(0, 5)
        out.append(_case(f"existing: E = 777, source starts at E - 1 with off = 1, M = {M0}", b))
    # the oldest byte the ring holds for certain lies in the history: under ring R the first four sub-batches of the block each open with a
    # match whose source is at lov (side 0) or lov - 1 (side 1) for one of the residues, and fill their span (seg_stage_cases.class_cases)
    for R in RINGS:
        E, span = 3 * R, R // 8
        b = HBlk(400 + R // 1024, existing=_bytes(1400 + R // 1024, E))
        for rb in RESIDUES:
            for side in (0, 1):
                P0 = b.opos
                lov = ((P0 + span + rb + 15) & ~15) + 3 * span + 64 - R
                off = P0 + rb - lov + side
                assert 1 <= off <= 0xFFFF and P0 - off < E, (R, rb, off)
                b.seq(0, off, 4); b.seq(0, 1, span - 4)
        out.append(_case(f"existing: E = 3 R, sources at the oldest byte the primed ring holds, R = {R}", b, lov_ring=R))
    # a block of literals only
    b = HBlk(501, existing=_bytes(1501, 333))
    out.append(_case("existing: literals only", b, tail=1000))
    # three tiles, two chunks; history sources in the first tile only
    b = HBlk(502, existing=_bytes(1502, 5000))
    for off_back in (1, 17, 4999, 2500):
        b.seq(2, b.opos + 2 - (5000 - off_back), 11)
    b.small_until(CHUNK + 3000)
    out.append(_case("existing: two chunks, history sources in the first tile only", b))
    return out


def prefix_cases():
    out = []
    pre = _bytes(77, 1000)
    b = HBlk(601, prefix=pre)
    b.seq(5, 5 + 600, 40)                                  # wholly in the prefix
    b.seq(3, b.opos + 3 + 9, 9)                            # ... ending at its last byte
    b.seq(1, b.opos + 1 + 1000, 4)                         # off == mo + P: the prefix's first byte
    b.seq(2, b.opos + 2 + 300, 64); b.seq(2, b.opos + 2 + 300, 65); b.seq(0, b.opos + 500, 200)     # own lane at its limit, the whole wave
    b.seq(4, b.opos + 4 + 3, 30)                           # three bytes of the prefix, then out[0 ..]: the same offset goes on
    b.near(2, 8); b.near(0, 5)
    b.seq(1, b.opos + 1 + 2, 4)                            # (another one: two bytes of the prefix, two of the output)
    for _ in range(10):
        b.near(int(b.rng.integers(0, 9)), 4 + int(b.rng.integers(0, 30)))
    out.append(_case("prefix: wholly inside, at its last and first byte, across into the block", b))
    b = HBlk(602, prefix=b"\x5c")
    b.seq(0, 1, 50)                                        # P = 1, off = mo + 1 at mo = 0: the prefix's byte, then its copies
    b.near(3, 6)
    out.append(_case("prefix: one byte that replicates", b))
    b = HBlk(603, prefix=pre)
    b.seq(0, 10, RINGS[-1] // 8 + 300)                     # across into the block AND larger than a sub-batch; overlapping (offset 10)
    b.near(2, 6)
    b.seq(7, b.opos + 7 + 900, RINGS[-1] // 8 + 5)         # larger than a sub-batch: 900 bytes of the prefix, then the output
    b.near(1, 4)
    out.append(_case("prefix: across into the block, larger than a sub-batch", b))
    b = HBlk(604, prefix=_bytes(78, 40000))
    b.seq(6, b.opos + 6 + 40000, RINGS[0] // 8 + 40)        # wholly in the prefix and larger than the smallest ring's sub-batch
    b.near(1, 4)
    out.append(_case("prefix: wholly inside, larger than a sub-batch", b))
    # all three areas: P > 0, 0 < E < M
    b = HBlk(605, prefix=pre, existing=_bytes(79, 10))
    b.seq(0, 10 + 4, 40)                                   # four bytes of the prefix, the ten existing bytes, then the block's own
    b.near(2, 7)
    b.seq(3, b.opos + 3 + 100, 12)                         # wholly in the prefix, from behind existing output
    b.near(1, 5)
    out.append(_case("prefix: a source across prefix, existing output and the block", b))
    # E >= 65 535: the prefix is out of reach
    for E in (65535, 65536):
        b = HBlk(606 + E % 2, prefix=pre, existing=_bytes(80 + E % 2, E))
        b.seq(0, 65535, 9)                                 # the furthest offset at mo = E
        b.near(2, 6)
        out.append(_case(f"prefix: out of reach behind E = {E}, off = 65 535 at mo = E", b))
    return out


def limit_cases():
    out = []
    def base(seed=701):
        b = HBlk(seed, existing=_bytes(1700, 500))
        for _ in range(20):
            b.near(int(b.rng.integers(0, 9)), 4 + int(b.rng.integers(0, 20)), reach=400)
        return b
    b = base(); b.seq(3, 50, 9)
    c = _case("limit: mo + M == output_limit", b, tail=0)
    c["limit"] = len(c["output"])                          # (the last literals are empty: the match ends the output)
    out.append(c)
    b = base(); b.seq(3, 50, 9)
    out.append(_damaged("limit: mo + M == output_limit + 1", b, S.MEMORY_LIMIT_EXCEEDED, "records", limit=b.opos - 1, out_cap=b.opos + 64))
    b = base(); b.raw(S._seq(b"abc", 0xFFFF, 9), b"abc" + bytes(9))
    out.append(_damaged("limit: passed by a match whose offset is bad too (the limit comes first)", b, S.MEMORY_LIMIT_EXCEEDED, "records",
                        limit=b.opos - 1, out_cap=b.opos + 64))
    b = base(); b.seq(3, 50, 9)
    c = _case("limit: out_cap one byte short", b)
    c.update(status=S.OUT_CAPACITY, gives_up="scan", out_cap=len(c["output"]) - 1)
    out.append(c)
    return out


def damaged_cases():
    out = []
    b = HBlk(801, existing=_bytes(1800, 100)); b.near(2, 6, reach=50)
    b.raw(S._seq(b"xy", b.opos + 2 + 1, 5))
    out.append(_damaged("damaged: off == mo + 1 with existing output and no prefix", b, S.INVALID_OFFSET, "records"))
    b = HBlk(802, existing=_bytes(1801, 100)); b.near(2, 6, reach=50)
    b.raw(S._seq(b"xy", 0, 5))
    out.append(_damaged("damaged: off == 0 with existing output", b, S.ZERO_OFFSET, "records"))
    b = HBlk(803, prefix=_bytes(81, 64)); b.seq(4, 4 + 20, 6)
    b.raw(S._seq(b"xy", b.opos + 2 + 64 + 1, 5))
    out.append(_damaged("damaged: off == mo + P + 1", b, S.INVALID_OFFSET, "records"))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = existing_cases() + prefix_cases() + limit_cases() + damaged_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def models():
    return tuple(HModel(c) for c in all_cases())


# ------------------------------------------------------------------------------------------------------------------------------ the census
def free_edges():
    e = {f"E = {E}" for E in E_LIST}
    e |= {f"off = 1 from E - 1, M = {M}" for M in M_AT_EDGE} | {"off = 1 from E - 1, larger than a sub-batch"}
    e |= {"source ends at E", "source ends one byte behind E", "source starts at E - 1", "first sequence without literals: match at E",
          "off == mo with existing output", "literals only behind existing output", "two chunks, history sources in the first tile only",
          "source wholly in the prefix", "source ends at the prefix's last byte", "off == mo + P", "one prefix byte that replicates",
          "prefix then block with the same offset", "source across prefix, existing output and the block", "prefix out of reach: off = 65535 at mo = E",
          "prefix source larger than a sub-batch", "mo + M == output_limit", "limit + 1", "limit first", "out_cap one byte short",
          "off == mo + 1 invalid", "off == 0", "off == mo + P + 1 invalid", "a level above 1 behind a prefix source"}
    return e


def ring_edges(R):
    e = {f"(E + rb) & 15 = {k}" for k in range(16)} | {"class 13", "class 8 from the prefix", "history source inside the ring", "history source at lov",
                                                          "history source at lov - 1", "history source across E inside the ring", "history source of class 7"}
    return e


def census_free(case, m):
    got = set()
    ly, E, P = m.layout, m.E, m.plen
    q = np.nonzero(ly.act)[0]
    L, M, off, mo = ly.L[q], ly.M[q], ly.off[q], ly.mo[q]
    has = M > 0
    s0 = mo - off
    e0 = s0 + np.minimum(M, off)
    if case["status"] != S.OK:
        k = len(q) - 1                                     # the damage is the last sequence
        lim = case["limit"]
        if case["status"] == S.MEMORY_LIMIT_EXCEEDED and mo[k] + M[k] == lim + 1:
            got.add("limit + 1")
            if off[k] > mo[k] + P:
                got.add("limit first")
        if case["status"] == S.INVALID_OFFSET and off[k] == mo[k] + P + 1:
            got.add("off == mo + 1 invalid" if P == 0 and E > 0 else "off == mo + P + 1 invalid")
        if case["status"] == S.ZERO_OFFSET and off[k] == 0 and E > 0:
            got.add("off == 0")
        if case["status"] == S.OUT_CAPACITY and case["out_cap"] == ly.outb - 1 and E > 0:
            got.add("out_cap one byte short")
        return got
    if E > 0 and P == 0:
        if "E_named" in case and E in E_LIST:
            got.add(f"E = {E}")
        if L[0] == 0 and has[0] and mo[0] == E:
            got.add("first sequence without literals: match at E")
            if off[0] == 1:
                got.add(f"off = 1 from E - 1, M = {int(M[0])}" if M[0] in M_AT_EDGE else "off = 1 from E - 1, larger than a sub-batch" if M[0] > RINGS[-1] // 8 else "-")
        if (has & (e0 == E)).any():
            got.add("source ends at E")
        if (has & (e0 == E + 1) & (off >= M)).any():
            got.add("source ends one byte behind E")
        if (has & (s0 == E - 1) & (off >= M) & (mo > E)).any():
            got.add("source starts at E - 1")
        if (has & (off == mo)).any():
            got.add("off == mo with existing output")
        if not has.any() and ly.outb > E:
            got.add("literals only behind existing output")
        if m.nch >= 2 and m.ntile >= 3:
            tile = np.array([t[0] for t in m.toks]) // TILE
            hist = has & (s0 < E)
            if hist.any() and (tile[hist] == 0).all():
                got.add("two chunks, history sources in the first tile only")
        if (has & (mo + M == case["limit"])).any():
            got.add("mo + M == output_limit")
    pre = has & (off > mo)
    if P and E == 0:
        if (pre & (off - mo >= M)).any():
            got.add("source wholly in the prefix")
        if (pre & (off - mo == M)).any():
            got.add("source ends at the prefix's last byte")
        if (pre & (off == mo + P)).any():
            got.add("off == mo + P")
        if P == 1 and (pre & (off == mo + 1) & (M > 1)).any():
            got.add("one prefix byte that replicates")
        if (pre & (off - mo < M) & (M - (off - mo) > off - mo)).any():
            got.add("prefix then block with the same offset")
        if (pre & (M > RINGS[-1] // 8)).any() or (pre & (off - mo >= M) & (M > RINGS[0] // 8)).any():
            got.add("prefix source larger than a sub-batch")
        if (ly.lvl_lo[q][~pre] > 1).any() and pre.any():
            got.add("a level above 1 behind a prefix source")
    if P and 0 < E and (pre & (off - mo + E < M)).any():
        got.add("source across prefix, existing output and the block")
    if len(case["prefix"]) and E >= PREFIX_REACH and has[0] and mo[0] == E and off[0] == 65535:
        got.add("prefix out of reach: off = 65535 at mo = E")
    return got


def census_ring(case, m, R, rb):
    got = set()
    if case["status"] != S.OK:
        return got
    ly, E = m.layout, m.E
    r = ly.records(R, rb)
    act, M, cls = ly.act, ly.M, r["cls"]
    has = act & (M > 0)
    if E:
        got.add(f"(E + rb) & 15 = {(E + rb) & 15}")
    if (cls == 13).any():
        got.add("class 13")
    pre = getattr(ly, "pre", np.zeros(ly.ntok, bool))
    if (pre & (cls == 8)).any():
        got.add("class 8 from the prefix")
    hist = has & ~pre & (ly.mo - ly.off < E)                # the source starts in the existing output
    ring_cls = hist & ~np.isin(cls, (7, 8))
    if ring_cls.any():
        got.add("history source inside the ring")
    if (ring_cls & (ly.mo - ly.off + np.minimum(M, ly.off) > E)).any():
        got.add("history source across E inside the ring")
    if (hist & (cls == 7)).any():
        got.add("history source of class 7")
    if case.get("lov_ring") == R:
        if (ring_cls & (r["sy"] == r["lov"]) & (r["lov"] > 0)).any():
            got.add("history source at lov")
        if (hist & (cls == 7) & (r["sy"] == r["lov"] - 1)).any():
            got.add("history source at lov - 1")
    return got
