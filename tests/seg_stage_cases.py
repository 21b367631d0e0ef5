"""Built edges of the segmented decompress pipeline (lz4_seg_*.hip) and a host model of its stages.  Plain Python and numpy: no
GPU, no library.  Three parts:

  * the builder: raw blocks assembled sequence by sequence (Blk; _seq / _block / _walk, which test_gpu_fed_decode_once.py and
    test_gpu_parse_staging.py share), the output bytes kept alongside;
  * the model, restated from the source: every chunk's own chain and exit (parse), the seam stage's outcome per chunk and the stitched
    token map, the tile / batch layout of the records, and for a ring R and an output residue rb = out & 15 every record — M, mo + rb,
    off, sub-batch, class, flag byte, padding — and the dependency levels (exact where every range of the batch is at most two lanes
    wide, two bounds elsewhere);
  * the cases, each named for the edge it is built for, and census_free() / census_ring(): the named edges a model run reaches.
    tests/test_seg_stage_cases_cpu.py requires every edge for every ring and residue; tests/test_gpu_seg_stages.py compares the stage
    dumps of the device with the model.

CORPUS_INPUT_MAX bounds the compressed bytes of all cases together."""
import functools

import numpy as np

CHUNK, OVERLAP, TILE = 16384, 2048, 2048                   # kSegChunk, kSegOverlap, kSegTile (kernels.h)
STRIDE = CHUNK - OVERLAP                                   # kSegStride
TILE_STAGE = TILE + 128                                    # kTileStage: bytes of a tile the tile kernels stage
TILE_TOK_MAX = TILE // 3 + 2                               # kTileTokMax
SEAM_WIN = 2048                                            # compressed bytes one staged window of a seam walk covers
PATCH_MAX = STRIDE // 3 + 8                                # entries of the seam stage's patch[]
LEN_CLAMP = 1 << 26                                        # kLenClamp
NONE = 0xFFFFFFFF                                          # kNone
RINGS = (32768, 65536, 131072)
RESIDUES = (0, 9)
CORPUS_INPUT_MAX = 4 << 20                                 # bound of the corpus' compressed bytes, all cases together
OK, UNEXPECTED_END, MEMORY_LIMIT_EXCEEDED, ZERO_OFFSET, INVALID_OFFSET, OUTPUT_FULL, CONTRACT, OUT_CAPACITY = range(8)    # oracle_ffi
CLASS_M = (4, 7, 8, 16, 17, 32, 33, 64, 65)
SEGJOB = np.dtype([("eligible", "<u4"), ("failed", "<u4"), ("done", "<u4"), ("nch", "<u4"), ("ntile", "<u4"), ("ntok", "<u4"),
                   ("outb", "<u4"), ("pad", "<u4"), ("rec_off", "<u8"), ("pad2", "<u8")])      # seg_job (kernels.h)


# ---------------------------------------------------------------------------------------------------- raw blocks, sequence by sequence
def _lsic(v):
    return b"\xff" * (v // 255) + bytes([v % 255])


def _seq(lit, off, mlen):
    """One sequence (off None: the last literals, no match)."""
    L = len(lit)
    b = bytearray([(min(L, 15) << 4) | (0 if off is None else min(mlen - 4, 15))])
    if L >= 15:
        b += _lsic(L - 15)
    b += lit
    if off is not None:
        b += off.to_bytes(2, "little")
        if mlen - 4 >= 15:
            b += _lsic(mlen - 19)
    return bytes(b)


def _block(seqs, tail=b"tail"):
    """seqs: (L, M) pairs -> a valid block (offsets inside the output so far) + the last literals."""
    rng = np.random.default_rng(len(seqs))
    out_len, blk = 0, bytearray()
    for L, M in seqs:
        lit = bytes(rng.integers(0, 256, L, dtype=np.uint8))
        out_len += L
        off = int(rng.integers(1, min(out_len, 3000) + 1)) if out_len else 1
        assert out_len >= 1, "a match needs output before it"
        blk += _seq(lit, off, M)
        out_len += M
    blk += _seq(tail, None, 0)
    return bytes(blk)


def _walk(blk):
    """The tokens of a valid block: (position, L, M, position of the length byte that follows the match offset or None)."""
    toks, p, n = [], 0, len(blk)
    while p < n:
        t = blk[p]; q = p + 1; L = t >> 4
        if L == 15:
            while True:
                b = blk[q]; q += 1; L += b
                if b != 255:
                    break
        q += L
        if n - q < 2:
            toks.append((p, L, 0, None)); break
        q += 2; M = (t & 15) + 4; mb = None
        if (t & 15) == 15:
            mb = q
            while True:
                b = blk[q]; q += 1; M += b
                if b != 255:
                    break
        toks.append((p, L, M, mb)); p = q
    return toks


def seq_size(L, M):
    """Compressed bytes of one sequence with a match."""
    return 1 + (0 if L < 15 else 1 + (L - 15) // 255) + L + 2 + (0 if M - 4 < 15 else 1 + (M - 19) // 255)


class Blk:
    """A block under construction: the compressed bytes (c) and the bytes they decode to (o), kept in step."""

    def __init__(self, seed=1):
        self.c, self.o = bytearray(), bytearray()
        self.rng = np.random.default_rng(seed)

    @property
    def cpos(self):
        return len(self.c)

    @property
    def opos(self):
        return len(self.o)

    def _lits(self, L, fill):
        return bytes([fill]) * L if fill is not None else bytes(self.rng.integers(0, 256, L, dtype=np.uint8))

    def seq(self, L, off, M, fill=None, lit=None):
        """L literals (random, `fill` repeated, or `lit`), then a match of M bytes at distance off (copy_overlapping, decompress.rs:80-138)."""
        lit = self._lits(L, fill) if lit is None else lit
        assert len(lit) == L
        self.o += lit
        assert 1 <= off <= len(self.o) and off <= 0xFFFF and M >= 4, (off, M, len(self.o))
        self.c += _seq(lit, off, M)
        if off >= M:
            s = len(self.o) - off
            self.o += self.o[s:s + M]
        else:
            pat = bytes(self.o[-off:])
            self.o += (pat * (M // off + 1))[:M]
        return self

    def near(self, L, M, fill=None, reach=3000):
        """A sequence whose offset is drawn from the last `reach` bytes."""
        return self.seq(L, int(self.rng.integers(1, min(self.opos + L, reach) + 1)), M, fill)

    def small_until(self, target):
        """Short sequences (0..11 literals, matches of 4..15) while the compressed position is below `target`."""
        while self.cpos < target:
            self.near(int(self.rng.integers(0, 12)), 4 + int(self.rng.integers(0, 12)))
        return self

    def fill_c(self, g, fill=None):
        """Sequences (one literal run and a 4-byte match, 3-byte sequences in front where one run cannot make the size) of exactly g
        compressed bytes."""
        assert g >= 3 and self.opos >= 1, g
        while True:
            L = g - 3 if g - 3 < 15 else next((x for x in range(max(g - 3 - 2 - (g // 255), 15), g - 3) if seq_size(x, 4) == g), None)
            if L is not None and seq_size(L, 4) == g:
                return self.near(L, 4, fill)
            self.near(0, 4); g -= 3
            assert g >= 3

    def to_c(self, target, fill=None):
        """Sequences up to compressed position `target`: the next token starts there."""
        return self.fill_c(target - self.cpos, fill) if target != self.cpos else self

    def out_to(self, target, fill=None):
        """One sequence (literals, then a 4-byte match) that ends at output position `target`."""
        return self.near(target - self.opos - 4, 4, fill)

    def end(self, L=5, fill=None):
        lit = self._lits(L, fill)
        self.o += lit
        self.c += _seq(lit, None, 0)
        return bytes(self.c), bytes(self.o)


# ------------------------------------------------------------------------------------------------------------------ the model: tokens
class Parse:
    """One token at any position of a block, as token_next_gen / tile_decode read it (decompress.rs:61-74 without the copies)."""

    def __init__(self, c):
        self.c, self.n = bytes(c), len(c)
        a = np.frombuffer(self.c, np.uint8)
        stop = np.nonzero(a != 255)[0]
        k = np.searchsorted(stop, np.arange(self.n))
        nxt = np.where(k < len(stop), stop[np.minimum(k, max(len(stop) - 1, 0))] if len(stop) else self.n, self.n)
        self.ff = (nxt - np.arange(self.n)).tolist()          # length of the run of 0xFF bytes that starts at q
        self.memo = {}

    def _lsic_tail(self, q):
        """read_lsic_tail: (value, position behind it) or None on UnexpectedEnd."""
        if q >= self.n:
            return None
        r = self.ff[q]
        if q + r >= self.n:
            return None
        return 15 + 255 * r + self.c[q + r], q + r + 1

    def token(self, p):
        """(L, M, off, src, next, err): M = 0 the last literals; err: UnexpectedEnd inside the token (next = len then, as the parse has it)."""
        t = self.memo.get(p)
        if t is None:
            t = self.memo[p] = self._token(p)
        return t

    def _token(self, p):
        c, n = self.c, self.n
        bad = (0, 0, 0, 0, n, True)
        tok = c[p]; q = p + 1; L = tok >> 4
        if L == 15:
            r = self._lsic_tail(q)
            if r is None:
                return bad
            L, q = r
        if n - q < L:
            return bad
        src = q; q += L
        if n - q < 2:
            return (L, 0, 0, src, n, False)
        off = c[q] | (c[q + 1] << 8); q += 2
        M = tok & 15
        if M == 15:
            r = self._lsic_tail(q)
            if r is None:
                return (L, 0, off, src, n, True)
            M, q = r
        return (L, M + 4, off, src, q, False)

    def chain(self, p=0):
        """The tokens of the chain that starts at p: [(pos, L, M, off, src)] and whether it ended in an error (the bad token is the last one)."""
        out = []
        while p < self.n:
            L, M, off, src, nx, err = self.token(p)
            out.append((p, L, M, off, src))
            if err:
                return out, True
            p = nx
        return out, False


def seg_nch(n):
    return 1 if n <= CHUNK else 1 + (n - CHUNK + STRIDE - 1) // STRIDE


def seg_ntile(n):
    return (n + TILE - 1) // TILE


def owner_of_tile(t):
    """The chunk whose marks tile t is listed from (tile_enumerate)."""
    return 0 if t < CHUNK // TILE else 1 + (t - CHUNK // TILE) // (STRIDE // TILE)


class Seam:
    """The parse and seam stages of one job.
    marks[h]   bool[CHUNK]: chunk h's chain from its first byte (lzf_seg_parse_kernel), as the seam stage leaves it (patched where walked);
    xexit[h]   first position of that chain at or beyond the chunk's end (the input's length where the chain ends first);
    vfrom[h]   position from which the chunk's marks are the true tokens, NONE where the true chain jumps over the chunk;
    outcome[h] "first" (chunk 0) | "enter" | "jump" | "walk";   walks[h] = dict(entry, merged, m, np, windows) for a walked chunk;
    failed     a walk met an UnexpectedEnd (the job is the pair kernel's)."""

    def __init__(self, c, parse=None):
        P = self.P = parse or Parse(c)
        n = self.n = P.n
        self.nch = nch = seg_nch(n)
        self.marks, self.xexit = [], []
        for h in range(nch):
            cs = h * STRIDE
            lim = min(cs + CHUNK, n)
            m = np.zeros(CHUNK, bool)
            p = cs
            while p < lim:
                m[p - cs] = True
                p = P.token(p)[4]
            self.marks.append(m); self.xexit.append(min(p, n))
        self.vfrom, self.outcome, self.walks, self.failed, self.entry = [0], ["first"], {}, False, [0]
        carry = None
        for h in range(1, nch):
            e = self.xexit[h - 1] if carry is None else carry
            self.entry.append(e)
            base = h * STRIDE; endk = base + CHUNK; ostart = base + OVERLAP
            assert e >= ostart, "a chunk is entered at or behind its overlap"
            if e >= n or e >= endk:
                self.vfrom.append(NONE); self.outcome.append("jump"); carry = e
            elif self.marks[h][e - base]:
                self.vfrom.append(e); self.outcome.append("enter"); carry = None
            else:
                p, patch, windows, merged, err = e, [], 0, False, False
                while p < endk and p < n and not merged and not err:
                    ws = p; windows += 1
                    while p < endk and p < n and p - ws < SEAM_WIN:
                        if p != e and self.marks[h][p - base]:
                            merged = True; break
                        patch.append(p)
                        tk = P.token(p)
                        if tk[5]:
                            err = True; break
                        p = tk[4]
                assert len(patch) <= PATCH_MAX
                self.walks[h] = dict(entry=e, merged=merged, m=p if merged else endk, np=len(patch), windows=windows)
                self.outcome.append("walk")
                if err:
                    self.failed = True; self.vfrom.append(ostart)       # (what the stage has stored by then is not looked at)
                    self.vfrom += [NONE] * (nch - h - 1); self.outcome += ["-"] * (nch - h - 1)
                    break
                m = self.walks[h]["m"]
                self.marks[h][OVERLAP:m - base] = False
                self.marks[h][np.array(patch, np.int64) - base] = True
                self.vfrom.append(ostart)
                carry = None if merged else p

    def stitched(self):
        """The token map the tile stages enumerate: every chunk's marks over the bytes it owns, from vfrom on."""
        got = np.zeros(self.n, bool)
        return stitch(self.n, self.nch, self.vfrom, lambda h: self.marks[h], got)


def stitch(n, nch, vfrom, row_of, got=None):
    """tile_enumerate's view of the maps: row_of(h) = bool[CHUNK] of chunk h."""
    got = np.zeros(n, bool) if got is None else got
    for h in range(nch):
        base = h * STRIDE
        o0 = 0 if h == 0 else base + OVERLAP
        o1 = min(base + CHUNK, n)
        vf = int(vfrom[h])
        if vf == NONE or o1 <= o0:
            continue
        a = max(o0, vf)
        if a < o1:
            got[a:o1] = row_of(h)[a - base:o1 - base]
    return got


# --------------------------------------------------------------------------------------------------------- the model: tiles and records
class Layout:
    """Tile and batch layout of a job's true tokens (tilesum + scan) and what of a record does not depend on the ring.
    toks: the chain from byte 0 (no error in it).  Per slot (ntok of them, padding included): tok (index into toks, -1 padding), act, L, M,
    off, lo (first output byte: the literals), mo (the match), endp; batch b = slots [64 b, 64 b + 64), nb[b] tokens in it."""

    def __init__(self, n, toks, seed=None):
        self.n, self.toks, self.seed = n, toks, seed          # seed: one of SEEDS, a rule moved by one (the census test: the corpus must notice)
        self.ntile = nt = seg_ntile(n)
        pos = np.array([t[0] for t in toks], np.int64)
        Ls = np.array([t[1] for t in toks], np.int64); Ms = np.array([t[2] for t in toks], np.int64)
        offs = np.array([t[3] for t in toks], np.int64)
        self.tile_n = np.bincount(pos // TILE, minlength=nt).astype(np.int64)                 # tokens that start in the tile
        batches = (self.tile_n + 63) // 64
        self.tile_tok = np.concatenate([[0], np.cumsum(batches)[:-1]]).astype(np.int64)      # after the scan: the tile's first batch
        tot = Ls + Ms
        per_tile_out = np.bincount(pos // TILE, weights=tot, minlength=nt).astype(np.int64)
        self.tile_out = np.concatenate([[0], np.cumsum(per_tile_out)[:-1]]).astype(np.int64)
        self.ntok = int(batches.sum()) * 64
        self.outb = int(tot.sum())
        first_in_tile = np.concatenate([[0], np.cumsum(self.tile_n)[:-1]])
        k = np.arange(len(toks))
        slot = self.tile_tok[pos // TILE] * 64 + (k - first_in_tile[pos // TILE])
        self.slot_of_tok = slot
        self.tok = np.full(self.ntok, -1, np.int64); self.tok[slot] = k
        self.act = self.tok >= 0
        lo_t = np.concatenate([[0], np.cumsum(tot)[:-1]])
        z = lambda v: np.where(self.act, v[np.maximum(self.tok, 0)], 0)
        self.L, self.M, self.off = z(Ls), z(Ms), z(offs)
        self.lo = z(lo_t); self.mo = self.lo + self.L; self.endp = self.mo + self.M
        self.nbatch = self.ntok // 64
        self.nb = self.act.reshape(-1, 64).sum(axis=1) if self.ntok else np.zeros(0, np.int64)
        self._levels()

    def _levels(self):
        """Dependency levels (records stage).  lvl_lo: 1 + the maximum over the matches whose destination the source overlaps; lvl_hi:
        1 + the maximum over all earlier lanes up to i_hi; exact[batch]: every range of the batch is at most two lanes wide, the
        kernel's level is lvl_lo there and lies within [lvl_lo, lvl_hi] elsewhere.  reads[slot]: the source overlaps a match of the batch."""
        N = self.ntok
        self.lvl_lo = np.where(self.act & (self.M > 0), 1, 0).astype(np.int64)
        self.lvl_hi = self.lvl_lo.copy()
        self.reads = np.zeros(N, bool); self.ilo = np.zeros(N, np.int64); self.ihi = np.zeros(N, np.int64)
        self.exact = np.ones(self.nbatch, bool)
        if not N:
            return
        b0 = (np.arange(N) // 64) * 64
        ob = self.lo[b0]                                              # the batch's first output byte
        s0 = self.mo - self.off
        e0 = s0 + np.minimum(self.M, self.off)
        has = self.act & (self.M > 0)
        aslot = np.nonzero(self.act)[0]                               # stream order: ends and starts grow
        ends, mos = self.endp[aslot], self.mo[aslot]
        first = np.searchsorted(aslot, b0)                            # rank of the batch's first token among all
        a = np.maximum(np.searchsorted(ends, s0, side="left" if self.seed == "end < s0" else "right") - first, 0)
        bb = np.maximum(np.searchsorted(mos, e0, side="right" if self.seed == "mo <= e0" else "left") - first, 0)
        bb = np.minimum(bb, np.arange(N) - b0)                        # (a lane never counts itself)
        dep = has & (e0 > ob) & (bb >= 1) & (a <= bb - 1)
        self.reads, self.ilo, self.ihi = dep, np.where(dep, a, 0), np.where(dep, bb - 1, 0)
        lo, hi = self.lvl_lo, self.lvl_hi
        for q in np.nonzero(dep)[0].tolist():
            b = q - q % 64
            i0, i1 = b + int(self.ilo[q]), b + int(self.ihi[q])
            assert i1 < q
            lo[q] = 1 + int(lo[i0:i1 + 1].max())
            hi[q] = 1 + int(hi[b:i1 + 1].max())
            if i1 - i0 > 1:
                self.exact[q // 64] = False

    def records(self, R, rb):
        """The records for ring R and output residue rb: dict of per-slot arrays sub, cls, fl, giant, oe, sob and the words w0..w3
        (w2 without the level: lvl_* above)."""
        N, span, seed = self.ntok, R // 8, self.seed
        cut = span + (seed == "span + 1")
        t8, t16, t32, t64 = 8 + (seed == "M < 9"), 16 + (seed == "M <= 17"), 32 + (seed == "M <= 33"), 64 + (seed == "M > 65")
        sub = np.zeros(N, np.int64); giant = np.zeros(N, bool); oe = np.zeros(N, np.int64); sob = np.zeros(N, np.int64)
        cut_over = np.zeros(N, np.int64)      # endp - sob of the lane that cut a sub-batch (0: none did), at the sub-batch's slots
        for b in range(self.nbatch):
            s, nb = b * 64, int(self.nb[b])
            endp, lo = self.endp[s:s + nb], self.lo[s:s + nb]
            a = sidx = 0
            while a < nb:
                so = int(lo[a])
                e = a + int(np.searchsorted(endp[a:], so + cut, side="right"))        # first lane with endp - sob > span
                over = int(endp[e]) - so if e < nb else 0
                g = e == a
                if g:
                    e = a + 1
                sub[s + a:s + e] = sidx; giant[s + a:s + e] = g; oe[s + a:s + e] = int(endp[e - 1]); sob[s + a:s + e] = so
                cut_over[s + a:s + e] = over
                a = e; sidx += 1
            sub[s + nb:s + 64] = sidx - 1
        act, M, off, mo = self.act, self.M, self.off, self.mo
        fpw = ((oe + rb + 15) & ~15) + 3 * span + 64
        lov = np.maximum(fpw - R, 0)
        s0 = mo - off
        sy, dy = s0 + rb, mo + rb
        di, si = dy & (R - 1), sy & (R - 1)
        wrap = (di + M > R - (seed == "di + M >= R")) | (si + M > R - (seed == "si + M >= R"))
        size = np.where(M < t8, 1, np.where(M <= t16, 2, np.where(M <= t32, 3, 4)))
        rle = (off == 1) | (off == 2) | (off == 4)
        cls = np.where(sy < lov + (seed == "sy <= lov"), 7, np.where((M > t64) | wrap, 6, np.where(off < M + (seed == "off <= M"), np.where(rle, 8 + size, 5), size)))
        cls = np.where(giant, 8, np.where(M != 0, cls, 0))
        cls = np.where(act, cls, 0)
        fl = (np.isin(cls, (1, 9)) * 1 | np.isin(cls, (2, 3, 4, 10, 11, 12)) * 2 | np.isin(cls, (3, 4, 11, 12)) * 4 | np.isin(cls, (4, 12)) * 8 |
              np.isin(cls, (5, 6)) * 16 | np.isin(cls, (9, 10, 11, 12)) * 32)
        # padding: an empty sequence at the end of the batch's last token, in its sub-batch
        last = (np.arange(N) // 64) * 64 + np.maximum(np.repeat(self.nb, 64) - 1, 0)
        w0 = np.where(act, M, 0)
        w1 = np.where(act, mo, self.endp[last] if N else 0) + rb
        w3 = np.where(act, off, 0)
        return dict(sub=sub, cls=cls, fl=fl, giant=giant & act, oe=oe, sob=sob, cut_over=cut_over, lov=lov, sy=sy, di=di, si=si, wrap=wrap,
                    w0=w0, w1=w1, w2_low=sub | (fl << 8), w3=w3)


SEEDS = ("span + 1", "M < 9", "M <= 17", "M <= 33", "M > 65", "di + M >= R", "si + M >= R", "sy <= lov", "off <= M", "end < s0", "mo <= e0")


def record_stage_failure(toks, limit, cap):
    """Does the records stage give the job up (decompress.rs:72-74, :83-89, our buffer)?"""
    o = 0
    for _, L, M, off, _ in toks:
        if o > cap or cap - o < L:
            return True
        mo = o + L
        if M and (mo + M > limit or off == 0 or off > mo or cap - mo < M):
            return True
        o = mo + M
    return False


class Model:
    """Everything the stages should hold for one case."""

    def __init__(self, case):
        c = case["input"]
        self.P = Parse(c)
        self.seam = Seam(c, self.P)
        self.toks, self.chain_err = self.P.chain(0)
        self.n = len(c)
        self.nch, self.ntile = seg_nch(self.n), seg_ntile(self.n)
        limit = case.get("limit", 1 << 62); cap = case.get("out_cap", 1 << 62)
        out_total = sum(t[1] + t[2] for t in self.toks)
        self.gives_up = ("seam" if self.seam.failed else "tilesum" if self.chain_err or any(t[1] > LEN_CLAMP or t[2] > LEN_CLAMP + 4 for t in self.toks) else
                         "scan" if out_total > cap else "records" if record_stage_failure(self.toks, limit, cap) else None)
        self.layout = Layout(self.n, self.toks) if not self.chain_err else None


# ------------------------------------------------------------------------------------------------------------------------- the cases
def _case(name, built, **kw):
    c, o = built
    return dict(name=name, input=c, output=o, status=OK, limit=max(len(o), 1), out_cap=len(o) + 64, **kw)


def three_phase(n_seq=40000, lead=256):
    """`00 00 01` repeated (L 0, M 4, offset 256) is a chain from each of its three byte phases, and kSegStride = 2 (mod 3): two chunks
    of every three start off the true chain and never fall in step — the seam stage walks them whole."""
    b = Blk(3)
    b.seq(lead, 256, 4)
    unit = _seq(b"", 256, 4)
    assert unit == b"\x00\x00\x01"
    for _ in range(n_seq - 1):
        b.c += unit
        s = len(b.o) - 256
        b.o += b.o[s:s + 4]
    return b


def seam_cases():
    out = []
    out.append(_case("seam: three-phase stream, chunks walked whole", three_phase().end(7), reaches=("seam walk to endk", "patch[] within 16 of its bound")))
    # a literal run that jumps over one whole chunk (chunk 2: bytes 28 672 .. 45 056), and over three in a row (chunks 2..4: carry)
    for name, skip, edge in (("seam: literal run over one chunk", 1, "jump over one chunk"), ("seam: literal run over three chunks", 3, "carry through three chunks")):
        b = Blk(11 + skip)
        b.small_until(2 * STRIDE - 300).to_c(2 * STRIDE - 40)              # the run starts in chunk 1, in front of chunk 2 ...
        b.near((1 + skip) * STRIDE + CHUNK - b.cpos - 3 + 500, 6)          # ... and ends behind the last skipped chunk's end
        b.small_until(b.cpos + 12000)
        out.append(_case(name, b.end(9), reaches=(edge,)))
    # a match-length run of 0xFF bytes that covers a whole chunk: 17 000 bytes of 0xFF, one giant match
    b = Blk(21)
    b.small_until(2 * STRIDE - 300).to_c(2 * STRIDE - 100)
    b.seq(3, 1, 19 + 255 * 17000 + 17)
    b.small_until(b.cpos + 6000)
    out.append(_case("seam: 0xFF match-length run over a whole chunk", b.end(4), reaches=("0xFF match run over a chunk",)))
    # walks that merge.  Chunk 2's own chain starts inside a literal run whose bytes read as four-byte sequences `10 AA 01 00` from the chunk's
    # first byte on; the run ends two bytes off that phase, with the offset 0x0110 (`10 01`: a sequence again), so that chain arrives two
    # bytes behind the true chain's entry e.  Four-byte sequences `10 AA 10 01` keep the two chains two bytes apart for `late` bytes; a
    # sequence of six literals whose second is 0x40 (L 4 to the chain that reads it as a token) ends both on the same byte.
    for name, late, edge in (("seam: merge on the first token behind the entry", 0, "merge on the first token"),
                             ("seam: walk over two windows before the merge", 2 * SEAM_WIN + 300, "walk over two windows, merged")):
        b = Blk(31 + late)
        base = 2 * STRIDE
        b.small_until(base - 300).to_c(base - 64)
        L = next(L for L in range(OVERLAP + 200, OVERLAP + 300) if (b.cpos + seq_size(L, 4) - base) % 4 == 2)
        first = b.cpos + seq_size(L, 4) - 2 - L                 # position of the run's first literal
        lit = bytes((0x10, 0xAA, 0x01, 0x00)[(q - base) % 4] if q >= base else 0x77 for q in range(first, first + L))
        b.seq(L, 0x0110, 4, lit=lit)
        e = b.cpos
        assert e > base + OVERLAP and (e - base) % 4 == 2
        while b.cpos - e < late:
            b.seq(1, 0x0110, 4, fill=0xAA)
        b.seq(6, 0x0110, 4, lit=b"\x01\x40\x02\x03\x04\x05")
        b.small_until(b.cpos + 12000)
        out.append(_case(name, b.end(6), reaches=(edge,)))
    # an entry exactly at endk and at endk - 1 of chunk 2: a literal run from in front of the chunk to that byte.  Zero literals read as
    # three-byte sequences from the chunk's first byte on (kSegChunk - 1 is a multiple of 3: the entry is marked), 0x11 as four-byte ones (it is not).
    for name, d, fill, edge in (("seam: entry at endk", 0, None, "entry at endk"), ("seam: entry at endk - 1, on a marked token", 1, 0x00, "entry at endk-1 marked"),
                                ("seam: entry at endk - 1, walked", 1, 0x11, "entry at endk-1 walked")):
        b = Blk(41 + d)
        b.small_until(2 * STRIDE - 400).to_c(2 * STRIDE - 120)                   # (the run's 66 length bytes end in front of the chunk)
        b.fill_c(2 * STRIDE + CHUNK - d - b.cpos, fill)
        b.small_until(b.cpos + 12000)
        out.append(_case(name, b.end(6), reaches=(edge,)))
    # 66 and 67 chunks (the seam's groups of 64 lanes), literal-heavy; the second with a literal run over chunks 64 and 65 (a carry
    # from the last lane of the first group into the second group)
    for name, nch, jump in (("seam: 66 chunks", 66, False), ("seam: 67 chunks, a jump-over on the group boundary", 67, True)):
        b = Blk(50 + nch)
        b.near(40, 8)
        target = CHUNK + (nch - 1) * STRIDE - 700
        while b.cpos < target - 4000:
            if jump and 64 * STRIDE - 3000 < b.cpos < 64 * STRIDE:
                b.near(66 * STRIDE + OVERLAP + 100 - b.cpos, 9); jump = False; continue
            b.near(600 + int(b.rng.integers(0, 900)), 4 + int(b.rng.integers(0, 40)))
            for _ in range(int(b.rng.integers(0, 6))):
                b.near(int(b.rng.integers(0, 5)), 4 + int(b.rng.integers(0, 12)))
        b.to_c(target)
        c, o = b.end(300)
        assert seg_nch(len(c)) == nch, (seg_nch(len(c)), nch)
        out.append(_case(name, (c, o), reaches=(f"{nch} chunks",) + (("carry across the seam's lane groups",) if nch == 67 else ())))
    return out


def tile_cases():
    out = []
    # a tile with no token (inside a long literal run), literal lengths 0, 1, 64, 65, 256, 257 and several KiB
    b = Blk(61)
    b.near(30, 6)
    for L in (0, 1, 64, 65, 256, 257, 0, 1, 64, 65, 256, 257, 5 * TILE + 123, 3, 4097):
        b.near(L, 4 + L % 7)
    out.append(_case("tile: a tile without a token, every literal copy routine", b.end(8)))
    # a tile of 3-byte tokens throughout: tiles 1 and 2 hold 682 / 683 tokens
    b = Blk(62)
    b.near(9, 4).to_c(TILE)
    while b.cpos < 4 * TILE:
        b.near(0, 4 + b.cpos % 3)
    out.append(_case("tile: 3-byte tokens throughout", b.end(5)))
    # tiles with exactly 64, 65 and 128 tokens: tile k of the block is filled by that many equal sequences and one run up to the tile's end
    b = Blk(63)
    b.near(20, 5).to_c(TILE)
    for k, cnt in ((1, 64), (2, 65), (3, 128), (4, 63), (5, 129)):
        assert b.cpos == k * TILE
        for i in range(cnt - 1):
            b.near(5 + i % 3, 4 + i % 9)
        b.to_c((k + 1) * TILE)                                     # the tile's last token: a run that ends with the tile
    out.append(_case("tile: 64, 65 and 128 tokens", b.end(5), reaches=("tile of 64 tokens", "tile of 65 tokens", "tile of 128 tokens")))
    # a token on a tile's last byte; tokens whose length bytes or offset lie behind the tile's staged bytes
    b = Blk(64)
    b.near(20, 5).to_c(TILE - 1)
    b.near(3, 9)                                                   # token byte at 2047
    b.to_c(2 * TILE - 1)
    b.near(15 + 255 + 7, 19 + 255 + 3)                             # at 4095: its literal-length bytes start in the next tile
    b.to_c(3 * TILE - 20)
    b.near(200, 19 + 255 * 3 + 4)                                  # literals end behind tile + 128: offset and match-length bytes behind the staged bytes
    b.to_c(4 * TILE - 2)
    b.near(15 + 255 * 2 + 9, 19 + 2)                               # length bytes inside the 128, literals and offset beyond
    b.to_c(5 * TILE - 3)
    b.near(126, 19 + 255)                                          # ends exactly on the staged bytes' last byte: offset at + 126, + 127, length bytes behind
    for _ in range(300):
        b.near(int(b.rng.integers(0, 9)), 4 + int(b.rng.integers(0, 9)))
    out.append(_case("tile: tokens on a tile's last byte and beyond the staged bytes", b.end(5)))
    return out


def _pad_tile(b):
    """The next token starts a tile (a batch of its own)."""
    t = (b.cpos + TILE - 1) // TILE * TILE
    if t - b.cpos < 3:
        t += TILE
    return b.to_c(t)


def class_cases():
    out = []
    # sources inside the ring, not overlapping and overlapping, at every length of CLASS_M
    b = Blk(71)
    b.near(300, 8)
    for M in CLASS_M:
        b.seq(2, M + 40, M)                                        # not overlapping
        for off in (1, 2, 4, 3, 5, M - 1, M):
            if off >= 1:
                b.seq(1, off, M)
    out.append(_case("class: every length, apart / run-length / overlapping", b.end(5)))
    # destination and source index ending exactly at the ring's end and one byte past it: output positions k * 131 072 (the end of every ring)
    # for both residues; every stretch between is a run-length match larger than any sub-batch
    b = Blk(72)
    b.near(64, 8)
    big = RINGS[-1]
    k = 1
    for M in CLASS_M:
        if M > 64:
            continue
        for rb in RESIDUES:
            for past in (0, 1):
                edge = k * big; k += 1
                mo = edge - rb - M + past
                b.seq(7, 1, mo - 300 - b.opos - 7)                # (a giant) up to 300 bytes in front
                b.out_to(mo - 40)
                b.seq(40, 90, M)                                   # the destination ends at the edge (+ past)
    out.append(_case("class: destination index ends at R and R + 1", b.end(5)))
    b = Blk(73)
    b.near(64, 8)
    edge = big
    b.seq(7, 1, edge - 200 - b.opos - 7)
    b.out_to(edge + 600)
    for M in CLASS_M:
        if M > 64:
            continue
        for rb in RESIDUES:
            for past in (0, 1):
                s0 = edge - rb - M + past
                b.seq(1, b.opos + 1 - s0, M)                       # the source ends at the edge (+ past); the destination is 600+ bytes behind it
    out.append(_case("class: source index ends at R and R + 1", b.end(5)))
    # s0 + rb == lov and lov - 1: the first match of a sub-batch whose span is all but full, for every ring and residue (at R = 131 072
    # the offset is near 65 535)
    b = Blk(74)
    b.near(64, 8)
    b.seq(7, 1, 70000)
    for R in RINGS:
        for rb in RESIDUES:
            for side in (0, 1):
                _pad_tile(b)
                span = R // 8
                P = b.opos                                          # the sub-batch's first output byte, and its first match (L 0)
                oe = P + span
                lov = ((oe + rb + 15) & ~15) + 3 * span + 64 - R
                off = P + rb - lov + side                           # side 0: s0 + rb == lov; side 1: lov - 1
                assert 1 <= off <= 0xFFFF, (R, rb, off)
                b.seq(0, off, 4)
                b.seq(0, 1, span - 4)                               # fills the span exactly
                b.near(3, 5)
    out.append(_case("class: source at the oldest byte the ring holds for certain", b.end(5)))
    return out


def sub_batch_cases():
    out = []
    b = Blk(81)
    b.near(64, 8)
    for R in RINGS:
        span = R // 8
        for extra in (0, 1):                                       # a span of exactly R / 8 and of R / 8 + 1
            _pad_tile(b)
            b.seq(0, 3, 10); b.seq(5, 1, span - 15 - 6 + extra); b.seq(0, 2, 6)
            b.near(2, 5)
    # giants: first in a batch, last in a batch, two in a row, one with no match (the last literals)
    top = RINGS[-1] // 8
    _pad_tile(b)
    b.seq(3, 1, top + 100); b.near(1, 5); b.near(2, 6)              # first in its batch
    _pad_tile(b)
    b.near(1, 5); b.near(2, 6); b.seq(0, 7, top + 9); b.seq(top + 50, 2, 77)   # two in a row (a match, then literals), the second last in its batch
    _pad_tile(b)
    b.near(4, 4)
    out.append(_case("sub-batch: spans at the limit, giants", b.end(top + 300)))
    return out


def level_cases():
    out = []
    b = Blk(91)
    b.near(200, 8)
    _pad_tile(b)
    for i in range(64):                                            # each match reads the one before: levels 1 .. 64
        b.seq(0, 4 if i else 50, 4)
    _pad_tile(b)
    for i in range(64):                                            # 64 independent far matches: all level 1
        b.seq(1, 2000 + 7 * i, 6)
    _pad_tile(b)
    # a source that ends exactly at the batch's first output byte (the batch's first lane has no literals), and one byte into it
    b.seq(0, 30, 8); b.seq(2, 10 + 8, 8); b.seq(1, 1 + 8 + 2 + 8 + 9, 9 + 1)
    _pad_tile(b)
    b.seq(0, 30, 8); b.seq(2, 10 + 8, 8); b.seq(1, 1 + 8 + 2 + 8 + 9, 9 + 2)
    _pad_tile(b)
    # a source that starts exactly where an earlier match ends, and one byte in front of that
    b.seq(0, 40, 8); b.seq(6, 6, 5); b.seq(3, 3 + 5 + 6 + 1, 5)
    _pad_tile(b)
    # one wide range (a 64-byte source over sixteen 4-byte matches) behind a deep chain
    for i in range(20):
        b.seq(0, 4 if i else 60, 4)
    for i in range(16):
        b.seq(0, 500 + i, 4)
    b.seq(2, 2 + 64, 64)
    b.seq(0, 64, 8)
    out.append(_case("level: chain of 64, 64 apart, sources at a batch's and a match's edge, a wide range", b.end(5)))
    return out


def damaged_cases():
    out = []
    # a truncated LSIC inside a seam walk: the three-phase stream cut inside chunk 2 (walked), its last token's literal length never ends
    b = three_phase(9000 + 2400)
    c = bytes(b.c)
    toks = Parse(c).chain(0)[0]
    p = next(t[0] for t in toks if t[0] >= 2 * STRIDE + OVERLAP + 3000)
    out.append(dict(name="damaged: truncated LSIC inside a seam walk", input=c[:p] + b"\xf0\xff\xff\xff", status=UNEXPECTED_END, gives_up="seam",
                    limit=1 << 20, out_cap=(1 << 20) + 64))
    # a token error in a tile: literals that run past the end of the input, in the block's third tile
    b = Blk(101)
    while b.cpos < 2 * TILE - 200:
        b.near(int(b.rng.integers(0, 9)), 4 + int(b.rng.integers(0, 9)))
    b.to_c(2 * TILE + 100)
    c = bytes(b.c) + bytes([0xF0, 200]) + bytes(50)
    out.append(dict(name="damaged: literals past the input's end in a tile", input=c, status=UNEXPECTED_END, gives_up="tilesum", limit=1 << 20,
                    out_cap=(1 << 20) + 64))
    # in the last batch of a block, after earlier batches' literals were written
    def base():
        b = Blk(102)
        for _ in range(900):
            b.near(3 + int(b.rng.integers(0, 9)), 4 + int(b.rng.integers(0, 9)))
        return b
    b = base(); b.seq(3, 5, 9); c = bytearray(b.c); q = len(c) - 2; c[q:q + 2] = b"\0\0"; b.c = c
    c, o = b.end(4)
    out.append(dict(name="damaged: offset 0 in the last batch", input=c, status=ZERO_OFFSET, gives_up="records", limit=1 << 20, out_cap=(1 << 20) + 64))
    b = base(); b.seq(3, 5, 9); c = bytearray(b.c); q = len(c) - 2; c[q:q + 2] = (b.opos - 9 + 1).to_bytes(2, "little"); b.c = c
    c, o = b.end(4)
    out.append(dict(name="damaged: offset behind the start of the output", input=c, status=INVALID_OFFSET, gives_up="records", limit=1 << 20,
                    out_cap=(1 << 20) + 64))
    b = base(); b.seq(3, 5, 9); c, o = b.end(4)
    out.append(dict(name="damaged: a match passes output_limit", input=c, status=MEMORY_LIMIT_EXCEEDED, gives_up="records", limit=len(o) - 4 - 3,
                    out_cap=len(o) + 64))
    out.append(dict(name="damaged: out_cap too small for the literals", input=c, status=OUT_CAPACITY, gives_up="scan", limit=len(o), out_cap=len(o) - 2))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = seam_cases() + tile_cases() + class_cases() + sub_batch_cases() + level_cases() + damaged_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def models():
    return tuple(Model(c) for c in all_cases())


# ------------------------------------------------------------------------------------------------------------------------ the census
def ring_edges():
    """The named edges that depend on the ring and the residue."""
    e = {f"class {k}" for k in range(13)}
    for M in CLASS_M:
        e |= {f"apart M={M}", f"off=M M={M}"}
        e |= {f"off={o} M={M}" for o in (1, 2, 4, 3, 5) if o < M} | ({f"off=M-1 M={M}"} if M > 4 else set())
        if M <= 64:
            e |= {f"destination ends at R M={M}", f"destination ends at R+1 M={M}", f"source ends at R M={M}", f"source ends at R+1 M={M}"}
    e |= {"source at lov", "source at lov-1", "span R/8", "span R/8+1", "giant first in a batch", "giant last in a batch", "two giants in a row",
          "giant without a match", "padding behind a cut batch"}
    return e


def free_edges():
    """The named edges that do not depend on the ring: seam, tiles, levels, damage."""
    return {"seam enter", "seam jump", "seam walk to endk", "seam walk merged", "patch[] within 16 of its bound", "jump over one chunk",
            "carry through three chunks", "0xFF match run over a chunk", "merge on the first token", "walk over two windows, merged",
            "entry at endk", "entry at endk-1 marked", "entry at endk-1 walked", "66 chunks", "67 chunks", "carry across the seam's lane groups",
            "tile without a token", "tile of kTileTokMax - 1 tokens", "tile of 64 tokens", "tile of 65 tokens", "tile of 128 tokens",
            "token on a tile's last byte", "match-length bytes behind the staged bytes", "offset behind the staged bytes",
            "literal-length bytes across the tile's end",
            "L=0", "L=1", "L=64", "L=65", "L=256", "L=257", "L>=4096",
            "level 64", "batch of 64 at level 1", "source ends at the batch's first byte", "source ends one byte into the batch",
            "source starts at a match's end", "source starts one byte inside a match", "wide range behind a deep chain", "bounded level",
            "gives up: seam", "gives up: tilesum", "gives up: scan", "gives up: records"}


def census_free(case, m):
    got = set()
    s = m.seam
    if m.gives_up:
        got.add(f"gives up: {m.gives_up}")
    for h in range(1, s.nch):
        oc = s.outcome[h]
        endk = h * STRIDE + CHUNK
        if oc == "enter":
            got.add("seam enter")
            if s.vfrom[h] == endk - 1:
                got.add("entry at endk-1 marked")
        elif oc == "jump":
            got.add("seam jump")
            if s.entry[h] == endk:
                got.add("entry at endk")
            if h == 64 and h + 1 < s.nch:                       # (lane 63 of the first group: the carry enters the second group)
                got.add("carry across the seam's lane groups")
        elif oc == "walk":
            w = s.walks[h]
            got.add("seam walk merged" if w["merged"] else "seam walk to endk")
            if w["np"] >= PATCH_MAX - 16:
                got.add("patch[] within 16 of its bound")
            if w["merged"] and w["np"] == 1:
                got.add("merge on the first token")
            if w["merged"] and w["windows"] >= 3:
                got.add("walk over two windows, merged")
            if w["entry"] == endk - 1:
                got.add("entry at endk-1 walked")
    runs = [len(r) for r in "".join("j" if o == "jump" else "." for o in s.outcome).split(".") if r]
    if 1 in runs:
        got.add("jump over one chunk")
    if any(r >= 3 for r in runs):
        got.add("carry through three chunks")
    if s.nch in (66, 67):
        got.add(f"{s.nch} chunks")
    if m.layout is None or m.gives_up:
        return got
    ly = m.layout
    c = case["input"]
    for h in range(1, s.nch):
        lo, hi = h * STRIDE, h * STRIDE + CHUNK
        if s.outcome[h] == "jump" and hi <= len(c) and all(x == 255 for x in c[lo:hi:97]) and c[lo:hi] == b"\xff" * CHUNK:
            got.add("0xFF match run over a chunk")
    for t, n in enumerate(ly.tile_n.tolist()):
        if n == 0:
            got.add("tile without a token")
        if n == TILE_TOK_MAX - 1:
            got.add("tile of kTileTokMax - 1 tokens")
        if n in (64, 65, 128):
            got.add(f"tile of {n} tokens")
    for pos, L, M, off, src in m.toks:
        ts = pos // TILE * TILE
        if pos % TILE == TILE - 1:
            got.add("token on a tile's last byte")
        if L >= 15 and src > ts + TILE and pos < ts + TILE:
            got.add("literal-length bytes across the tile's end")
        if M:
            if src + L + 2 > ts + TILE_STAGE:
                got.add("offset behind the staged bytes")
            if M >= 19 and src + L + 2 >= ts + TILE_STAGE:
                got.add("match-length bytes behind the staged bytes")
        if L in (0, 1, 64, 65, 256, 257):
            got.add(f"L={L}")
        if L >= 4096:
            got.add("L>=4096")
    for b in range(ly.nbatch):
        sl = slice(b * 64, b * 64 + 64)
        lv = ly.lvl_lo[sl]
        if ly.exact[b] and lv.max() == 64:
            got.add("level 64")
        if ly.nb[b] == 64 and ly.exact[b] and (lv == 1).all():
            got.add("batch of 64 at level 1")
        if not ly.exact[b]:
            wide = ly.reads[sl] & (ly.ihi[sl] - ly.ilo[sl] > 1)
            if (ly.lvl_hi[sl][wide] > 16).any():
                got.add("wide range behind a deep chain")
            if (ly.lvl_hi[sl] > ly.lvl_lo[sl]).any():
                got.add("bounded level")
        ob = int(ly.lo[b * 64])
        for q in range(b * 64, b * 64 + int(ly.nb[b])):
            M, off, mo = int(ly.M[q]), int(ly.off[q]), int(ly.mo[q])
            if not M:
                continue
            s0 = mo - off; e0 = s0 + min(M, off)
            if int(ly.L[b * 64]) == 0 and int(ly.M[b * 64]) and q > b * 64:
                if e0 == ob:
                    got.add("source ends at the batch's first byte")
                if e0 == ob + 1:
                    got.add("source ends one byte into the batch")
            if e0 > ob:
                ends = ly.endp[b * 64:q]; Ms = ly.M[b * 64:q]
                if ((ends == s0) & (Ms > 0)).any() and not ly.reads[q]:
                    got.add("source starts at a match's end")
                if ((ends == s0 + 1) & (Ms > 0)).any() and ly.reads[q]:
                    got.add("source starts one byte inside a match")
    return got


def census_ring(m, R, rb):
    got = set()
    if m.layout is None or m.gives_up:
        return got
    ly = m.layout
    r = ly.records(R, rb)
    act, M, off, cls = ly.act, ly.M, ly.off, r["cls"]
    for k in np.unique(cls[act]).tolist():
        got.add(f"class {k}")
    inring = act & (M > 0) & ~np.isin(cls, (6, 7, 8)) | (act & (M == 65) & (cls == 6) & ~r["wrap"])
    for Mv in CLASS_M:
        sel = inring & (M == Mv)
        o = off[sel]
        if (o > Mv).any():
            got.add(f"apart M={Mv}")
        if (o == Mv).any():
            got.add(f"off=M M={Mv}")
        if Mv > 4 and (o == Mv - 1).any():
            got.add(f"off=M-1 M={Mv}")
        for ov in (1, 2, 4, 3, 5):
            if ov < Mv and (o == ov).any():
                got.add(f"off={ov} M={Mv}")
        if Mv <= 64:
            near = act & (M == Mv) & (off >= M) & ~r["giant"] & (r["sy"] >= r["lov"])
            for what, idx in (("destination", r["di"]), ("source", r["si"])):
                if (near & (idx + Mv == R)).any():
                    got.add(f"{what} ends at R M={Mv}")
                if (near & (idx + Mv == R + 1)).any():
                    got.add(f"{what} ends at R+1 M={Mv}")
    live = act & (M > 0) & ~r["giant"]
    if (live & (r["sy"] == r["lov"]) & (r["lov"] > 0)).any():
        got.add("source at lov")
    if (live & (r["sy"] == r["lov"] - 1)).any():
        got.add("source at lov-1")
    span = R // 8
    if (act & ~r["giant"] & (r["oe"] - r["sob"] == span)).any():
        got.add("span R/8")
    if (act & ~r["giant"] & (r["cut_over"] == span + 1)).any():
        got.add("span R/8+1")
    g = r["giant"]
    for b in range(ly.nbatch):
        s, nb = b * 64, int(ly.nb[b])
        if nb > 1 and g[s]:
            got.add("giant first in a batch")
        if nb > 1 and g[s + nb - 1]:
            got.add("giant last in a batch")
        if (g[s:s + nb - 1] & g[s + 1:s + nb]).any():
            got.add("two giants in a row")
        if nb < 64 and r["sub"][s + nb - 1] > 0:
            got.add("padding behind a cut batch")
    if (g & (M == 0)).any():
        got.add("giant without a match")
    return got


# ------------------------------------------------------------------------------------------------------ the device's dumps against the model
def host_parse(c):
    """[(pos, L, M, off, src)] of a valid block (decompress.rs:61-74)."""
    toks, err = Parse(c).chain(0)
    assert not err, "not a valid block"
    return toks


def device_token_map(n, nch, vfrom, bits):
    """The stitched map of a job from the device's bit rows (bits: uint32 [maxch, CHUNK / 32]) and vfrom."""
    return stitch(n, nch, vfrom, lambda h: np.unpackbits(np.ascontiguousarray(bits[h]).view(np.uint8), bitorder="little").astype(bool))


def check_records(ly, recs, R, rb):
    """Compare a job's records (uint32 [ntok, 4]) with the model, word for word.  Returns (messages, records compared, levels exact,
    levels bounded)."""
    msgs = []
    r = ly.records(R, rb)
    got_lvl = ((recs[:, 2] >> 16) & 0xFF).astype(np.int64)
    got_cls = (recs[:, 2] >> 24).astype(np.int64)
    for name, got, exp in (("w0 (M)", recs[:, 0], r["w0"]), ("w1 (mo + rb)", recs[:, 1], r["w1"]), ("w3 (off)", recs[:, 3], r["w3"]),
                           ("sub-batch", recs[:, 2] & 0xFF, r["sub"]), ("flags", (recs[:, 2] >> 8) & 0xFF, r["fl"]), ("class", got_cls, r["cls"])):
        bad = np.nonzero(got.astype(np.int64) != exp)[0]
        if len(bad):
            q = int(bad[0])
            msgs.append(f"{name}: {len(bad)} records differ, first slot {q} (batch {q // 64} lane {q % 64}): got {int(got[q])}, model {int(exp[q])}; "
                        f"M {int(ly.M[q])} off {int(ly.off[q])} mo {int(ly.mo[q])} L {int(ly.L[q])}")
    ex = np.repeat(ly.exact, 64)
    has = ly.act & (ly.M > 0)
    bad = np.nonzero(ex & (got_lvl != ly.lvl_lo))[0]
    if len(bad):
        q = int(bad[0])
        msgs.append(f"level: {len(bad)} differ where the model is exact, first slot {q}: got {int(got_lvl[q])}, model {int(ly.lvl_lo[q])}")
    bad = np.nonzero(~ex & ((got_lvl < ly.lvl_lo) | (got_lvl > ly.lvl_hi)))[0]
    if len(bad):
        q = int(bad[0])
        msgs.append(f"level: {len(bad)} outside the bounds, first slot {q}: got {int(got_lvl[q])}, bounds {int(ly.lvl_lo[q])}..{int(ly.lvl_hi[q])}")
    if (got_lvl[has & ~ly.reads] != 1).any():
        msgs.append("level: a match that reads nothing of its batch is not at level 1")
    if (got_lvl > 64).any() or (got_lvl[~has] != 0).any():
        msgs.append("level: above 64, or set on a slot without a match")
    return msgs, len(recs), int((ex & has).sum()), int((~ex & has).sum())
