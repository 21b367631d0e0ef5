"""Handcrafted token streams for the plain-hop loop of lzf_seg_parse_kernel (lz4_seg_front.hip: two hops per trip, the halves with
the two position registers in each other's role), and a model of what that kernel does with a chunk: pass 0, the fixed-point passes, the
rows.  The model walks lane by lane exactly as the kernel's C++ twin does and keeps, for every hop, where in the loop it ended (plain,
stop, step back on a 0xFF match-length extension, parked on a 0xFF literal-length extension, fe, merged on a mark of row A) and in which
half of a trip (hop 1, 3, 5 .. of a walk's loop: the first half; 2, 4 ..: the second).  census() names the edges a job reaches;
tests/test_parse_hop_cases_cpu.py asserts that every named edge is reached, tests/test_gpu_parse_hop.py asks the device.
Every job is one chunk (at most 16 384 compressed bytes) or two (14 336 + a few hundred)."""
import numpy as np

CHUNK, STRIDE, REGION = 16384, 14336, 256          # kSegChunk, kSegStride, kSegRegion
OVERLAP = CHUNK - STRIDE
LIMIT = 1 << 22


def nch(n):
    return 1 if n <= CHUNK else 1 + (n - CHUNK + STRIDE - 1) // STRIDE


# ------------------------------------------------------------------------------------------------------------------ the block writer
class Writer:
    """A raw LZ4 block, sequence by sequence; every match has offset 1 (valid once one byte is out)."""

    def __init__(self):
        self.b = bytearray()
        self.out = 0

    @property
    def pos(self):
        return len(self.b)

    def tok(self, L, mn=0, mext=b"", lit=None):
        """A sequence of L literals and a match whose nibble is mn (15: followed by the bytes mext, the last one below 255)."""
        lit = bytes(L) if lit is None else bytes(lit)
        assert len(lit) == L and (self.out + L) >= 1 and (mn == 15) == bool(mext)
        assert not mext or (mext[-1] != 255 and all(x == 255 for x in mext[:-1]))
        self.b.append((min(L, 15) << 4) | mn)
        if L >= 15:
            self.b += b"\xff" * ((L - 15) // 255) + bytes([(L - 15) % 255])
        self.b += lit + b"\x01\x00" + bytes(mext)
        self.out += L + 4 + mn + sum(mext)
        return self

    def sized(self, n, **kw):
        """A sequence of exactly n compressed bytes with a plain match (3..17, 19..273) or, with mn/mext given, that much more."""
        extra = len(kw.get("mext", b""))
        body = n - extra
        assert 3 <= body <= 273 and body != 18, n
        return self.tok(body - 3 if body <= 17 else body - 4, **kw)

    def fill_to(self, pos, hops):
        """`hops` sequences that end exactly at pos."""
        room = pos - self.pos
        sizes = [room // hops + (1 if i < room % hops else 0) for i in range(hops)]
        for i, s in enumerate(sizes):                      # 18 is no size of a plain sequence
            if s == 18:
                k = (i + 1) % hops
                assert hops > 1
                sizes[i] += 1; sizes[k] -= 1
        assert all(3 <= s <= 273 and s != 18 for s in sizes) and sum(sizes) == room, sizes
        for s in sizes:
            if self.out == 0 and s == 3:
                raise AssertionError("the first sequence needs a literal")
            self.sized(s)
        return self

    def end(self, total=None, tail=40):
        """The last literals; total: the block's length in bytes."""
        if total is not None:
            rest = total - self.pos
            tail = next(t for t in range(rest, -1, -1) if 1 + (0 if t < 15 else 1 + (t - 15) // 255) + t == rest)
        self.b.append(min(tail, 15) << 4)
        if tail >= 15:
            self.b += b"\xff" * ((tail - 15) // 255) + bytes([(tail - 15) % 255])
        self.b += bytes((7 * i + 3) & 0x7F for i in range(tail))
        assert total is None or self.pos == total
        return bytes(self.b)


def true_tokens(blk):
    """Positions of the tokens of a valid block: the plain walk of src/raw/decompress.rs without the copies."""
    toks, p, n = [], 0, len(blk)
    while p < n:
        toks.append(p)
        t = blk[p]; q = p + 1; L = t >> 4
        if L == 15:
            while True:
                b = blk[q]; q += 1; L += b
                if b != 255:
                    break
        q += L
        if n - q < 2:
            break
        q += 2
        if (t & 15) == 15:
            while blk[q] == 255:
                q += 1
            q += 1
        p = q
    return toks


# ------------------------------------------------------------------------------------------------------------------ the kernel's model
def _token_next(buf, p):
    """token_next_gen: the next token's position, or None (UnexpectedEnd)."""
    n = len(buf)

    def lsic(q):
        if q >= n:
            return None
        k = 0
        while q + k < n and buf[q + k] == 255:
            k += 1
        if q + k >= n:
            return None
        return 15 + 255 * k + buf[q + k], q + k + 1
    tok = buf[p]; q = p + 1; L = tok >> 4
    if L == 15:
        r = lsic(q)
        if r is None:
            return None
        L, q = r
    if n - q < L:
        return None
    q += L
    if n - q < 2:
        return n
    q += 2
    if (tok & 15) == 15:
        r = lsic(q)
        if r is None:
            return None
        q = r[1]
    return q


class Chunk:
    """What lzf_seg_parse_kernel makes of chunk h of `buf`: .bits (bool per chunk byte: the row written out), .hops (one record per
    hop of the plain-hop loop: dict(lane, pss, mode, n, how, r, rn, fe, stop, end_r)), .passes (fixed-point passes that walked)."""

    def __init__(self, buf, h):
        self.buf, self.h = buf, h
        n = len(buf)
        self.cstart = cs = h * STRIDE
        self.cb = bytes(buf[cs:cs + CHUNK]) + bytes(max(0, CHUNK - (n - cs)) + 4)
        room = n - cs
        self.fe = (min(room - 24, CHUNK - 2) if room > 24 else 0)
        self.hops, self.passes = [], 0
        A = [set() for _ in range(64)]
        B = [set() for _ in range(64)]
        in_input = [cs + REGION * i < n for i in range(64)]
        x0 = [self._walk(i, REGION * i, in_input[i], False, 0, 0, A, B)[0] for i in range(64)]
        X = [x0[i] if in_input[i] else 0 for i in range(64)]
        walked = [REGION * i for i in range(64)]
        mpos = list(walked)
        for pss in range(1, 81):
            entry, m = [0] * 64, 0
            for i in range(64):
                entry[i] = m; m = max(m, X[i])
            redo = [in_input[i] and entry[i] != walked[i] and i != 0 for i in range(64)]
            if not any(redo):
                break
            self.passes = pss
            for i in range(64):
                if not redo[i]:
                    continue
                end_r = REGION * (i + 1)
                inreg = entry[i] < end_r and cs + entry[i] < n
                walked[i] = entry[i]; B[i] = set()
                x1, mg = self._walk(i, entry[i] if inreg else end_r, inreg, False, 1, pss, A, B)
                if not inreg:
                    X[i], mpos[i] = entry[i], end_r
                elif mg:
                    X[i], mpos[i] = x0[i], x1
                else:
                    X[i], mpos[i] = x1, end_r
        self.bits = np.zeros(CHUNK, bool)
        for i in range(64):
            if in_input[i]:
                for p in A[i]:
                    if p >= mpos[i]:
                        self.bits[p] = True
                for p in B[i]:
                    self.bits[p] = True
        self.exit = min(cs + max(X), n)

    def _walk(self, lane, r, go, merged, mode, pss, A, B):
        cb, cs, n, fe = self.cb, self.cstart, len(self.buf), self.fe
        end_r = REGION * (lane + 1)
        stop = min(end_r, fe) if go else 0
        rows = A if mode == 0 else B
        while True:
            mxp, rprev, k = False, r, 0
            act = go and not merged and r < stop
            while act:
                k += 1
                rec = dict(lane=lane, pss=pss, mode=mode, n=k, r=r, rn=None, fe=fe, stop=stop, end_r=end_r, front=cb[r - 1] if r else None, b1=None)
                self.hops.append(rec)
                if mxp and cb[r - 1] == 255:
                    rec["how"] = "step back"; r = rprev; break
                if r >= stop:
                    rec["how"] = "stop"; break
                if mode == 1 and r in A[lane]:
                    rec["how"] = "merged"; merged = True; break
                t, b1 = cb[r], cb[r + 1]
                L0, M0 = t >> 4, t & 15
                isx = L0 == 15
                rn = r + 3 + isx + L0 + (b1 if isx else 0) + (M0 == 15)
                rec["rn"] = rn; rec["b1"] = b1 if isx else None
                if isx and b1 == 255:
                    rec["how"] = "parked"; break
                if rn >= fe:
                    rec["how"] = "fe"; break
                rec["how"] = "plain"
                rows[lane].add(r); rprev, r, mxp = r, rn, M0 == 15
            pa = cs + r
            if not (go and not merged and r < end_r and pa < n):
                break
            if mode == 1 and r in A[lane]:
                merged = True
            else:
                rows[lane].add(r)
                nx = _token_next(self.buf, pa)
                r = (n if nx is None else nx) - cs
        return r, merged


def expected_rows(blk):
    """The rows the device writes for each chunk of blk, as the model has them: uint32 words, (nch, CHUNK // 32)."""
    out = np.zeros((nch(len(blk)), CHUNK // 32), np.uint32)
    for h in range(out.shape[0]):
        out[h] = np.packbits(Chunk(blk, h).bits, bitorder="little").view(np.uint32)
    return out


def compare_with_truth(blk, rows):
    """`rows` (nch, CHUNK // 32) against the true token positions: chunk 0 whole; a later chunk from the first mark that is a true token
    on (from there the chunk's chain IS the true one).  Returns the first differing position or None."""
    truth = np.zeros(len(blk) + CHUNK, bool)
    truth[true_tokens(blk)] = True
    for h in range(rows.shape[0]):
        bits = np.unpackbits(rows[h].view(np.uint8), bitorder="little").astype(bool)
        cs = h * STRIDE
        want = truth[cs:cs + CHUNK]
        both = np.nonzero(bits & want)[0]
        if both.size == 0:
            if h == 0 or want.any() and not bits.any():
                return cs
            continue
        f = 0 if h == 0 else int(both[0])
        d = np.nonzero(bits[f:] != want[f:])[0]
        if d.size:
            return cs + f + int(d[0])
    return None


# ------------------------------------------------------------------------------------------------------------------ the cases
def _half(n):
    return "first half" if n % 2 == 1 else "second half"


def census(blk):
    """The named edges the parse of blk reaches."""
    got = set()
    for h in range(nch(len(blk))):
        c = Chunk(blk, h)
        if c.passes >= 2:
            got.add("a third pass runs")
        for r in c.hops:
            how, n, m = r["how"], r["n"], r["mode"]
            plain_before = n - 1
            if m == 0 and how == "stop" and r["stop"] == r["end_r"] and 1 <= plain_before <= 5 and r["fe"] > r["end_r"] + 3:
                got.add(f"stop after {plain_before} plain hops")
            if m == 0 and how == "fe" and 1 <= plain_before <= 5 and 0 <= r["fe"] - r["end_r"] <= 3:
                got.add(f"fe after {plain_before} plain hops")
                got.add(f"input ends 24 + {r['fe'] - r['end_r']} behind the region")
            if how == "step back":
                got.add(f"step back, {_half(n)}")
            if n == 1 and r["front"] == 255 and how == "plain":
                got.add("first hop of a walk behind a 0xFF byte")
            if r["b1"] is not None and r["b1"] in (0, 254, 255) and n <= 6:
                got.add(f"literal extension byte {r['b1']}, {_half(n)}")
            if how == "plain" and r["fe"] > r["end_r"] + 3 and abs(r["rn"] - r["end_r"]) <= 1:
                got.add(f"successor at end_r {r['rn'] - r['end_r']:+d}")
            if how in ("plain", "fe") and r["fe"] < r["end_r"] and abs(r["rn"] - r["fe"]) <= 1:
                got.add(f"successor at fe {r['rn'] - r['fe']:+d}")
            if how == "fe" and r["fe"] == CHUNK - 2 and r["rn"] in (CHUNK - 2, CHUNK - 1):
                got.add(f"would land on staged byte {r['rn'] - CHUNK}")
            if m == 1 and how == "merged" and n <= 4:
                got.add(f"mode 1 merges on hop {n}")
            if m == 1 and how == "stop" and n >= 2 and r["stop"] == r["end_r"]:
                got.add(f"mode 1 leaves the region unmerged, {'odd' if (n - 1) % 2 else 'even'} hops")
        # lanes leaving in different halves while their neighbours go on: pass-0 walks of 1..6 plain hops side by side
        counts = {}
        for r in c.hops:
            if r["mode"] == 0 and r["how"] == "stop":
                counts[r["lane"]] = r["n"] - 1
        if len(counts) >= 60 and set(counts.values()) >= {1, 2, 3, 4, 5, 6}:       # (the last lanes end on fe: the staged bytes end there)
            got.add("64 regions with 1..6 hops side by side")
    return got


EDGES = (
    [f"stop after {k} plain hops" for k in range(1, 6)] + [f"fe after {k} plain hops" for k in range(1, 6)] +
    [f"input ends 24 + {j} behind the region" for j in range(4)] +
    ["step back, first half", "step back, second half", "first hop of a walk behind a 0xFF byte"] +
    [f"literal extension byte {b}, {h}" for b in (0, 254, 255) for h in ("first half", "second half")] +
    [f"successor at end_r {d:+d}" for d in (-1, 0, 1)] + [f"successor at fe {d:+d}" for d in (-1, 0, 1)] +
    ["would land on staged byte -2", "would land on staged byte -1"] +
    [f"mode 1 merges on hop {n}" for n in range(1, 5)] +
    ["mode 1 leaves the region unmerged, odd hops", "mode 1 leaves the region unmerged, even hops", "a third pass runs",
     "64 regions with 1..6 hops side by side"])


def _stop_after(k):
    w = Writer().fill_to(REGION, k).fill_to(2 * REGION, 2)
    return w.end(tail=60)


def _fe_after(k, j):
    """Region 0 is the last one: k plain hops, then a token that reaches past fe = 256 + j."""
    w = Writer().fill_to(200, k).sized(60)
    return w.end(total=REGION + 24 + j)


def _step_back(hop):
    """The token in front of hop number `hop` of lane 0's walk has match nibble 15 and the extension bytes 0xFF, 7."""
    w = Writer()
    if hop > 2:
        w.fill_to(12 * (hop - 2), hop - 2)
    w.sized(14, mn=15, mext=b"\xff\x07")
    w.fill_to(REGION, 3).fill_to(2 * REGION, 2)
    return w.end(tail=60)


def _lit_ext(b, hop):
    """Hop number `hop` of lane 0's walk reads a literal length of 15 + 255 * (b == 255) + b's last byte."""
    w = Writer()
    if hop > 1:
        w.fill_to(10 * (hop - 1), hop - 1)
    if b == 255:
        w.tok(15 + 255 + 3)
        w.fill_to(3 * REGION, 4)
    else:
        w.tok(15 + b)
        w.fill_to(2 * REGION, 3 if b == 0 else 1)
    return w.end(tail=60)


def _first_hop_behind_ff():
    """Region 1 starts inside a literal run: 0xFF in front of the region start, bytes that read as tokens from it on."""
    w = Writer().fill_to(240, 3)
    lit = bytes(13) + b"\xff" + bytes([0x20, 9, 9, 9, 9]) + bytes(11)
    w.tok(len(lit), lit=lit)
    assert w.b[REGION - 1] == 255 and w.b[REGION] == 0x20
    w.fill_to(2 * REGION, 2)
    return w.end(tail=60)


def _succ_end_r(d):
    w = Writer().fill_to(REGION + d, 3).fill_to(2 * REGION, 4).fill_to(3 * REGION, 2)
    return w.end(tail=60)


def _succ_fe(d):
    """fe = 400 lies inside region 1; a token of region 1 whose successor is at fe + d."""
    w = Writer().fill_to(REGION, 2).fill_to(330, 2).fill_to(400 + d, 1)
    return w.end(total=424)


def _staged_end(d):
    """Two chunks; a hop of chunk 0's last region whose successor is staged byte CHUNK - 2 + d."""
    w = Writer()
    for i in range(1, 64):
        w.fill_to(REGION * i, 2)
    w.fill_to(CHUNK - 100, 2).fill_to(CHUNK - 2 + d, 1).fill_to(CHUNK + 300, 5)
    return w.end(tail=60)


def _mode1(delta, t0, sizes, regions=2):
    """A token straddles into region 1 and ends at 256 + delta: the region's true entry.  Its literals at the region start read as a
    token t0; true tokens of `sizes` (cycled) follow to the end of region `regions`, then two regions of two."""
    w = Writer().fill_to(200, 2)
    L = REGION + delta - 200 - 4                             # token, one length byte, L literals, offset
    lit = bytearray(L)
    lit[REGION - 202] = t0
    w.tok(L, lit=bytes(lit))
    assert w.pos == REGION + delta and w.b[REGION] == t0
    i = 0
    while w.pos + sizes[i % len(sizes)] <= (regions + 1) * REGION - 3:
        w.sized(sizes[i % len(sizes)]); i += 1
    w.fill_to((regions + 2) * REGION, 2).fill_to((regions + 4) * REGION, 4)
    return w.end(tail=60)


def _mixed64():
    w = Writer()
    for i in range(64):
        w.fill_to(REGION * (i + 1), [4, 1, 6, 2, 5, 3][i % 6] if i else 4)
    return w.end(total=CHUNK + 700)


def _two_chunks(seed):
    """Two chunks of short sequences with a 0xFF extension now and then: chunk 1's run-in and its owned regions both exist."""
    rng = np.random.default_rng(seed)
    w = Writer().tok(5)
    while w.pos < STRIDE + 300 + 40 * seed:
        r = int(rng.integers(0, 40))
        if r == 0:
            w.tok(int(rng.integers(0, 4)), mn=15, mext=b"\xff" + bytes([int(rng.integers(0, 200))]))
        elif r == 1:
            w.tok(15 + 255 + int(rng.integers(0, 30)))
        elif r == 2:
            w.tok(15 + int(rng.choice([0, 254])))
        elif r <= 4:
            w.tok(int(rng.integers(0, 15)), mn=15, mext=bytes([int(rng.integers(0, 255))]))
        else:
            w.tok(int(rng.integers(0, 15)), mn=int(rng.integers(0, 15)))
    return w.end(tail=50)


def all_cases():
    """[(name, block)] — what each is for is in its name; census() says what it reaches."""
    cases = [(f"stop after {k} plain hops", _stop_after(k)) for k in range(1, 6)]
    cases += [(f"fe after {k} plain hops, input ends 24 + {j} behind the region", _fe_after(k, j)) for k in range(1, 6) for j in range(4)]
    cases += [(f"step back found by hop {h}", _step_back(h)) for h in (2, 3, 4, 5)]
    cases += [("first hop behind a 0xFF byte", _first_hop_behind_ff())]
    cases += [(f"literal extension byte {b} on hop {h}", _lit_ext(b, h)) for b in (0, 254, 255) for h in (1, 2, 3, 4)]
    cases += [(f"successor at end_r {d:+d}", _succ_end_r(d)) for d in (-1, 0, 1)]
    cases += [(f"successor at fe {d:+d}", _succ_fe(d)) for d in (-1, 0, 1)]
    cases += [(f"successor on staged byte {d - 2}", _staged_end(d)) for d in (0, 1)]
    cases += [(f"mode 1: {name}", _mode1(*a)) for name, a in MODE1]
    cases += [("64 regions, 1..6 hops", _mixed64())]
    cases += [(f"two chunks, seed {s}", _two_chunks(s)) for s in (1, 2)]
    return cases


def built_for():
    """{case name: the edges that case was built to reach} — every case of all_cases() has an entry (the two-chunk cases: none)."""
    m = {f"stop after {k} plain hops": (f"stop after {k} plain hops",) for k in range(1, 6)}
    for k in range(1, 6):
        for j in range(4):
            m[f"fe after {k} plain hops, input ends 24 + {j} behind the region"] = (f"fe after {k} plain hops", f"input ends 24 + {j} behind the region")
    for h in (2, 3, 4, 5):
        m[f"step back found by hop {h}"] = (f"step back, {_half(h)}",)
    m["first hop behind a 0xFF byte"] = ("first hop of a walk behind a 0xFF byte",)
    for b in (0, 254, 255):
        for h in (1, 2, 3, 4):
            m[f"literal extension byte {b} on hop {h}"] = (f"literal extension byte {b}, {_half(h)}",)
    for d in (-1, 0, 1):
        m[f"successor at end_r {d:+d}"] = (f"successor at end_r {d:+d}",)
        m[f"successor at fe {d:+d}"] = (f"successor at fe {d:+d}",)
    for d in (0, 1):
        m[f"successor on staged byte {d - 2}"] = (f"would land on staged byte {d - 2}",)
    for n in range(1, 5):
        m[f"mode 1: merges on hop {n}"] = (f"mode 1 merges on hop {n}",)
    m["mode 1: never merges, 3-byte sequences from 256 + 4"] = ("mode 1 leaves the region unmerged, even hops",)
    m["mode 1: never merges, 3-byte sequences from 256 + 7"] = ("mode 1 leaves the region unmerged, odd hops",)
    m["mode 1: never merges in two regions"] = ("a third pass runs",)
    m["64 regions, 1..6 hops"] = ("64 regions with 1..6 hops side by side",)
    m.update({f"two chunks, seed {s}": () for s in (1, 2)})
    return m


# (true entry 256 + delta, the byte read as a token at the region start, the true sequences' sizes, regions they fill)
MODE1 = [
    ("merges on hop 1", (5, 0x20, (7, 5, 9), 1)),
    ("merges on hop 2", (5, 0x90, (7, 5, 9), 1)),
    ("merges on hop 3", (5, 0xe0, (7, 5, 9), 1)),
    ("merges on hop 4", (4, 0xf0, (7, 5, 9), 1)),
    ("never merges, 3-byte sequences from 256 + 4", (4, 0x20, (3,), 1)),
    ("never merges, 3-byte sequences from 256 + 7", (7, 0x50, (3,), 1)),
    ("never merges in two regions", (4, 0x20, (3,), 2)),
]
