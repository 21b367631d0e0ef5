"""The cases of the compressed-size calls (lzf_compressed_size_batch and the frame / stream calls above it), built once, with
every expectation pinned to the oracle (tests/oracle_ffi.py) on the CPU.  tests/test_compressed_size_cases_cpu.py proves by a census
of the oracle's own output that each class is reached in the reference; tests/compressed_size_check.py runs the cases on the GPU.

A case is a list of CALLS, a call a list of JOBS run as one batch; a job names a table SLOT of its case or none (a fresh table):
    job   dict(input, cursor, kind, cap (None: UINT64_MAX), slot (None | key), readonly, in_low (None | the input address's low bits))
    case  dict(name, cls, calls, tables {slot: dict(kind, init = the table's bytes before call 0)}, adds [per call {slot: offset added
          before the call}], kinds (None: from the jobs | the table_kinds word of every call), contract [(call, job)]: jobs that break the
          LZF_KINDS_U32_FRESH_ONLY promise of `kinds`)
expectations(case) -> per call (results [(status, out_len)], tables {slot: bytes after the call}).

out_len on LZF_OUTPUT_FULL is the library's: the bytes in front of the refused sequence (a sequence is written whole or not at all;
the reference's writer is dropped with the error, src/framed/compress.rs:250-255, so its partial count is nobody's).  It is pinned to
the oracle all the same: the start of the first sequence of the oracle's unbounded output that ends beyond the capacity."""
import ctypes as C
import functools

import numpy as np

import oracle_ffi as o

U32, U16 = o.TABLE_U32, o.TABLE_U16
KINDS_U32, KINDS_U16, KINDS_FRESH_ONLY = 1, 2, 4
UINT64_MAX = (1 << 64) - 1


def bound(n):
    return n + n // 255 + 64


def _rng(seed):
    return np.random.default_rng(seed)


def rand(n, seed):
    return _rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def texty(n, seed, symbols=6):
    """few symbols: short matches everywhere"""
    return _rng(seed).integers(97, 97 + symbols, n, dtype=np.uint8).tobytes()


def tiled(n, seed, period=5000, flip=97):
    """a random block repeated with one byte changed every `flip` bytes: matches of ~flip bytes at distance `period`, everywhere"""
    r = _rng(seed)
    base = r.integers(0, 256, period, dtype=np.uint8)
    a = np.tile(base, n // period + 1)[:n].copy()
    a[period + flip // 2::flip] ^= 0x55
    return a.tobytes()


def epoch_input(n, seed):
    """tiled, with a changed byte right in front of every 64 KiB boundary: the match in flight ends there, and the next one starts at
    the boundary or just behind it, its source 5000 bytes back — in the epoch before"""
    a = bytearray(tiled(n, seed))
    for e in range(65536, n, 65536):
        a[e - 1] ^= 0xAA
    return bytes(a)


def job(data, cursor=0, kind=U32, cap=None, slot=None, readonly=False, in_low=None):
    return dict(input=bytes(data), cursor=cursor, kind=kind, cap=cap, slot=slot, readonly=readonly, in_low=in_low)


def case(name, cls, calls, tables=None, adds=None, kinds=None, contract=()):
    calls = [list(c) for c in calls]
    return dict(name=name, cls=cls, calls=calls, tables=tables or {}, adds=adds or [{} for _ in calls], kinds=kinds, contract=list(contract))


def sequences(block):
    """The sequences of an LZ4 block: (start, literal_len, offset, match_len, end); offset 0 / match_len 0 for the last literals."""
    out, p, n = [], 0, len(block)
    while p < n:
        start = p
        tok = block[p]; p += 1
        L = tok >> 4
        if L == 15:
            while block[p] == 255:
                L += 255; p += 1
            L += block[p]; p += 1
        p += L
        if p >= n:
            out.append((start, L, 0, 0, p))
            break
        off = block[p] | (block[p + 1] << 8); p += 2
        M = tok & 15
        if M == 15:
            while block[p] == 255:
                M += 255; p += 1
            M += block[p]; p += 1
        out.append((start, L, off, M + 4, p))
    return out


def seeded_table(dictionary):
    """A U32 table as compress2 over `dictionary` leaves it: positions inside the dictionary, offset 0."""
    t = o.new_table(U32)
    o.compress2(dictionary, table=t)
    return bytes(t)


# ---- the case list ---------------------------------------------------------------------------------------------------------------

def lsic_literals(L, seed):
    x, y, tail = rand(8, seed), rand(L - 8, seed + 1), bytearray(rand(16, seed + 2))
    tail[0] = y[0] ^ 0xFF
    return x + y + x + bytes(tail)


def lsic_match(M, seed):
    x, y, tail = rand(M, seed), rand(20, seed + 1), bytearray(rand(16, seed + 2))
    tail[0] = y[0] ^ 0xFF
    return x + y + x + bytes(tail)


REPEAT256 = bytes(range(256)) * 258
REPEAT256 = REPEAT256[:256 + 65535 + 5]
CAP_INPUT = texty(20000, 11)
DICT = texty(4096, 21)
CHAIN2 = texty(32768, 31) + texty(32768, 31)[:20000] + texty(12768, 32)                    # block 1 starts as block 0 does
CHAIN3 = tiled(196608, 41, period=40000)
ALIGN_INPUT = texty(3000, 51)
BIG = tiled(5000 * 1024, 61, period=300, flip=41)
MIXED = tiled(300 * 700, 71, period=3000, flip=61)


@functools.lru_cache(maxsize=None)
def cases():
    cs = []
    tiny = []
    for n in (0, 1, 12, 13):
        d = rand(n, 100 + n)
        for cur in sorted({0, n, 1 if n > 1 else 0, n - 1 if n > 1 else 0}):
            tiny += [job(d, cursor=cur), job(d, cursor=cur, kind=U16)]
    cs.append(case("tiny inputs", "tiny", [tiny]))
    cs.append(case("lsic edges", "lsic", [[job(lsic_literals(L, 200 + L)) for L in (14, 15, 269, 270)] +
                                          [job(lsic_match(M, 300 + M)) for M in (18, 19, 273, 274)] +
                                          [job(lsic_literals(L, 200 + L), kind=U16) for L in (14, 15, 269, 270)] +
                                          [job(lsic_match(M, 300 + M), kind=U16) for M in (18, 19, 273, 274)]]))
    cs.append(case("repeat256", "repeat256", [[job(REPEAT256)]]))
    c_exact = len(o.compress2(CAP_INPUT)[1])
    cs.append(case("capacities", "caps", [[job(CAP_INPUT, cap=c) for c in (c_exact, c_exact - 1, 0, None)] +
                                          [job(CAP_INPUT[:12000], kind=U16, cap=c) for c in (len(o.compress2(CAP_INPUT[:12000], kind=U16)[1]) - 1, 0, None)]]))
    block = texty(3000, 22) + DICT[100:1500] + texty(800, 23)
    cs.append(case("read-only template", "template", [[job(DICT + block, cursor=len(DICT), slot="tmpl", readonly=True),
                                                       job(DICT + block[:1500], cursor=len(DICT), slot="tmpl", readonly=True),
                                                       job(block)]],
                   tables={"tmpl": dict(kind=U32, init=seeded_table(DICT))}))
    cs.append(case("u16 limits", "u16", [[job(texty(65535, 81), kind=U16), job(texty(65536, 82), kind=U16)]]))
    empty32 = bytes(o.new_table(U32))
    cs.append(case("two-block chain", "chain", [[job(CHAIN2[:32768], slot="t")], [job(CHAIN2, cursor=32768, slot="t")]],
                   tables={"t": dict(kind=U32, init=empty32)}))
    cs.append(case("three-block chain", "chain", [[job(CHAIN3[:65536], slot="t")], [job(CHAIN3[:131072], cursor=65536, slot="t")],
                                                  [job(CHAIN3[65536:], cursor=65536, slot="t")]],
                   tables={"t": dict(kind=U32, init=empty32)}, adds=[{}, {}, {"t": 65536}]))
    cs.append(case("epoch sweep", "epoch", [[job(epoch_input(65536 + 40, 91)), job(epoch_input(131072 + 40, 92))]]))
    cs.append(case("input residues", "residues", [[job(ALIGN_INPUT, in_low=r) for r in range(16)] + [job(ALIGN_INPUT[:2000], kind=U16, in_low=r) for r in range(16)]]))
    cs.append(case("5000 jobs", "big", [[job(BIG[i * 1024:(i + 1) * 1024]) for i in range(5000)]]))
    cs.append(case("300 mixed jobs", "mixed", [[job(MIXED[i * 700:(i + 1) * 700 + (i % 7) * 13], kind=U16 if i % 3 == 0 else U32) for i in range(300)]]))
    cs.append(case("fresh-only promise", "promise", [[job(CAP_INPUT[:4000]), job(CAP_INPUT[4000:9000]), job(CAP_INPUT[:5000], slot="w"), job(CAP_INPUT[9000:12000])]],
                   tables={"w": dict(kind=U32, init=empty32)}, kinds=KINDS_U32 | KINDS_FRESH_ONLY, contract=[(0, 2)]))
    return cs


def call_kinds(c, call):
    if c["kinds"] is not None:
        return c["kinds"]
    k = 0
    for j in call:
        k |= KINDS_U16 if j["kind"] == U16 else KINDS_U32
    return k


def _table_from(kind, raw):
    t = o.new_table(kind)
    C.memmove(C.addressof(t), raw, len(raw))
    return t


def full_out_len(seqs, cap):
    """the start of the first sequence that ends beyond cap"""
    for s in seqs:
        if s[4] > cap:
            return s[0]
    raise AssertionError("every sequence fits: not an OutputFull case")


@functools.lru_cache(maxsize=None)
def expectations(name):
    """Per call of the case: ([(status, out_len)], {slot: table bytes after the call}, [the oracle's unbounded output per job])."""
    c = next(x for x in cases() if x["name"] == name)
    tables = {k: _table_from(v["kind"], v["init"]) for k, v in c["tables"].items()}
    per_call = []
    for ci, call in enumerate(c["calls"]):
        for slot, add in c["adds"][ci].items():
            tables[slot].offset += add
        res, plain = [], []
        for ji, j in enumerate(call):
            if (ci, ji) in c["contract"]:                       # the API's rule, not compress2's: the promise is broken, nothing runs
                res.append((o.CONTRACT, 0)); plain.append(b"")
                continue
            live = tables[j["slot"]] if j["slot"] is not None else o.new_table(j["kind"])
            before = bytes(live)
            t = _table_from(j["kind"], before) if j["readonly"] else live
            n = len(j["input"]) - min(j["cursor"], len(j["input"]))
            cap = bound(n) if j["cap"] is None else min(j["cap"], bound(n))
            rc, out = o.compress2(j["input"], cursor=j["cursor"], kind=j["kind"], table=t, cap=cap)
            whole = out
            if rc == o.OUTPUT_FULL:
                rc2, whole = o.compress2(j["input"], cursor=j["cursor"], kind=j["kind"], table=_table_from(j["kind"], before), cap=bound(n))
                assert rc2 == o.OK
                res.append((rc, full_out_len(sequences(whole), cap)))
            else:
                res.append((rc, len(out)))
            plain.append(whole)
        per_call.append((res, {k: bytes(t) for k, t in tables.items()}, plain))
    return per_call


# ---- the frame-level cases ---------------------------------------------------------------------------------------------------------

FRAME_BS = 65536


def frame_inputs():
    mid = texty(FRAME_BS, 111) + rand(FRAME_BS, 112) + texty(30000, 113)
    return [b"", b"x", (FRAME_DICT[500:2500] + texty(65536, 114))[:65536], texty(65537, 115), mid]


FRAME_DICT = texty(3000, 116)       # (>= 8 bytes: a template table; the frame inputs repeat parts of it)


def flag_combos():
    """The 32 combinations of independent blocks, block checksums, content checksum, a dictionary and a content size, as
    (settings keywords for oracle_ffi.make_settings and the product's builder, content size in the header?)."""
    out = []
    for m in range(32):
        kw = dict(independent_blocks=bool(m & 1), block_checksums=bool(m & 2), content_checksum=bool(m & 4), block_size=FRAME_BS)
        if m & 8:
            kw["dictionary"] = FRAME_DICT
        out.append((kw, bool(m & 16)))
    return out


def oracle_frame_len(kw, data, with_size):
    rc, frame = o.frame_compress(data, o.make_settings(content_size=len(data) if with_size else None, **kw))
    assert rc == o.OK
    return len(frame)


STREAM_FRAME_BYTES = (65536, 100000)


def stream_inputs():
    big = tiled(1 << 20, 121, period=70000)
    return [b"", b"y", texty(65536, 122), texty(100000, 123) + rand(100001, 124), big]
