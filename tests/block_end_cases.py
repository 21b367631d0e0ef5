"""Cases of the block-end sweep (test_block_end_cases_cpu.py, block_end_check.py, test_gpu_block_ends.py): raw blocks cut at every byte,
with the cut placed at the chunk, tile and window boundaries of every kernel that walks tokens.

The reference's loop (src/raw/decompress.rs:58-78) ends in seven ways, by where the input stops:

    1  empty input                                      Ok, nothing written
    2  inside a literal-length run                      UnexpectedEnd (:63)
    3  inside the literals                              UnexpectedEnd (:67; the literals are not limit-checked)
    4  right behind the literals                        Ok (the conformant end)
    5  one byte where an offset should start            Ok (:70 read_u16 fails, the byte is dropped, the loop stops)
    6  inside a match-length run                        UnexpectedEnd (:71, in front of the limit :72-74 and the offset tests :83-89)
    7  right behind a complete match                    Ok (non-conformant LZ4, accepted)

classify() is that walk, written from the reference; every EXPECTATION is the oracle's (oracle_ffi.decompress_raw: the status and, on Ok,
the bytes; verify_cases.expect for the verify call's MISMATCH results).  test_block_end_cases_cpu.py holds the two against each other.

A job is dict(name, block, blk, k, prefix, existing, limit, cap, end, exp): the input is blk[:k] (`block` is the index of blk in the
list decode_jobs() returns: the aliased layout keeps ONE device copy of every block and gives every cut of it as an input_len), `cap` the smallest
out_cap the decode call is given (the oracle's decoded length on Ok), `end` classify()'s class, exp = (status, bytes incl. existing).

    sweep_jobs()        fill8(F) ++ TAIL cut at every k in [max(0, F - 32), len], long literal runs thinned to their first and last four
                        cuts, for every front length F of FRONTS: the tail's first token 40 bytes in front of a boundary, and a second
                        front that puts the boundary between the literals and the offset of a tail sequence
    giant_jobs()        one token whose literals are longer than a whole chunk, cut through its length runs, its offset and behind it
    dropped_jobs()      blocks that end `literals ++ b`, b in 00 0F F0 FF (each would read as another token), behind 0, 1, 64 sequences
    precedence_jobs()   UnexpectedEnd in front of out_cap, the limit and both offset errors; the limit in front of both offset errors
                        on a complete last sequence; each alone and behind a prefix and existing output, at the start of the input
                        and in a later chunk

What each stage in front of a fallback must finish ITSELF (block_end_check.py asserts it, per end class):
    the segmented pipeline (lzf_debug_seg)   every job seg_stage_cases.Model.gives_up is None for: ends 1 (no token, no tile), 4, 5 and 7
    the fed kernel (lzf_debug_fed)           every Ok job it is eligible for: ends 4, 5 and 7.  End 1 it hands to the pair kernel BY DESIGN:
                                             the forced path's smallest input is 1 byte (LZF_FED_MIN_IN=1), an empty input is not in its window
    the size and verify classes              every Ok job (lzf_size_rules.h: clean tiles): reserved = the job's tile count, ends 1 (0 tiles), 4, 5, 7
and every job with an error is left, untouched, to the kernel behind."""
import os
import re

import numpy as np

import oracle_ffi as o
import verify_cases as V
from verify_cases import MISMATCH, _rand, fill8, seq

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-lz-fear_amd", "csrc")

WAVE = 64
# the boundaries, as the kernels' headers state them (header_constants() reads them back; the CPU test holds these copies to it)
FED_ROUND = 1024            # kFedwRound; 64 lanes x 16 bytes: a chunk of the batched kernel's staged16 form
FED_STAGE = 1024 + 128      # the fed kernel's staged window (lz4_decompress_fed.hip: kCB = kRound + 128)
SEG_TILE = 2048             # kSegTile
TILE_STAGE = 2048 + 128     # kTileStage (lzf_seg_common.h)
SEG_CHUNK = 16384           # kSegChunk = kFedwChunk
SEG_STRIDE = 16384 - 2048   # kSegStride = kFedwStride
REGIONS = (16, 24, 48)      # region bytes of staged16 / paired16, paired24, paired48 + the size and verify kernels: a chunk is 64 regions
BOUNDARIES = (("start of input", 0), ("batched S = 16, fed round", FED_ROUND), ("fed staged window", FED_STAGE), ("pair S = 24", WAVE * 24),
              ("seg tile", SEG_TILE), ("staged tile", TILE_STAGE), ("pair, size and verify S = 48", WAVE * 48), ("seg stride", SEG_STRIDE),
              ("seg chunk", SEG_CHUNK), ("second chunk", SEG_CHUNK + SEG_STRIDE))
assert [b for _, b in BOUNDARIES] == [0, 1024, 1152, 1536, 2048, 2176, 3072, 14336, 16384, 16384 + 14336]
BACK = 40                   # the tail's first token lies this far in front of a boundary
THIN = 4                    # cuts kept at either end of a long literal run
OK_ENDS = (1, 4, 5, 7)
UNEXPECTED_END, LIMIT, ZERO_OFFSET, INVALID_OFFSET = 1, 2, 3, 4


def header_constants():
    """The same numbers read from kernels.h, lzf_dispatch.h, lzf_fed_window.h (and the two files that size a staged window)."""
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def num(text, pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    fw, kh, dh = src("lzf_fed_window.h"), src("kernels.h"), src("lzf_dispatch.h")
    chunk, overlap = num(fw, r"kFedwChunk = (\d+),"), num(fw, r"kFedwOverlap = (\d+),")
    assert re.search(r"kFedwStride = kFedwChunk - kFedwOverlap,", fw)
    assert re.search(r"kSegChunk = 64u \* kSegRegion, kSegOverlap = (\d+), kSegStride = kSegChunk - kSegOverlap", kh) and num(kh, r"kSegRegion = (\d+),") * 64 == chunk
    assert re.search(r"static_assert\(kSegChunk == \(uint32_t\)kFedwChunk && kSegOverlap == \(uint32_t\)kFedwOverlap", kh)
    assert re.search(r"kSegChunk = \(uint32_t\)kFedwChunk, kSegStride = \(uint32_t\)kFedwStride", dh)
    tile = num(kh, r"kSegTile = (\d+);")
    assert num(dh, r"kSegTile = (\d+)u;") == tile
    assert re.search(r"constexpr uint32_t kTileStage = kSegTile \+ (\d+)u;", src("lzf_seg_common.h"))
    rnd = num(fw, r"kFedwRound = (\d+),")
    regions = {int(m.group(2)) for m in re.finditer(r"X\((staged16|paired16|paired24|paired48), 4096, (\d+),", kh)}
    regions |= {int(m.group(1)) for m in re.finditer(r"lzf_(?:decoded_size|verify)_kernel<(\d+), 768, false>", kh)}
    return dict(FED_ROUND=rnd, FED_STAGE=rnd + num(src("lz4_decompress_fed.hip"), r"kCB = kRound \+ (\d+)u;"), SEG_TILE=tile,
                TILE_STAGE=tile + num(src("lzf_seg_common.h"), r"kTileStage = kSegTile \+ (\d+)u;"), SEG_CHUNK=chunk, SEG_STRIDE=chunk - overlap,
                REGIONS=tuple(sorted(regions)))


# ------------------------------------------------------------------------------------------------------------------- the walk
def classify(b):
    """Which of the seven ends the byte string has: the plain walk of decompress.rs:61-71, no copies and no checks but the reads."""
    n, p = len(b), 0
    if n == 0:
        return 1
    while p < n:                                   # :61 read_u8
        tok = b[p]; p += 1
        L = tok >> 4
        if L == 15:                                # :63 read_lsic
            while True:
                if p >= n:
                    return 2
                more = b[p]; p += 1
                L += more
                if more != 255:
                    break
        if n - p < L:                              # :67 read_exact
            return 3
        p += L
        if n - p < 2:                              # :70 read_u16 fails: no match; a byte that is left is dropped
            return 4 if n == p else 5
        p += 2
        if tok & 15 == 15:                         # :71 read_lsic
            while True:
                if p >= n:
                    return 6
                more = b[p]; p += 1
                if more != 255:
                    break
    return 7                                       # `while let Ok(token)` fails behind a complete match


# ------------------------------------------------------------------------------------------------------------------- the tail
def _tail():
    """[(what, bytes)]: every token form.  The head is laid out byte by byte: the sequence at 18 is five bytes — token, one literal, offset,
    one match-length byte — so that the cuts 18 .. 22 are ends 7, 3, 4, 5, 6; the sequence at 34 puts ends 4, 5, 7 on the cuts 38 .. 40, and
    the literal-length token at 40 ends 2 and 3 on 41 and 42.  A front of B - 40 and one of B - 20 thus put every end within 2 bytes of B."""
    r = lambda seed, n: bytes(0x61 + (x % 26) for x in _rand(seed, n))      # noqa: E731
    t = [("a plain token", seq(b"plain!", 3, 6)),
         ("L = 0", seq(b"", 2, 8)),
         ("the smallest match, M = 4", seq(b"abc", 5, 4)),
         ("one literal, match nibble 15 with one length byte", seq(b"q", 4, 19 + 3)),
         ("a plain token", seq(r(1, 8), 6, 5)),
         ("a plain token", seq(b"xyz", 9, 7)),
         ("literal nibble 15, one length byte", seq(r(2, 15 + 20), 7, 9)),
         ("literal nibble 15, two length bytes", seq(r(3, 15 + 255 + 10), 300, 12)),
         ("literal nibble 15, three length bytes", seq(r(4, 15 + 510 + 5), 64, 6)),
         ("match nibble 15, one length byte", seq(b"mn", 2, 19 + 30)),
         ("match nibble 15, two length bytes", seq(b"opq", 500, 19 + 255 + 7)),
         ("match nibble 15, three length bytes", seq(b"r", 17, 19 + 510 + 3)),
         ("both nibbles 15", seq(r(5, 15 + 5), 11, 19 + 21)),
         ("both nibbles 15, a length byte of 0", seq(r(6, 15), 33, 19)),
         ("an overlapping match at offset 1", seq(b"z", 1, 30)),
         ("L = 0 and M = 4", seq(b"", 8, 4)),
         ("last literals", seq(b"the end", None, 0))]
    at = np.cumsum([0] + [len(b) for _, b in t]).tolist()
    assert at[3] == 18 and len(t[3][1]) == 5 and at[5] == 34 and at[6] == BACK
    return t


TAIL_SEQS = _tail()
TAIL = b"".join(b for _, b in TAIL_SEQS)
MICRO_OFFSET_AT = 20                                # the tail position of the offset of the five-byte sequence: literals | offset
FRONTS = [(0, BOUNDARIES[0])] + [(b - back, (name, b)) for name, b in BOUNDARIES[1:] for back in (BACK, MICRO_OFFSET_AT)]


def block_of(front):
    return (fill8(front, salt=front) if front else b"") + TAIL


def thinned(blk, lo, at=0):
    """The cut positions lo .. len(blk), less the middle of the literal runs of more than 2 * THIN + 1 bytes of the sequences from `at` on."""
    keep = set(range(lo, len(blk) + 1))
    for p, _, L, _, _ in V.walk(blk[at:]):
        lit0 = at + p + 1 + ((L - 15) // 255 + 1 if L >= 15 else 0)                 # the first literal; cut lit0 + i holds i literals
        if L > 2 * THIN + 1:
            keep -= set(range(lit0 + THIN + 1, lit0 + L - THIN))
    return sorted(keep)


def cuts_of(front):
    """The cut positions of block_of(front): every k of [max(0, front - 32), len], less the middle of the tail's long literal runs."""
    return thinned(block_of(front), max(0, front - 32), at=front)


# ------------------------------------------------------------------------------------------------------------------- jobs
class Blocks:
    """The distinct blocks, in the order they were first used."""

    def __init__(self):
        self.list, self.index, self.full = [], {}, {}

    def add(self, blk):
        if blk not in self.index:
            self.index[blk] = len(self.list); self.list.append(blk)
        return self.index[blk]


def _job(blocks, name, blk, k, prefix=b"", existing=b"", limit=None, cap=None):
    """cap None: the oracle's decoded length on Ok, room for the whole block's decode otherwise."""
    key = (blk, prefix, existing)
    if key not in blocks.full:                      # the whole block's decode, whatever its status: how much room a cut of it may need
        blocks.full[key] = len(o.decompress_raw(blk, prefix=prefix, existing=existing, limit=1 << 30, cap=len(existing) + 300 * len(blk) + 64)[1])
    room = blocks.full[key] + 64
    limit = blocks.full[key] + len(blk) if limit is None else limit
    rc, dec = o.decompress_raw(blk[:k], prefix=prefix, existing=existing, limit=limit, cap=room if cap is None else cap)
    assert rc != o.OUT_CAPACITY, name
    if cap is None:
        cap = len(dec) if rc == 0 else room
    return dict(name=name, block=blocks.add(blk), blk=blk, k=k, prefix=prefix, existing=existing, limit=limit, cap=cap, end=classify(blk[:k]),
                exp=(rc, dec))


def sweep_jobs(blocks, fronts=None):
    out = []
    for front, (bname, b) in FRONTS:
        if fronts is not None and front not in fronts:
            continue
        blk = block_of(front)
        assert len(blk) == front + len(TAIL)
        for k in cuts_of(front):
            out.append(dict(_job(blocks, f"front {front} ({bname} {b}), cut {k}", blk, k), front=front, boundary=b))
    return out


DROPPED = (0x00, 0x0F, 0xF0, 0xFF)


def dropped_jobs(blocks):
    out = []
    for nseq in (0, 1, 64):
        head = b"".join(seq(bytes([0x41 + j % 26]) * 3 + bytes([0x30 + j % 10]), 2, 6) for j in range(nseq))
        for b in DROPPED:
            blk = head + seq(b"last!", None, 0) + bytes([b])
            j = _job(blocks, f"dropped byte {b:02X} behind {nseq} sequences", blk, len(blk))
            out.append(dict(j, want=(0, 5)))
    return out


def precedence_jobs(blocks):
    """[(job with `want`: the status the name says)]"""
    out = []
    pre, ex = _rand(71, 10), _rand(72, 20)
    for where, front in (("first in the input", 0), ("in a later chunk", WAVE * 48 - 8)):
        head = fill8(front, salt=5) if front else b""
        grown = 9 * (front // 8) + front % 8                                  # fill8's output
        for hist, (p, e) in (("", (b"", b"")), (", behind a prefix and existing output", (pre, ex))):
            base = len(e) + grown
            lit = _rand(73, 40)
            # UnexpectedEnd inside the literals, out_cap and output_limit both short of the announced run
            blk = head + seq(lit, 3, 8)
            out.append(dict(_job(blocks, f"precedence/{where}{hist}: cut inside the literals, out_cap and limit below them", blk, front + 2 + 20, p, e,
                                 limit=base + 10, cap=base + 10), want=(UNEXPECTED_END, 3)))
            # a match of 19 + 255 + 50 that would pass output_limit / has offset 0 / reaches one byte beyond existing + prefix: cut inside its length
            M = 19 + 255 + 50
            beyond = len(p) + base + 4 + 1
            for what, off, limit in (("a match that would pass output_limit", 2, base + 4 + 10), ("offset 0", 0, base + 4 + 10),
                                     ("an offset one beyond existing + prefix", beyond, base + 4 + 10)):
                s = seq(b"abcd", off, M)
                assert len(s) == 1 + 4 + 2 + 2
                blk = head + s
                out.append(dict(_job(blocks, f"precedence/{where}{hist}: cut inside the match length of {what}", blk, len(blk) - 1, p, e, limit=limit),
                                want=(UNEXPECTED_END, 6)))
                # ... and complete, last in the block: the limit wins
                out.append(dict(_job(blocks, f"precedence/{where}{hist}: {what}, complete and last", blk, len(blk), p, e, limit=limit), want=(LIMIT, 7)))
            # the offset errors alone (the limit far away), complete and last: end 7 with their own status
            for what, off, st in (("offset 0", 0, ZERO_OFFSET), ("an offset one beyond existing + prefix", beyond, INVALID_OFFSET)):
                blk = head + seq(b"abcd", off, M)
                out.append(dict(_job(blocks, f"precedence/{where}{hist}: {what} within the limit, complete and last", blk, len(blk), p, e, limit=base + 4 + M + 100),
                                want=(st, 7)))
    return out


GIANTS = (WAVE * 48 + 300, SEG_CHUNK + 600)        # literals of one token: beyond a chunk of the one-wave kernels, beyond every chunk and tile


def giant_jobs(blocks):
    """A token whose body is longer than a whole chunk is taken in one step by most kernels (the size and verify kernels look at it ahead
    of the parse, the pipeline's parse jumps over chunks): 64 bytes of sequences, the token — long literals and a match length of three
    bytes — and last literals, the token first in the input and behind 64 bytes, cut at every byte of its two length runs, around its literals' ends, in its offset and behind it."""
    out = []
    for L in GIANTS:
        for front in (0, 64):                       # first in the input: the kernels that look at a chunk's first token ahead of the parse take it there
            blk = (fill8(front, salt=L) if front else b"") + seq(_rand(L, L), 70, 19 + 510 + 9) + seq(b"end", None, 0)
            for k in thinned(blk, front, at=front):
                out.append(dict(_job(blocks, f"giant/{L} literals in one token behind {front} bytes, cut {k}", blk, k), giant=L))
    return out


def decode_jobs():
    """(blocks, jobs): the sweep and the three lists."""
    blocks = Blocks()
    jobs = sweep_jobs(blocks) + dropped_jobs(blocks) + precedence_jobs(blocks) + giant_jobs(blocks)
    assert len({j["name"] for j in jobs}) == len(jobs)
    return blocks.list, jobs


CARVED_FRONTS = (0, WAVE * 48 - BACK)


def carved(jobs):
    """The sample of the carved layout: every cut of the front-0 block and of the 3072 block, and the three lists."""
    return [j for j in jobs if j.get("front", CARVED_FRONTS[0]) in CARVED_FRONTS]


# ------------------------------------------------------------------------------------------------------------------- the verify call
def verify_case(j, flip=None):
    """verify_cases' dict for a job: mem = existing ++ the EXPECTED bytes — the oracle's decode, with out_cap its length (64 wrong
    bytes where the input does not decode) — ++ what lies behind out_cap; flip: a position of the expected bytes changed by one bit."""
    rc, dec = j["exp"]
    mem = bytearray(dec if rc == 0 else j["existing"] + b"\x55" * 64)
    n = len(mem)
    behind = bytes((b ^ 0xA5) for b in mem[-1:] or b"\x00") * 3 + b"\x00" * 29
    if flip is not None:
        assert len(j["existing"]) <= flip < n
        mem[flip] ^= 0x01
    return dict(name=j["name"] + (f", flip at {flip}" if flip is not None else ""), input=j["blk"][:j["k"]], prefix=j["prefix"], prefix_len=len(j["prefix"]),
                existing_len=len(j["existing"]), mem=bytes(mem) + behind, out_cap=n, limit=j["limit"])


def verify_jobs(jobs):
    """[(index of the job, flip or None, (status, out_len or None))]: every job against its expected bytes, and every Ok job once more
    with one byte flipped in the output of its last sequence that has any.  The expectation is verify_cases.expect's (decode-then-compare)."""
    out = []
    for i, j in enumerate(jobs):
        c = verify_case(j)
        out.append((i, None, V.expect(c)))
        if j["exp"][0] == 0 and c["out_cap"] > c["existing_len"]:
            at = c["existing_len"] + [t for t in V.walk(c["input"]) if t[2] + t[3]][-1][1]
            e = V.expect(verify_case(j, at))
            assert e == (MISMATCH, at), (j["name"], at, e)
            out.append((i, at, e))
    return out


# ------------------------------------------------------------------------------------------------------------------- the census
def census(jobs):
    """{front: {end: cuts}} and {boundary: {end: cuts within 2 bytes of it}} over the sweep's jobs."""
    per_front, near = {}, {}
    for j in jobs:
        if "front" not in j:
            continue
        f = per_front.setdefault(j["front"], dict.fromkeys(range(1, 8), 0))
        f[j["end"]] += 1
        if j["boundary"] and abs(j["k"] - j["boundary"]) <= 2:
            b = near.setdefault(j["boundary"], dict.fromkeys(range(1, 8), 0))
            b[j["end"]] += 1
    return per_front, near


def counts():
    """The number of jobs of each kind, from the construction alone (no oracle): what every setting of the GPU test must report."""
    sweep = sum(len(cuts_of(f)) for f, _ in FRONTS)
    carved_sweep = sum(len(cuts_of(f)) for f in CARVED_FRONTS)
    giants = 2 * sum(2 + (L - 15) // 255 + 1 + 2 * THIN + 1 + 2 + 3 + 4 for L in GIANTS)      # token, length run, literal ends, offset, match length run, last literals
    lists = 3 * len(DROPPED) + 2 * 2 * (1 + 3 * 2 + 2) + giants
    return dict(all=sweep + lists, carved=carved_sweep + lists)


# what every setting of the GPU test reports (test_block_end_cases_cpu.py holds the three to the construction)
COUNTS = dict(all=3678, carved=618, verify=4873)
