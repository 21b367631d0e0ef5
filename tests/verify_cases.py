"""Cases of the verify tests (test_verify_cases_cpu.py, test_gpu_verify.py): raw blocks built sequence by sequence or compressed
by the oracle, the memory a job's `out` points at (history, expected bytes, and what lies behind out_cap), and the expectation.

Every expectation comes from the oracle: lzfo_decompress_raw gives the status and the bytes, numpy the first difference — that is
decode-then-compare, the thing the verify call replaces.  The one exception is LZF_CONTRACT, which the oracle cannot produce; it is
stated by hand, under the size call's own condition (a length of 2 GiB).

A case is dict(name, input, prefix, prefix_len, existing_len, mem, out_cap, limit): `mem` is the memory at `out` — mem[:existing_len]
the history, mem[existing_len:out_cap] the expected bytes, mem[out_cap:] what follows in memory and must not be looked at.  The module
asserts its own preconditions where the cases are built: a planted difference changes exactly the byte it names, and every expected
position is what decode-then-compare gives (expect() is the only source of expectations).

Frames (test_gpu_frame_verify.py) follow at the end: frames written by the oracle, expected-byte variants and damaged frames, with
frame_expect() — the oracle's frame decode compared by numpy — as the only source of their expectations."""
import numpy as np

import oracle_ffi as o
from rust_lz_fear_amd import synth

MISMATCH = 8
CONTRACT = 6
CHUNK = 3072          # compressed bytes one parse of lzf_verify_kernel<48, 768> covers
TOKCAP = 768          # tokens one parse lists
N_FF = 4000           # 0xFF length bytes of a token that reaches beyond a whole chunk
OWN = 64              # bytes of a run a lane compares by itself (lz4_verify.hip: kOwn)
OFFSETS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 64, 65535)
MATCH_LENS = (4, 5, 15, 16, 17, 19, 64, 300)


def _lsic(v):
    return b"\xff" * (v // 255) + bytes([v % 255])


def seq(lit, off, mlen):
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


def fill8(n_bytes, salt=0):
    """Exactly n_bytes (>= 8) of input in 8-byte sequences (5 literals that differ from sequence to sequence, a match of 4 at
    offset 3), the first one longer by n_bytes % 8: 128 tokens per KiB, so a parse is never cut by its token list."""
    def lits(k):
        return bytes(((k * 7 + salt + i * 13) & 0x3F) + 0x30 for i in range(5))
    return seq(lits(0) + b"x" * (n_bytes % 8), 3, 4) + b"".join(seq(lits(k), 3, 4) for k in range(1, n_bytes // 8))


def _rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _oracle(blk, prefix, existing, limit):
    cap = len(existing) + min(limit, 1 << 26) + len(blk) + 64
    rc, dec = o.decompress_raw(blk, prefix=prefix, existing=existing, limit=limit, cap=cap)
    assert rc != o.OUT_CAPACITY
    return rc, dec


def expect(c):
    """(status, out_len or None) by decode-then-compare: the oracle's decode behind the history mem[:existing_len], numpy's first
    difference against mem[:out_cap]."""
    if c["prefix_len"] >= 0x7FFFFF00:
        return CONTRACT, None
    ex, cap = c["existing_len"], c["out_cap"]
    rc, dec = _oracle(c["input"], c["prefix"], c["mem"][:ex], c["limit"])
    if rc != 0:
        return rc, None
    n = len(dec)
    m = min(n, cap)
    if m > ex:
        d = np.flatnonzero(np.frombuffer(dec, dtype=np.uint8)[ex:m] != np.frombuffer(c["mem"], dtype=np.uint8)[ex:m])
        if d.size:
            return MISMATCH, ex + int(d[0])
    if n != cap:
        return MISMATCH, m
    return 0, n


def make(name, blk, prefix=b"", existing=b"", limit=1 << 22, flip=None, cap_delta=0, history=None, prefix_len=None):
    """A case around the block's true decode: mem = history ++ decode (64 wrong bytes where the block does not decode).
    flip: a position of mem whose byte is changed (it must lie in the expected bytes);  cap_delta: out_cap = n + cap_delta, the
    true bytes staying in memory behind a shorter out_cap;  history: other bytes in the place of `existing` in mem."""
    blk, prefix, existing = bytes(blk), bytes(prefix), bytes(existing)
    rc, dec = _oracle(blk, prefix, existing, limit)
    mem = bytearray(dec if rc == 0 else existing + b"\x55" * 64)
    n = len(mem)
    if flip is not None:
        assert len(existing) <= flip < n + min(cap_delta, 0), (name, flip, n)
        before = bytes(mem)
        mem[flip] ^= 0x01
        assert [i for i in range(max(0, flip - 2), min(n, flip + 3)) if mem[i] != before[i]] == [flip] and sum(a != b for a, b in zip(mem, before)) == 1, name
    if history is not None:
        assert len(history) == len(existing)
        mem[:len(existing)] = history
    cap = n + cap_delta
    mem += bytes((b ^ 0xA5) for b in mem[-1:] or b"\x00") * 3 + b"\x00" * 29       # what lies behind: never the bytes that would fit
    c = dict(name=name, input=blk, prefix=prefix, prefix_len=len(prefix) if prefix_len is None else prefix_len,
             existing_len=len(existing), mem=bytes(mem), out_cap=cap, limit=limit)
    return c


def _match_block(off, M, seed):
    """History of at least `off` bytes as literals (as existing output for the longest offset), then one match, then last literals.
    Returns (block, existing, position of the match)."""
    if off == 65535:
        ex = _rand(seed, off)
        return seq(b"", off, M) + seq(b"tail!", None, 0), ex, off
    lit = _rand(seed, max(off, 6) if (seed & 1) else off)      # odd seeds: the source may start behind out[0]; even: at out[0] exactly
    return seq(lit, off, M) + seq(b"tail!", None, 0), b"", len(lit)


def token_cases():
    out = []
    for k in (1, 63, 64, 65):
        blk = b"".join(seq(bytes([0x41 + (j % 26)]) * 3 + bytes([j & 0xFF, 0x30 + j % 10]), 2, 6) for j in range(k - 1)) + seq(b"end", None, 0)
        out.append(make(f"tokens/{k} sequences", blk))
        n = 11 * (k - 1) + 3
        out.append(make(f"tokens/{k} sequences, last byte flipped", blk, flip=n - 1))
        if k > 1:
            out.append(make(f"tokens/{k} sequences, last match flipped", blk, flip=n - 4))
    for n_in in (3071, 3072, 3073, 6200):
        blk = fill8(n_in - 4, salt=n_in) + seq(b"end", None, 0)
        assert len(blk) == n_in
        out.append(make(f"tokens/input of {n_in}", blk))
        c = out[-1]
        for at in (0, c["out_cap"] // 2, c["out_cap"] - 1):
            out.append(make(f"tokens/input of {n_in}, flip at {at}", blk, flip=at))
    lit = _rand(5, 15 + 255 + 40)
    for start in (CHUNK - 10, CHUNK - 2, 2 * CHUNK - 100):
        for tag, s in (("literal run", seq(lit, 5, 8)), ("match", seq(b"ab", 7, 19 + 255 * 2 + 3))):
            blk = fill8(start, salt=start) + s + fill8(200) + seq(b"z", None, 0)
            base = make(f"tokens/{tag} over a chunk end at {start}", blk)
            out.append(base)
            pos = 9 * (start // 8) + start % 8          # output behind fill8(start)
            for at in (pos, pos + 100, pos + (len(lit) if tag == "literal run" else 2 + 19 + 255 * 2 + 3) - 1):
                out.append(make(f"tokens/{tag} over a chunk end at {start}, flip at {at}", blk, flip=at))
    # one token beyond a whole chunk: N_FF length bytes, once as literals, once as a match of about 1 MB at offset 1
    big_l = _rand(6, 15 + 255 * (N_FF - 1) + 77)
    giant_l = seq(big_l, 9, 12)
    giant_m = seq(b"q", 1, 19 + 255 * (N_FF - 1) + 7)
    assert len(giant_l) - len(big_l) - 3 == N_FF and len(giant_m) - 4 == N_FF
    for tag, g, span in (("literals", giant_l, len(big_l)), ("match", giant_m, 1 + 19 + 255 * (N_FF - 1) + 7)):
        blk = fill8(500) + g + fill8(100) + seq(b"end", None, 0)
        pos = 9 * 62 + 500 % 8
        out.append(make(f"tokens/beyond a chunk, {tag}", blk))
        for at in (pos, pos + 1, pos + span // 2, pos + span - 1, pos + span, pos + span + 20):
            out.append(make(f"tokens/beyond a chunk, {tag}, flip at +{at - pos}", blk, flip=at))
        out.append(make(f"tokens/beyond a chunk first, {tag}", g + seq(b"end", None, 0)))
        out.append(make(f"tokens/beyond a chunk first, {tag}, flip at 4100", g + seq(b"end", None, 0), flip=4100))
        out.append(make(f"tokens/beyond a chunk, {tag}, out_cap inside it", blk, cap_delta=-(span // 3 + 130)))
    return out


def match_cases():
    out = []
    for i, off in enumerate(OFFSETS):
        for k, M in enumerate(MATCH_LENS):
            blk, ex, at = _match_block(off, M, 100 + 8 * i + k)
            tag = f"match/off {off} M {M}" + (" (overlapping)" if off < M else "")
            out.append(make(tag, blk, existing=ex))
            out.append(make(tag + ", first byte flipped", blk, existing=ex, flip=at))
            out.append(make(tag + ", last byte flipped", blk, existing=ex, flip=at + M - 1))
    pre = _rand(7, 100)
    hist = _rand(8, 50)
    for M in (4, 20, 64, 65, 300):
        out.append(make(f"match/source wholly in the prefix, M {M}", seq(b"ab", 2 + 100, min(M, 100)) + seq(b"", None, 0), prefix=pre))
        out.append(make(f"match/source wholly in the prefix, M {M}, flipped", seq(b"ab", 2 + 100, min(M, 100)) + seq(b"", None, 0), prefix=pre, flip=2 + min(M, 100) // 2))
        for back in (1, 10, 63):
            blk = seq(b"ab", 2 + back, back + M) + seq(b"x", None, 0)
            out.append(make(f"match/source from the prefix into out, {back} + {M}", blk, prefix=pre))
            for at in sorted({2, 2 + back - 1, 2 + back, 2 + back + M - 1}):
                out.append(make(f"match/source from the prefix into out, {back} + {M}, flip at {at}", blk, prefix=pre, flip=at))
            blk = seq(b"", 50 + back, back + 50 + M) + seq(b"x", None, 0)
            out.append(make(f"match/prefix, existing output and out, {back} + 50 + {M}", blk, prefix=pre, existing=hist))
            out.append(make(f"match/prefix, existing output and out, {back} + 50 + {M}, flip", blk, prefix=pre, existing=hist, flip=50 + back + 50 + M - 2))
        out.append(make(f"match/source in the existing output, M {M}", seq(b"abc", 3 + 40, M) + seq(b"", None, 0), existing=hist))
        out.append(make(f"match/source in the existing output, M {M}, flipped", seq(b"abc", 3 + 40, M) + seq(b"", None, 0), existing=hist, flip=50 + 3 + M - 1))
    return out


def planted_cases():
    out = []
    text = synth.gen_text_zipf(17, 9000).tobytes()
    rc, comp = o.compress2(text)
    assert rc == 0
    n = len(text)
    out.append(make("planted/text, equal", comp))
    for at in (0, 1, 15, 16, 17, n - 1):
        out.append(make(f"planted/text, flip at {at}", comp, flip=at))
    # literal runs and matches of known places: 20 literals, a match of 30, 70 literals, a match of 90, last literals
    la, lb = _rand(11, 20), _rand(12, 70)
    blk = seq(la, 20, 30) + seq(lb, 100, 90) + seq(b"end", None, 0)
    for tag, at in (("first literal of a run", 0), ("last literal of a run", 19), ("first byte of a match", 20), ("last byte of a match", 49),
                    ("first literal of a long run", 50), ("last literal of a long run", 119), ("first byte of a long match", 120),
                    ("last byte of a long match", 209), ("the last literals", 212)):
        out.append(make(f"planted/{tag}", blk, flip=at))
    # a flipped byte that later matches copy from: the verdict names the flipped byte, not a copy
    blk = seq(b"abcdefgh", 8, 40) + seq(b"ijkl", 4, 100) + seq(b"", None, 0)
    for at in (3, 11, 50):
        c = make(f"planted/a byte that later matches copy from, at {at}", blk, flip=at)
        assert expect(c) == (MISMATCH, at)
        out.append(c)
    # a flipped compressed literal: the decode differs there, the expected bytes are the true ones
    good = make("planted/compressed literal", comp)
    b = bytearray(comp)
    first_lit = 1 + (1 if comp[0] >> 4 == 15 else 0)
    b[first_lit + 2] ^= 0x20
    c = dict(good, name="planted/flipped compressed literal", input=bytes(b))
    assert expect(c)[0] == MISMATCH
    out.append(c)
    # a match offset changed to one whose source bytes happen to be equal: LZF_OK
    blk4 = seq(b"abcdabcdabcd", 4, 8) + seq(b"!", None, 0)
    blk8 = seq(b"abcdabcdabcd", 8, 8) + seq(b"!", None, 0)
    c = dict(make("planted/another offset, equal source bytes", blk4), input=blk8)
    assert blk4 != blk8 and expect(c) == (0, 21)
    out.append(c)
    # out_cap one short and one long, the true continuation in memory behind it
    for tag, blk_ in (("text", comp), ("sequences", blk), ("one match", seq(b"ab", 2, 200))):
        short = make(f"planted/{tag}, out_cap = n - 1", blk_, cap_delta=-1)
        assert expect(short) == (MISMATCH, short["out_cap"])
        out.append(short)
        rc, dec = _oracle(blk_, b"", b"", 1 << 22)
        longer = dict(make(f"planted/{tag}, out_cap = n + 1", blk_), out_cap=len(dec) + 1)
        assert expect(longer) == (MISMATCH, len(dec))
        out.append(longer)
    # history that differs inside the existing output: it is trusted, the verdict follows from the rule
    hist = _rand(13, 100)
    blk = seq(b"xy", 2 + 60, 10) + seq(b"", None, 0)          # copies hist[40:50]
    other = bytearray(hist); other[44] ^= 1
    c = make("planted/history differs where a match reads it", blk, existing=hist, history=bytes(other))
    assert expect(c) == (MISMATCH, 100 + 2 + 4)
    out.append(c)
    other = bytearray(hist); other[70] ^= 1
    c = make("planted/history differs where nothing reads it", blk, existing=hist, history=bytes(other))
    assert expect(c) == (0, 112)
    out.append(c)
    out.append(make("planted/empty input, nothing expected", b""))
    out.append(dict(make("planted/empty input, one byte expected", b""), out_cap=1))
    out.append(make("planted/empty input behind existing output", b"", existing=b"0123456"))
    return out


def status_cases():
    """Every status of the size call on a job whose expected bytes are also wrong: the status wins."""
    out = []
    text = synth.gen_text_zipf(19, 6000).tobytes()
    comp = o.compress2(text)[1]
    out.append(make("status/truncated input", comp[:len(comp) // 2]))
    out.append(make("status/truncated inside the last literals", comp[:-2]))
    out.append(make("status/offset 0", seq(b"abcd", 0, 8) + seq(b"", None, 0)))
    out.append(make("status/offset 0 behind 100 clean sequences", fill8(800) + seq(b"abcd", 0, 8) + seq(b"", None, 0)))
    out.append(make("status/offset beyond history and prefix", seq(b"abcd", 4 + 10 + 20 + 1, 8) + seq(b"", None, 0), prefix=_rand(1, 10), existing=_rand(2, 20)))
    out.append(make("status/match past output_limit", seq(b"abcd", 2, 100) + seq(b"", None, 0), limit=103))
    out.append(make("status/match past output_limit in a later chunk", fill8(2 * CHUNK) + seq(b"abcd", 2, 100), limit=9 * 768 + 50))
    out.append(make("status/missing length byte", b"\xf0"))
    # a mismatch in front of the error: the status still wins
    bad = bytearray(seq(b"abcdefgh", 3, 8) * 40 + seq(b"abcd", 0, 8))
    c = make("status/a mismatch in front of offset 0", bytes(bad))
    out.append(c)
    # LZF_CONTRACT on a length without a buffer, as the size call's tests build it
    out.append(make("status/prefix of 2 GiB", seq(b"hello", None, 0), prefix_len=1 << 31))
    return out


def text_cases():
    """Blocks of 64 KiB .. 200 KiB of compressed text: many rounds and chunks of real sequences, a difference in the first and the last
    2 KiB of input and one in the middle."""
    out = []
    for k, n_plain in enumerate((150_000, 400_000)):
        text = synth.gen_text_zipf(23 + k, n_plain).tobytes()
        comp = o.compress2(text)[1]
        assert 65536 <= len(comp) <= 200 * 1024, len(comp)
        out.append(make(f"text/{n_plain} bytes, equal", comp))
        for at in (100, n_plain // 2 + 1, n_plain - 50):
            out.append(make(f"text/{n_plain} bytes, flip at {at}", comp, flip=at))
    return out


TILE = 2048           # compressed bytes one wavefront of the latency class covers
CLASS_MIN_IN = 65536  # the class's smallest input (lzf_dispatch.h: size_seg_min_in)


def walk(blk):
    """[(input position, output position, L, M, offset)] of a block's sequences (M = 0: the last literals)."""
    p, o, toks = 0, 0, []
    while p < len(blk):
        t, q = blk[p], p + 1
        L = t >> 4
        if L == 15:
            while True:
                b = blk[q]; q += 1; L += b
                if b != 255:
                    break
        q += L
        if len(blk) - q < 2:
            toks.append((p, o, L, 0, 0))
            break
        off = blk[q] | (blk[q + 1] << 8); q += 2
        M = t & 15
        if M == 15:
            while True:
                b = blk[q]; q += 1; M += b
                if b != 255:
                    break
        M += 4
        toks.append((p, o, L, M, off))
        o += L + M; p = q
    return toks


def class_cases():
    """Jobs for the latency class: 64 KiB .. 200 KiB of compressed text; equal, and one difference each in tile 0, in the last tile,
    in the last byte of one tile's output and in the first of the next, and in the first byte of a match whose source lies in the
    tile before; one job with a prefix and one with existing output; and one job with an error (an offset of 0 in a later tile),
    which the class must leave to the one-wave kernel.  The module's preconditions: every case but the error job has an input of
    at least 64 KiB and decodes LZF_OK in the oracle."""
    out = []
    for k, n_plain in enumerate((150_000, 250_000, 400_000)):
        text = synth.gen_text_zipf(61 + k, n_plain).tobytes()
        comp = o.compress2(text)[1]
        assert CLASS_MIN_IN <= len(comp) <= 200 * 1024, len(comp)
        toks = walk(comp)
        assert toks[-1][1] + toks[-1][2] == n_plain
        ntile = (len(comp) + TILE - 1) // TILE
        first = {}                                            # tile -> its first token
        for tk in toks:
            first.setdefault(tk[0] // TILE, tk)
        mid = ntile // 2
        while mid not in first or mid - 1 not in first:
            mid += 1
        base = first[mid][1]                                  # the output position of tile mid's first token
        src_before = next(tk for tk in toks if tk[0] // TILE == mid and tk[3] and tk[1] + tk[2] - tk[4] < base)
        tag = f"class/{n_plain} bytes"
        out.append(make(f"{tag}, equal", comp))
        for what, at in (("tile 0", 5), ("the last tile", n_plain - 3), ("the last byte of a tile's output", base - 1),
                         ("the first byte of the next tile's output", base), ("a match whose source lies in the tile before", src_before[1] + src_before[2])):
            out.append(make(f"{tag}, difference in {what}", comp, flip=at))
        out.append(make(f"{tag}, out_cap inside a tile", comp, cap_delta=-(n_plain - base - 7)))
    d = synth.gen_text_zipf(67, 220_000).tobytes()
    dic, payload = d[:20_000], d[20_000:]
    comp = o.compress2(dic + payload, cursor=len(dic))[1]
    assert len(comp) >= CLASS_MIN_IN
    out.append(make("class/behind a prefix", comp, prefix=dic))
    out.append(make("class/behind a prefix, difference", comp, prefix=dic, flip=100))
    out.append(make("class/behind existing output", comp, existing=dic))
    out.append(make("class/behind existing output, difference", comp, existing=dic, flip=len(dic) + len(payload) - 9))
    for c in out:
        assert len(c["input"]) >= CLASS_MIN_IN and _oracle(c["input"], c["prefix"], c["mem"][:c["existing_len"]], c["limit"])[0] == 0, c["name"]
    text = synth.gen_text_zipf(61, 150_000).tobytes()
    comp = o.compress2(text)[1]
    tk = next(t for t in walk(comp) if t[0] > 40_000 and t[3])
    bad = bytearray(comp)
    lit_at = tk[0] + 1 + ((tk[2] - 15) // 255 + 1 if tk[2] >= 15 else 0)
    bad[lit_at + tk[2]:lit_at + tk[2] + 2] = b"\x00\x00"
    err = make("class/an offset of 0 in a later tile", bytes(bad))
    assert expect(err) == (3, None)
    out.append(err)
    return [(c, expect(c)) for c in out]


def block_cases():
    """[(case, (status, out_len or None))] — the expectation of every case by decode-then-compare."""
    cs = token_cases() + match_cases() + planted_cases() + status_cases() + text_cases()
    assert len({c["name"] for c in cs}) == len(cs)
    return [(c, expect(c)) for c in cs]


def assert_covers(rows):
    """What both tests state on the ORACLE's results before anything is compared."""
    kinds = {e[0] for _, e in rows}
    assert {0, 1, 2, 3, 4, CONTRACT, MISMATCH} <= kinds, kinds
    assert sum(e[0] == 0 for _, e in rows) > 100 and sum(e[0] == MISMATCH for _, e in rows) > 200


# ---------------------------------------------------------------------------------------------------- frames
F_INPUT_ERROR, F_BLOCK_CHECKSUM_FAIL, F_FRAME_CHECKSUM_FAIL = 16, 19, 20
BLOCK = 64 << 10
FRAME_INPUT_LENS = (0, 1, 65535, 65536, 65537, 200000)
DICT_LENS = (0, 4, 100, 65536)


def frame_expect(c):
    """(status, at) of a frame case by decode-then-compare: the oracle's frame decode; a status other than Ok (FrameChecksumFail
    aside: the size query does not see it) wins with the partial length; else numpy's first difference or the shorter length; else
    the content checksum's verdict."""
    rc, out, _ = o.frame_decompress(c["frame"], c["dictionary"], cap=1 << 19)          # (every content here is shorter)
    if rc not in (0, F_FRAME_CHECKSUM_FAIL):
        return rc, len(out)
    exp = c["expected"]
    m = min(len(out), len(exp))
    d = np.flatnonzero(np.frombuffer(out, dtype=np.uint8)[:m] != np.frombuffer(exp, dtype=np.uint8)[:m])
    if d.size:
        return MISMATCH, int(d[0])
    if len(out) != len(exp):
        return MISMATCH, m
    return rc, len(out)


def _flipped(data, at):
    b = bytearray(data)
    b[at] ^= 0x01
    assert sum(x != y for x, y in zip(b, data)) == 1 and b[at] != data[at]
    return bytes(b)


def _block_payloads(frame):
    """[(offset of the payload, its length, stored)] of a frame without content size and dictionary id."""
    assert not frame[4] & 0x09
    at, out = 7, []
    while True:
        n = int.from_bytes(frame[at:at + 4], "little")
        if n == 0:
            return out
        out.append((at + 4, n & 0x7FFFFFFF, bool(n >> 31)))
        at += 4 + (n & 0x7FFFFFFF) + (4 if frame[4] & 0x10 else 0)


def frame_cases():
    """[(case, (status, at))]: case = dict(name, frame, dictionary, expected).  Frames written by the oracle: text of the listed
    lengths and noise (stored blocks), independent and linked, the four dictionaries, block and content checksums on and off; every
    frame against its own content and against one planted variant, a few frames against every variant; damaged frames."""
    text = synth.gen_text_zipf(41, 300000).tobytes()
    dic = synth.gen_text_zipf(42, 65536).tobytes()
    inputs = [(f"text {n}", text[1000:1000 + n]) for n in FRAME_INPUT_LENS] + [("noise 150000", _rand(43, 150000)),
                                                                                 ("text, noise, text", text[:70000] + _rand(44, 65536) + text[70000:120000])]
    cs = []

    def variants(data):
        n, v = len(data), []
        if n:
            last0 = (n - 1) // BLOCK * BLOCK
            for tag, at in (("first block", min(7, n - 1)), ("middle block", n // 2), ("last block", n - 1), ("a block's first byte", last0),
                            ("a block's last byte", min(BLOCK, n) - 1)):
                v.append((f"flip in {tag}", _flipped(data, at)))
            v.append(("one byte shorter", data[:-1]))
        v.append(("one byte longer", data + b"!"))
        return v

    k = 0
    for dl in DICT_LENS:
        for indep in (True, False):
            for bsum in (False, True):
                for csum in (True, False):
                    for tag, data in inputs:
                        s = o.make_settings(independent_blocks=indep, block_checksums=bsum, content_checksum=csum, block_size=BLOCK,
                                            dictionary=dic[:dl] if dl else None, dictionary_id=7 if dl else None)
                        rc, frame = o.frame_compress(data, s)
                        assert rc == 0
                        name = f"{tag}, {'independent' if indep else 'linked'}, dictionary {dl}, block sums {int(bsum)}, content sum {int(csum)}"
                        base = dict(frame=frame, dictionary=dic[:dl])
                        cs.append(dict(base, name=name, expected=data))
                        vs = variants(data)
                        every = dl in (0, 100) and bsum != csum and tag in ("text 200000", "text, noise, text", "text 1")
                        for q, (vt, exp) in enumerate(vs):
                            if every or q == k % len(vs):
                                cs.append(dict(base, name=f"{name}: {vt}", expected=exp))
                        k += 1
    # damaged frames
    data = text[5000:205000]
    for indep in (True, False):
        kind = "independent" if indep else "linked"
        f = o.frame_compress(data, o.make_settings(independent_blocks=indep, block_size=BLOCK))[1]
        bad = bytearray(f); bad[-1] ^= 1
        cs.append(dict(name=f"damaged/{kind}, wrong content checksum, equal bytes", frame=bytes(bad), dictionary=b"", expected=data))
        cs.append(dict(name=f"damaged/{kind}, wrong content checksum, flipped byte", frame=bytes(bad), dictionary=b"", expected=_flipped(data, 70000)))
        cs.append(dict(name=f"damaged/{kind}, truncated frame", frame=f[:len(f) // 2], dictionary=b"", expected=data))
        cs.append(dict(name=f"damaged/{kind}, EndMark missing", frame=f[:-8], dictionary=b"", expected=data))
        at, n, stored = _block_payloads(f)[2]
        assert not stored
        L0, q = f[at] >> 4, at + 1
        if L0 == 15:
            while f[q] == 255:
                L0 += 255; q += 1
            L0 += f[q]; q += 1
        bad = bytearray(f); bad[q + L0:q + L0 + 2] = b"\x00\x00"                 # the first sequence's offset
        c = dict(name=f"damaged/{kind}, codec error in block 2", frame=bytes(bad), dictionary=b"", expected=data)
        assert frame_expect(c) == (ZERO_OFFSET, 2 * BLOCK)
        cs.append(c)
        cs.append(dict(c, name=c["name"] + ", flipped byte in block 0", expected=_flipped(data, 5)))
        fb = o.frame_compress(data, o.make_settings(independent_blocks=indep, block_size=BLOCK, block_checksums=True))[1]
        at, n, stored = _block_payloads(fb)[1]
        bad = bytearray(fb); bad[at + n] ^= 0x10                                 # block 1's checksum word
        c = dict(name=f"damaged/{kind}, block checksum of block 1", frame=bytes(bad), dictionary=b"", expected=data)
        assert frame_expect(c) == (F_BLOCK_CHECKSUM_FAIL, BLOCK)
        cs.append(c)
    cs.append(dict(name="damaged/wrong magic", frame=b"\x00" * 20, dictionary=b"", expected=b""))
    assert len({c["name"] for c in cs}) == len(cs)
    return [(c, frame_expect(c)) for c in cs]


ZERO_OFFSET = 3


def assert_frames_cover(rows):
    kinds = {e[0] for _, e in rows}
    assert {0, MISMATCH, F_FRAME_CHECKSUM_FAIL, F_BLOCK_CHECKSUM_FAIL, F_INPUT_ERROR, ZERO_OFFSET} <= kinds, kinds
    assert sum(e[0] == 0 for _, e in rows) >= 250 and sum(e[0] == MISMATCH for _, e in rows) >= 250
