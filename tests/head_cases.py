"""Cases of the head tests (test_head_cases_cpu.py, test_gpu_head.py): raw blocks built sequence by sequence from the head kernel's own
constants (header_constants(): the chunk, the tokens of a round, the own-lane threshold — read from the sources) or compressed by
the oracle, each with a TARGET — the job's out_cap — and the expectation.

Every expectation comes from the oracle (expect() is the only source):
    a block the oracle decodes cleanly to D           (LZF_OK, min(len(D), t), D[existing:t])
    a block the oracle fails with status e            ref_walk() — the reference's loop written out in Python — names the failing
                                                      sequence: its output position p and its input position.  t > p: (e, None, None).
                                                      t <= p: (LZF_OK, t, the oracle's decode of the block cut in front of that
                                                      sequence, up to t).
ref_walk is pinned on every case: it reproduces the oracle's status and, on clean blocks, the oracle's length.  The one exception is
LZF_CONTRACT, which the oracle cannot produce; it is stated by hand, under the decoder's condition (a length of 2 GiB - 256).

A case is dict(name, cls, sub, input, prefix, prefix_len, existing, origin, target, limit): the job's out_existing_len is
origin + len(existing), its out_cap origin + target, its output_limit origin + limit; `origin` (0 but for class j) is history that
is not in memory: the job is stated over its tail, as a trimmed job sees it.  `target` and the expectation's out_len are relative
to the origin.  room(c) is the memory a test puts behind `existing`."""
import os
import re

import oracle_ffi as o
from rust_lz_fear_amd import synth
from verify_cases import N_FF, _rand, fill8, seq

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-lz-fear_amd", "csrc")
CONTRACT = 6
MAX_LEN = 0x7FFFFF00


def header_constants():
    """The head kernel's constants, read from its sources."""
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def num(text, pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    head, dev, capi = src("lz4_decode_head.hip"), src("lzf_device.h"), src("capi_head.hip")
    m = re.search(r"template __global__ void lzf_decode_head_kernel<(\d+), (\d+)>", head)
    assert m and f"lzf_decode_head_kernel<{m.group(1)}, {m.group(2)}>;" in capi
    wave = num(dev, r"constexpr uint32_t kWave = (\d+);")
    assert re.search(r"constexpr uint32_t kChunk = 64u \* S;", head) and re.search(r"tidx \+= kWave\)", head)
    return dict(CHUNK=wave * int(m.group(1)), TOKCAP=int(m.group(2)), ROUND=wave, OWN=num(head, r"constexpr uint32_t kOwn = (\d+);"),
                STEP=num(head, r"constexpr uint32_t kStep = (\d+);"))


K = header_constants()
CHUNK, TOKCAP, ROUND, OWN, STEP = K["CHUNK"], K["TOKCAP"], K["ROUND"], K["OWN"], K["STEP"]
FAR = 1 << 40               # a target far past every block's end
SWEEP_MAX = 2048            # clean cases that decode to no more are also run at every target (the CPU test)


def ref_walk(blk, prefix_len, existing_len, limit):
    """The reference's loop (src/raw/decompress.rs:61-77, :83-89) over lengths alone: (status, pos, tp, seqs).  On Ok pos is
    output.len() and tp None; on an error pos / tp are the output / input position at which the failing sequence starts.
    seqs: [(tp, pos, L, M, off)] of the sequences taken (M = 0: no match)."""
    p, pos, n, seqs = 0, existing_len, len(blk), []
    while p < n:
        tp, start = p, pos
        t = blk[p]; p += 1
        L = t >> 4
        if L == 15:
            while True:
                if p >= n:
                    return 1, start, tp, seqs
                b = blk[p]; p += 1; L += b
                if b != 255:
                    break
        if n - p < L:
            return 1, start, tp, seqs
        p += L; pos += L
        if n - p < 2:
            seqs.append((tp, start, L, 0, 0))
            break
        off = blk[p] | (blk[p + 1] << 8); p += 2
        M = t & 15
        if M == 15:
            while True:
                if p >= n:
                    return 1, start, tp, seqs
                b = blk[p]; p += 1; M += b
                if b != 255:
                    break
        M += 4
        if pos + M > limit:
            return 2, start, tp, seqs
        if off == 0:
            return 3, start, tp, seqs
        if off > pos and off - pos > prefix_len:
            return 4, start, tp, seqs
        seqs.append((tp, start, L, M, off))
        pos += M
    return 0, pos, None, seqs


_decodes = {}


def _oracle(blk, prefix, existing, limit):
    key = (blk, prefix, existing, limit)
    if key not in _decodes:
        cap = len(existing) + min(limit, 1 << 26) + 255 * len(blk) + 64
        rc, dec = o.decompress_raw(blk, prefix=prefix, existing=existing, limit=limit, cap=min(cap, 1 << 27))
        assert rc != o.OUT_CAPACITY
        _decodes[key] = (rc, dec)
    return _decodes[key]


def expect(c):
    """(status, out_len or None, bytes of out[existing, out_len) or None), lengths relative to the case's origin."""
    ex, t = len(c["existing"]), c["target"]
    if c["prefix_len"] >= MAX_LEN or c["origin"] + ex >= MAX_LEN or len(c["input"]) >= MAX_LEN:
        return CONTRACT, None, None
    if t <= ex:
        return 0, ex, b""
    rc, dec = _oracle(c["input"], c["prefix"], c["existing"], c["limit"])
    st, pos, tp, _ = ref_walk(c["input"], c["prefix_len"], ex, c["limit"])
    assert st == rc and (rc != 0 or pos == len(dec)), (c["name"], "ref_walk does not reproduce the oracle", st, rc)
    if rc == 0:
        return 0, min(len(dec), t), dec[ex:t]
    if t > pos:
        return rc, None, None
    rc2, dec2 = _oracle(c["input"][:tp], c["prefix"], c["existing"], c["limit"])
    assert rc2 == 0 and len(dec2) == pos, c["name"]
    return 0, t, dec2[ex:t]


def room(c):
    """Bytes of memory behind `existing` that a job may write: up to the target, and no further than the walk gets."""
    ex = len(c["existing"])
    if c["target"] <= ex or c["prefix_len"] != len(c["prefix"]):
        return 0
    _, pos, _, _ = ref_walk(c["input"], c["prefix_len"], ex, c["limit"])
    return min(c["target"], pos) - ex


def case(name, cls, sub, blk, target, prefix=b"", existing=b"", limit=1 << 22, prefix_len=None, origin=0):
    prefix, existing = bytes(prefix), bytes(existing)
    return dict(name=f"{cls}/{name}, target {target}", cls=cls, sub=sub, input=bytes(blk), prefix=prefix,
                prefix_len=len(prefix) if prefix_len is None else prefix_len, existing=existing, origin=origin, target=target, limit=limit)


def at(name, cls, sub, blk, targets, **kw):
    return [case(name, cls, sub, blk, t, **kw) for t in targets]


END = seq(b"tail!", None, 0)


def literal_cases():
    """(a) the target inside a literal run: runs a lane moves by itself (up to OWN bytes) and runs the wave moves."""
    la, lb, lc = _rand(11, 20), _rand(12, OWN + 6), _rand(13, 3 * OWN + 8)
    blk = seq(la, 20, 30) + seq(lb, 100, 90) + seq(lc, 7, 12) + seq(_rand(14, OWN), 3, 5) + seq(b"end", None, 0)
    s = ref_walk(blk, 0, 0, 1 << 22)[3]
    out = []
    for (tp, pos, L, M, off), sub in zip(s, ("own-lane", "wave-wide", "wave-wide", "own-lane", "own-lane")):
        out += at(f"a run of {L} literals at {pos}", "a", sub, blk, sorted({pos + 1, pos + L // 2, pos + L - 1} - {pos}))
    big = _rand(15, STEP + 2 * OWN + 5)
    blk = seq(b"ab", 2, 4) + seq(big, 1, 4) + END
    out += at(f"a run of {len(big)} literals", "a", "wave-wide", blk, (6 + 1, 6 + 15, 6 + 16, 6 + 17, 6 + STEP - 1, 6 + STEP, 6 + STEP + 1, 6 + len(big) - 1))
    return out


def match_cases():
    """(b) the target inside a match."""
    out = []
    lit = _rand(21, 40)
    for M in (30, OWN, OWN + 1, 300):
        blk = seq(lit, 40, min(M, 40)) + seq(_rand(22, 300), 310, M) + END
        p2 = 40 + min(M, 40) + 300
        out += at(f"a match of {M} that does not overlap", "b", "apart", blk, sorted({41, 40 + min(M, 40) - 1, p2 + 1, p2 + M // 2, p2 + M - 1}))
    for off in (1, 2, 3, 4, 8, 15, 16, 17, OWN, 100):
        for M in (19, OWN + 3, 300, 2 * STEP + 77):
            if off >= M:
                continue
            L = max(off, 6)
            blk = seq(_rand(23 + off, L), off, M) + END
            ts = {L + 1, L + off, L + off + 1, L + M // 2, L + M - 1}
            out += at(f"a match of {M} at offset {off} over itself", "b", f"overlap {off}", blk, sorted(t for t in ts if L < t < L + M))
    pre = _rand(24, 400)
    for M in (20, OWN + 2, 300):
        blk = seq(b"ab", 2 + 390, M) + END
        out += at(f"a match of {M} from the prefix", "b", "prefix", blk, (3, 2 + M // 2, 2 + M - 1), prefix=pre)
        for back in (1, 10, 63):
            blk = seq(b"ab", 2 + back, back + M) + seq(b"x", None, 0)
            ts = sorted({3, 2 + back - 1, 2 + back, 2 + back + 1, 2 + back + M - 1} - {2})
            out += at(f"a match of {back} + {M} from the prefix into out", "b", "prefix into out", blk, ts, prefix=pre)
    hist = _rand(25, 500)
    for M in (5, OWN, 300):
        blk = seq(b"abc", 3 + 400, M) + END
        out += at(f"a match of {M} from the existing output", "b", "existing", blk, (500 + 4, 500 + 3 + M // 2, 500 + 3 + M - 1), existing=hist)
        blk = seq(b"", 5, M) + END
        out += at(f"a match of {M} at offset 5 over the end of the existing output", "b", "existing", blk, (501, 500 + M - 1), existing=hist)
    blk = seq(b"", 60 + 50, 40 + 50 + 30) + END                  # prefix, existing output and out in one match
    out += at("a match through the prefix, the existing output and out", "b", "prefix into out", blk, (51, 50 + 39, 50 + 40, 50 + 41, 50 + 90, 50 + 119),
              prefix=pre, existing=hist[:50])
    return out


LIT8 = b"lit8lit8"


def _bad(status, pos):
    """(a malformed sequence of `status` with 8 literals, the job's output_limit) for a sequence whose first literal sits at `pos`."""
    if status == 1:
        return bytes([0x8F]) + LIT8 + b"\x01\x00\xff", 1 << 22      # the match length run ends with the input
    if status == 2:
        return seq(LIT8, 1, 8), pos + 8 + 7                        # the match ends one byte beyond the limit
    if status == 3:
        return seq(LIT8, 0, 8), 1 << 22
    return seq(LIT8, pos + 8 + 1, 8), 1 << 22                      # one byte in front of out[0], no prefix


def boundary_cases():
    """(c) the target on a sequence boundary in front of a malformed sequence: not seen.  (d) the target between a sequence's literals
    and its malformed match: reported."""
    out = []
    good = seq(b"hello", 5, 10)                                  # 15 bytes of output
    for k in (1, ROUND, ROUND + 1):
        front = good * k
        p = 15 * k
        for status in (1, 2, 3, 4):
            bad, limit = _bad(status, p)
            if status == 1:
                out += at(f"{k} sequences, then a token without its length byte", "c", f"status {status}", front + b"\xf0", (p,))
                out += at(f"{k} sequences, then a token without its length byte", "h", f"status {status}", front + b"\xf0", (p + 1, FAR))
            blk = front + bad
            out += at(f"{k} sequences, then one of status {status}", "c", f"status {status}", blk, (p,), limit=limit)
            out += at(f"{k} sequences, then one of status {status}", "h", f"status {status}", blk, (p + 1, p + 3, FAR), limit=limit)
            if status != 1:
                out += at(f"{k} sequences, then literals and a match of status {status}", "d", f"status {status}", blk, (p + 8,), limit=limit)
    return out


def round_cases():
    """(e) the target in sequences 63, 64 and 65 of a round (and of the round behind)."""
    out = []
    n = 2 * ROUND + 10
    blk = b"".join(seq(bytes([0x41 + (j % 26)]) * 3 + bytes([j & 0xFF, 0x30 + j % 10]), 2, 6) for j in range(n)) + seq(b"end", None, 0)
    for k in (ROUND - 1, ROUND, ROUND + 1, 2 * ROUND - 1, 2 * ROUND, 2 * ROUND + 1):
        j = k - 1                                                # sequence k, counted from 1
        out += at(f"sequence {k} of {n}", "e", f"sequence {k}", blk, (11 * j, 11 * j + 2, 11 * j + 5, 11 * j + 8, 11 * j + 11))
    return out


def chunk_cases():
    """(f) the target on either side of a chunk boundary; inside a token that reaches beyond a whole chunk; around a parse whose
    token list is cut."""
    out = []
    blk = fill8(2 * CHUNK + 200) + seq(b"end", None, 0)
    s = ref_walk(blk, 0, 0, 1 << 22)[3]
    for b in (CHUNK, 2 * CHUNK):
        last = max(q for q in s if q[0] < b)
        first = min(q for q in s if q[0] >= b)
        assert last[1] + last[2] + last[3] == first[1]
        out += at(f"the last sequence in front of input byte {b}", "f", "chunk boundary", blk, (last[1], last[1] + 1, last[1] + last[2], first[1] - 1))
        out += at(f"the first sequence behind input byte {b}", "f", "chunk boundary", blk, (first[1], first[1] + 1, first[1] + first[2] + 1, first[1] + first[2] + first[3]))
    # a sequence whose literals lie across the boundary, and one whose match length bytes do
    lit = _rand(5, 15 + 255 + 40)
    for tag, sq, span in (("literal run", seq(lit, 5, 8), len(lit)), ("match", seq(b"ab", 7, 19 + 255 * 2 + 3), 2 + 19 + 255 * 2 + 3)):
        blk = fill8(CHUNK - 10, salt=3) + sq + fill8(200) + seq(b"z", None, 0)
        pos = 9 * ((CHUNK - 10) // 8) + (CHUNK - 10) % 8
        out += at(f"a {tag} over a chunk end", "f", "chunk boundary", blk, (pos, pos + 1, pos + span // 2, pos + span - 1, pos + span, pos + span + 1))
    big_l = _rand(6, 15 + 255 * (N_FF - 1) + 77)
    giant_l, giant_m = seq(big_l, 9, 12), seq(b"q", 1, 19 + 255 * (N_FF - 1) + 7)
    assert len(giant_l) - len(big_l) - 3 == N_FF > CHUNK and len(giant_m) - 4 == N_FF
    pos = 9 * 62 + 500 % 8
    for tag, g, span in (("literals", giant_l, len(big_l)), ("match", giant_m, 1 + 19 + 255 * (N_FF - 1) + 7)):
        blk = fill8(500) + g + fill8(100) + seq(b"end", None, 0)
        out += at(f"a token beyond a chunk, {tag}", "f", "beyond a chunk", blk, (pos, pos + 1, pos + 2, pos + 4097, pos + span - 1, pos + span, pos + span + 5, FAR))
        out += at(f"a token beyond a chunk first, {tag}", "f", "beyond a chunk", g + seq(b"end", None, 0), (1, 2, 4100, span + 3))
    blk = seq(b"abcd", 4, 4) + seq(b"", 4, 4) * (TOKCAP + 200) + seq(b"end", None, 0)      # 3 bytes a token: more tokens in a chunk than a parse lists
    assert TOKCAP < (TOKCAP + 200) * 3 < CHUNK
    out += at("a chunk of more tokens than a parse lists", "f", "token list cut", blk, [4 + 4 * k + d for k in (TOKCAP - 1, TOKCAP, TOKCAP + 1) for d in (0, 1, 3)])
    return out


def degenerate_cases():
    """(g) degenerate targets."""
    out = []
    blk = seq(b"hello world", 6, 9) + END
    hist = _rand(31, 70)
    out += at("nothing asked for", "g", "target == existing", blk, (0,))
    out += at("nothing asked for behind existing output", "g", "target == existing", blk, (70,), existing=hist)
    out += at("a target inside the existing output", "g", "target < existing", blk, (0, 1, 69), existing=hist)
    out += at("a malformed block, nothing asked for", "g", "target == existing", b"\xf0", (0,))
    out += at("one past the end", "g", "one past the end", blk, (25, 26))
    out += at("one past the end behind existing output", "g", "one past the end", blk, (70 + 25, 70 + 26), existing=hist)
    out += at("far past the end", "g", "far past the end", blk, (FAR, (1 << 63) - 1))
    out += at("an empty input", "g", "empty input", b"", (0, 5, FAR))
    out += at("an empty input behind existing output", "g", "empty input", b"", (70, 75), existing=hist)
    return out


def error_cases():
    """(h) an error in front of the target: every status, the precedence inside one sequence, errors in a later round and chunk."""
    out = []
    text = synth.gen_text_zipf(19, 6000).tobytes()
    comp = o.compress2(text)[1]
    out += at("truncated input", "h", "status 1", comp[:len(comp) // 2], (FAR,))
    out += at("truncated inside the last literals", "h", "status 1", comp[:-2], (FAR, 5990))
    out += at("missing length byte", "h", "status 1", b"\xf0", (1,))
    for where, front in (("a later round", fill8(800)), ("a later chunk", fill8(2 * CHUNK + 16))):
        p = ref_walk(front, 0, 0, 1 << 22)[1]
        for status in (1, 2, 3, 4):
            bad, limit = _bad(status, p)
            out += at(f"status {status} in {where}", "h", f"status {status}", front + bad, (p + 1, p + 8, FAR), limit=limit)
            out += at(f"status {status} in {where}", "c", f"status {status}", front + bad, (p,), limit=limit)
    # inside one sequence: UnexpectedEnd in front of the limit and the offsets; the limit in front of the offsets; offset 0 is its own test
    lit = LIT8
    out += at("a match length run that ends with the input, offset 0, beyond the limit", "h", "precedence", bytes([0x8F]) + lit + b"\x00\x00\xff", (FAR,), limit=4)
    out += at("beyond the limit and offset 0", "h", "precedence", seq(lit, 0, 100), (FAR, 9), limit=50)
    out += at("beyond the limit and an offset in front of the prefix", "h", "precedence", seq(lit, 500, 100), (FAR, 9), limit=50)
    out += at("literals beyond the limit are not checked", "h", "precedence", seq(lit * 10, None, 0), (FAR, 50), limit=4)
    out += at("the limit, exactly met", "h", "precedence", seq(lit, 8, 12) + END, (FAR, 15), limit=20)
    out += at("the limit, one short", "h", "precedence", seq(lit, 8, 12) + END, (FAR, 9, 8), limit=19)
    out += at("an offset one byte in front of prefix ++ existing", "h", "status 4", seq(b"abcd", 4 + 10 + 20 + 1, 8) + END, (FAR, 24), prefix=_rand(1, 10), existing=_rand(2, 20))
    out += at("an offset that reaches the first prefix byte", "b", "prefix into out", seq(b"abcd", 4 + 10 + 20, 40) + END, (25, 35, 60), prefix=_rand(1, 10), existing=_rand(2, 20))
    return out


def contract_cases():
    """(i) lengths at the 31-bit contract, stated without buffers."""
    blk = seq(b"hello", None, 0)
    return [case("a prefix of 2 GiB - 256", "i", "prefix", blk, 5, prefix_len=MAX_LEN),
            case("a prefix of 2 GiB", "i", "prefix", blk, FAR, prefix_len=1 << 31),
            case("existing output of 2 GiB - 256", "i", "existing", blk, 70, existing=_rand(3, 64), origin=MAX_LEN - 64),
            case("existing output of 2 GiB - 257", "j", "below the contract", blk, 67, existing=_rand(3, 64), origin=MAX_LEN - 65)]


def history_cases():
    """(j) more than 1 GiB of existing output, stated over its last bytes (a trimmed job sees it that way): the origin moves, the
    target with it.  No match of these blocks reaches further back than the tail that is in memory."""
    out = []
    tail = _rand(41, 65536 + 40)
    for origin in ((1 << 30) + 5, (1 << 31) - 70000 - 300):
        E = len(tail)
        blk = seq(b"abc", 3 + 400, 30) + seq(b"defgh", 65535, 20) + seq(_rand(42, 100), 1, 40) + END
        out += at(f"behind {origin + E} bytes of existing output", "j", "long history", blk, (E, E + 1, E + 3 + 15, E + 33 + 5 + 10, E + 58 + 50, E + 158 + 20, FAR),
                  existing=tail, origin=origin)
        out += at(f"an offset of 0 behind {origin + E} bytes of existing output", "j", "long history", seq(b"abc", 3 + 400, 30) + seq(b"x", 0, 4), (E + 33, E + 34),
                  existing=tail, origin=origin)
    return out


def text_cases():
    """(t) blocks the oracle compressed: text, alone, behind a dictionary as prefix and as existing output."""
    out = []
    text = synth.gen_text_zipf(17, 9000).tobytes()
    comp = o.compress2(text)[1]
    n = len(text)
    out += at("text", "t", "text", comp, (1, 63, 64, 65, 256, 1000, 4096, n - 1, n, n + 1))
    d = synth.gen_text_zipf(67, 30_000).tobytes()
    dic, payload = d[:20_000], d[20_000:]
    comp = o.compress2(dic + payload, cursor=len(dic))[1]
    out += at("text behind a dictionary", "t", "prefix", comp, (1, 64, 700, 5000, len(payload)), prefix=dic)
    out += at("text behind existing output", "t", "existing", comp, (20_001, 20_064, 20_700, 25_000, 20_000 + len(payload)), existing=dic)
    return out


def all_cases():
    """[(case, (status, out_len or None, bytes or None))] — the expectation of every case by the oracle."""
    cs = (literal_cases() + match_cases() + boundary_cases() + round_cases() + chunk_cases() + degenerate_cases() + error_cases()
          + contract_cases() + history_cases() + text_cases())
    assert len({c["name"] for c in cs}) == len(cs)
    return [(c, expect(c)) for c in cs]


COUNTS = dict(a=22, b=271, c=23, d=9, e=30, f=61, g=17, h=84, i=3, j=19, t=20)
SUBS = dict(a={"own-lane", "wave-wide"},
            b={"apart", "prefix", "prefix into out", "existing"} | {f"overlap {k}" for k in (1, 2, 3, 4, 8)},
            c={f"status {k}" for k in (1, 2, 3, 4)}, d={f"status {k}" for k in (2, 3, 4)},
            e={f"sequence {k}" for k in (ROUND - 1, ROUND, ROUND + 1)},
            f={"chunk boundary", "beyond a chunk", "token list cut"},
            g={"target == existing", "target < existing", "one past the end", "far past the end", "empty input"},
            h={f"status {k}" for k in (1, 2, 3, 4)} | {"precedence"}, i={"prefix", "existing"}, j={"long history", "below the contract"})


def census(rows):
    return {k: sum(c["cls"] == k for c, _ in rows) for k in COUNTS}


def assert_covers(rows):
    """What both tests state on the ORACLE's results before anything is compared: every class is there with every kind it names, in
    the pinned numbers, and holds the verdicts it is about."""
    assert census(rows) == COUNTS, census(rows)
    for k, subs in SUBS.items():
        have = {c["sub"] for c, _ in rows if c["cls"] == k}
        assert subs <= have, (k, subs - have)
    by = lambda k: [(c, e) for c, e in rows if c["cls"] == k]      # noqa: E731
    assert all(e[0] == 0 and e[1] == c["target"] for c, e in by("a") + by("b") + by("c") + by("e"))
    assert all(e[0] == int(c["sub"][-1]) for c, e in by("d"))
    assert all(e[0] == CONTRACT for _, e in by("i"))
    assert {e[0] for _, e in by("h")} == {0, 1, 2, 3, 4} and {e[0] for _, e in by("j")} == {0, 3}
    assert all(e[0] == 0 for _, e in by("g") + by("t"))
