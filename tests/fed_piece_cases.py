"""Built cases for the PIECE HAND-OVER of the bitmap-fed decompress kernel (test infrastructure; used by tests/test_fed_piece_cases_cpu.py on
the CPU and tests/test_gpu_fed_pieces.py on the GPU).

A launch with more jobs than resident wavefronts cuts every job into pieces; each piece takes the decoder state (flag, expect, o) its predecessor
parked and continues the chain (lz4_decompress_fed.hip, the piece rules of rust-lz-fear_amd/csrc/lzf_fed_window.h).  The model is the emulator of
the kernel's window loop run piece by piece (tests/emu/emu_fed_window.cpp, lzf_emu_fed_pieces): per piece what it does, the state it parks and its
windows and batches.  Blocks are a few to a few dozen rounds of 1 024 compressed bytes, built sequence by sequence (the builder of
seg_stage_cases.py, the stretches and token-like literals of fed_window_cases.py); every case names the edges it is built for and the piece counts
at which it reaches them, and asserts that on the CPU — from the model and the token walk, never from the kernel.  edges() is the census the CPU
test requires over the whole corpus."""
import collections
import ctypes as C
import functools

import numpy as np

import fed_window_cases as fw
from fed_window_cases import CARRY, CHUNK, LIMIT, OVERLAP, ROUND, STRIDE
from seg_stage_cases import Blk, _seq  # noqa: F401

ENDED = 0x80000000                    # kFedEnded (kernels.h)
PIECES = (2, 3, 16)                   # the piece counts the GPU tests run; the census adds one more than a block's rounds
PASS, PARKED, PARKED_AT_ONCE, FINISHED, WALK_FAILED, STATUS, EXPIRED = range(7)      # lzf_emu_fed_pieces: what a piece does
WHAT = ("passes", "parks", "parks at once", "finishes", "fails in walk mode", "fails a copy-stage check", "expires")

Model = collections.namedtuple("Model", "rc rec end_piece done flag taken stats log")


def _lib():
    L = fw.emu_lib()
    if not getattr(L, "_pieces", False):
        u32, p32, p64 = C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        L.lzf_emu_fed_pieces.restype = C.c_int
        L.lzf_emu_fed_pieces.argtypes = [C.c_char_p, u32, u32, u32, u32, u32, C.c_uint64, u32, C.c_int, p32, p32, p64, p32, u32, p32]
        for name, n in (("piece_end", 3), ("group_jobs", 3), ("ticket_piece", 2), ("ticket_rank", 5)):
            f = getattr(L, "lzf_emu_fedw_" + name)
            f.restype, f.argtypes = u32, [u32] * n
        L._pieces = True
    return L


def piece_end(n, pieces, p):
    return int(_lib().lzf_emu_fedw_piece_end(n, pieces, p))


def rounds_of(n):
    return (n + ROUND - 1) // ROUND


def emulate_pieces(blk, pieces, prefix_len=0, existing_len=0, limit=LIMIT, cap=None, carry=CARRY, expire=-1):
    """The window loop over one job, piece by piece -> Model: rec[p] = dict(what, expect, o, listed, walked, batches, tokens, took), the piece
    that ended the job for the kernel (None: none), done, the job's flag after all pieces, true tokens taken, the stats of fw.emulate, and the log
    per piece that ran: {p: [(kind, position)]} — kind 0 a window listed from the map, 1 a window walked, 2 a batch left for the next window."""
    blk = bytes(blk)
    cap = (1 << 24) if cap is None else cap
    rec, summ, st = (C.c_uint32 * (8 * pieces))(), (C.c_uint32 * 4)(), (C.c_uint64 * 8)()
    lcap = len(blk) // 8 + 64 + 2 * pieces
    log, n = (C.c_uint32 * (2 * lcap))(), C.c_uint32(0)
    rc = _lib().lzf_emu_fed_pieces(blk, len(blk), pieces, carry, prefix_len, existing_len, limit, cap, expire, rec, summ, st, log, lcap, C.byref(n))
    assert n.value <= lcap
    names = ("what", "expect", "o", "listed", "walked", "batches", "tokens", "took")
    recs = [dict(zip(names, [int(v) for v in rec[8 * p:8 * p + 8]])) for p in range(pieces)]
    by_piece, cur = {}, None
    for i in range(n.value):
        k, pos = int(log[2 * i]), int(log[2 * i + 1])
        if k == 3:
            cur = by_piece.setdefault(pos, [])
        else:
            cur.append((k, pos))
    end = None if summ[0] == 0xFFFFFFFF else int(summ[0])
    return Model(rc, recs, end, int(summ[1]), int(summ[2]), int(summ[3]), dict(zip(fw.STAT_NAMES, [int(v) for v in st])), by_piece)


def state_after(m, k):
    """(flag, expect, o, under_way) the model holds after the first k pieces of the job: what lzf_debug_fed shows with stop_piece = k.
    under_way: the job is parked in front of piece k (expect, o count); else it has ended (flag kFedEnded) and m.done says how."""
    if m.end_piece is not None and m.end_piece < k:
        return ENDED, None, None, False
    r = m.rec[k - 1]
    assert r["what"] in (PARKED, PARKED_AT_ONCE)
    return k, r["expect"], r["o"], True


def tokens(blk):
    """The chain of a block as far as it can be walked: [(position, L, M, offset or None, next)]."""
    out, p, n = [], 0, len(blk)
    while p < n:
        t = blk[p]; q = p + 1; L = t >> 4
        if L == 15:
            while True:
                if q >= n:
                    return out
                b = blk[q]; q += 1; L += b
                if b != 255:
                    break
        if n - q < L:
            return out
        q += L
        if n - q < 2:
            out.append((p, L, 0, None, n)); break
        off = blk[q] | (blk[q + 1] << 8); q += 2; M = (t & 15) + 4
        if (t & 15) == 15:
            while True:
                if q >= n:
                    return out
                b = blk[q]; q += 1; M += b
                if b != 255:
                    break
        out.append((p, L, M, off, q)); p = q
    return out


def decode_below(c, expect):
    """The job's output (existing included) once the tokens that start below `expect` are decoded: a plain decoder over the token walk
    (decompress.rs:58-138), for the bytes a job has written when it is parked — of a damaged block too, which the oracle only rejects.  The CPU
    test holds it to the oracle over every valid block."""
    blk, pre = c["input"], c["prefix"]
    out = bytearray(pre + c["existing"])
    for p, L, M, off, nxt in tokens(blk):
        if p >= expect:
            break
        q = p + 1 + (0 if L < 15 else 1 + (L - 15) // 255)
        out += blk[q:q + L]
        if off is not None:
            assert 1 <= off <= len(out), (c["name"], p, off)
            s = len(out) - off
            out += out[s:s + M] if off >= M else (bytes(out[s:]) * (M // off + 1))[:M]
    return bytes(out[len(pre):])


# ------------------------------------------------------------------------------------------------------------------------ the census
RESIDUE_EDGES = tuple(f"history: o at the hand-over at output residue {r}" for r in (0, 1, 15))
OFFSET_EDGES = tuple(f"history: first match of a piece at offset {x}" for x in (1, 2, 3, 4095, 4096, 4097, 65535))


def edges():
    """Every named edge of the hand-over."""
    return {"boundary: a token starts at piece_end", "boundary: a token starts one byte below piece_end",
            "boundary: a token in the last 31 bytes below piece_end, the window runs across it",
            "boundary: a literal run crosses piece_end", "boundary: a match-length tail crosses piece_end",
            "empty: one piece parks at once", "empty: three pieces in a row park at once",
            "carry: the tail's first token below piece_end, the piece overruns by a window",
            "carry: the tail at or behind piece_end, the next piece's first batch",
            "early end: a window reaches the input's end although piece_end < len", "early end: finished in a piece that is not the last, later tickets pass",
            "rounds < pieces", "rounds == pieces", "rounds == k * pieces", "rounds == k * pieces + 1", "one round",
            "history: the match reaches into the existing output", "history: the match reaches into the prefix",
            "history: o at the hand-over below 4 096", "history: o at the hand-over above 4 096",
            "walk: a piece's first window is walked at the start of a chunk's share",
            "damage: invalid, a piece > 0 ends the job", "damage: still valid, other bytes", "damage: truncated inside a piece > 0",
            } | set(RESIDUE_EDGES) | set(OFFSET_EDGES)


def census(case, pieces, m):
    """The edges one case reaches at one piece count, from the model and the token walk."""
    blk, n = case["input"], len(case["input"])
    toks = tokens(blk)
    starts = {t[0]: t for t in toks}
    ex, plen = len(case["existing"]), len(case["prefix"])
    got = set()
    R = rounds_of(n)
    if R == 1:
        got.add("one round")
    if R < pieces:
        got.add("rounds < pieces")
    elif R == pieces:
        got.add("rounds == pieces")
    elif R % pieces == 0:
        got.add("rounds == k * pieces")
    elif R % pieces == 1:
        got.add("rounds == k * pieces + 1")
    if case["damage"]:
        if case["damage"] == "invalid" and m.end_piece and not m.done:
            got.add("damage: invalid, a piece > 0 ends the job")
        if case["damage"] == "valid" and m.done:
            got.add("damage: still valid, other bytes")
        if case["damage"] == "truncated" and m.end_piece and not m.done:
            got.add("damage: truncated inside a piece > 0")
        return got
    out_at = {}                              # token position -> output position of its literals
    o = ex
    for t in toks:
        out_at[t[0]] = o; o += t[1] + t[2]
    run = 0
    for p in range(pieces):
        r = m.rec[p]
        E = piece_end(n, pieces, p)
        run = run + 1 if r["what"] == PARKED_AT_ONCE else 0
        if run == 1 and (p + 1 == pieces or m.rec[p + 1]["what"] != PARKED_AT_ONCE) and (p == 0 or m.rec[p - 1]["what"] != PARKED_AT_ONCE):
            got.add("empty: one piece parks at once")
        if run >= 3:
            got.add("empty: three pieces in a row park at once")
        if r["what"] == FINISHED and p + 1 < pieces:
            got.add("early end: finished in a piece that is not the last, later tickets pass")
            assert all(x["what"] == PASS for x in m.rec[p + 1:])
            if E < n:
                got.add("early end: a window reaches the input's end although piece_end < len")
        log = m.log.get(p, [])
        if r["what"] in (PARKED, PARKED_AT_ONCE) and E < n:
            # ---- the boundary E between this piece and the next
            if E in starts:
                got.add("boundary: a token starts at piece_end")
            if E - 1 in starts:
                got.add("boundary: a token starts one byte below piece_end")
            if any(E - 31 <= t < E for t in starts) and any(k in (0, 1) and c == E - 32 for k, c in log):
                got.add("boundary: a token in the last 31 bytes below piece_end, the window runs across it")
            for t in toks:
                if t[0] < E and t[4] >= E + 100:           # the next token lies well inside the next piece
                    lit_end = t[4] if t[3] is None else t[4] - 2 - max(0, 1 + (t[2] - 19) // 255 if t[2] >= 19 else 0)
                    if lit_end > E and t[1] >= 100:
                        got.add("boundary: a literal run crosses piece_end")
                    elif t[2] >= 19 + 255 * 100:
                        got.add("boundary: a match-length tail crosses piece_end")
            for i, (k, pos) in enumerate(log):
                if k == 2 and pos < E and i + 1 < len(log) and log[i + 1][0] == 0 and log[i + 1][1] < E < log[i + 1][1] + ROUND:
                    got.add("carry: the tail's first token below piece_end, the piece overruns by a window")
            if log and log[-1][0] == 2 and log[-1][1] >= E and r["what"] == PARKED and m.rec[p + 1]["took"] == log[-1][1] and m.rec[p + 1]["batches"]:
                got.add("carry: the tail at or behind piece_end, the next piece's first batch")
        if p > 0 and r["what"] in (PARKED, FINISHED) and r["took"] in starts:
            # ---- the hand-over into this piece: its first token, the state it took
            t = starts[r["took"]]
            o_in = out_at[t[0]]
            assert o_in == m.rec[p - 1]["o"]
            got.add("history: o at the hand-over below 4 096" if o_in - ex < 4096 else "history: o at the hand-over above 4 096")
            res = (case["rb"] + o_in) & 15
            if res in (0, 1, 15):
                got.add(f"history: o at the hand-over at output residue {res}")
            if t[3] is not None:
                mo = o_in + t[1]
                if t[3] in (1, 2, 3, 4095, 4096, 4097, 65535) and t[3] <= mo - ex:
                    got.add(f"history: first match of a piece at offset {t[3]}")
                if ex and mo - ex >= 1 and mo - ex < t[3] <= mo:
                    got.add("history: the match reaches into the existing output")
                if plen and t[3] > mo:
                    got.add("history: the match reaches into the prefix")
            Eprev = piece_end(n, pieces, p - 1)
            if Eprev > CHUNK - 1 and (Eprev - OVERLAP) % STRIDE == 0 and len(log) >= 2 and log[0][0] == 0 and log[1] == (1, log[0][1]) and log[0][1] < Eprev + ROUND:
                got.add("walk: a piece's first window is walked at the start of a chunk's share")
    return got


# ------------------------------------------------------------------------------------------------------------------ building blocks
def dense(b, n_rounds, n_tok=70):
    """n_rounds stretches of n_tok sequences in exactly 1 KiB each (more than a batch per window: tails that wait for the next window)."""
    for _ in range(n_rounds):
        for L, M in fw.stretch(n_tok):
            b.near(L, M)
    return b


def dense_to(b, target, n_tok=70):
    """Dense sequences up to compressed position `target` exactly: the next token starts there."""
    assert target == b.cpos or target - b.cpos >= 3, (target, b.cpos)
    while target - b.cpos >= 2 * ROUND:
        dense(b, 1, n_tok)
    while target - b.cpos >= 40:
        b.near(13, 4 + (b.cpos >> 4) % 5)                       # 16 bytes
    return b.to_c(target)


def hand_over_at(b, E):
    """... and one sequence of some 1 100 literals that ends at E: it is the last token its window lists (its successor lies beyond the window),
    so a piece that ends at E parks with expect == E and the token built next is the first of the piece behind it."""
    dense_to(b, E - 1100)
    return b.to_c(E)


def finish(b, total):
    """... and the last literals, so that the block is `total` bytes."""
    dense_to(b, total - 6)
    return b.end(5)


def start(seed, prefix=b"", existing=b""):
    b = Blk(seed)
    b.o += prefix + existing
    return b


def case(name, b_or_blk, wants, at=PIECES, rb=0, prefix=b"", existing=b"", damage=None, total=None):
    """One job: the block (a Blk is finished to `total` bytes), the edges it is built for and the piece counts at which it reaches them."""
    if isinstance(b_or_blk, Blk):
        blk, out = finish(b_or_blk, total) if total else b_or_blk.end(5)
        assert out[:len(prefix) + len(existing)] == prefix + existing
        out = out[len(prefix):]
    else:
        blk, out = bytes(b_or_blk), None
    return dict(name=name, input=blk, prefix=prefix, existing=existing, rb=rb, wants=set(wants), at=tuple(at), damage=damage, built_out=out)


def _rnd(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def valid_cases():
    out = []
    # ---- boundary tokens.  Four rounds: 2 048 is the end of a piece at 2, 3 and 16 pieces (per = 2, 2, 1).
    for d, edge in ((0, "boundary: a token starts at piece_end"), (1, "boundary: a token starts one byte below piece_end"),
                    (17, "boundary: a token in the last 31 bytes below piece_end, the window runs across it"),
                    (31, "boundary: a token in the last 31 bytes below piece_end, the window runs across it")):
        b = hand_over_at(start(10 + d), 2048 - d)                # (the window in front lists nothing behind the token before it: a window starts on this one)
        b.near(9, 7)
        out.append(case(f"token {d} below piece_end", b, {edge}, rb=(0, 1, 15)[d % 3], total=4 * ROUND))
    b = dense_to(start(20), 2048 - 60); b.near(700, 9)
    out.append(case("literal run across piece_end", b, {"boundary: a literal run crosses piece_end"}, rb=1, total=4 * ROUND))
    b = dense_to(start(21), 2048 - 20); b.seq(2, 1, 19 + 255 * 140 + 3)
    out.append(case("match-length tail across piece_end", b, {"boundary: a match-length tail crosses piece_end"}, rb=15, total=4 * ROUND))
    # ---- empty pieces: 48 rounds in 16 pieces of 3 KiB; a literal run over the whole of piece 5, one over pieces 9, 10 and 11
    b = dense_to(start(30), 5 * 3072 - 100); b.near(3072 + 300, 8)
    dense_to(b, 9 * 3072 - 50); b.near(3 * 3072 + 200, 8)
    out.append(case("literal runs over whole pieces", b, {"empty: one piece parks at once", "empty: three pieces in a row park at once"}, at=(16,), total=48 * ROUND))
    # ---- carry at the boundary: dense stretches, every round of 16 and of 3 a piece (fed_window_cases: tails in front of piece boundaries)
    for rounds in (16, 3):
        out.append(case(f"tails at piece boundaries, {rounds} rounds", dense(start(40 + rounds), rounds - 1), {
            "carry: the tail's first token below piece_end, the piece overruns by a window",
            "carry: the tail at or behind piece_end, the next piece's first batch", "rounds == pieces"}, at=(rounds,), total=rounds * ROUND))
    # ---- early end: three rounds of which the last is 200 bytes, in two pieces: a window that starts below 2 048 reaches the end
    b = hand_over_at(start(50), 1500); b.near(12, 4)           # (a window starts at 1 472: its 1 024 bytes reach the end of the input)
    out.append(case("a last round of 200 bytes", b, {"early end: a window reaches the input's end although piece_end < len", "rounds == k * pieces + 1",
                                                      "early end: finished in a piece that is not the last, later tickets pass"}, at=(2,), total=2 * ROUND + 200))
    # ---- rounds against pieces
    out.append(case("one round", dense_to(start(60), 700), {"one round", "rounds < pieces"}, rb=15, total=ROUND - 24))
    out.append(case("five rounds", dense(start(61), 3), {"rounds < pieces", "rounds == k * pieces + 1", "early end: finished in a piece that is not the last, later tickets pass"}, total=5 * ROUND))
    out.append(case("two rounds", dense(start(62), 1), {"rounds == pieces"}, at=(2,), rb=1, total=2 * ROUND - 3))
    out.append(case("thirty-two rounds", dense(start(63), 20), {"rounds == k * pieces"}, at=(2, 16), total=32 * ROUND))
    out.append(case("thirty-three rounds", dense(start(64), 20), {"rounds == k * pieces + 1"}, at=(2, 16), rb=15, total=32 * ROUND + 9))
    out.append(case("six rounds", dense(start(65), 2), {"rounds == k * pieces"}, at=(2, 3), total=6 * ROUND))
    # ---- history across the hand-over: the token at 2 048 of a four-round block is the first of a piece at every piece count
    for k, off in enumerate((1, 2, 3, 4095, 4096, 4097, 65535)):
        b = start(70 + k)
        b.seq(6, 3, 70000 if off == 65535 else 5000)            # output enough for the offset, in a few bytes
        hand_over_at(b, 2048)
        want_res = (0, 1, 15)[k % 3]
        b.seq(0, off, 40 + k)
        out.append(case(f"first match of a piece at offset {off}", b, {f"history: first match of a piece at offset {off}", "history: o at the hand-over above 4 096",
                                                                       f"history: o at the hand-over at output residue {want_res}"},
                        rb=(want_res - len(b.o) + 40 + k) & 15, total=4 * ROUND))
    ex = _rnd(300, 80)
    b = hand_over_at(start(81, existing=ex), 2048)
    b.seq(0, b.opos - 10, 24)
    out.append(case("first match of a piece reaches into the existing output", b, {"history: the match reaches into the existing output", "history: o at the hand-over below 4 096"},
                    existing=ex, rb=1, total=4 * ROUND))
    pre, ex = _rnd(3000, 82), _rnd(17, 83)
    b = hand_over_at(start(84, prefix=pre, existing=ex), 2048)
    b.seq(0, b.opos - (len(pre) - 50), 50 + len(ex) + 100)      # from the prefix through the existing output into the job's own
    out.append(case("first match of a piece reaches into the prefix", b, {"history: the match reaches into the prefix"},
                    prefix=pre, existing=ex, rb=15, total=4 * ROUND))
    # ---- walk mode as a piece's first window: 32 rounds, the piece boundary 16 384 of 2 and 16 pieces is where chunk 1's share of the bit map
    # starts; a run of token-like literals from in front of chunk 1's first byte (14 336) to behind the boundary keeps chunk 1's own chain
    # out of step, so the window the next piece starts with comes wrong from the map
    for rem in (2, 1):
        b = dense_to(start(90 + rem), STRIDE - 200)
        at = b.cpos
        L = 200 + OVERLAP + 40
        while True:
            lit_start = at + 1 + (1 + (L - 15) // 255)
            if (lit_start + L - STRIDE) % 3 == rem:
                break
            L += 1
        lit = bytearray(_rnd(L, 92)); lit = bytearray(x or 1 for x in lit)
        lit[STRIDE - lit_start:] = fw.token_like(L - (STRIDE - lit_start))
        b.seq(L, 7, 9, lit=bytes(lit))
        assert CHUNK < b.cpos < CHUNK + 64
        dense(b, 4)
        wants = {"walk: a piece's first window is walked at the start of a chunk's share"} if rem == 2 else set()
        out.append(case(f"chunk 1 not in step at the piece boundary, run ends {rem} mod 3", b, wants, at=(2, 16), rb=rem - 1, total=32 * ROUND))
    return out


def damaged_cases():
    """A token of piece p > 0 changed (the reference rejects the block / it stays valid and decodes to other bytes) and a truncation inside piece p."""
    import oracle_ffi as o
    out = []
    base = finish(dense(start(100), 9), 12 * ROUND)[0]
    good = o.decompress_raw(base, limit=LIMIT, cap=LIMIT)
    assert good[0] == 0
    for r in (7, 10):                       # pieces 2: piece 1; 3: pieces 1 and 2; 16: pieces 7 and 10
        p = next(t[0] for t in tokens(base) if t[0] >= r * ROUND + 300)
        bad = other = None
        for v in range(256):
            if v == base[p]:
                continue
            b = base[:p] + bytes([v]) + base[p + 1:]
            e = o.decompress_raw(b, limit=LIMIT, cap=LIMIT)
            if e[0] != 0 and bad is None:
                bad = b
            if e[0] == 0 and e[1] != good[1] and other is None:
                other = b
        assert bad is not None and other is not None
        t = next(t for t in tokens(base) if t[0] == p)
        q = p + 1 + t[1]                    # its match offset
        zero = base[:q] + b"\0\0" + base[q + 2:]
        out.append(case(f"token of round {r} changed: invalid", bad, {"damage: invalid, a piece > 0 ends the job"}, damage="invalid", rb=1))
        out.append(case(f"match offset of round {r} zeroed", zero, {"damage: invalid, a piece > 0 ends the job"}, damage="invalid", rb=15))
        out.append(case(f"token of round {r} changed: still valid", other, {"damage: still valid, other bytes"}, damage="valid"))
        out.append(case(f"truncated inside round {r}", base[:p + 2], {"damage: truncated inside a piece > 0"}, damage="truncated", rb=1))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """Every case with what the oracle makes of it: exp = (status, bytes incl. existing), cap = the output capacity the jobs get."""
    import oracle_ffi as o
    cs = valid_cases() + damaged_cases()
    for c in cs:
        c["limit"] = LIMIT
        e = o.decompress_raw(c["input"], prefix=c["prefix"], existing=c["existing"], limit=LIMIT, cap=LIMIT)
        c["exp"] = e
        c["cap"] = (len(e[1]) if e[0] == 0 else 1 << 17) + 37
        if c["built_out"] is not None:
            assert e == (0, c["built_out"]), c["name"]
        assert rounds_of(len(c["input"])) <= 48 and c["cap"] <= 1 << 18, c["name"]
    return cs


def model(c, pieces, **kw):
    return emulate_pieces(c["input"], pieces, prefix_len=len(c["prefix"]), existing_len=len(c["existing"]), limit=c["limit"], cap=c["cap"], **kw)


@functools.lru_cache(maxsize=None)
def reach():
    """{edge: [(case name, pieces)]} over the corpus at the piece counts of the GPU tests and at one more than each block's rounds; every case is
    held to the edges it was built for."""
    got = collections.defaultdict(list)
    for c in corpus():
        mine = set()
        for pieces in sorted(set(PIECES) | {rounds_of(len(c["input"])) + 1}):
            m = model(c, pieces)
            assert m.rc == 0, (c["name"], pieces, m.rc)
            e = census(c, pieces, m)
            for x in e:
                got[x].append((c["name"], pieces))
            if pieces in c["at"]:
                mine |= e
        assert c["wants"] <= mine, (c["name"], sorted(c["wants"] - mine))
    return dict(got)
